// launch_log.h — the record of a context's kernel launches (pbrt_gpu_launch_log,
// include/pbrt_diag.h). Every launch a context makes goes through launch_logged(),
// which appends one record (the kernel's host function pointer and the launch
// shape) and launches; names are resolved only when the log is read, from the
// pointer-to-name tables the translation units build with PBRT_KERNEL_NAME.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace pbrt {

struct LaunchRec {
    const void* fn;
    uint32_t grid[3], block[3];
    uint32_t lds;     // dynamic LDS bytes of the launch
    int32_t stream;   // the context's stream: 0 main, 2, 3
};

struct LaunchLog {
    static constexpr size_t kMax = 4096;   // records kept; later launches only count
    std::vector<LaunchRec> recs;
    uint64_t overflow = 0;
    void clear() {
        recs.clear();
        overflow = 0;
    }
    void add(const void* fn, dim3 g, dim3 b, unsigned lds, int stream) {
        if (recs.size() >= kMax) {
            overflow++;
            return;
        }
        recs.push_back(LaunchRec{fn, {g.x, g.y, g.z}, {b.x, b.y, b.z}, lds, stream});
    }
};

// One entry per kernel a unit can launch: PBRT_KERNEL_NAME(k_chain_ci<1, 0, false, 0, false, false>)
// names the instantiation as its explicit instantiation spells it.
struct KernelName {
    const void* fn;
    const char* name;
};
#define PBRT_KERNEL_NAME(...) {reinterpret_cast<const void*>(&__VA_ARGS__), #__VA_ARGS__}

// hipLaunchKernelGGL with the record (log may be null: a launch outside any context).
template <class... P, class... A>
inline void launch_logged(LaunchLog* log, int stream_id, void (*kern)(P...), dim3 grid, dim3 block, unsigned lds,
                          hipStream_t st, A&&... args) {
    if (log) log->add(reinterpret_cast<const void*>(kern), grid, block, lds, stream_id);
    hipLaunchKernelGGL(kern, grid, block, lds, st, std::forward<A>(args)...);
}

}  // namespace pbrt

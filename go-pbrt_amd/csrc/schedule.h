// schedule.h — the host arithmetic of k_chain_ci's heaviest-first schedule: the
// learning step after a measured frame, and the process-wide cache of learned
// schedules. No HIP: tests/host_tables_check.cpp compiles this header on its own.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <unordered_map>
#include <vector>

namespace pbrt {

// The learning step (pbrt_gpu_synchronize): from every slot's chain ticks and the
// waves per tile it ran with (slot_kw; 1 where it has no entry), the slot order
// for the next frame of the configuration, heaviest first, and the return value:
// how many slots at its front are heavy. ci_wps: waves/SIMD of the one-wave chain
// launch, n_simd: the device's SIMDs, heavy_override: PBRT_CI_HEAVY (< 0: none).
inline int64_t learn_order(const std::vector<uint32_t>& t, const std::vector<uint8_t>& slot_kw, int ci_wps, int n_simd,
                           int64_t heavy_override, std::vector<uint32_t>& order) {
    // cost at 1 wave per tile: 2 and 4 waves measured 1.3x / 1.8x faster per tile
    std::vector<double> cost(t.size());
    double sum = 0;
    for (size_t i = 0; i < t.size(); i++) {
        const int w = i < slot_kw.size() ? slot_kw[i] : 1;
        cost[i] = (double)t[i] * (w == 8 ? 2.3 : w == 4 ? 1.8 : w == 2 ? 1.3 : 1.0);
        sum += cost[i];
    }
    order.resize(t.size());
    for (size_t i = 0; i < t.size(); i++) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
    // heavy: tiles whose 1-wave chain alone would take over 0.7x the
    // frame's throughput bound (summed cost over the chain's waves/SIMD)
    const double thr = 0.7 * sum / ((double)ci_wps * (double)n_simd);
    int64_t k = 0;
    while (k < (int64_t)t.size() && cost[order[(size_t)k]] > thr) k++;
    // at most a quarter of the wave slots; at most 1/16 of them when the tiles
    // outnumber the one-wave slots (one GPU, 1/2 shards), whose light launch then
    // fills the GPU longer than the heavy tiles take (1/2 of B: 216 -> 202 ms with
    // 64 against 256; 1/4 of B: best at 256, 126-129 ms against 131-142 at 128-384)
    const int64_t cap = (int64_t)t.size() > (int64_t)ci_wps * n_simd ? n_simd / 16 : n_simd / 4;
    return heavy_override >= 0 ? heavy_override : std::min<int64_t>(k, cap);
}

// Process-wide schedule cache. internal/render/server.go:29-164 builds a fresh
// scene, integrator and renderer for every request, so each request's context
// would otherwise start from the cold-frame probe. A context that measured a
// frame stores its heaviest-first slot order here, keyed by a hash of the scene's
// content, the frame's schedule key and the device's size; a fresh context on the
// same scene and configuration starts from it. Only the schedule changes, never a
// result, so a hash collision could only cost speed.
struct SchedEntry {
    std::vector<uint32_t> order;   // slot order, heaviest first
    int64_t heavy_k = 0;           // slots at its front that run at 4 waves
};
inline std::mutex g_sched_mu;
inline std::unordered_map<uint64_t, SchedEntry> g_sched;
constexpr size_t kSchedCacheMax = 64;   // configurations kept (a full frame's order is 32 KB)

inline bool sched_cache_get(uint64_t key, int64_t nb, SchedEntry& out) {
    std::lock_guard<std::mutex> lk(g_sched_mu);
    auto it = g_sched.find(key);
    if (it == g_sched.end() || (int64_t)it->second.order.size() != nb) return false;
    out = it->second;
    return true;
}
inline void sched_cache_put(uint64_t key, const std::vector<uint32_t>& order, int64_t heavy_k) {
    std::lock_guard<std::mutex> lk(g_sched_mu);
    if (g_sched.size() >= kSchedCacheMax && !g_sched.count(key)) g_sched.clear();
    SchedEntry& e = g_sched[key];
    e.order = order;
    e.heavy_k = heavy_k;
}
inline void sched_cache_clear() {
    std::lock_guard<std::mutex> lk(g_sched_mu);
    g_sched.clear();
}

}  // namespace pbrt

// kernel_select.hip — the selectors' tables (kernel_select.h), each once in the library, and
// the launch log's names of every kernel it compiles (pbrt_gpu_kernel_names,
// pbrt_diag_kernel_choice: include/pbrt_diag.h).
#include <hip/hip_runtime.h>

#include <string>

#include "kernel_select.h"

#include "../../include/pbrt_diag.h"

namespace pbrtk {

namespace {
struct ChainRow { int w, depth; bool kx; int eu; bool spwin, multi; ChainKernel fn; const char* name; };
#define CHAIN_ROW(...) {__VA_ARGS__, &k_chain_ci<__VA_ARGS__>, "k_chain_ci<" #__VA_ARGS__ ">"}
const ChainRow kChainKernels[] = {
    // one wave per tile, the group's state in scalar registers (k_chain_1.hip)
    CHAIN_ROW(1, 0, false, 0, false, false),  CHAIN_ROW(1, 0, false, 2, false, false),
    CHAIN_ROW(1, 64, false, 0, false, false), CHAIN_ROW(1, 64, false, 2, false, false),
    CHAIN_ROW(1, 0, false, 0, true, false),   CHAIN_ROW(1, 0, false, 2, true, false),
    CHAIN_ROW(1, -1, false, 0, false, false),
    // 2, 4 or 8 waves per tile (k_chain_n.hip)
    CHAIN_ROW(2, 0, false, 0, false, false),  CHAIN_ROW(4, 0, false, 0, false, false),
    CHAIN_ROW(8, 0, false, 0, false, false),  CHAIN_ROW(2, 64, false, 0, false, false),
    CHAIN_ROW(4, 64, false, 0, false, false), CHAIN_ROW(8, 64, false, 0, false, false),
    CHAIN_ROW(2, 0, false, 0, true, false),   CHAIN_ROW(4, 0, false, 0, true, false),
    CHAIN_ROW(8, 0, false, 0, true, false),   CHAIN_ROW(2, -1, false, 0, false, false),
    CHAIN_ROW(4, -1, false, 0, false, false), CHAIN_ROW(8, -1, false, 0, false, false),
    // kX at 2 or 4 waves per tile (k_chain_x.hip)
    CHAIN_ROW(2, 0, true, 0, false, false),   CHAIN_ROW(4, 0, true, 0, false, false),
    CHAIN_ROW(2, 64, true, 0, false, false),  CHAIN_ROW(4, 64, true, 0, false, false),
    // the per-lane code: several tiles per wave, and the one-wave kX chain (k_chain_g.hip)
    CHAIN_ROW(1, 0, false, 0, false, true),   CHAIN_ROW(1, 0, false, 2, false, true),
    CHAIN_ROW(1, 64, false, 0, false, true),  CHAIN_ROW(1, 64, false, 2, false, true),
    CHAIN_ROW(1, 0, false, 0, true, true),    CHAIN_ROW(1, 0, false, 2, true, true),
    CHAIN_ROW(1, -1, false, 0, false, true),  CHAIN_ROW(1, 0, true, 0, false, true),
    CHAIN_ROW(1, 64, true, 0, false, true),
};
#undef CHAIN_ROW

struct PathsCiRow { int P; bool mb, kx; PathsCiKernel fn; const char* name; };
#define PATHS_CI_ROW(...) {__VA_ARGS__, &k_paths_ci<__VA_ARGS__>, "k_paths_ci<" #__VA_ARGS__ ">"}
const PathsCiRow kPathsCiKernels[] = {   // (kX: 4 or 8 pixels per wave)
    PATHS_CI_ROW(2, false, false), PATHS_CI_ROW(4, false, false), PATHS_CI_ROW(8, false, false),
    PATHS_CI_ROW(2, true, false),  PATHS_CI_ROW(4, true, false),  PATHS_CI_ROW(8, true, false),
    PATHS_CI_ROW(4, false, true),  PATHS_CI_ROW(8, false, true),
    PATHS_CI_ROW(4, true, true),   PATHS_CI_ROW(8, true, true),
};
#undef PATHS_CI_ROW

struct PathsCamRow { int P; bool mb, stack; PathsCamKernel fn; const char* name; };
#define PATHS_CAM_ROWS(P, mb)                                             \
    {P, mb, false, &k_paths_cam<P, mb>, "k_paths_cam<" #P ", " #mb ">"}, \
    {P, mb, true, &k_paths_cam_stack<P, mb>, "k_paths_cam_stack<" #P ", " #mb ">"}
const PathsCamRow kPathsCamKernels[] = {   // stack: the k_paths_cam_stack kernels of trees beyond kLdsNodes
    PATHS_CAM_ROWS(4, false), PATHS_CAM_ROWS(16, false), PATHS_CAM_ROWS(64, false),
    PATHS_CAM_ROWS(4, true),  PATHS_CAM_ROWS(16, true),  PATHS_CAM_ROWS(64, true),
};
#undef PATHS_CAM_ROWS

// The device queries' families (k_li, k_li_strat, k_li_direct, k_path_step) are each instantiated over
// <kX, kDepth> alike: one row type, one set of rows, one lookup.
template <class K>
struct QueryRow { bool kx; int depth; K fn; const char* name; };
#define QUERY_ROW(k, kx, depth) {kx, depth, &k<kx, depth>, #k "<" #kx ", " #depth ">"}
#define QUERY_ROWS(k) {QUERY_ROW(k, false, 0), QUERY_ROW(k, true, 0), QUERY_ROW(k, false, 64), QUERY_ROW(k, true, 64)}
const QueryRow<LiKernel> kLiKernels[] = QUERY_ROWS(k_li);
const QueryRow<LiStratKernel> kLiStratKernels[] = QUERY_ROWS(k_li_strat);
const QueryRow<DirectLiKernel> kDirectLiKernels[] = QUERY_ROWS(k_li_direct);
const QueryRow<PathStepKernel> kPathStepKernels[] = QUERY_ROWS(k_path_step);
#undef QUERY_ROWS
#undef QUERY_ROW
template <class K, size_t N>
K query_kernel(const QueryRow<K> (&rows)[N], bool kx, int depth) {
    for (const QueryRow<K>& r : rows)
        if (r.kx == kx && r.depth == depth) return r.fn;
    return nullptr;
}
}  // namespace

ChainKernel chain_kernel(int w, int depth, bool kx, int eu, bool spwin, bool multi) {
    for (const ChainRow& r : kChainKernels)
        if (r.w == w && r.depth == depth && r.kx == kx && r.eu == eu && r.spwin == spwin && r.multi == multi)
            return r.fn;
    return nullptr;
}

PathsCiKernel paths_ci_kernel(int P, bool mb, bool kx) {
    for (const PathsCiRow& r : kPathsCiKernels)
        if (r.P == P && r.mb == mb && r.kx == kx) return r.fn;
    return nullptr;
}
int paths_ci_lds(int P, int staged_values) {
    switch (P) {
    case 2: return paths_group_lds<2>(staged_values);
    case 4: return paths_group_lds<4>(staged_values);
    case 8: return paths_group_lds<8>(staged_values);
    default: return -1;
    }
}

PathsCamKernel paths_cam_kernel(int P, bool mb, bool stack) {
    for (const PathsCamRow& r : kPathsCamKernels)
        if (r.P == P && r.mb == mb && r.stack == stack) return r.fn;
    return nullptr;
}

LiKernel li_kernel(bool kx, int depth) { return query_kernel(kLiKernels, kx, depth); }
LiStratKernel li_strat_kernel(bool kx, int depth) { return query_kernel(kLiStratKernels, kx, depth); }
DirectLiKernel direct_li_kernel(bool kx, int depth) { return query_kernel(kDirectLiKernels, kx, depth); }
PathStepKernel path_step_kernel(bool kx, int depth) { return query_kernel(kPathStepKernels, kx, depth); }

SerialKernel serial_kernel(int min_waves) {
    switch (min_waves) {
    case 1: return k_render_exact<1>;
    case 2: return k_render_exact<2>;
    case 4: return k_render_exact<4>;
    case 8: return k_render_exact<8>;
    default: return nullptr;
    }
}

// ---- the launch log (pbrt_diag.h): names by host function pointer. One entry per
// kernel the library compiles, spelled as its explicit instantiation is
// (tests/test_kernel_manifest.py compares the names with the sources). The k_chain_ci,
// k_paths_ci, k_paths_cam[_stack], k_li, k_li_strat, k_li_direct and k_path_step families are named by their selectors' tables.
namespace {
const KernelName kKernelNames[] = {
    // k_paths_m.hip, k_paths_x.hip
    PBRT_KERNEL_NAME(k_mb_setup<false>),
    PBRT_KERNEL_NAME(k_mb_setup<true>),
    // k_chain_c.hip, k_paths_c.hip
    PBRT_KERNEL_NAME(k_chain_cam),
    PBRT_KERNEL_NAME(k_cam_setup),
    PBRT_KERNEL_NAME(k_chain_cam_stack),
    PBRT_KERNEL_NAME(k_film_cam<false>),
    PBRT_KERNEL_NAME(k_film_cam<true>),
    // k_serial.hip
    PBRT_KERNEL_NAME(k_render_exact<1>),
    PBRT_KERNEL_NAME(k_render_exact<2>),
    PBRT_KERNEL_NAME(k_render_exact<4>),
    PBRT_KERNEL_NAME(k_render_exact<8>),
    // k_pw.hip
    PBRT_KERNEL_NAME(k_pw_trace<false>),
    PBRT_KERNEL_NAME(k_pw_trace<true>),
    PBRT_KERNEL_NAME(k_pw_shadow<false>),
    PBRT_KERNEL_NAME(k_pw_shadow<true>),
    PBRT_KERNEL_NAME(k_pw_cache<false>),
    PBRT_KERNEL_NAME(k_pw_cache<true>),
    PBRT_KERNEL_NAME(k_pw_start<false, false>),
    PBRT_KERNEL_NAME(k_pw_start<false, true>),
    PBRT_KERNEL_NAME(k_pw_start<true, false>),
    PBRT_KERNEL_NAME(k_pw_start<true, true>),
    PBRT_KERNEL_NAME(k_pw_shade<false>),
    PBRT_KERNEL_NAME(k_pw_shade<true>),
    PBRT_KERNEL_NAME(k_pw_scan),
    PBRT_KERNEL_NAME(k_pw_scatter),
    PBRT_KERNEL_NAME(k_pw_panics),
    // k_frame.hip
    PBRT_KERNEL_NAME(k_film),
    PBRT_KERNEL_NAME(k_panic_reduce),
    PBRT_KERNEL_NAME(k_wf_primary<false>),
    PBRT_KERNEL_NAME(k_wf_primary<true>),
    PBRT_KERNEL_NAME(k_dl_setup),
    PBRT_KERNEL_NAME(k_dl_samples<false>),
    PBRT_KERNEL_NAME(k_dl_samples<true>),
    PBRT_KERNEL_NAME(k_dl_panics),
    PBRT_KERNEL_NAME(k_tile_cost<false>),
    PBRT_KERNEL_NAME(k_tile_cost<true>),
    PBRT_KERNEL_NAME(k_gate),
    PBRT_KERNEL_NAME(k_order_of_keys),
    PBRT_KERNEL_NAME(k_merge_film),
    PBRT_KERNEL_NAME(k_intersect),
    // k_group.hip, k_query.hip
    PBRT_KERNEL_NAME(k_merge_film_group),
    PBRT_KERNEL_NAME(k_query_hit<false, false>),
    PBRT_KERNEL_NAME(k_query_hit<true, false>),
    PBRT_KERNEL_NAME(k_query_hit<false, true>),
    PBRT_KERNEL_NAME(k_query_hit<true, true>),
    PBRT_KERNEL_NAME(k_query_hit_staged<false>),
    PBRT_KERNEL_NAME(k_query_hit_staged<true>),
    PBRT_KERNEL_NAME(k_query_camera),
    // k_film_q.hip
    PBRT_KERNEL_NAME(k_frame_samples),
    PBRT_KERNEL_NAME(k_film_add_tiles<false>),
    PBRT_KERNEL_NAME(k_film_add_tiles<true>),
    PBRT_KERNEL_NAME(k_film_add_merge),
    PBRT_KERNEL_NAME(k_film_rgba8),
    // k_path_step.hip
    PBRT_KERNEL_NAME(k_path_begin),
    // k_strat.hip
    PBRT_KERNEL_NAME(k_strat_pixels),
};

template <class F>
void each_kernel(F f) {   // f(pointer, name) of every kernel: the selectors' tables, kKernelNames, the LBVH and diagnostics units'
    for (const ChainRow& r : kChainKernels) f(reinterpret_cast<const void*>(r.fn), r.name);
    for (const PathsCiRow& r : kPathsCiKernels) f(reinterpret_cast<const void*>(r.fn), r.name);
    for (const PathsCamRow& r : kPathsCamKernels) f(reinterpret_cast<const void*>(r.fn), r.name);
    for (const auto& r : kLiKernels) f(reinterpret_cast<const void*>(r.fn), r.name);
    for (const auto& r : kLiStratKernels) f(reinterpret_cast<const void*>(r.fn), r.name);
    for (const auto& r : kDirectLiKernels) f(reinterpret_cast<const void*>(r.fn), r.name);
    for (const auto& r : kPathStepKernels) f(reinterpret_cast<const void*>(r.fn), r.name);
    for (const KernelName& k : kKernelNames) f(k.fn, k.name);
    for (const auto names : {mesh_bvh_kernel_names, diag_kernel_names}) {
        size_t n = 0;
        const KernelName* k = names(&n);
        for (size_t i = 0; i < n; i++) f(k[i].fn, k[i].name);
    }
}
}  // namespace

const char* kernel_name_of(const void* fn, const char* unknown) {
    const char* name = unknown;
    each_kernel([&](const void* f, const char* n) { if (f == fn) name = n; });
    return name;
}

}  // namespace pbrtk

using namespace pbrtk;

extern "C" int pbrt_gpu_kernel_names(const char** out, int n) {
    int k = 0;
    each_kernel([&](const void*, const char* name) {
        if (out && k < n) out[k] = name;
        k++;
    });
    return k;
}

extern "C" const char* pbrt_diag_kernel_choice(const char* family, const int* a, int n) {
    if (!family || !a) return nullptr;
    const std::string f = family;
    const void* fn = nullptr;
    if (f == "k_chain_ci" && n == 6)
        fn = reinterpret_cast<const void*>(chain_kernel(a[0], a[1], a[2] != 0, a[3], a[4] != 0, a[5] != 0));
    else if (f == "k_paths_ci" && n == 3)
        fn = reinterpret_cast<const void*>(paths_ci_kernel(a[0], a[1] != 0, a[2] != 0));
    else if (f == "k_paths_cam" && n == 3)
        fn = reinterpret_cast<const void*>(paths_cam_kernel(a[0], a[1] != 0, a[2] != 0));
    else if (f == "k_render_exact" && n == 1)
        fn = reinterpret_cast<const void*>(serial_kernel(a[0]));
    else if (f == "k_li" && n == 2)
        fn = reinterpret_cast<const void*>(li_kernel(a[0] != 0, a[1]));
    else if (f == "k_li_strat" && n == 2)
        fn = reinterpret_cast<const void*>(li_strat_kernel(a[0] != 0, a[1]));
    else if (f == "k_li_direct" && n == 2)
        fn = reinterpret_cast<const void*>(direct_li_kernel(a[0] != 0, a[1]));
    else if (f == "k_path_step" && n == 2)
        fn = reinterpret_cast<const void*>(path_step_kernel(a[0] != 0, a[1]));
    return fn ? kernel_name_of(fn, nullptr) : nullptr;
}

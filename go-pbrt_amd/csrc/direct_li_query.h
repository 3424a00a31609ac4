// direct_li_query.h — the host side of pbrt_gpu_direct_li_device
// (include/pbrt_gpu.h) that needs no device: the argument checks, the refusals
// (prepare's for a DirectLighting render, render.hip), the choice of the
// k_li_direct instantiation and its capped grid, and the size of the level
// records the kX instantiations keep in global memory.
// Plain C++ with no dependency on HIP: queries.hip passes in what it knows of the
// context, and tests/direct_li_query_check.cpp compiles this header on its own.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/pbrt_gpu.h"
#include "li_query.h"

namespace pbrtdli {

constexpr int kRays = pbrtli::kLiRays;   // rays of one work list, as k_li's
constexpr int kMaxLevels = 32;           // level records of a ray (pbrt_path.h: kDlMaxLevels)
constexpr int kMaxDepthX = 2 * kMaxLevels;   // prepare's bound on Mirror / Glass / OrenNayar scenes
constexpr int kWaveLanes = 64;
constexpr int kRecDoubles = 7;           // a level record: own (3), f (3), |wi.ns| / pdf
constexpr int kGridCapMax = 65536;       // the knob's upper bound (PBRT_DIRECT_LI_GRID)

// PBRT_E_INVALID's conditions, in the header's order; `why` names the first.
// ctx_ok: the context is not NULL. in_flight: a render is in flight on it.
inline int check_args(bool ctx_ok, const pbrt_direct_li_desc* d, const pbrt_ray_soa* rays, const pbrt_rng_soa* rng,
                      size_t n, const pbrt_radiance_soa* out, bool in_flight, const char** why) {
    auto bad = [&](const char* m) {
        *why = m;
        return (int)PBRT_E_INVALID;
    };
    if (!ctx_ok) return bad("null context");
    if (!d) return bad("the direct li desc is NULL");
    if (!rays) return bad("rays is NULL");
    if (!pbrtli::rays_complete(*rays)) return bad("a ray array is NULL");
    if (!rng) return bad("rng is NULL");
    if (!pbrtli::rng_complete(*rng)) return bad("an rng array is NULL");
    if (!out) return bad("out is NULL");
    if (!pbrtli::radiance_complete(*out)) return bad("a radiance array is NULL");
    if (n > (size_t)INT32_MAX) return bad("more than 2^31 - 1 rays in one query");
    if (d->max_depth < 1) return bad("max_depth < 1");
    if (d->reserved[0] != 0 || d->reserved[1] != 0) return bad("reserved must be 0");
    if (in_flight) return bad("a render is in flight on this context");
    *why = "";
    return PBRT_OK;
}

// Where the kernel is not the reference. non_matte: the scene has a Mirror, Glass
// or OrenNayar material, so the recursion through smooth glass can start and the
// level records bound its depth; on a Matte-only scene any max_depth is served.
inline int check_supported(const pbrt_direct_li_desc& d, bool rough_glass, bool non_matte, const char** why) {
    auto no = [&](const char* m) {
        *why = m;
        return (int)PBRT_E_UNSUPPORTED;
    };
    if (d.dl_strategy != PBRT_DL_UNIFORM_SAMPLE_ALL && d.dl_strategy != PBRT_DL_UNIFORM_SAMPLE_ONE)
        return no("unsupported direct lighting strategy");
    if (rough_glass) return no("rough glass: every BSDF sample panics in the reference");
    if (non_matte && d.max_depth > kMaxDepthX)
        return no("DirectLighting maxDepth > 64 on a scene with Mirror / Glass / OrenNayar materials");
    *why = "";
    return PBRT_OK;
}

// Levels a ray can push at max_depth: one at each depth 0, 2, 4, .. with
// depth + 1 < max_depth (directlighting.go:95-101, the recursion enters at
// depth + 2, SURVEY #23), at most kMaxLevels.
inline int levels(int max_depth) {
    const int l = max_depth / 2;
    return l < 0 ? 0 : l > kMaxLevels ? kMaxLevels : l;
}

// Doubles of level-record storage, laid out [workgroup][level][field][lane]:
// bounded by the grid, not by n. (At most 65536 * 32 * 7 * 64 = 2^20 * 896.)
inline size_t level_doubles(uint32_t grid, int max_depth) {
    return (size_t)grid * (size_t)levels(max_depth) * (size_t)kRecDoubles * (size_t)kWaveLanes;
}

// The k_li_direct instantiation and its launch, chosen as pbrtli::kernel_args
// chooses k_li's: kX for Mirror / Glass / OrenNayar scenes; kDepth 0 walks a tree
// staged in LDS, 64 is the reference's stack beyond; a mesh changes neither.
// The grid is the work lists of n, capped at grid_cap (clamped to 1 ..
// kGridCapMax): a workgroup strides over the lists beyond. Only the kX kernels
// have level records.
struct KernelArgs {
    bool kx;
    int depth;
    uint32_t grid;          // workgroups of one wave
    int levels;             // level records per lane (0: kX false, or max_depth 1)
    size_t level_doubles;   // of the whole grid
};
inline KernelArgs kernel_args(bool non_matte, int n_nodes, bool mesh, size_t n, int lds_nodes, int grid_cap,
                              int max_depth) {
    const pbrtli::KernelArgs la = pbrtli::kernel_args(non_matte, n_nodes, mesh, n, lds_nodes);
    const uint32_t cap = (uint32_t)(grid_cap < 1 ? 1 : grid_cap > kGridCapMax ? kGridCapMax : grid_cap);
    KernelArgs a;
    a.kx = la.kx;
    a.depth = la.depth;
    a.grid = la.grid < cap ? la.grid : cap;
    a.levels = a.kx ? levels(max_depth) : 0;
    a.level_doubles = a.kx ? level_doubles(a.grid, max_depth) : 0;
    return a;
}

}  // namespace pbrtdli

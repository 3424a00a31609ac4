// li_query.h — the host side of pbrt_gpu_li_device (include/pbrt_gpu.h) that
// needs no device: the argument checks, the conditions under which path_step is
// not the reference (wave_eligible's, frame_route.h), and the choice of the k_li
// instantiation and its grid from the scene.
// Plain C++ with no dependency on HIP: queries.hip passes in what it knows of
// the context, and tests/li_query_check.cpp compiles this header on its own.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/pbrt_gpu.h"

namespace pbrtli {

constexpr int kLiRays = 256;        // rays of one wave's work list (k_li)
constexpr int kLiMaxDepth = 2048;   // draws of a path < 2^32 (wave_eligible)

// Every array a query requires of its rays (tmax may be NULL), its rng and its
// radiance: the one test each for every query that takes them (a caller words
// its own refusal). R: pbrt_ray_soa, or the camera rays' pbrt_ray_soa_out.
template <class R>
inline bool rays_complete(const R& r) { return r.ox && r.oy && r.oz && r.dx && r.dy && r.dz; }
inline bool rng_complete(const pbrt_rng_soa& g) { return g.state && g.inc; }
inline bool radiance_complete(const pbrt_radiance_soa& o) { return o.r && o.g && o.b; }

// PBRT_E_INVALID's conditions, in the header's order; `why` names the first.
// ctx_ok: the context is not NULL. in_flight: a render is in flight on it.
inline int check_args(bool ctx_ok, const pbrt_li_desc* d, const pbrt_ray_soa* rays, const pbrt_rng_soa* rng, size_t n,
                      const pbrt_radiance_soa* out, bool in_flight, const char** why) {
    auto bad = [&](const char* m) {
        *why = m;
        return (int)PBRT_E_INVALID;
    };
    if (!ctx_ok) return bad("null context");
    if (!d) return bad("the li desc is NULL");
    if (!rays) return bad("rays is NULL");
    if (!rays_complete(*rays)) return bad("a ray array is NULL");
    if (!rng) return bad("rng is NULL");
    if (!rng_complete(*rng)) return bad("an rng array is NULL");
    if (!out) return bad("out is NULL");
    if (!radiance_complete(*out)) return bad("a radiance array is NULL");
    if (n > (size_t)INT32_MAX) return bad("more than 2^31 - 1 rays in one query");
    if (d->max_depth < 1) return bad("max_depth < 1");
    if (d->reserved != 0) return bad("reserved must be 0");
    if (in_flight) return bad("a render is in flight on this context");
    *why = "";
    return PBRT_OK;
}

// What the scene and the desc say before a light distribution is built.
inline int check_supported(const pbrt_li_desc& d, bool rough_glass, const char** why) {
    auto no = [&](const char* m) {
        *why = m;
        return (int)PBRT_E_UNSUPPORTED;
    };
    if (d.integrator != PBRT_INTEGRATOR_PATH) return no("Path integrator only (DirectLighting.Li is pbrt_gpu_direct_li_device)");
    if (d.max_depth > kLiMaxDepth) return no("maxDepth > 2048");
    if (d.light_strategy != PBRT_LIGHT_STRATEGY_UNIFORM && d.light_strategy != PBRT_LIGHT_STRATEGY_POWER)
        return no("unsupported light sample strategy");
    if (rough_glass) return no("rough glass: every BSDF sample panics in the reference");
    *why = "";
    return PBRT_OK;
}

// The light distributions k_li replays: every light's pdf > 0 (one draw picks a
// light, four more sample it), or every pdf 0 -- func_int == 0 with every func
// 0, the reference's Power strategy, whose 2n entries are Y() == 0 (SURVEY
// #28): UniformSampleOneLight returns black after its one draw and never reads
// the picked index, which may lie beyond the lights. A distribution that mixes
// the two, a negative or a NaN entry is refused: a picked index could then
// reach the light array, which the builder's 2n entries overrun.
inline bool all_positive(const double* func, int count, double func_int) {
    if (!(func_int > 0)) return false;
    for (int i = 0; i < count; i++)
        if (!(func[i] > 0)) return false;
    return true;
}
inline bool all_zero(const double* func, int count, double func_int) {
    if (!(func_int == 0)) return false;
    for (int i = 0; i < count; i++)
        if (!(func[i] == 0)) return false;
    return true;
}
inline int check_distribution(int n_lights, const double* func, int count, double func_int, const char** why) {
    *why = "";
    if (n_lights <= 0 || all_zero(func, count, func_int)) return PBRT_OK;
    if (count != n_lights || !all_positive(func, count, func_int)) {
        *why = "a light distribution that mixes lights of pdf 0 with others";
        return PBRT_E_UNSUPPORTED;
    }
    return PBRT_OK;
}

// The k_li instantiation and its launch: kX for Mirror / Glass / OrenNayar
// scenes; kDepth 0 walks a tree staged in LDS (at most lds_nodes nodes) without
// a stack, 64 is the reference's stack beyond. A mesh changes neither: the
// mesh walk needs no stack and runs after the analytic one in either kernel.
struct KernelArgs {
    bool kx;
    int depth;
    uint32_t grid;   // workgroups of one wave, kLiRays rays each
};
inline KernelArgs kernel_args(bool non_matte, int n_nodes, bool mesh, size_t n, int lds_nodes) {
    (void)mesh;
    KernelArgs a;
    a.kx = non_matte;
    a.depth = n_nodes > lds_nodes ? 64 : 0;
    a.grid = (uint32_t)((n + kLiRays - 1) / kLiRays);
    return a;
}

}  // namespace pbrtli

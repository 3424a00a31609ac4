// k_li.hip — batched Integrator.Li over ray and RNG arrays resident on the
// device (pbrt_gpu_li_device): k_li
#pragma clang fp contract(off)

#include "render_common.h"
#include "li_query.h"

namespace pbrtk {

// paths_cam's lane refill (k_paths_c.hip) with the camera taken out: a wave owns
// the kLiRays rays from blockIdx.x * kLiRays on; an idle lane takes the next of
// them by its rank in the idle ballot (so a refill's loads are contiguous),
// starts Path.Li at bounce 0 from the caller's ray and PCG32 stream, and runs
// path_step<2, kX> (with kZeroPdf: a picked light may have pdf 0, the reference's
// Power strategy) until the path ends. sampler.RandomSampler: no dimension is
// stratified (SpecSampler n_dims 0, Cursor k = -1), every value is a draw.
// A path's values depend on its ray and stream only, never on its lane.
// kDepth 0: an LDS-staged tree, walked without a stack; 64: the reference's
// stack, one uint16 column per lane, for trees beyond kLdsNodes (the host
// chooses by the node count, pbrtli::kernel_args).
// A panicking ray is written as L = 0 (its optional outputs as they stand) and
// recorded as k_query_hit records its own. Li leaves a NaN radiance alone.
template <bool kX, int kDepth>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(kPathsWaves, 8))) void k_li(
    DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng,
    pbrt_radiance_soa out, QueryRec* __restrict__ rec) {
    __shared__ uint16_t stack_lds[kDepth > 0 ? kDepth * kStackStride : 1];
    __shared__ Spec lslots[3 * kWave];   // per lane: the radiance sum, then PathStateLds::aux
    __shared__ uint32_t rslots[kWave];
    // (kDepth > 0: launched on trees beyond kLdsNodes only, which stage_nodes leaves alone)
    if (kDepth > 0) sc.use_lds_nodes = 0;
    else stage_nodes(sc);
    const int lane = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * pbrtli::kLiRays;
    const int T = (int)(n - i0 < (int64_t)pbrtli::kLiRays ? n - i0 : (int64_t)pbrtli::kLiRays);   // > 0 by the grid
    const unsigned long long lt_mask = (1ULL << lane) - 1ULL;
    NoCache none;   // (never read: no code is generated for it)
    int base = 0;
    int w = -1;
    PathStateLds ps;
    ps.L = lslots + lane;
    ps.aux = lslots + kWave + 2 * lane;
    ps.rays = rslots + lane;
    Cursor c;
    c.rri = -1;
    c.rrn = 0;
    int pnc = 0, bnc = 1;
    const SpecSampler ss{nullptr, 1, 0, nullptr};
    for (;;) {
        const bool idle = w < 0;
        const unsigned long long m = __ballot(idle);
        if (idle) {
            const int t = base + __popcll(m & lt_mask);
            if (t < T) {
                const int64_t i = i0 + t;
                w = t;
                c.rng.state = rng.state[i];
                c.rng.inc = rng.inc[i];
                c.draws = 0;
                c.cur1d = 0;
                c.cur2d = 0;
                c.k = -1;
                c.kdep = 0;
                ps.ray = Ray{V3{rays.ox[i], rays.oy[i], rays.oz[i]}, V3{rays.dx[i], rays.dy[i], rays.dz[i]},
                             rays.tmax ? rays.tmax[i] : kInf, 0.0};
                *ps.L = spec(0);
                *ps.rays = 0;
                ps.beta = spec(1);
                ps.eta_scale = 1.0;
                ps.bounces = 0;
                ps.first = 0;
                pnc = 0;
                bnc = 1;
            }
        }
        base += __popcll(m);
        if (!__any(w >= 0)) {
            if (base >= T) break;
            continue;
        }
        if (w >= 0) {
            if (path_step<2, kX, true>(sc, none, ss, c, ps, max_depth, rr_threshold, kDepth > 0 ? stack_lds + lane : nullptr,
                                 pnc, bnc)) {
                const int64_t i = i0 + w;
                Spec Lp = *ps.L;
                if (pnc) Lp = spec(0);
                out.r[i] = Lp.r;
                out.g[i] = Lp.g;
                out.b[i] = Lp.b;
                if (out.state) out.state[i] = c.rng.state;
                if (out.draws) out.draws[i] = c.draws;
                if (out.rays) out.rays[i] = *ps.rays;
                if (pnc) query_panic(rec, i, pnc);
                w = -1;
            }
        }
    }
}

template __global__ void k_li<false, 0>(DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_radiance_soa out, QueryRec* __restrict__ rec);
template __global__ void k_li<true, 0>(DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_radiance_soa out, QueryRec* __restrict__ rec);
template __global__ void k_li<false, 64>(DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_radiance_soa out, QueryRec* __restrict__ rec);
template __global__ void k_li<true, 64>(DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_radiance_soa out, QueryRec* __restrict__ rec);

}  // namespace pbrtk

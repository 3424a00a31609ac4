// k_strat.hip — the public pieces under sampler.Stratified
// (pbrt_gpu_frame_samples_stratified_device, pbrt_gpu_li_stratified_device):
// k_strat_pixels, k_li_strat. The checks, the StartPixel form and the LDS
// carve: strat_query.h.
#pragma clang fp contract(off)

#include "render_common.h"
#include "cam_sample.h"
#include "film_query.h"
#include "li_query.h"

namespace pbrtk {

// The tables and traced samples of a THROUGHPUT render with n_dims >= 1, one
// wave per pixel of the range: what k_mb_setup and paths_group do for the
// library's own frame before a ray is traced. StartPixel on mb_state(tile, pi,
// 0) in whichever form rp selects (buffered, serial, windowed:
// start_pixel_wave) on layout_L's carve, the table copied out coalesced, then
// the lanes write the pixel's ns = spp - 1 samples: mb_state(tile, pi, k), the
// camera sample's draws (cam_sample.h: none for n_dims >= 2, pLens for n_dims =
// 1), the ray, pFilm = the pixel, k and the pixel's index in the range.
__global__ __launch_bounds__(kWave) void k_strat_pixels(const pbrt_camera_desc* __restrict__ cam, RenderParams rp,
                                                        ChainLayout lay, const PcgJump* __restrict__ jump,
                                                        pbrtfilm::Layout fl, int64_t px_begin, int64_t npx,
                                                        pbrt_frame_samples_soa out, pbrt_strat_samples_soa so) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ uint64_t sh_state;
    const int lane = threadIdx.x;
    const int64_t e = blockIdx.x;
    if (e >= npx) return;   // (the whole workgroup)
    const pbrtfilm::Where w = pbrtfilm::locate(fl, px_begin + e);
    const uint64_t inc = pcg_inc_of((uint64_t)w.tile);
    const int n = rp.spp, nd = rp.ndims, ns = n - 1;
    double* s1d = (double*)(lds + lay.s1d);
    (void)start_pixel_wave(rp, *jump, mb_state((uint64_t)w.tile, (uint64_t)w.pi, 0), inc, s1d,
                           (uint16_t*)(lds + lay.other), (uint32_t*)(lds + lay.vbuf), &sh_state);
    double* table = so.s1d + e * ((int64_t)nd * n);
    for (int idx = lane; idx < nd * n; idx += kWave) table[idx] = s1d[idx];
    const double fx = (double)w.px + 0.0, fy = (double)w.py + 0.0;
    for (int j = lane; j < ns; j += kWave) {
        const int k = j + 1;
        const int64_t i = e * ns + j;
        uint64_t st = mb_state((uint64_t)w.tile, (uint64_t)w.pi, (uint64_t)k);
        const pbrtcam::CamSample cs = pbrtcam::cam_sample(st, inc, nd);
        const Ray r = camera_ray(*cam, fx, fy, s1d[k], V2{cs.lens_x, cs.lens_y});
        out.ox[i] = r.o.x; out.oy[i] = r.o.y; out.oz[i] = r.o.z;
        out.dx[i] = r.d.x; out.dy[i] = r.d.y; out.dz[i] = r.d.z;
        if (out.tmax) out.tmax[i] = r.tmax;
        out.pfilm_x[i] = fx;
        out.pfilm_y[i] = fy;
        out.state[i] = st;
        out.inc[i] = inc;
        if (out.px) out.px[i] = (int32_t)w.px;
        if (out.py) out.py[i] = (int32_t)w.py;
        so.k[i] = k;
        so.table[i] = (int32_t)e;
    }
}

// k_li (k_li.hip) under the stratified sampler: the same lane refill over
// kLiRays-ray work lists and the same path_step<2, kX, true>, with the Cursor
// started at the caller's cursors and sample index and the SpecSampler built per
// lane from the ray's table pointer. A table value is read from global memory
// where it is used, as k_paths_ci reads its pixels' by default. table[i] and
// k[i] are clamped into [0, n_tables) and [0, spp) before they index anything
// (n_dims 0: neither array is read, the table pointer is never followed).
template <bool kX, int kDepth>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(kPathsWaves, 8))) void k_li_strat(
    DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng,
    pbrt_radiance_soa out, pbrt_strat_soa st, QueryRec* __restrict__ rec) {
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
    const int64_t per = (int64_t)st.n_dims * st.spp;
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
    c.k = 0;
    int pnc = 0, bnc = 1;
    SpecSampler ss{nullptr, st.spp, st.n_dims, nullptr};
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
                c.cur1d = st.first_1d;
                c.cur2d = st.first_2d;
                c.kdep = 0;
                if (st.n_dims > 0) {
                    const int tb = min(max(st.table[i], 0), st.n_tables - 1);
                    c.k = min(max(st.k[i], 0), st.spp - 1);
                    ss.s1d = st.s1d + (int64_t)tb * per;
                }
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

template __global__ void k_li_strat<false, 0>(DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_radiance_soa out, pbrt_strat_soa st, QueryRec* __restrict__ rec);
template __global__ void k_li_strat<true, 0>(DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_radiance_soa out, pbrt_strat_soa st, QueryRec* __restrict__ rec);
template __global__ void k_li_strat<false, 64>(DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_radiance_soa out, pbrt_strat_soa st, QueryRec* __restrict__ rec);
template __global__ void k_li_strat<true, 64>(DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_radiance_soa out, pbrt_strat_soa st, QueryRec* __restrict__ rec);

}  // namespace pbrtk

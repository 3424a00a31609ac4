// k_paths_c.hip — the path and film stages of the camera-start wave route
// (PBRT_KERNEL_WAVE_CAM; the chain: k_chain_c.hip): k_paths_cam, k_cam_setup
// and k_film_cam
#pragma clang fp contract(off)

#include "render_common.h"
#include "cam_sample.h"

namespace pbrtk {

// THROUGHPUT mode has no chain: sample k of pixel pi starts at mb_state(tile,
// pi, k). One wave per pixel record: the records k_chain_cam writes in EXACT
// mode (nvalid, the tile's pixel count) and, with n_dims = 1, StartPixel on
// the pixel's own stream mb_state(tile, pi, 0) for the stratified time values.
__global__ __launch_bounds__(kWave) void k_cam_setup(DevScene sc, RenderParams rp, ChainLayout lay,
                                                     const PcgJump* __restrict__ jump, WaveBufs wb, int64_t slot_base,
                                                     int64_t nslots_batch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ uint64_t sh_state;
    const int lane = threadIdx.x;
    if (cancel_requested(sc, (blockIdx.x & 63) == 0)) return;
    // n_dims = 0 has no StartPixel: one lane per record
    const int64_t rec = rp.ndims > 0 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * kWave + lane;
    const int64_t bslot = rec / wb.ppt, pi = rec % wb.ppt;
    if (bslot >= nslots_batch) return;
    const int64_t tile = tile_of_slot(rp, slot_base + bslot);
    int64_t x0, y0, x1, y1;
    tile_bounds(rp, tile, x0, y0, x1, y1);
    const int64_t npx = (x1 - x0) * (y1 - y0);
    if (pi == 0 && (lane == 0 || rp.ndims == 0)) wb.tile_npx[bslot] = rp.spp > 1 ? (int32_t)npx : 0;
    if (pi >= npx || rp.spp < 2) return;
    if (rp.ndims > 0) {   // (the whole workgroup: one record)
        double* gs1d = wb.s1d + rec * wb.s1d_stride;
        double* s1d = lay.s1d >= 0 ? (double*)(lds + lay.s1d) : gs1d;
        (void)start_pixel_wave<false>(rp, *jump, mb_state((uint64_t)tile, (uint64_t)pi, 0), pcg_inc_of((uint64_t)tile),
                                      s1d, (uint16_t*)(lds + lay.other), (uint32_t*)(lds + lay.vbuf), &sh_state);
        if (lay.s1d >= 0)
            for (int idx = lane; idx < rp.ndims * rp.spp; idx += kWave) gs1d[idx] = s1d[idx];
    }
    if (lane == 0 || rp.ndims == 0) {
        PixelRec& pr = wb.prec[rec];
        pr.hit = 1;
        pr.panic0 = 0;
        pr.nvalid = rp.spp;
    }
}

// k_paths_cam_stack is k_paths_cam for trees beyond kLdsNodes: the same body
// with the [64] traversal stack, one uint16 column per lane in LDS (8 KB more
// than k_paths_cam, whose 2 waves/SIMD on a small tree would not survive them).
//
// k_paths_ci's lane refill (render_common.h paths_group) with every path
// started at the camera: a wave owns P pixel records and their (pixel, sample)
// work list; a path starts from its sample's RNG state (the chain's wb.memb,
// or kMB: mb_state) with its own camera sample (cam_sample.h) and camera ray,
// and runs Path.Li's iterations (path_step<2>) from the first bounce. There is
// no pixel record to share: no bounce-1 NEE phase, no PixelCache. L and the ray
// counts are written pixel-major, the pixel's first panic to wb.ppanic.
struct CamMeta {
    uint64_t inc, tile;
    int32_t nv, cum, px, py;
};

template <int P, bool kMB, int kDepth>
__device__ __forceinline__ void paths_cam(DevScene sc, const RenderParams& rp, const WaveBufs& wb, int64_t slot_base,
                                          int64_t nrec, Counters* __restrict__ ctr) {
    // kDepth 0: an LDS-staged tree, walked without a stack (no stack array)
    __shared__ uint16_t stack_lds[kDepth > 0 ? kDepth * kStackStride : 1];
    __shared__ CamMeta meta[P + 1];
    __shared__ unsigned long long pkey[P];
    __shared__ Spec lslots[3 * kWave];   // per lane: the radiance sum, then PathStateLds::aux
    __shared__ uint32_t rslots[kWave];
    if (cancel_requested(sc, (blockIdx.x & 63) == 0)) return;   // one wave per workgroup
    // (kDepth > 0: launched on trees beyond kLdsNodes only, which stage_nodes leaves alone; said
    // at compile time, the staged walk and its LDS arrays drop out of the kernel)
    if (kDepth > 0) sc.use_lds_nodes = 0;
    else stage_nodes(sc);
    const int lane = threadIdx.x;
    const int n = rp.spp, ndims = rp.ndims;
    const int64_t rec0 = (int64_t)blockIdx.x * P;
    for (int j = lane; j < P; j += kWave) {
        const int64_t rec = rec0 + j;
        CamMeta m{0, 0, 0, 0, 0, 0};
        if (rec < nrec) {
            const int64_t bslot = rec / wb.ppt, pi = rec % wb.ppt;
            if (pi < wb.tile_npx[bslot]) {
                m.nv = wb.prec[rec].nvalid;
                m.tile = (uint64_t)tile_of_slot(rp, slot_base + bslot);
                m.inc = pcg_inc_of(m.tile);
                int64_t x0, y0, x1, y1;
                tile_bounds(rp, (int64_t)m.tile, x0, y0, x1, y1);
                m.px = (int32_t)(x0 + pi % (x1 - x0));
                m.py = (int32_t)(y0 + pi / (x1 - x0));
            }
        }
        meta[j] = m;
        pkey[j] = ~0ULL;
    }
    wave_sync();
    if (lane == 0) {
        int cum = 0;
        for (int j = 0; j < P; j++) {
            meta[j].cum = cum;
            cum += meta[j].nv > 1 ? meta[j].nv - 1 : 0;
        }
        meta[P].cum = cum;
    }
    wave_sync();
    const unsigned long long lt_mask = (1ULL << lane) - 1ULL;
    const int T = meta[P].cum;
    const pbrt_camera_desc& cam = *sc.camera;
    NoCache none;   // (never read: no code is generated for it)
    int base = 0;
    int w = -1, j = 0, k = 0;
    PathStateLds ps;
    ps.L = lslots + lane;
    ps.aux = lslots + kWave + 2 * lane;
    ps.rays = rslots + lane;
    Cursor c;
    c.rri = -1;
    c.rrn = 0;
    int pnc = 0, bnc = 1;
    const SpecSampler ss{nullptr, n, ndims, nullptr};   // no request after the camera sample is stratified (n_dims <= 1)
    for (;;) {
        const bool idle = w < 0;
        const unsigned long long m = __ballot(idle);
        if (idle) {
            const int t = base + __popcll(m & lt_mask);
            if (t < T) {
                // the work item's pixel: the last j with cum <= t
                int lo = 0, hi = P - 1;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (t >= meta[mid].cum) lo = mid;
                    else hi = mid - 1;
                }
                j = lo;
                k = 1 + (t - meta[j].cum);
                const int64_t rec = rec0 + j;
                w = t;
                uint64_t st = kMB ? mb_state(meta[j].tile, (uint64_t)(rec % wb.ppt), (uint64_t)k) : wb.memb[rec * n + k];
                const pbrtcam::CamSample cs = pbrtcam::cam_sample(st, meta[j].inc, ndims);
                c.rng.state = st;
                c.rng.inc = meta[j].inc;
                c.draws = cs.draws;
                c.cur1d = ndims < 1 ? ndims : 1;
                c.cur2d = ndims < 2 ? ndims : 2;
                c.k = k;
                c.kdep = 0;
                const double time_u = cs.time_drawn ? cs.time_u : wb.s1d[rec * wb.s1d_stride + k];
                ps.ray = camera_ray(cam, (double)meta[j].px + cs.film_x, (double)meta[j].py + cs.film_y, time_u,
                                    V2{cs.lens_x, cs.lens_y});
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
            if (path_step<2, false>(sc, none, ss, c, ps, rp.max_depth, rp.rr_threshold,
                                    kDepth > 0 ? stack_lds + lane : nullptr, pnc, bnc)) {
                const int64_t rec = rec0 + j;
                double* o = wb.L + sample_index(wb, rec, n, k) * 3;
                const Spec Lp = *ps.L;
                o[0] = Lp.r;
                o[1] = Lp.g;
                o[2] = Lp.b;
                wb.rays[sample_index(wb, rec, n, k)] = *ps.rays;
                if (pnc)
                    atomicMin(&pkey[j], ((unsigned long long)k << 32) | ((unsigned long long)(bnc & 0xFFFFFF) << 8) |
                                            (unsigned long long)((pnc + 1) & 0xFF));
                w = -1;
            }
        }
    }
    wave_sync();
    for (int q = lane; q < P; q += kWave) {
        if (meta[q].nv <= 0) continue;
        PanicRec p{0, 0, 0, 0, meta[q].px, meta[q].py};
        if (pkey[q] != ~0ULL) {
            p.kind = (int)(pkey[q] & 0xFF) - 1;
            p.bounce = (int)((pkey[q] >> 8) & 0xFFFFFF);
            p.sample = (int)(pkey[q] >> 32);
        }
        wb.ppanic[rec0 + q] = p;
        if (!p.kind && meta[q].nv > 1) {
            atomicAdd(&ctr->paths, (unsigned long long)(meta[q].nv - 1));
            atomicAdd(&ctr->camera_samples, (unsigned long long)(meta[q].nv - 1));
        }
    }
}

template <int P, bool kMB>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(kPathsWaves, 8))) void k_paths_cam(
    DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr) {
    paths_cam<P, kMB, 0>(sc, rp, wb, slot_base, nrec, ctr);
}

template <int P, bool kMB>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(kPathsWaves, 8))) void k_paths_cam_stack(
    DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr) {
    paths_cam<P, kMB, 64>(sc, rp, wb, slot_base, nrec, ctr);
}

// The tile film with one filter footprint per sample (n_dims = 0: pFilm is a
// draw). One workgroup per tile slot, one film pixel per work item. The serial
// replay (k_serial.hip, FilmTile.AddSample, film.go:211-248) adds a sample to
// every film pixel of its footprint, source pixels in tile order and samples in
// order; a film pixel's value is therefore the sum, in that order, of the
// samples whose footprint holds it, and each film pixel gathers exactly those:
// the source pixels that can reach it, row-major, each sample's pFilm recomputed
// from its stored RNG state (two draws; kMB: mb_state) and tested with film.go's
// own arithmetic. The workgroup also adds up its pixels' reference ray counts.
template <bool kMB>
__global__ __launch_bounds__(kFilmThreads) void k_film_cam(const pbrt_film_desc* __restrict__ film_desc, RenderParams rp,
                                                           WaveBufs wb, int64_t slot_base, int64_t nslots_batch,
                                                           double* __restrict__ films,
                                                           const int* __restrict__ cancel_seen,
                                                           Counters* __restrict__ ctr) {
    if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(cancel_seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))
        return;
    const int64_t bslot = blockIdx.x;
    if (bslot >= nslots_batch) return;
    const int tid = threadIdx.x;
    const pbrt_film_desc& film = *film_desc;
    const int64_t slot = slot_base + bslot;
    const uint64_t tile = (uint64_t)tile_of_slot(rp, slot);
    const uint64_t inc = pcg_inc_of(tile);
    int64_t x0, y0, x1, y1, px0, py0, px1, py1;
    tile_bounds(rp, (int64_t)tile, x0, y0, x1, y1);
    film_tile_bounds(film, x0, y0, x1, y1, px0, py0, px1, py1);
    const int tw = (int)(px1 - px0), nfp = (int)(tw * (py1 - py0));
    const int sw = (int)(x1 - x0), shh = (int)(y1 - y0);
    const int n = rp.spp;
    const int npx = wb.tile_npx[bslot];
    const int64_t rec0 = bslot * wb.ppt;
    const double rx = film.filter_radius_x, ry = film.filter_radius_y;
    const double ifx = 1.0 / rx, ify = 1.0 / ry;   // film.go:231-232
    // pFilm - 0.5 lies in [s - 0.5, s + 0.5): the source pixels s whose footprint
    // [ceil(pFilm - 0.5 - r), floor(pFilm - 0.5 + r)] can hold f, widened by one
    const int reach_x = (int)gomath::ceil(rx) + 1, reach_y = (int)gomath::ceil(ry) + 1;
    double* tf = films + slot * rp.slot_w * rp.slot_h * 3;
    for (int fi = tid; fi < nfp; fi += kFilmThreads) {
        const int fr = fi / tw, fc = fi - fr * tw;
        const int64_t fx = px0 + fc, fy = py0 + fr;
        const int sy_lo = max(0, (int)(fy - y0) - reach_y), sy_hi = min(shh - 1, (int)(fy - y0) + reach_y);
        const int sx_lo = max(0, (int)(fx - x0) - reach_x), sx_hi = min(sw - 1, (int)(fx - x0) + reach_x);
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int sy = sy_lo; sy <= sy_hi; sy++) {
            for (int sx = sx_lo; sx <= sx_hi; sx++) {
                const int pi = sy * sw + sx;
                if (pi >= npx) continue;
                const int64_t rec = rec0 + pi;
                const int nv = wb.prec[rec].nvalid;
                for (int k = 1; k < nv; k++) {
                    uint64_t st = kMB ? mb_state(tile, (uint64_t)pi, (uint64_t)k) : wb.memb[rec * n + k];
                    const pbrtcam::CamSample cs = pbrtcam::cam_sample(st, inc, 0);
                    const double dx = ((double)(x0 + sx) + cs.film_x) - 0.5, dy = ((double)(y0 + sy) + cs.film_y) - 0.5;
                    const int64_t p0x = gomath::to_int(gomath::max(gomath::ceil(dx - rx), (double)px0));
                    const int64_t p0y = gomath::to_int(gomath::max(gomath::ceil(dy - ry), (double)py0));
                    const int64_t p1x = gomath::to_int(gomath::min(gomath::floor(dx + rx) + 1, (double)px1));
                    const int64_t p1y = gomath::to_int(gomath::min(gomath::floor(dy + ry) + 1, (double)py1));
                    if (fx < p0x || fx >= p1x || fy < p0y || fy >= p1y) continue;
                    const int iy = (int)gomath::to_int(
                        gomath::min(gomath::floor(gomath::abs(((double)fy - dy) * ify * 16.0)), 16.0 - 1));
                    const int ix = (int)gomath::to_int(
                        gomath::min(gomath::floor(gomath::abs(((double)fx - dx) * ifx * 16.0)), 16.0 - 1));
                    const double* l = wb.L + sample_index(wb, rec, n, k) * 3;
                    Spec Ls{l[0], l[1], l[2]};
                    if (has_nans(Ls)) Ls = spec(0.1);   // integrator.go:256-262
                    if (0.0 > film.max_sample_luminance) Ls = smuls(Ls, film.max_sample_luminance / 0.0);
                    const Spec add = smuls(Ls, 1.0 * film.filter_table[iy * 16 + ix]);
                    a0 += add.r;
                    a1 += add.g;
                    a2 += add.b;
                }
            }
        }
        tf[fi * 3 + 0] = a0;
        tf[fi * 3 + 1] = a1;
        tf[fi * 3 + 2] = a2;
    }
    unsigned long long cl = 0, sh = 0;
    for (int i = tid; i < npx * (n - 1); i += kFilmThreads) {
        const int pi = i / (n - 1), k = 1 + (i - pi * (n - 1));
        if (k >= wb.prec[rec0 + pi].nvalid) continue;
        const uint32_t v = wb.rays[(rec0 + pi) * n + k];
        cl += v & 0xFFFFu;
        sh += v >> 16;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        cl += __shfl_down(cl, off);
        sh += __shfl_down(sh, off);
    }
    if ((tid & (kWave - 1)) == 0 && (cl | sh)) {
        atomicAdd(&ctr->closest_rays, cl);
        atomicAdd(&ctr->shadow_rays, sh);
    }
}

template __global__ void k_paths_cam<4, false>(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr);
template __global__ void k_paths_cam<16, false>(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr);
template __global__ void k_paths_cam<64, false>(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr);
template __global__ void k_paths_cam<4, true>(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr);
template __global__ void k_paths_cam<16, true>(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr);
template __global__ void k_paths_cam<64, true>(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr);
template __global__ void k_paths_cam_stack<4, false>(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr);
template __global__ void k_paths_cam_stack<16, false>(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr);
template __global__ void k_paths_cam_stack<64, false>(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr);
template __global__ void k_paths_cam_stack<4, true>(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr);
template __global__ void k_paths_cam_stack<16, true>(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr);
template __global__ void k_paths_cam_stack<64, true>(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr);
template __global__ void k_film_cam<false>(const pbrt_film_desc* __restrict__ film_desc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nslots_batch, double* __restrict__ films, const int* __restrict__ cancel_seen, Counters* __restrict__ ctr);
template __global__ void k_film_cam<true>(const pbrt_film_desc* __restrict__ film_desc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nslots_batch, double* __restrict__ films, const int* __restrict__ cancel_seen, Counters* __restrict__ ctr);

}  // namespace pbrtk

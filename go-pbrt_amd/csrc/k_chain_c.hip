// k_chain_c.hip — k_chain_cam, the offset chain of renders whose camera ray
// belongs to the sample (PBRT_KERNEL_WAVE_CAM, EXACT mode)
//
// With n_dims = 0 (Stratified without sampled dimensions, sampler.RandomSampler)
// or n_dims = 1 and a thin lens, every sample draws its own camera ray from the
// tile's PCG32 stream (cam_sample.h), so there is no bounce-1 record per pixel
// for k_chain_ci's trajectories to start from. Here a trajectory starts at the
// camera: a whole path, camera ray included, is a function of its offset in the
// tile's stream and of its pixel's raster coordinates only. After the camera
// sample no request can land on a stratified dimension (n_dims <= 1: the only
// one is the camera's time), so D(offset) never depends on the sample index:
// no kBadSpecD re-issue and no RrBranches, and a trajectory that panics is
// exact wherever it was speculated.
//
// The loop is k_chain_ci's continuous issue (k_chain.h) for one wave per tile
// over an LDS-staged tree: ring of resolved offsets, the leader's walk, the drop
// of candidates the chain left behind, the tail cap, wb.memb sample states, the
// wall_clock64 tile time, the launch order and the cancel polls. A lane that
// takes an offset draws its camera sample and joins the next traversal; every
// lane with a pending hit runs the one scatter. Stride 1 (D is often odd: five
// camera draws); no next-pixel speculation, no several tiles per wave, no
// multi-wave tiles.
//
// Trees beyond kLdsNodes are not staged: k_chain_cam_stack is the same loop
// with the reference's [64] traversal stack, one uint16 column per lane in LDS
// (8 KB), and without the staged walk's code and LDS arrays.
//
// Out of scope (the host refuses them for this route): DirectLighting, per-pixel
// camera rays (n_dims >= 2, or n_dims = 1 with a pinhole), Mirror / Glass /
// OrenNayar materials and triangle meshes.
#pragma clang fp contract(off)

#include "render_common.h"
#include "cam_sample.h"
#include "k_chain.h"   // uni(): wave-uniform values to scalar registers

namespace pbrtk {

#ifndef PBRT_CAM_EU_WAVES
#define PBRT_CAM_EU_WAVES 3   // k_chain_cam waves/SIMD (build option)
#endif
#ifndef PBRT_CAM_STACK_EU_WAVES
// k_chain_cam_stack waves/SIMD (build option). Without the staged walk and its LDS
// arrays the kernel has 8.1 KB of static LDS (the stack is 8 KB of it) and fits 168
// VGPRs without scratch, so with the 4 KB ring 13 workgroups share a CU's 160 KB
// and the 3-wave build really runs 3 per SIMD. Measured on crowd(60) Matte, 1080p,
// RandomSampler(64), Path(10): 4.59-4.62 s a frame against 5.62-5.66 s for the 2-wave
// build (169 VGPRs: 2 per SIMD by registers); profiles/large_trees/
#define PBRT_CAM_STACK_EU_WAVES 3
#endif

struct CamGroup {
    uint64_t S;      // PCG32 state at absolute offset A
    int64_t pi;      // current pixel (row-major index in the tile)
    int64_t npx;     // pixels of the tile
    uint32_t A;      // absolute offset of S
    uint32_t head;   // offset of sample kh
    uint32_t nxt;    // next offset to issue
    uint64_t Sn;     // PCG32 state at nxt, moved with it (k_chain_ci's carried state, k_chain.h kCarry)
    int kh;          // next sample without an offset
    int phase;       // 0 needs a pixel, 1 resolving offsets, 2 tile finished
    int px, py;      // the current pixel's raster coordinates
};

// The chain of one tile on one wave; the kernels below own its static LDS (CAM_CHAIN_LDS)
// and differ in the traversal stack: kDepth entries per lane, one uint16 column per lane,
// kWave apart (0: an LDS-staged tree, walked without a stack; 64: the reference's, bvh.go:670).
// A macro in each kernel, not statics of the template: function statics of a template are laid
// out differently in LDS, and k_chain_cam keeps the static LDS size it had as a plain kernel.
#define CAM_CHAIN_LDS(kDepth)                                    \
    __shared__ uint16_t stack_lds[kDepth > 0 ? kDepth * kWave : 1]; \
    __shared__ CamGroup gs;                                      \
    __shared__ uint64_t sh_state;                                \
    __shared__ uint32_t sh_draws
template <int kDepth>
__device__ __forceinline__ void chain_cam(DevScene sc, const RenderParams& rp, const ChainLayout& lay,
                                          const PcgJump* __restrict__ jump, const WaveBufs& wb, int64_t slot_base,
                                          int64_t nslots_batch, const uint32_t* __restrict__ order,
                                          uint32_t* __restrict__ ticks, uint16_t* stack_lds, CamGroup& gs,
                                          uint64_t& sh_state, uint32_t& sh_draws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint64_t t_begin = wall_clock64();
    const int tid = threadIdx.x;
    // (kDepth > 0: the host launches the kernel on trees beyond kLdsNodes only, which
    // stage_nodes leaves alone; said at compile time, the staged walk and its LDS
    // arrays drop out of the kernel)
    if (kDepth > 0) sc.use_lds_nodes = 0;
    else stage_nodes(sc);
    const int64_t bs = order ? (int64_t)order[blockIdx.x] : (int64_t)blockIdx.x;
    if (bs >= nslots_batch) return;
    constexpr uint32_t R = kCiRingBytes / sizeof(RingEnt);   // a power of two
    const PcgJump& J = *jump;
    double* s1d = lay.s1d >= 0 ? (double*)(lds + lay.s1d) : nullptr;
    uint16_t* other = (uint16_t*)(lds + lay.other);
    uint32_t* vbuf = (uint32_t*)(lds + lay.vbuf);
    RingEnt* ring = (RingEnt*)(lds + lay.ring);   // aliases the StartPixel staging: never live together
    uint16_t* stack = stack_lds + tid;
    const int n = rp.spp, ndims = rp.ndims;
    // an upper bound of a path's draw count (k_chain_ci's tail cap): the camera
    // sample, then per bounce at most 8
    const uint32_t dmax = pbrtcam::cam_draws(ndims) + (uint32_t)(8 * (rp.max_depth + 1) + 8);
    const pbrt_camera_desc& cam = *sc.camera;
    const int64_t tile = tile_of_slot(rp, slot_base + bs);
    const uint64_t inc = pcg_inc_of((uint64_t)tile);
    int64_t x0, y0, x1, y1;
    tile_bounds(rp, tile, x0, y0, x1, y1);
    if (tid == 0) {
        Pcg seed;
        pcg_seed(seed, (uint64_t)tile);   // Sampler.Clone(tile), integrator.go:318,328
        gs.S = seed.state;
        gs.pi = 0;
        gs.npx = (x1 - x0) * (y1 - y0);
        gs.A = gs.head = gs.nxt = 0;
        gs.Sn = 0;
        gs.kh = 1;
        gs.phase = (gs.npx > 0 && n > 1) ? 0 : 2;   // sample 0 is never traced (#2): one sample, no path
        gs.px = gs.py = 0;
        wb.tile_npx[bs] = 0;
    }
    __syncthreads();

    uint32_t cancel_poll = 0;
    uint64_t last_host_poll = t_begin;
    // lane trajectory state
    uint32_t off = kNoOff;
    bool tracing = false;
    Cursor c;
    c.rri = -1;
    c.rrn = 0;
    c.rng.state = 0;
    c.rng.inc = inc;
    c.draws = 0;
    c.cur1d = c.cur2d = 0;
    c.k = -1;
    c.kdep = 0;
    Spec beta = spec(1);
    double eta_scale = 1.0;
    int bounces = 1;
    Ray ray;
    ray.o = ray.d = V3{0, 0, 0};
    ray.tmax = kInf;
    ray.time = 0;
    const SpecSampler ss{nullptr, n, ndims, nullptr};   // k < 0: no stratified value is ever read

    // the trajectory's end: its draw count (or kBadExactD: it panics) to its ring entry
    auto finish = [&](uint32_t d) {
        RingEnt& e = ring[off & (R - 1u)];
        e.d = d;
        e.tag = off;
        off = kNoOff;
        tracing = false;
    };

    for (;;) {
        // ---- (1) every live trajectory's ray, then the scatter of the lanes that hit
        if (tracing) {
            int panic = 0, best = -1;
            V3 ph{0, 0, 0};
            bvh_walk<false, kWave, PBRT_CHAIN_LB, false>(sc, ray, stack, panic, best, ph);
            if (panic || best < 0) {
                finish(panic ? kBadExactD : c.draws);
            } else {
                SI si;
                BSDF b;
                BSDFX x;
                const V3 wo = ray.d;
                prim_si(sc, best, ray, ph, si);
                const int r = compute_bsdf(sc, si, b) < 0
                                  ? 2
                                  : traj_scatter<false>(sc, si, b, x, wo, c, ss, beta, eta_scale, bounces, ray,
                                                        rp.max_depth, rp.rr_threshold);
                if (r != 0) finish(r == 1 ? c.draws : kBadExactD);
            }
        }
        // ---- (2) the leader walks the chain through the ring; candidates it left behind are dropped
        __syncthreads();
        if (tid == 0 && gs.phase == 1) {
            CamGroup s = gs;
            if ((++cancel_poll & 127u) == 0) {
                const uint64_t now = wall_clock64();
                const bool host = now - last_host_poll >= 100000;
                if (host) last_host_poll = now;
                if (cancel_requested(sc, host)) s.phase = 2;
            }
            const int64_t rec = bs * wb.ppt + s.pi;
            // the last walked entry's draw count: the state at head is that entry's, dl draws on
            uint32_t dl = 0;
            bool walked = false;
            for (; s.phase == 1;) {
                const RingEnt& e = ring[s.head & (R - 1u)];
                if (e.tag != s.head) break;
                const uint32_t d = e.d;
                wb.memb[rec * n + s.kh] = e.st;
                if (d == kBadExactD) {   // the trajectory panics: the tile ends at this sample
                    wb.prec[rec].nvalid = s.kh + 1;
                    s.phase = 2;
                    break;
                }
                s.kh++;
                s.head += d;
                dl = d;
                walked = true;
                if (s.kh >= n) {   // every sample of the pixel has its offset
                    s.S = pcg_advance_near(J, e.st, inc, (uint64_t)d);
                    s.A = s.head;
                    s.pi++;
                    s.phase = s.pi < s.npx ? 0 : 2;
                    break;
                }
            }
            if (s.nxt < s.head) {   // the chain overtook the issue
                s.nxt = s.head;
                if (s.phase == 1)
                    gs.Sn = walked ? pcg_advance_near(J, ring[(s.head - dl) & (R - 1u)].st, inc, (uint64_t)dl)
                                   : pcg_advance(J, s.S, inc, (uint64_t)(s.head - s.A));
            }
            gs.S = s.S;
            gs.A = s.A;
            gs.pi = s.pi;
            gs.head = s.head;
            gs.nxt = s.nxt;
            gs.kh = s.kh;
            gs.phase = s.phase;
        }
        __syncthreads();
        if (off != kNoOff) {
            // a pixel's end drops every candidate (its camera ray is the old pixel's)
            const uint32_t head = uni(gs.head);
            const bool keep = uni(gs.phase) == 1 && off >= head && off <= head + (uint32_t)(n - 1 - uni(gs.kh)) * dmax;
            if (!keep) {
                off = kNoOff;
                tracing = false;
            }
        }
        // ---- (3) the next pixel: StartPixel (n_dims = 1; none with n_dims = 0), an empty ring
        while (gs.phase == 0) {
            const int64_t pi = gs.pi;
            const int64_t rec = bs * wb.ppt + pi;
            uint64_t S1 = gs.S;
            uint32_t sp_draws = 0;
            if (ndims > 0) {
                double* gs1d = wb.s1d + rec * wb.s1d_stride;
                // (inlined: as a call it takes rp through scratch)
                [[clang::always_inline]] S1 = start_pixel_wave<false>(rp, J, gs.S, inc, s1d ? s1d : gs1d, other, vbuf, &sh_state, &sh_draws);
                sp_draws = sh_draws;
                if (s1d)
                    for (int idx = tid; idx < ndims * n; idx += kWave) gs1d[idx] = s1d[idx];
            }
            __syncthreads();
            for (uint32_t i = (uint32_t)tid; i < R; i += kWave) ring[i].tag = kNoOff;
            if (tid == 0) {
                const uint64_t now = wall_clock64();
                const bool host = now - last_host_poll >= 100000;   // 1 ms at 100 MHz
                if (host) last_host_poll = now;
                PixelRec& pr = wb.prec[rec];
                pr.hit = 1;
                pr.panic0 = 0;
                pr.nvalid = n;
                wb.tile_npx[bs] = (int32_t)(pi + 1);
                gs.S = S1;
                gs.A += sp_draws;
                gs.head = gs.nxt = gs.A;
                gs.Sn = S1;
                gs.kh = 1;
                gs.px = (int)(x0 + pi % (x1 - x0));
                gs.py = (int)(y0 + pi / (x1 - x0));
                gs.phase = cancel_requested(sc, host) ? 2 : 1;
            }
            __syncthreads();
        }
        if (gs.phase != 1) break;

        // ---- (4) idle lanes take the next offsets, draw their camera sample and join the next traversal
        {
            const uint32_t head = uni(gs.head), nx0 = uni(gs.nxt);
            const int kh = uni(gs.kh);
            const uint64_t Sn = uni(gs.Sn);
            const int px = uni(gs.px), py = uni(gs.py);
            const bool idle = off == kNoOff;
            const unsigned long long m = __ballot(idle);
            const int nidle = __popcll(m);
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            // offsets < head + R keep the ring collision-free; none beyond the tail cap is ever on the chain
            const int avail = nx0 < head + R ? (int)(head + R - nx0) : 0;
            const uint32_t tail = head + (uint32_t)(n - 1 - kh) * dmax;
            const int capn = nx0 <= tail ? (int)(tail - nx0) + 1 : 0;
            const int nspec = min(min(nidle, avail), capn);
            // the state at nxt moves with it (wave-uniform operands: scalar); a lane's
            // state is one table step from it (rank <= 63)
            const uint64_t nSn = nspec > 0 ? pcg_advance_near(J, Sn, inc, (uint64_t)nspec) : Sn;
            if (tid == 0) {
                gs.nxt = nx0 + (uint32_t)nspec;
                gs.Sn = nSn;
            }
            if (idle && rank < nspec) {
                off = nx0 + (uint32_t)rank;
                uint64_t st = pcg_step(J, Sn, inc, (uint32_t)rank);
                ring[off & (R - 1u)].st = st;
                const pbrtcam::CamSample cs = pbrtcam::cam_sample(st, inc, ndims);
                c.rng.state = st;
                c.draws = cs.draws;
                c.cur1d = ndims < 1 ? ndims : 1;   // the camera's time
                c.cur2d = ndims < 2 ? ndims : 2;   // pFilm, pLens
                c.kdep = 0;
                beta = spec(1);
                eta_scale = 1.0;
                bounces = 1;
                if (bounces >= rp.max_depth) {   // path.go:66: no bounce is traced
                    finish(c.draws);
                } else {
                    // (n_dims = 1: the time is the stratified s1d[0][k] of a sample index not
                    // known yet; a ray's time reaches no draw and no output)
                    ray = camera_ray(cam, (double)px + cs.film_x, (double)py + cs.film_y, cs.time_u,
                                     V2{cs.lens_x, cs.lens_y});
                    tracing = true;
                }
            }
        }
    }
    if (tid == 0 && ticks) {
        const uint64_t t_end = wall_clock64();
        ticks[bs] = (uint32_t)min(t_end - t_begin, (uint64_t)0xFFFFFFFFu);
    }
}

__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(PBRT_CAM_EU_WAVES, 8))) void k_chain_cam(
    DevScene sc, RenderParams rp, ChainLayout lay, const PcgJump* __restrict__ jump, WaveBufs wb, int64_t slot_base,
    int64_t nslots_batch, const uint32_t* __restrict__ order, uint32_t* __restrict__ ticks) {
    CAM_CHAIN_LDS(0);
    chain_cam<0>(sc, rp, lay, jump, wb, slot_base, nslots_batch, order, ticks, stack_lds, gs, sh_state, sh_draws);
}

__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(PBRT_CAM_STACK_EU_WAVES, 8))) void k_chain_cam_stack(
    DevScene sc, RenderParams rp, ChainLayout lay, const PcgJump* __restrict__ jump, WaveBufs wb, int64_t slot_base,
    int64_t nslots_batch, const uint32_t* __restrict__ order, uint32_t* __restrict__ ticks) {
    CAM_CHAIN_LDS(64);
    chain_cam<64>(sc, rp, lay, jump, wb, slot_base, nslots_batch, order, ticks, stack_lds, gs, sh_state, sh_draws);
}

}  // namespace pbrtk

// render_params.h — what the host decides about a frame and hands to its kernels: the
// render's parameters, the chain kernels' LDS layout, and the sizes both sides must
// agree on (k_film's LDS, the StartPixel draw area, k_chain_ci's ring, k_paths_ci's light
// cache). Host and device; no HIP include: frame_route.h and tests/frame_route_check.cpp
// compile it on their own.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PBRT_RP_HD __host__ __device__
#else
#define PBRT_RP_HD
#endif

namespace pbrt {

constexpr int kMaxCachedLights = 16;   // PixelCache::ld[] (pbrt_spec.h): k_paths_ci's bounce-1 light estimates

}  // namespace pbrt

namespace pbrtk {

constexpr int kWave = 64;

struct RenderParams {
    int64_t film_min_x, film_min_y, film_w, film_h;   // CroppedPixelBounds
    int64_t tile_size, ntx, nty;
    int64_t tile_begin, tile_stride, n_slots;
    int64_t slot_w, slot_h;                            // max tile-film extent
    int32_t spp, xs, ys, ndims, jitter;
    int32_t integrator, max_depth, dl_strategy;
    double rr_threshold;
    int32_t lanes_per_wave;
    int32_t flags;   // pbrt_render_desc.flags
    int32_t sp_events, sp_draws, sp_serial;   // wave kernel StartPixel: events, raw draws buffered
    int32_t mode;                             // PBRT_MODE_EXACT / _THROUGHPUT
    int32_t sp_window;                        // sp_serial without jitter: the windowed wave StartPixel
    int32_t ci_nps;                           // k_chain_ci multi-wave tiles: next-pixel speculation
    int32_t ci_scap;                          // k_chain_ci statistical speculation cap, tenths of a sigma (0: off)
    int32_t pad1;
};

constexpr int kFilmThreads = 256;           // k_film workgroup (one per tile slot)
constexpr int kFilmStageBytes = 24 * 1024;  // k_film: LDS staging of a run of source pixels' L
// k_film: source pixels per staged run (a row of a 16-px tile at 64 spp, one
// pixel at 1024), and its dynamic LDS: running sums [slot_w x slot_h][3],
// then the run [S][spp - 1][3]
PBRT_RP_HD inline int film_run_pixels(const RenderParams& rp) {
    const int64_t m = rp.spp - 1, npx = rp.tile_size * rp.tile_size;
    int64_t S = m > 0 ? kFilmStageBytes / (m * 24) : 1;
    if (S > npx) S = npx;
    if (S > kFilmThreads) S = kFilmThreads;
    return S < 1 ? 1 : (int)S;
}
PBRT_RP_HD inline int film_lds_bytes(const RenderParams& rp) {
    const int64_t nfp = rp.slot_w * rp.slot_h, m = rp.spp - 1;
    return (int)(((nfp * 3 + 1) & ~int64_t(1)) * 8 + (int64_t)film_run_pixels(rp) * (m > 0 ? m : 1) * 24);
}
struct ChainLayout {   // byte offsets into the chain / setup kernels' dynamic LDS block
    int s1d, other, sbuf, dbuf, vbuf, total;
    int ring;      // k_chain_ci: offset ring after the StartPixel staging (no sbuf / dbuf)
    int staging;   // k_chain_ci: bytes of the StartPixel staging (s1d, other, vbuf)
    int pcs;       // k_chain_ci: the lane groups' bounce-1 ChainCache records (ci_layout)
};
#ifndef PBRT_CI_RING_KB
#define PBRT_CI_RING_KB 4
#endif
constexpr int kCiRingBytes = PBRT_CI_RING_KB * 1024;   // k_chain_ci offset ring (all lane groups of a wave)
constexpr int kCiMaxGroups = 4;          // k_chain_ci lane groups (tiles) per wave
constexpr int kCiMaxRing = 4 * kCiRingBytes / 16;   // ring entries of a tile at the most waves of a kX tile (4)

constexpr int kSpRing = 256;   // windowed StartPixel: raw draws in flight (a power of two)
// Bytes of the StartPixel draw area (ChainLayout.vbuf): every raw draw (the wave
// StartPixel), or for the windowed one its uint16 permutations then the draw
// ring, or nothing (the serial StartPixel)
PBRT_RP_HD inline int64_t sp_vbuf_bytes(const RenderParams& rp) {
    if (rp.sp_window) return (((int64_t)rp.ndims * rp.spp * 2 + 15) & ~int64_t(15)) + kSpRing * 4;
    return rp.sp_serial ? 4 : (int64_t)rp.sp_draws * 4;
}

}  // namespace pbrtk

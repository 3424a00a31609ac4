// k_film_q.hip — a frame from public pieces (pbrt_gpu_frame_samples_device,
// pbrt_gpu_film_add_device, pbrt_gpu_film_rgba8_device): k_frame_samples,
// k_film_add_tiles, k_film_add_merge, k_film_rgba8. The frame layout and its
// arithmetic: film_query.h.
#pragma clang fp contract(off)

#include "render_common.h"
#include "cam_sample.h"
#include "film_query.h"

namespace pbrtk {

// The traced samples of a THROUGHPUT render with n_dims = 0, one per work item:
// element i is sample 1 + i % ns of the pixel at position px_begin + i / ns of
// the layout. What k_cam_setup / paths_cam do for the library's own frame:
// mb_state, the five camera draws of cam_sample.h, camera_ray.
__global__ __launch_bounds__(kQueryBlock) void k_frame_samples(const pbrt_camera_desc* __restrict__ cam,
                                                              pbrtfilm::Layout lay, int64_t px_begin, int ns, int64_t n,
                                                              pbrt_frame_samples_soa out) {
    const int64_t i = (int64_t)blockIdx.x * kQueryBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t e = i / ns, k = 1 + (i - e * ns);
    const pbrtfilm::Where w = pbrtfilm::locate(lay, px_begin + e);
    const uint64_t inc = pcg_inc_of((uint64_t)w.tile);
    uint64_t st = mb_state((uint64_t)w.tile, (uint64_t)w.pi, (uint64_t)k);
    const pbrtcam::CamSample cs = pbrtcam::cam_sample(st, inc, 0);
    const double fx = (double)w.px + cs.film_x, fy = (double)w.py + cs.film_y;
    const Ray r = camera_ray(*cam, fx, fy, cs.time_u, V2{cs.lens_x, cs.lens_y});
    out.ox[i] = r.o.x; out.oy[i] = r.o.y; out.oz[i] = r.o.z;
    out.dx[i] = r.d.x; out.dy[i] = r.d.y; out.dz[i] = r.d.z;
    if (out.tmax) out.tmax[i] = r.tmax;
    out.pfilm_x[i] = fx;
    out.pfilm_y[i] = fy;
    out.state[i] = st;
    out.inc[i] = inc;
    if (out.px) out.px[i] = (int32_t)w.px;
    if (out.py) out.py[i] = (int32_t)w.py;
}

// One sample's contribution as the Render loop and FilmTile.AddSample see it:
// integrator.go:256-262's NaN replacement, film.go:218-220's luminance test.
__device__ __forceinline__ Spec film_sample_L(const pbrt_film_desc& film, double r, double g, double b) {
    Spec Ls{r, g, b};
    if (has_nans(Ls)) Ls = spec(0.1);
    if (0.0 > film.max_sample_luminance) Ls = smuls(Ls, film.max_sample_luminance / 0.0);
    return Ls;
}

constexpr int kFqChunk = 512;   // samples of a source-pixel row staged at a time (kLds): 48 B each
constexpr int kFqPix = 2;       // film pixels of a work item (kLds): tile films of at most kFqPix * kFilmThreads pixels
static_assert(kFqPix * kFilmThreads == pbrtfilm::kLdsFilmPixels, "pbrtfilm::lds_gather chooses by this bound");

// The tile films of a tile range from samples in device arrays: k_film_cam with
// pFilm and L read from the caller's arrays. One workgroup per tile, one film
// pixel per work item; a film pixel gathers, source pixels in tile order and
// samples in order, the samples whose footprint holds it, tested with film.go's
// own arithmetic. Nothing is scattered: a caller's pFilm decides only whether a
// sample is added and which of the 256 filter weights it gets.
//
// !kLds: the direct gather. Every (film pixel, sample within reach) pair reads
// the sample's pFilm and recomputes its footprint.
// kLds: a sample's footprint (relative to the tile film, clamped to it: the
// same test on every input), pFilm - 0.5 and L are computed once, a run of one
// source-pixel row at a time into LDS (the run is contiguous in the arrays);
// the film pixels then test four 16-bit bounds per sample. The accumulators stay
// in registers, so the host launches it for tile films of at most kFqPix *
// kFilmThreads pixels.
template <bool kLds>
__global__ __launch_bounds__(kFilmThreads) void k_film_add_tiles(const pbrt_film_desc* __restrict__ film_desc,
                                                                 RenderParams rp, pbrtfilm::Layout lay,
                                                                 int64_t tile_begin, int ns, pbrt_film_samples_soa in,
                                                                 double* __restrict__ films) {
    const int tid = threadIdx.x;
    const pbrt_film_desc& film = *film_desc;
    const int64_t tile = tile_begin + blockIdx.x;
    int64_t x0, y0, x1, y1, px0, py0, px1, py1;
    tile_bounds(rp, tile, x0, y0, x1, y1);
    film_tile_bounds(film, x0, y0, x1, y1, px0, py0, px1, py1);
    const int tw = (int)(px1 - px0), th = (int)(py1 - py0), nfp = tw * th;
    const int sw = (int)(x1 - x0), shh = (int)(y1 - y0);
    // the tile's first element
    const int64_t e0 = (pbrtfilm::pixels_before(lay, tile) - pbrtfilm::pixels_before(lay, tile_begin)) * ns;
    const double rx = film.filter_radius_x, ry = film.filter_radius_y;
    const double ifx = 1.0 / rx, ify = 1.0 / ry;   // film.go:231-232
    // pFilm - 0.5 lies in [s - 0.5, s + 0.5): the source pixels s whose footprint
    // [ceil(pFilm - 0.5 - r), floor(pFilm - 0.5 + r)] can hold f, widened by one
    const int reach_x = (int)gomath::ceil(rx) + 1, reach_y = (int)gomath::ceil(ry) + 1;
    double* tf = films + (tile - tile_begin) * (rp.slot_w * rp.slot_h * 3);
    if constexpr (!kLds) {
        for (int fi = tid; fi < nfp; fi += kFilmThreads) {
            const int fr = fi / tw, fc = fi - fr * tw;
            const int64_t fx = px0 + fc, fy = py0 + fr;
            const int sy_lo = max(0, (int)(fy - y0) - reach_y), sy_hi = min(shh - 1, (int)(fy - y0) + reach_y);
            const int sx_lo = max(0, (int)(fx - x0) - reach_x), sx_hi = min(sw - 1, (int)(fx - x0) + reach_x);
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
            for (int sy = sy_lo; sy <= sy_hi; sy++) {
                for (int sx = sx_lo; sx <= sx_hi; sx++) {
                    const int64_t es = e0 + (int64_t)(sy * sw + sx) * ns;
                    for (int k = 0; k < ns; k++) {
                        const double dx = in.pfilm_x[es + k] - 0.5, dy = in.pfilm_y[es + k] - 0.5;
                        const int64_t p0x = gomath::to_int(gomath::max(gomath::ceil(dx - rx), (double)px0));
                        const int64_t p0y = gomath::to_int(gomath::max(gomath::ceil(dy - ry), (double)py0));
                        const int64_t p1x = gomath::to_int(gomath::min(gomath::floor(dx + rx) + 1, (double)px1));
                        const int64_t p1y = gomath::to_int(gomath::min(gomath::floor(dy + ry) + 1, (double)py1));
                        if (fx < p0x || fx >= p1x || fy < p0y || fy >= p1y) continue;
                        const int iy = (int)gomath::to_int(
                            gomath::min(gomath::floor(gomath::abs(((double)fy - dy) * ify * 16.0)), 16.0 - 1)) & 15;
                        const int ix = (int)gomath::to_int(
                            gomath::min(gomath::floor(gomath::abs(((double)fx - dx) * ifx * 16.0)), 16.0 - 1)) & 15;
                        const Spec Ls = film_sample_L(film, in.r[es + k], in.g[es + k], in.b[es + k]);
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
    } else {
        __shared__ uint64_t s_box[kFqChunk];   // lo x | hi x << 16 | lo y << 32 | hi y << 48, tile-film relative
        __shared__ double s_dx[kFqChunk], s_dy[kFqChunk], s_l[3][kFqChunk];
        __shared__ double s_table[16 * 16];
        for (int i = tid; i < 16 * 16; i += kFilmThreads) s_table[i] = film.filter_table[i];
        int fc[kFqPix], fr[kFqPix], sy_lo[kFqPix], sy_hi[kFqPix], q_lo[kFqPix], q_hi[kFqPix];
        double a[kFqPix][3];
#pragma unroll
        for (int j = 0; j < kFqPix; j++) {
            const int fi = tid + j * kFilmThreads;
            fr[j] = fi / tw;
            fc[j] = fi - fr[j] * tw;
            const int ry0 = (int)(py0 - y0) + fr[j], rx0 = (int)(px0 - x0) + fc[j];   // relative to the tile
            sy_lo[j] = max(0, ry0 - reach_y);
            sy_hi[j] = fi < nfp ? min(shh - 1, ry0 + reach_y) : -1;
            q_lo[j] = max(0, rx0 - reach_x) * ns;
            q_hi[j] = (min(sw - 1, rx0 + reach_x) + 1) * ns;
            a[j][0] = a[j][1] = a[j][2] = 0.0;
        }
        // relative to the tile film and clamped to it: fc in [lo, hi) is fx in [p0, p1) for every p0, p1
        auto rel = [](int64_t p, int64_t lo, int64_t hi) -> uint64_t {
            return (uint64_t)(p < lo ? 0 : (p > hi ? hi - lo : p - lo));
        };
        const int nrow = sw * ns;
        for (int sy = 0; sy < shh; sy++) {
            const int64_t er = e0 + (int64_t)sy * nrow;
            for (int c0 = 0; c0 < nrow; c0 += kFqChunk) {
                const int cnt = min(kFqChunk, nrow - c0);
                __syncthreads();   // the previous run has been read (and s_table written)
                for (int t = tid; t < cnt; t += kFilmThreads) {
                    const int64_t e = er + c0 + t;
                    const double dx = in.pfilm_x[e] - 0.5, dy = in.pfilm_y[e] - 0.5;
                    const int64_t p0x = gomath::to_int(gomath::max(gomath::ceil(dx - rx), (double)px0));
                    const int64_t p0y = gomath::to_int(gomath::max(gomath::ceil(dy - ry), (double)py0));
                    const int64_t p1x = gomath::to_int(gomath::min(gomath::floor(dx + rx) + 1, (double)px1));
                    const int64_t p1y = gomath::to_int(gomath::min(gomath::floor(dy + ry) + 1, (double)py1));
                    s_box[t] = rel(p0x, px0, px1) | rel(p1x, px0, px1) << 16 | rel(p0y, py0, py1) << 32 |
                               rel(p1y, py0, py1) << 48;
                    s_dx[t] = dx;
                    s_dy[t] = dy;
                    const Spec Ls = film_sample_L(film, in.r[e], in.g[e], in.b[e]);
                    s_l[0][t] = Ls.r;
                    s_l[1][t] = Ls.g;
                    s_l[2][t] = Ls.b;
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < kFqPix; j++) {
                    if (sy < sy_lo[j] || sy > sy_hi[j]) continue;
                    const int64_t fx = px0 + fc[j], fy = py0 + fr[j];
                    const int qe = min(q_hi[j], c0 + cnt) - c0;
                    for (int q = max(q_lo[j], c0) - c0; q < qe; q++) {
                        const uint64_t box = s_box[q];
                        const int lx = (int)(box & 0xFFFF), hx = (int)((box >> 16) & 0xFFFF);
                        const int ly = (int)((box >> 32) & 0xFFFF), hy = (int)(box >> 48);
                        if (fc[j] < lx || fc[j] >= hx || fr[j] < ly || fr[j] >= hy) continue;
                        const double dx = s_dx[q], dy = s_dy[q];
                        const int iy = (int)gomath::to_int(
                            gomath::min(gomath::floor(gomath::abs(((double)fy - dy) * ify * 16.0)), 16.0 - 1)) & 15;
                        const int ix = (int)gomath::to_int(
                            gomath::min(gomath::floor(gomath::abs(((double)fx - dx) * ifx * 16.0)), 16.0 - 1)) & 15;
                        const Spec add = smuls(Spec{s_l[0][q], s_l[1][q], s_l[2][q]}, 1.0 * s_table[iy * 16 + ix]);
                        a[j][0] += add.r;
                        a[j][1] += add.g;
                        a[j][2] += add.b;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kFqPix; j++) {
            const int fi = tid + j * kFilmThreads;
            if (fi >= nfp) continue;
            tf[fi * 3 + 0] = a[j][0];
            tf[fi * 3 + 1] = a[j][1];
            tf[fi * 3 + 2] = a[j][2];
        }
    }
}

// Film.MergeFilmTile (film.go:115-132) of the tile films of [tile_begin,
// tile_end) into the film, one film pixel per work item over the rows [row0,
// row0 + rows) of the crop: k_merge_film, continuing from the pixel's value
// (clear: from 0). A film pixel is covered by at most the 3x3 tiles around its
// own (filter radius < tile size), visited in ascending tile index.
__global__ __launch_bounds__(256) void k_film_add_merge(const pbrt_film_desc* __restrict__ film_desc, RenderParams rp,
                                                        int64_t tile_begin, int64_t tile_end, int64_t row0, int64_t rows,
                                                        int clear, const double* __restrict__ films,
                                                        double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= rp.film_w * rows) return;
    const int64_t i = row0 * rp.film_w + j;
    const pbrt_film_desc& f = *film_desc;
    const int64_t x = rp.film_min_x + i % rp.film_w, y = rp.film_min_y + i / rp.film_w;
    const int64_t tx = (x - rp.film_min_x) / rp.tile_size, ty = (y - rp.film_min_y) / rp.tile_size;
    double v0 = 0, v1 = 0, v2 = 0;
    if (!clear) {
        v0 = out[i * 3 + 0];
        v1 = out[i * 3 + 1];
        v2 = out[i * 3 + 2];
    }
    for (int64_t dy = -1; dy <= 1; dy++) {
        for (int64_t dx = -1; dx <= 1; dx++) {
            const int64_t cx = tx + dx, cy = ty + dy;
            if (cx < 0 || cy < 0 || cx >= rp.ntx || cy >= rp.nty) continue;
            const int64_t tile = cy * rp.ntx + cx;
            if (tile < tile_begin || tile >= tile_end) continue;
            int64_t x0, y0, x1, y1, px0, py0, px1, py1;
            tile_bounds(rp, tile, x0, y0, x1, y1);
            film_tile_bounds(f, x0, y0, x1, y1, px0, py0, px1, py1);
            if (x < px0 || x >= px1 || y < py0 || y >= py1) continue;
            const double* c =
                films + (tile - tile_begin) * (rp.slot_w * rp.slot_h * 3) + ((x - px0) + (y - py0) * (px1 - px0)) * 3;
            // spectrum.go:35-41 RGBToXYZ
            v0 += 0.412453 * c[0] + 0.357580 * c[1] + 0.180423 * c[2];
            v1 += 0.212671 * c[0] + 0.715160 * c[1] + 0.072169 * c[2];
            v2 += 0.019334 * c[0] + 0.119193 * c[1] + 0.950227 * c[2];
        }
    }
    out[i * 3 + 0] = v0;
    out[i * 3 + 1] = v1;
    out[i * 3 + 2] = v2;
}

// film.go:157-159: pbrt_film_to_rgba8's expression, one pixel per work item,
// its four bytes as one 32-bit store.
__global__ __launch_bounds__(256) void k_film_rgba8(const double* __restrict__ film, int64_t n,
                                                    uint32_t* __restrict__ rgba) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t v = 255u << 24;
    for (int c = 0; c < 3; c++)
        v |= (uint32_t)(gomath::to_int(gomath::clamp(film[i * 3 + c], 0, 1) * 255) & 0xFF) << (8 * c);
    rgba[i] = v;
}

template __global__ void k_film_add_tiles<false>(const pbrt_film_desc* __restrict__ film_desc, RenderParams rp, pbrtfilm::Layout lay, int64_t tile_begin, int ns, pbrt_film_samples_soa in, double* __restrict__ films);
template __global__ void k_film_add_tiles<true>(const pbrt_film_desc* __restrict__ film_desc, RenderParams rp, pbrtfilm::Layout lay, int64_t tile_begin, int ns, pbrt_film_samples_soa in, double* __restrict__ films);

}  // namespace pbrtk

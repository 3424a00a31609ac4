// film_query.h — the frame layout of pbrt_gpu_frame_samples_device and
// pbrt_gpu_film_add_device (include/pbrt_gpu.h), and the host side of those
// calls and of pbrt_gpu_film_rgba8_device that needs no device: the argument
// checks and the refusals.
// Plain C++ with no dependency on HIP: queries.hip passes in what it knows of the
// context, the kernels of k_film_q.hip call the layout functions on the device
// (PBRT_FQ_HD), and tests/film_query_check.cpp compiles this header on its own.
//
// The layout: tiles in index order over the film's cropped pixel bounds at
// tile_size (integrator.go:316-325), pixels row-major inside their tile, ns
// consecutive samples per pixel, dense. A tile row ty holds ts * W pixels but
// for the last, so the pixels before tile (tx, ty) are ty * ts * W + tx * ts *
// h(ty): every tile left of it in its row is ts wide and h(ty) high.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/pbrt_gpu.h"

#if defined(__HIPCC__)
#define PBRT_FQ_HD __host__ __device__ __forceinline__
#else
#define PBRT_FQ_HD inline
#endif

namespace pbrtfilm {

constexpr int64_t kMaxTileSize = 256;        // a tile's pixel index and its film's extent stay far inside int32
constexpr int64_t kMaxNs = (1 << 20) - 1;    // spp <= 2^20, as a render's (prepare)

struct Layout {
    int64_t min_x, min_y, w, h;   // CroppedPixelBounds
    int64_t ts, ntx, nty;
};
struct Where {
    int64_t tile, pi, px, py;   // the tile, the pixel's index inside it (row-major) and its raster position
};

PBRT_FQ_HD int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

PBRT_FQ_HD Layout layout(const pbrt_film_desc& f, int64_t ts) {
    Layout l;
    l.min_x = f.crop_min_x;
    l.min_y = f.crop_min_y;
    l.w = f.crop_max_x - f.crop_min_x;
    l.h = f.crop_max_y - f.crop_min_y;
    l.ts = ts;
    l.ntx = (l.w + ts - 1) / ts;
    l.nty = (l.h + ts - 1) / ts;
    return l;
}
PBRT_FQ_HD int64_t num_tiles(const Layout& l) { return l.ntx * l.nty; }
PBRT_FQ_HD int64_t row_height(const Layout& l, int64_t ty) { return min64(l.ts, l.h - ty * l.ts); }
PBRT_FQ_HD int64_t col_width(const Layout& l, int64_t tx) { return min64(l.ts, l.w - tx * l.ts); }

// pixels of the tiles [0, tile); tile == num_tiles gives the whole film's
PBRT_FQ_HD int64_t pixels_before(const Layout& l, int64_t tile) {
    if (tile >= num_tiles(l)) return l.w * l.h;
    const int64_t tx = tile % l.ntx, ty = tile / l.ntx;
    return ty * l.ts * l.w + tx * l.ts * row_height(l, ty);
}
PBRT_FQ_HD int64_t pixels_in(const Layout& l, int64_t tile_begin, int64_t tile_end) {
    return tile_begin < tile_end ? pixels_before(l, tile_end) - pixels_before(l, tile_begin) : 0;
}
// the inverse: the pixel at position g (0 <= g < w * h) of the layout. Only a
// film's last tile row is lower than ts and only a row's last tile narrower, so
// both divisions land in the right tile.
PBRT_FQ_HD Where locate(const Layout& l, int64_t g) {
    const int64_t ty = g / (l.ts * l.w), rem = g - ty * l.ts * l.w;
    const int64_t hh = row_height(l, ty);
    const int64_t tx = rem / (l.ts * hh), pi = rem - tx * l.ts * hh;
    const int64_t tw = col_width(l, tx);
    Where wh;
    wh.tile = ty * l.ntx + tx;
    wh.pi = pi;
    wh.px = l.min_x + tx * l.ts + pi % tw;
    wh.py = l.min_y + ty * l.ts + pi / tw;
    return wh;
}

// A tile film's largest extent (RenderParams.slot_w / slot_h) and the doubles
// the tile films of a range take in the context's scratch buffer.
PBRT_FQ_HD int64_t slot_extent(int64_t ts, double radius) { return ts + 2 * ((int64_t)radius + 1); }
inline size_t scratch_doubles(const pbrt_film_desc& f, int64_t ts, int64_t tile_begin, int64_t tile_end) {
    if (tile_begin >= tile_end) return 0;
    return (size_t)(tile_end - tile_begin) * (size_t)(slot_extent(ts, f.filter_radius_x) * slot_extent(ts, f.filter_radius_y) * 3);
}

// Which k_film_add_tiles runs: the LDS-staged gather keeps a work item's film
// pixels in registers, two of them, so it serves tile films of at most 512
// pixels (tile 16 up to radius 2.99); the direct gather serves every size.
// `knob`: Knobs::film_add_lds.
constexpr int64_t kLdsFilmPixels = 512;
inline bool lds_gather(bool knob, const pbrt_film_desc& f, int64_t ts) {
    return knob && slot_extent(ts, f.filter_radius_x) * slot_extent(ts, f.filter_radius_y) <= kLdsFilmPixels;
}

// ---------------------------------------------------------------- the checks
// PBRT_E_INVALID's conditions of the two frame calls, in the header's order;
// `why` names the first. On PBRT_OK *count is the range's element count.
// flags_ok: the flags the call takes (frame_samples none, film_add the clear flag).
inline int check_frame(bool ctx_ok, const pbrt_film_desc* f, const pbrt_frame_desc* d, int32_t flags_ok, bool in_flight,
                       int64_t* count, const char** why) {
    auto bad = [&](const char* m) {
        *why = m;
        return (int)PBRT_E_INVALID;
    };
    *count = 0;
    if (!ctx_ok || !f) return bad("null context");
    if (!d) return bad("the frame desc is NULL");
    if (d->tile_size < 1) return bad("tile_size < 1");
    if (d->ns < 1) return bad("ns < 1");
    if (d->flags & ~flags_ok) return bad("flags the call does not take");
    if (d->reserved != 0) return bad("reserved must be 0");
    if (d->tile_size > kMaxTileSize || d->ns > kMaxNs) {   // (refused below; the layout is not evaluated)
        if (in_flight) return bad("a render is in flight on this context");
        *why = "";
        return PBRT_OK;
    }
    const Layout l = layout(*f, d->tile_size);
    if (d->tile_begin < 0 || d->tile_end < d->tile_begin || d->tile_end > num_tiles(l))
        return bad("tile range outside 0 <= tile_begin <= tile_end <= the film's tiles");
    const int64_t px = pixels_in(l, d->tile_begin, d->tile_end);
    if (px > (int64_t)INT32_MAX / d->ns) return bad("more than 2^31 - 1 samples in one call");
    if (in_flight) return bad("a render is in flight on this context");
    *count = px * d->ns;
    *why = "";
    return PBRT_OK;
}

// PBRT_E_UNSUPPORTED of the frame calls: what the kernels do not handle. with_filter:
// pbrt_gpu_film_add_device, whose merge reads the 3x3 tiles around a film pixel's own
// (k_merge_film's assumption: a tile film reaches no further than its neighbours).
inline int check_frame_supported(const pbrt_film_desc& f, const pbrt_frame_desc& d, bool with_filter, const char** why) {
    auto no = [&](const char* m) {
        *why = m;
        return (int)PBRT_E_UNSUPPORTED;
    };
    if (d.tile_size > kMaxTileSize) return no("tile_size > 256");
    if (d.ns > kMaxNs) return no("ns > 2^20 - 1");
    if (with_filter && !(f.filter_radius_x > 0 && f.filter_radius_y > 0 && f.filter_radius_x < (double)d.tile_size &&
                         f.filter_radius_y < (double)d.tile_size))
        return no("filter radius must be in (0, tile_size): a tile film would reach beyond its neighbouring tiles");
    *why = "";
    return PBRT_OK;
}

inline int check_samples_out(const pbrt_frame_samples_soa* out, const char** why) {
    auto bad = [&](const char* m) {
        *why = m;
        return (int)PBRT_E_INVALID;
    };
    if (!out) return bad("out is NULL");
    if (!out->ox || !out->oy || !out->oz || !out->dx || !out->dy || !out->dz) return bad("a ray array is NULL");
    if (!out->pfilm_x || !out->pfilm_y) return bad("a pfilm array is NULL");
    if (!out->state || !out->inc) return bad("an rng array is NULL");
    *why = "";
    return PBRT_OK;
}
inline int check_film_in(const pbrt_film_samples_soa* in, const double* film, const char** why) {
    auto bad = [&](const char* m) {
        *why = m;
        return (int)PBRT_E_INVALID;
    };
    if (!in) return bad("samples is NULL");
    if (!in->pfilm_x || !in->pfilm_y) return bad("a pfilm array is NULL");
    if (!in->r || !in->g || !in->b) return bad("a radiance array is NULL");
    if (!film) return bad("the film is NULL");
    *why = "";
    return PBRT_OK;
}
inline int check_rgba8(bool ctx_ok, const double* film, int64_t w, int64_t h, const uint8_t* rgba, bool in_flight,
                       const char** why) {
    auto bad = [&](const char* m) {
        *why = m;
        return (int)PBRT_E_INVALID;
    };
    if (!ctx_ok) return bad("null context");
    if (!film) return bad("the film is NULL");
    if (!rgba) return bad("rgba is NULL");
    if (((uintptr_t)film & 7) || ((uintptr_t)rgba & 3)) return bad("the film must be 8-byte and rgba 4-byte aligned");
    if (w <= 0 || h <= 0) return bad("w <= 0 or h <= 0");
    if (w > (int64_t)INT32_MAX / h) return bad("more than 2^31 - 1 pixels");
    if (in_flight) return bad("a render is in flight on this context");
    *why = "";
    return PBRT_OK;
}

// The film rows a film_add of a tile range can reach: the tile films of its
// first and last tile row, as Film.GetFilmTile bounds them (film.go:106-113;
// reach = floor(radius + 0.5) rows beyond the tiles, cropped). With the clear
// flag the call writes the whole film. Rows are relative to the crop.
struct Rows {
    int64_t y0, y1;
};
inline Rows rows_touched(const Layout& l, const pbrt_film_desc& f, int64_t tile_begin, int64_t tile_end, bool clear) {
    if (clear || tile_begin >= tile_end) return Rows{0, clear ? l.h : 0};
    const int64_t reach = (int64_t)(f.filter_radius_y + 0.5);
    const int64_t ty0 = tile_begin / l.ntx, ty1 = (tile_end - 1) / l.ntx;
    int64_t y0 = ty0 * l.ts - reach, y1 = min64(l.h, (ty1 + 1) * l.ts) + reach;
    if (y0 < 0) y0 = 0;
    if (y1 > l.h) y1 = l.h;
    return Rows{y0, y1};
}

}  // namespace pbrtfilm

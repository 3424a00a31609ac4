// strat_query.h — the host side of pbrt_gpu_frame_samples_stratified_device and
// pbrt_gpu_li_stratified_device (include/pbrt_gpu.h) that needs no device: the
// argument checks and the refusals in the header's order, the pixel and table
// counts, the cursors after a camera sample, the StartPixel form and LDS carve
// of k_strat_pixels (render_params' and layout_L's, frame_route.h) and the
// k_li_strat instantiation.
// Plain C++ with no dependency on HIP: queries.hip passes in what it knows of
// the context, and tests/strat_query_check.cpp compiles this header on its own.
// The frame's own checks are film_query.h's and the li desc's li_query.h's:
// called here, not restated.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/pbrt_gpu.h"
#include "film_query.h"
#include "frame_route.h"
#include "li_query.h"

namespace pbrtstrat {

constexpr int64_t kMaxLds = 48 * 1024;   // k_strat_pixels' dynamic LDS (wave_eligible's bound on layout_L)

// The pixels of a tile range: the tables frame_samples_stratified writes, and
// the elements of the frame layout with one element a pixel.
inline int64_t pixel_count(const pbrt_film_desc& f, const pbrt_frame_desc& d) {
    return pbrtfilm::pixels_in(pbrtfilm::layout(f, d.tile_size), d.tile_begin, d.tile_end);
}
// doubles of one pixel's table
inline int64_t table_doubles(const pbrt_strat_sampler_desc& s) {
    return (int64_t)s.n_dims * s.sampler_x * s.sampler_y;
}

// GetCameraSample (sampler.go:75-80) asks Get2D pFilm, Get2D pLens, Get1D time:
// the cursors it leaves, and its PCG32 draws (pbrt_spec.h: camera_draws).
struct Cursors {
    int first_1d, first_2d;
};
inline Cursors cursors_after_camera(int n_dims) {
    return Cursors{n_dims < 1 ? n_dims : 1, n_dims < 2 ? n_dims : 2};
}
inline uint32_t camera_draws(int n_dims) {
    return (n_dims < 1 ? 2u : 0u) + (n_dims < 2 ? 2u : 0u) + (n_dims < 1 ? 1u : 0u);
}

// ------------------------------------------------ frame_samples_stratified
// PBRT_E_INVALID's conditions in the header's order; `why` names the first. On
// PBRT_OK *count is the range's sample count (pixels * ns).
inline int check_samples_args(bool ctx_ok, const pbrt_film_desc* f, const pbrt_frame_desc* d,
                              const pbrt_strat_sampler_desc* s, const pbrt_frame_samples_soa* out,
                              const pbrt_strat_samples_soa* strat, bool in_flight, int64_t* count, const char** why) {
    auto bad = [&](const char* m) {
        *why = m;
        return (int)PBRT_E_INVALID;
    };
    if (int rc = pbrtfilm::check_frame(ctx_ok, f, d, 0, in_flight, count, why)) return rc;
    if (!s) return bad("the sampler desc is NULL");
    if (s->sampler_x < 1 || s->sampler_y < 1) return bad("sampler_x < 1 or sampler_y < 1");
    if (s->reserved != 0) return bad("the sampler's reserved must be 0");
    if ((int64_t)d->ns != (int64_t)s->sampler_x * s->sampler_y - 1) return bad("ns != sampler_x * sampler_y - 1");
    if (int rc = pbrtfilm::check_samples_out(out, why)) return rc;
    if (!strat) return bad("strat is NULL");
    if (!strat->k || !strat->table) return bad("a sample index array is NULL");
    if (!strat->s1d) return bad("the table array is NULL");
    *why = "";
    return PBRT_OK;
}

// The RenderParams a THROUGHPUT render of the same sampler would give its
// StartPixel (render_params: the event and draw counts, sp_serial, sp_window)
// and the LDS carve of k_mb_setup (layout_L): k_strat_pixels runs on both.
struct Plan {
    pbrtk::RenderParams rp;
    pbrtk::ChainLayout lay;
};
inline Plan plan(const pbrtroute::Facts& facts, const pbrt::Knobs& knobs, const pbrt_film_desc& f,
                 const pbrt_frame_desc& d, const pbrt_strat_sampler_desc& s) {
    pbrt_render_desc rd{};
    rd.tile_size = d.tile_size;
    rd.sampler_x = s.sampler_x;
    rd.sampler_y = s.sampler_y;
    rd.n_dims = s.n_dims;
    rd.jitter = s.jitter ? 1 : 0;
    rd.integrator = PBRT_INTEGRATOR_PATH;
    rd.max_depth = 1;
    rd.mode = PBRT_MODE_THROUGHPUT;
    Plan p;
    p.rp = pbrtroute::render_params(facts, knobs, f, rd, pbrtk::kWave);
    p.lay = pbrtroute::layout_L(p.rp);
    return p;
}
// which StartPixel start_pixel_wave takes for the plan: 0 buffered, 1 serial, 2 windowed
inline int start_pixel_form(const pbrtk::RenderParams& rp) { return !rp.sp_serial ? 0 : rp.sp_window ? 2 : 1; }

// PBRT_E_UNSUPPORTED: the frame calls' own, then what the wave StartPixel does not take.
inline int check_samples_supported(const pbrtroute::Facts& facts, const pbrt::Knobs& knobs, const pbrt_film_desc& f,
                                   const pbrt_frame_desc& d, const pbrt_strat_sampler_desc& s, const char** why) {
    auto no = [&](const char* m) {
        *why = m;
        return (int)PBRT_E_UNSUPPORTED;
    };
    if (int rc = pbrtfilm::check_frame_supported(f, d, false, why)) return rc;
    if (s.n_dims < 1) return no("n_dims < 1: the frame of pbrt_gpu_frame_samples_device");
    const int64_t spp = (int64_t)s.sampler_x * s.sampler_y;
    if (spp > 4096) return no("more than 4096 samples per pixel");
    if ((int64_t)s.n_dims * spp > 8192) return no("n_dims * spp > 8192");
    if (plan(facts, knobs, f, d, s).lay.total > kMaxLds) return no("the StartPixel staging does not fit 48 KB of LDS");
    *why = "";
    return PBRT_OK;
}

// ------------------------------------------------------------ li_stratified
// After pbrtli::check_args: PBRT_E_INVALID's conditions of the strat block.
inline int check_li_strat(const pbrt_strat_soa* st, const char** why) {
    auto bad = [&](const char* m) {
        *why = m;
        return (int)PBRT_E_INVALID;
    };
    if (!st) return bad("strat is NULL");
    if (st->reserved != 0) return bad("strat's reserved must be 0");
    if (st->n_dims < 0) return bad("n_dims < 0");
    if (st->first_1d < 0 || st->first_1d > st->n_dims || st->first_2d < 0 || st->first_2d > st->n_dims)
        return bad("a cursor outside [0, n_dims]");
    if (st->n_dims > 0) {
        if (!st->s1d) return bad("the table array is NULL");
        if (!st->table || !st->k) return bad("a sample index array is NULL");
        if (st->spp < 1) return bad("spp < 1");
        if (st->n_tables < 1) return bad("n_tables < 1");
    }
    *why = "";
    return PBRT_OK;
}
// every check of pbrt_gpu_li_stratified_device before the scene's: li_device's, then the strat block's
// (a render in flight is the last of li_device's, so a bad strat block of a blocked context reads "in flight")
inline int check_li_args(bool ctx_ok, const pbrt_li_desc* d, const pbrt_ray_soa* rays, const pbrt_rng_soa* rng, size_t n,
                         const pbrt_radiance_soa* out, const pbrt_strat_soa* st, bool in_flight, const char** why) {
    if (int rc = pbrtli::check_args(ctx_ok, d, rays, rng, n, out, in_flight, why)) return rc;
    return check_li_strat(st, why);
}

// The k_li_strat instantiation and its grid: k_li's rule (kX by the materials, the [64] stack
// beyond an LDS-staged tree, kLiRays rays a wave).
inline pbrtli::KernelArgs kernel_args(bool non_matte, int n_nodes, bool mesh, size_t n, int lds_nodes) {
    return pbrtli::kernel_args(non_matte, n_nodes, mesh, n, lds_nodes);
}

}  // namespace pbrtstrat

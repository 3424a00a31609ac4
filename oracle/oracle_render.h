/*
 * oracle/oracle_render.h — TEST INFRASTRUCTURE (oracle). Not part of the product.
 * CPU restatement of go-pbrt's hot path; see oracle_render.c.
 */
#ifndef ORACLE_RENDER_H
#define ORACLE_RENDER_H

#include "oracle_core.h"

#define ORACLE_FLAG_MIS_RAY 1   /* trace EstimateDirect's (no-op) BSDF-sampled ray */
#define ORACLE_FLAG_RANDOM_SAMPLER 2   /* sampler.RandomSampler (random.go) with spp = sampler_x * sampler_y */

typedef struct { uint64_t state, inc; } orc_pcg;
uint32_t orc_pcg_next(orc_pcg* r);
void orc_pcg_set_sequence(orc_pcg* r, uint64_t seed);
uint32_t orc_pcg_bounded(orc_pcg* r, uint32_t b);
double orc_pcg_float(orc_pcg* r);

typedef struct {
    const pbrt_scene_desc* scene;
    const pbrt_render_desc* rd;
    int flags;
    pbrt_distribution_desc dist;
    panic_ctx pc;
    int64_t cur_tile, cur_px, cur_py;
    int32_t cur_sample, cur_bounce;
    int unsupported;
    uint64_t paths, camera_samples, closest_rays, shadow_rays;
    const struct orc_mesh* mesh;   /* triangle meshes of the scene (extension), or NULL */
    int64_t* pixel_draws;          /* orc_tile_draws: PCG32 draws per pixel of the tile, or NULL */
} orc_ctx;

typedef struct {
    uint64_t tiles, paths, camera_samples, closest_rays, shadow_rays;
    uint64_t flops;   /* fp64 add/sub/mul/div/sqrt executed (liboracle_flops.so only) */
    int32_t panic_kind;
    int64_t panic_tile, panic_px, panic_py, panic_sample, panic_bounce;
    uint64_t flops_light;   /* the part of flops spent in UniformSampleOneLight + L += beta*Ld */
} orc_stats;

void orc_light_distribution(const pbrt_scene_desc* sc, const pbrt_render_desc* rd,
                            pbrt_distribution_desc* d);
int64_t orc_num_tiles(const pbrt_scene_desc* sc, const pbrt_render_desc* rd);
void orc_tile_bounds(const pbrt_scene_desc* sc, const pbrt_render_desc* rd, int64_t tile,
                     int64_t* x0, int64_t* y0, int64_t* x1, int64_t* y1);
void orc_film_tile_bounds(const pbrt_scene_desc* sc, int64_t x0, int64_t y0, int64_t x1, int64_t y1,
                          int64_t* px0, int64_t* py0, int64_t* px1, int64_t* py1);
int orc_render(const pbrt_scene_desc* sc, const pbrt_render_desc* rd, int n_threads, int flags,
               double* film_xyz, orc_stats* stats);
int orc_tile_draws(const pbrt_scene_desc* sc, const pbrt_render_desc* rd, int64_t tile, int64_t* out);
int orc_intersect(const pbrt_scene_desc* sc, const double* rays, size_t n, int closest, double* out);

/* Path.Li (path.go:32-157) on caller rays, ray i with sampler.RandomSampler on the
 * PCG32 stream (state[i], inc[i]). rays: n x 7 (o, d, TMax).
 * start_f (n x 7: L, beta, etaScale) and start_i (n x 4: bounces, draws,
 * closest-hit queries, visibility rays) give the state a path starts from;
 * NULL is the state Li itself starts from. At most k iterations of the loop
 * run (k <= 0: to the end), the statements render_tile's path_li runs.
 * out_f: n x 14 (L, beta, etaScale, the next ray o d TMax); out_state: the
 * stream's state; out_i: n x 6 (bounces, draws, closest-hit queries,
 * visibility rays, status ORC_PATH_*, PBRT_PANIC_* kind). A path that is not
 * ALIVE has no next ray: its ray, beta and etaScale are those its last
 * iteration started from. A panicking path has L = 0 and its counters and
 * stream as they stand at the panic. */
enum { ORC_PATH_ALIVE = 1, ORC_PATH_ENDED = 2, ORC_PATH_PANICKED = 3 };   /* PBRT_PATH_*'s values */
int orc_path_li(const pbrt_scene_desc* sc, int max_depth, int light_strategy, double rr_threshold, size_t n,
                const double* rays, const uint64_t* state, const uint64_t* inc, const double* start_f,
                const int32_t* start_i, int k, double* out_f, uint64_t* out_state, int32_t* out_i);
/* DirectLighting.Li (directlighting.go:62-104) at depth 0 on the same inputs.
 * out_L: n x 3; out_i: n x 4 (draws, closest-hit queries, visibility rays,
 * PBRT_PANIC_* kind); a panicking ray as above. */
int orc_direct_li(const pbrt_scene_desc* sc, int max_depth, int dl_strategy, size_t n, const double* rays,
                  const uint64_t* state, const uint64_t* inc, double* out_L, uint64_t* out_state, int32_t* out_i);

#endif

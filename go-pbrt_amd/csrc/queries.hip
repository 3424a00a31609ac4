// queries.hip — what a context answers between frames: the ray queries (over host
// arrays, and over arrays resident on the device), the camera rays of a pixel
// window, Integrator.Li batched or one bounce at a time, a frame from public
// pieces, the queries' panic record and the buffers a context owns
// (include/pbrt_gpu.h). The checks, the kernel choices and the grids that need
// no device are in the HIP-free headers li_query.h, direct_li_query.h,
// path_query.h, film_query.h, strat_query.h and query_buffers.h.
#pragma clang fp contract(off)

#include "../../include/pbrt_diag.h"
#include "context.h"
#include "direct_li_query.h"
#include "film_query.h"
#include "kernel_select.h"
#include "path_query.h"
#include "strat_query.h"

using namespace pbrt;
using namespace pbrtk;

// after a query's launches: what the runtime says of them
static int launched(pbrt_gpu_ctx* c) {
    HIPCHK(c, hipGetLastError());
    return PBRT_OK;
}

extern "C" {

static int intersect_batch(pbrt_gpu_ctx* c, const pbrt_ray_soa* rays, size_t n, int any, pbrt_hit_soa* hits,
                           uint8_t* occluded) {
    if (!c || !rays || (!hits && !occluded)) return PBRT_E_INVALID;
    if (n == 0) return PBRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<double> packed(n * 7);
    for (size_t i = 0; i < n; i++) {
        double* q = &packed[7 * i];
        q[0] = rays->ox[i]; q[1] = rays->oy[i]; q[2] = rays->oz[i];
        q[3] = rays->dx[i]; q[4] = rays->dy[i]; q[5] = rays->dz[i];
        q[6] = rays->tmax ? rays->tmax[i] : gomath::kInf;
    }
    size_t nout = any ? n : 9 * n;
    DevBuf<double> in_buf, out_buf;
    if (int rc = in_buf.ensure(c, packed.size())) return rc;
    if (int rc = out_buf.ensure(c, nout)) return rc;
    double *d_in = in_buf.get(), *d_o = out_buf.get();
    std::vector<double> o(nout);
    hipError_t e = hipMemcpyAsync(d_in, packed.data(), sizeof(double) * packed.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        DevScene sc = dev_scene(c, false);
        launch_k(c, k_intersect, dim3((unsigned)((n + kWave - 1) / kWave)), dim3(kWave), 0, c->stream,
                           with_slot(sc, 7),
                           (int64_t)n, d_in, d_o, any);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(o.data(), d_o, sizeof(double) * nout, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return set_err(c, PBRT_E_HIP, hipGetErrorString(e));
    int rc = PBRT_OK;
    for (size_t i = 0; i < n; i++) {
        if (any) {
            if (gomath::is_nan(o[i])) rc = PBRT_E_REF_PANIC;
            occluded[i] = o[i] == 1.0;
        } else {
            const double* r = &o[9 * i];
            if (gomath::is_nan(r[0])) { rc = PBRT_E_REF_PANIC; hits->hit[i] = 0; continue; }
            hits->hit[i] = r[0] == 1.0;
            if (hits->t_max) hits->t_max[i] = r[1];
            if (hits->prim) hits->prim[i] = (int32_t)r[2];
            if (hits->px) hits->px[i] = r[3];
            if (hits->py) hits->py[i] = r[4];
            if (hits->pz) hits->pz[i] = r[5];
            if (hits->nx) hits->nx[i] = r[6];
            if (hits->ny) hits->ny[i] = r[7];
            if (hits->nz) hits->nz[i] = r[8];
        }
    }
    if (rc != PBRT_OK) set_err(c, rc, "the Go reference panics on at least one ray");
    return rc;
}

int pbrt_gpu_intersect(pbrt_gpu_ctx* c, const pbrt_ray_soa* rays, size_t n, pbrt_hit_soa* hits) {
    return intersect_batch(c, rays, n, 0, hits, nullptr);
}
int pbrt_gpu_intersect_p(pbrt_gpu_ctx* c, const pbrt_ray_soa* rays, size_t n, uint8_t* occluded) {
    return intersect_batch(c, rays, n, 1, nullptr, occluded);
}

// ------------------------------------------------ device-resident queries
// (between frames only: query_blocked, context.h)
// the record cleared, in stream order (so after the queries already enqueued)
static hipError_t query_rec_clear(pbrt_gpu_ctx* c) {
    hipError_t e = hipMemsetAsync(&c->d_qrec.get()->panics, 0, sizeof(c->d_qrec.get()->panics), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(&c->d_qrec.get()->first, 0xFF, sizeof(c->d_qrec.get()->first), c->stream);
    return e;
}
// the one allocation of the query path, on a context's first query
static int query_rec_ensure(pbrt_gpu_ctx* c) {
    if (c->d_qrec.get()) return PBRT_OK;
    if (int rc = c->d_qrec.ensure(c, 1)) return rc;
    HIPCHK(c, query_rec_clear(c));
    return PBRT_OK;
}

// What a query over the scene does once its checks have passed and it has rays to trace: the
// device, the panic record, and the scene view its kernel reads (li_dist: with the distribution
// li_distribution uploaded). An empty query has returned before: it allocates and launches nothing.
static int query_begin(pbrt_gpu_ctx* c, bool li_dist, DevScene& sc) {
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = query_rec_ensure(c)) return rc;
    sc = with_slot(dev_scene(c, false), 7);
    if (li_dist) sc.dist = c->li.d_dist.get();
    return PBRT_OK;
}

// staged: the diagnostic k_query_hit_staged (pbrt_diag.h), for trees the render kernels stage in LDS
static int query_hit(pbrt_gpu_ctx* c, const pbrt_ray_soa* rays, size_t n, bool any, const pbrt_hit_soa& hits,
                     bool staged = false) {
    if (!c || !rays || !hits.hit) return PBRT_E_INVALID;
    if (staged && (c->host_scene.n_nodes > kLdsNodes || c->host_scene.n_meshes > 0))
        return set_err(c, PBRT_E_INVALID, "the staged query takes trees of at most 64 nodes and no mesh");
    if (!pbrtli::rays_complete(*rays)) return set_err(c, PBRT_E_INVALID, "a ray array is NULL");
    if (n > (size_t)INT32_MAX) return set_err(c, PBRT_E_INVALID, "more than 2^31 - 1 rays in one query");
    if (query_blocked(c)) return set_err(c, PBRT_E_INVALID, "a render is in flight on this context");
    if (n == 0) return PBRT_OK;
    DevScene sc;
    if (int rc = query_begin(c, false, sc)) return rc;
    const bool mesh_only = c->host_scene.n_prims == 0;   // as the render path chooses its kMeshOnly kernels
    const auto kern = staged ? (any ? k_query_hit_staged<true> : k_query_hit_staged<false>)
                      : any  ? (mesh_only ? k_query_hit<true, true> : k_query_hit<true, false>)
                             : (mesh_only ? k_query_hit<false, true> : k_query_hit<false, false>);
    launch_k(c, kern, dim3((unsigned)((n + kQueryBlock - 1) / kQueryBlock)), dim3(kQueryBlock), 0, c->stream, sc,
             (int64_t)n, *rays, hits, c->d_qrec.get());
    return launched(c);
}

int pbrt_gpu_intersect_device(pbrt_gpu_ctx* c, const pbrt_ray_soa* rays, size_t n, const pbrt_hit_soa* hits) {
    if (!hits) return PBRT_E_INVALID;
    return query_hit(c, rays, n, false, *hits);
}
int pbrt_gpu_intersect_p_device(pbrt_gpu_ctx* c, const pbrt_ray_soa* rays, size_t n, uint8_t* occluded) {
    pbrt_hit_soa h{};
    h.hit = occluded;
    return query_hit(c, rays, n, true, h);
}

// pbrt_diag.h: the same queries through the LDS-staged walks of the render kernels
int pbrt_diag_intersect_staged_device(pbrt_gpu_ctx* c, const pbrt_ray_soa* rays, size_t n, const pbrt_hit_soa* hits) {
    if (!hits) return PBRT_E_INVALID;
    return query_hit(c, rays, n, false, *hits, true);
}
int pbrt_diag_intersect_p_staged_device(pbrt_gpu_ctx* c, const pbrt_ray_soa* rays, size_t n, uint8_t* occluded) {
    pbrt_hit_soa h{};
    h.hit = occluded;
    return query_hit(c, rays, n, true, h, true);
}
int pbrt_gpu_cull_groups(pbrt_gpu_ctx* c) { return c ? c->n_groups : -PBRT_E_INVALID; }

int pbrt_gpu_camera_rays_device(pbrt_gpu_ctx* c, const pbrt_camera_rays_desc* d, const pbrt_ray_soa_out* rays) {
    if (!c || !d || !rays) return PBRT_E_INVALID;
    if (!pbrtli::rays_complete(*rays)) return set_err(c, PBRT_E_INVALID, "a ray array is NULL");
    const pbrt_film_desc& f = c->host_scene.film;
    if (d->x0 < 0 || d->x0 >= d->x1 || d->x1 > f.res_x || d->y0 < 0 || d->y0 >= d->y1 || d->y1 > f.res_y)
        return set_err(c, PBRT_E_INVALID, "pixel window outside the film resolution");
    const int64_t n = (d->x1 - d->x0) * (d->y1 - d->y0);
    if (n > (int64_t)INT32_MAX) return set_err(c, PBRT_E_INVALID, "more than 2^31 - 1 rays in one query");
    if (query_blocked(c)) return set_err(c, PBRT_E_INVALID, "a render is in flight on this context");
    HIPCHK(c, hipSetDevice(c->device));
    launch_k(c, k_query_camera, dim3((unsigned)((n + kQueryBlock - 1) / kQueryBlock)), dim3(kQueryBlock), 0,
                       c->stream, c->d_camera.get(), *d, *rays);
    return launched(c);
}

// The light distribution of a Li query's strategy in the query's own buffer (li_device, path_step_device):
// built, checked and uploaded when the strategy differs from the one last uploaded. n == 0 uploads nothing.
static int li_distribution(pbrt_gpu_ctx* c, const pbrt_li_desc* d, size_t n) {
    const char* why = "";
    if (c->li.strategy == d->light_strategy) return PBRT_OK;
    // (a refused strategy leaves the uploaded one in place)
    pbrt_distribution_desc dist;
    if (int rc = pbrt_scene_light_distribution(&c->host_scene, d->light_strategy, &dist))
        return set_err(c, rc, "unsupported light sample strategy");
    if (int rc = pbrtli::check_distribution(c->host_scene.n_lights, dist.func, dist.count, dist.func_int, &why))
        return set_err(c, rc, why);
    if (n == 0) return PBRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = c->li.d_dist.ensure(c, 1)) return rc;
    c->li.host_dist = dist;
    c->li.strategy = 0;
    HIPCHK(c, hipMemcpyAsync(c->li.d_dist.get(), &c->li.host_dist, sizeof(dist), hipMemcpyHostToDevice, c->stream));
    c->li.strategy = d->light_strategy;
    return PBRT_OK;
}

// Integrator.Li over device arrays (k_li.hip). The checks and the kernel choice: li_query.h.
int pbrt_gpu_li_device(pbrt_gpu_ctx* c, const pbrt_li_desc* d, const pbrt_ray_soa* rays, const pbrt_rng_soa* rng,
                       size_t n, const pbrt_radiance_soa* out) {
    const char* why = "";
    if (int rc = pbrtli::check_args(c != nullptr, d, rays, rng, n, out, c && query_blocked(c), &why))
        return set_err(c, rc, why);
    if (int rc = pbrtli::check_supported(*d, c->facts.rough_glass, &why)) return set_err(c, rc, why);
    if (int rc = li_distribution(c, d, n)) return rc;
    if (n == 0) return PBRT_OK;
    DevScene sc;
    if (int rc = query_begin(c, true, sc)) return rc;
    const pbrtli::KernelArgs ka =
        pbrtli::kernel_args(c->facts.non_matte, c->host_scene.n_nodes, c->mesh.n_nodes != 0, n, kLdsNodes);
    const LiKernel kern = li_kernel(ka.kx, ka.depth);
    if (!kern) return set_err(c, PBRT_E_HIP, "no k_li instantiation for depth " + std::to_string(ka.depth));
    launch_k(c, kern, dim3(ka.grid), dim3(kWave), 0, c->stream, sc, (int)d->max_depth, d->rr_threshold, (int64_t)n,
             *rays, *rng, *out, c->d_qrec.get());
    return launched(c);
}

// Path.Li one iteration at a time over device path state (k_path_step.hip). The checks, the queue rules and the
// grids: path_query.h; the desc's refusals, the distribution and the instantiation's choice are the li query's.
int pbrt_gpu_path_begin_device(pbrt_gpu_ctx* c, const pbrt_ray_soa* rays, const pbrt_rng_soa* rng, size_t n,
                               const pbrt_path_soa* paths) {
    const char* why = "";
    if (int rc = pbrtpath::check_begin(c != nullptr, rays, rng, n, paths, c && query_blocked(c), &why))
        return set_err(c, rc, why);
    if (n == 0) return PBRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    launch_k(c, k_path_begin, dim3(pbrtpath::begin_grid(n)), dim3(pbrtpath::kBeginBlock), 0, c->stream, (int64_t)n, *rays,
             *rng, *paths);
    return launched(c);
}

int pbrt_gpu_path_step_device(pbrt_gpu_ctx* c, const pbrt_li_desc* d, const pbrt_path_soa* paths, const pbrt_path_queue* in,
                              const pbrt_path_queue* out, size_t n, const pbrt_path_step_soa* step) {
    const char* why = "";
    if (int rc = pbrtpath::check_step(c != nullptr, d, paths, in, out, n, c && query_blocked(c), &why))
        return set_err(c, rc, why);
    if (int rc = pbrtli::check_supported(*d, c->facts.rough_glass, &why)) return set_err(c, rc, why);
    if (int rc = li_distribution(c, d, n)) return rc;
    if (n == 0) return PBRT_OK;
    DevScene sc;
    if (int rc = query_begin(c, true, sc)) return rc;
    const pbrtli::KernelArgs ka =
        pbrtpath::step_args(c->facts.non_matte, c->host_scene.n_nodes, c->mesh.n_nodes != 0, n, kLdsNodes);
    const PathStepKernel kern = path_step_kernel(ka.kx, ka.depth);
    if (!kern) return set_err(c, PBRT_E_HIP, "no k_path_step instantiation for depth " + std::to_string(ka.depth));
    if (out) HIPCHK(c, hipMemsetAsync(out->count, 0, sizeof(uint32_t), c->stream));
    launch_k(c, kern, dim3(ka.grid), dim3(kWave), 0, c->stream, sc, (int)d->max_depth, d->rr_threshold, (int64_t)n,
             *paths, in ? *in : pbrt_path_queue{nullptr, nullptr}, out ? *out : pbrt_path_queue{nullptr, nullptr},
             step ? *step : pbrt_path_step_soa{}, c->d_qrec.get());
    return launched(c);
}

// DirectLighting.Li over device arrays (k_li_direct.hip). The checks, the kernel choice, the capped grid and
// the size of the level records: direct_li_query.h. No light distribution: one launch a call.
int pbrt_gpu_direct_li_device(pbrt_gpu_ctx* c, const pbrt_direct_li_desc* d, const pbrt_ray_soa* rays,
                              const pbrt_rng_soa* rng, size_t n, const pbrt_radiance_soa* out) {
    const char* why = "";
    if (int rc = pbrtdli::check_args(c != nullptr, d, rays, rng, n, out, c && query_blocked(c), &why))
        return set_err(c, rc, why);
    if (int rc = pbrtdli::check_supported(*d, c->facts.rough_glass, c->facts.non_matte, &why)) return set_err(c, rc, why);
    if (n == 0) return PBRT_OK;
    DevScene sc;
    if (int rc = query_begin(c, false, sc)) return rc;
    const pbrtdli::KernelArgs ka = pbrtdli::kernel_args(c->facts.non_matte, c->host_scene.n_nodes, c->mesh.n_nodes != 0, n,
                                                        kLdsNodes, c->knobs.direct_li_grid, d->max_depth);
    const DirectLiKernel kern = direct_li_kernel(ka.kx, ka.depth);
    if (!kern) return set_err(c, PBRT_E_HIP, "no k_li_direct instantiation for depth " + std::to_string(ka.depth));
    if (ka.level_doubles > 0)   // (grows only: a smaller query runs in the buffer of a larger one)
        if (int rc = c->d_dli_levels.ensure(c, ka.level_doubles)) return rc;
    launch_k(c, kern, dim3(ka.grid), dim3(kWave), 0, c->stream, sc, (int)d->max_depth, (int)d->dl_strategy, ka.levels,
             (int64_t)n, *rays, *rng, *out, c->d_qrec.get(), ka.level_doubles > 0 ? c->d_dli_levels.get() : nullptr);
    return launched(c);
}

// (diagnostics) the capacity of the level-record buffer in bytes: it changes only when the buffer is allocated anew
size_t pbrt_gpu_direct_li_scratch_bytes(const pbrt_gpu_ctx* c) { return c ? c->d_dli_levels.cap() * sizeof(double) : 0; }

// ---- a frame from public pieces (k_film_q.hip). The layout, the checks and the refusals: film_query.h.
// The RenderParams the film kernels' tile_bounds / film_tile_bounds read, for a tile size of the caller's.
static RenderParams frame_params(const pbrt_gpu_ctx* c, const pbrtfilm::Layout& l) {
    const pbrt_film_desc& f = c->host_scene.film;
    RenderParams rp{};
    rp.film_min_x = l.min_x;
    rp.film_min_y = l.min_y;
    rp.film_w = l.w;
    rp.film_h = l.h;
    rp.tile_size = l.ts;
    rp.ntx = l.ntx;
    rp.nty = l.nty;
    rp.tile_stride = 1;
    rp.slot_w = pbrtfilm::slot_extent(l.ts, f.filter_radius_x);
    rp.slot_h = pbrtfilm::slot_extent(l.ts, f.filter_radius_y);
    return rp;
}

int64_t pbrt_gpu_frame_count(const pbrt_gpu_ctx* c, const pbrt_frame_desc* d) {
    const char* why = "";
    int64_t n = 0;
    if (pbrtfilm::check_frame(c != nullptr, c ? &c->host_scene.film : nullptr, d, PBRT_FILM_ADD_CLEAR, false, &n, &why))
        return -PBRT_E_INVALID;
    return n;
}

int pbrt_gpu_frame_samples_device(pbrt_gpu_ctx* c, const pbrt_frame_desc* d, const pbrt_frame_samples_soa* out) {
    const char* why = "";
    int64_t n = 0;
    const pbrt_film_desc* f = c ? &c->host_scene.film : nullptr;
    if (int rc = pbrtfilm::check_frame(c != nullptr, f, d, 0, c && query_blocked(c), &n, &why)) return set_err(c, rc, why);
    if (int rc = pbrtfilm::check_samples_out(out, &why)) return set_err(c, rc, why);
    if (int rc = pbrtfilm::check_frame_supported(*f, *d, false, &why)) return set_err(c, rc, why);
    if (n == 0) return PBRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const pbrtfilm::Layout l = pbrtfilm::layout(*f, d->tile_size);
    launch_k(c, k_frame_samples, dim3((unsigned)((n + kQueryBlock - 1) / kQueryBlock)), dim3(kQueryBlock), 0, c->stream,
             c->d_camera.get(), l, pbrtfilm::pixels_before(l, d->tile_begin), (int)d->ns, n, *out);
    return launched(c);
}

// ---- the same pieces under sampler.Stratified (k_strat.hip). The checks, the StartPixel plan and the
// kernel choice: strat_query.h.
int pbrt_gpu_frame_samples_stratified_device(pbrt_gpu_ctx* c, const pbrt_frame_desc* d, const pbrt_strat_sampler_desc* s,
                                             const pbrt_frame_samples_soa* out, const pbrt_strat_samples_soa* strat) {
    const char* why = "";
    int64_t n = 0;
    const pbrt_film_desc* f = c ? &c->host_scene.film : nullptr;
    if (int rc = pbrtstrat::check_samples_args(c != nullptr, f, d, s, out, strat, c && query_blocked(c), &n, &why))
        return set_err(c, rc, why);
    if (int rc = pbrtstrat::check_samples_supported(c->facts, c->knobs, *f, *d, *s, &why)) return set_err(c, rc, why);
    if (n == 0) return PBRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const pbrtfilm::Layout l = pbrtfilm::layout(*f, d->tile_size);
    const pbrtstrat::Plan p = pbrtstrat::plan(c->facts, c->knobs, *f, *d, *s);
    const int64_t npx = n / d->ns;
    launch_k(c, k_strat_pixels, dim3((unsigned)npx), dim3(kWave), (unsigned)p.lay.total, c->stream, c->d_camera.get(), p.rp,
             p.lay, c->d_jump.get(), l, pbrtfilm::pixels_before(l, d->tile_begin), npx, *out, *strat);
    return launched(c);
}

int pbrt_gpu_li_stratified_device(pbrt_gpu_ctx* c, const pbrt_li_desc* d, const pbrt_ray_soa* rays, const pbrt_rng_soa* rng,
                                  size_t n, const pbrt_radiance_soa* out, const pbrt_strat_soa* strat) {
    const char* why = "";
    if (int rc = pbrtstrat::check_li_args(c != nullptr, d, rays, rng, n, out, strat, c && query_blocked(c), &why))
        return set_err(c, rc, why);
    if (int rc = pbrtli::check_supported(*d, c->facts.rough_glass, &why)) return set_err(c, rc, why);
    if (int rc = li_distribution(c, d, n)) return rc;
    if (n == 0) return PBRT_OK;
    DevScene sc;
    if (int rc = query_begin(c, true, sc)) return rc;
    const pbrtli::KernelArgs ka =
        pbrtstrat::kernel_args(c->facts.non_matte, c->host_scene.n_nodes, c->mesh.n_nodes != 0, n, kLdsNodes);
    const LiStratKernel kern = li_strat_kernel(ka.kx, ka.depth);
    if (!kern) return set_err(c, PBRT_E_HIP, "no k_li_strat instantiation for depth " + std::to_string(ka.depth));
    launch_k(c, kern, dim3(ka.grid), dim3(kWave), 0, c->stream, sc, (int)d->max_depth, d->rr_threshold, (int64_t)n,
             *rays, *rng, *out, *strat, c->d_qrec.get());
    return launched(c);
}

int pbrt_gpu_film_add_device(pbrt_gpu_ctx* c, const pbrt_frame_desc* d, const pbrt_film_samples_soa* in,
                             double* film_device) {
    const char* why = "";
    int64_t n = 0;
    const pbrt_film_desc* f = c ? &c->host_scene.film : nullptr;
    if (int rc = pbrtfilm::check_frame(c != nullptr, f, d, PBRT_FILM_ADD_CLEAR, c && query_blocked(c), &n, &why))
        return set_err(c, rc, why);
    if (int rc = pbrtfilm::check_film_in(in, film_device, &why)) return set_err(c, rc, why);
    if (int rc = pbrtfilm::check_frame_supported(*f, *d, true, &why)) return set_err(c, rc, why);
    const bool clear = (d->flags & PBRT_FILM_ADD_CLEAR) != 0;
    if (n == 0 && !clear) return PBRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const pbrtfilm::Layout l = pbrtfilm::layout(*f, d->tile_size);
    const RenderParams rp = frame_params(c, l);
    const int64_t nt = d->tile_end - d->tile_begin;
    if (nt > 0) {
        if (int rc = c->d_fq_films.ensure(c, pbrtfilm::scratch_doubles(*f, d->tile_size, d->tile_begin, d->tile_end)))
            return rc;
        launch_k(c, pbrtfilm::lds_gather(c->knobs.film_add_lds, *f, d->tile_size) ? k_film_add_tiles<true> : k_film_add_tiles<false>,
                 dim3((unsigned)nt), dim3(kFilmThreads), 0, c->stream, c->d_film.get(), rp, l, (int64_t)d->tile_begin,
                 (int)d->ns, *in, c->d_fq_films.get());
    }
    const pbrtfilm::Rows rows = pbrtfilm::rows_touched(l, *f, d->tile_begin, d->tile_end, clear);
    const int64_t npx = (rows.y1 - rows.y0) * l.w;
    if (npx > 0)
        launch_k(c, k_film_add_merge, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, c->stream, c->d_film.get(), rp,
                 (int64_t)d->tile_begin, (int64_t)d->tile_end, rows.y0, rows.y1 - rows.y0, clear ? 1 : 0,
                 (const double*)c->d_fq_films.get(), film_device);
    return launched(c);
}

int pbrt_gpu_film_rgba8_device(pbrt_gpu_ctx* c, const double* film_device, int64_t w, int64_t h, uint8_t* rgba_device) {
    const char* why = "";
    if (int rc = pbrtfilm::check_rgba8(c != nullptr, film_device, w, h, rgba_device, c && query_blocked(c), &why))
        return set_err(c, rc, why);
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = w * h;
    launch_k(c, k_film_rgba8, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, film_device, n,
             (uint32_t*)rgba_device);
    return launched(c);
}

// (diagnostics) the capacity of film_add's scratch buffer in bytes: it changes only when the buffer is allocated anew
size_t pbrt_gpu_film_scratch_bytes(const pbrt_gpu_ctx* c) { return c ? c->d_fq_films.cap() * sizeof(double) : 0; }

int pbrt_gpu_query_status(pbrt_gpu_ctx* c, pbrt_query_record* out) {
    if (!c) return PBRT_E_INVALID;
    if (query_blocked(c)) return set_err(c, PBRT_E_INVALID, "a render is in flight on this context");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    QueryRec rec{0, ~0ull};
    if (c->d_qrec.get()) {
        HIPCHK(c, hipMemcpy(&rec, c->d_qrec.get(), sizeof(rec), hipMemcpyDeviceToHost));
        if (rec.panics) HIPCHK(c, query_rec_clear(c));
    }
    if (out) {
        out->panics = rec.panics;
        out->first_ray = rec.panics ? (int64_t)(rec.first >> 8) : -1;
        out->panic_kind = rec.panics ? (int32_t)(rec.first & 0xFF) : PBRT_PANIC_NONE;
        out->pad0 = 0;
    }
    if (rec.panics) return set_err(c, PBRT_E_REF_PANIC, "the Go reference panics on at least one ray");
    return PBRT_OK;
}

// ---- buffers the context owns (bookkeeping: query_buffers.h)
int pbrt_gpu_buffer_create(pbrt_gpu_ctx* c, size_t bytes, pbrt_gpu_buffer** out) {
    if (out) *out = nullptr;
    if (!c || !out || bytes == 0) return PBRT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    hipError_t e = hipSuccess;
    pbrt_gpu_buffer* b = pbrtq::list_create(c->qbufs, c, bytes, [&e](size_t nb) {
        void* p = nullptr;
        e = hipMalloc(&p, nb);
        return e == hipSuccess ? p : nullptr;
    });
    if (!b) return set_err(c, PBRT_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    *out = b;
    return PBRT_OK;
}
void* pbrt_gpu_buffer_ptr(const pbrt_gpu_buffer* b) { return b ? b->ptr : nullptr; }
size_t pbrt_gpu_buffer_size(const pbrt_gpu_buffer* b) { return b ? b->bytes : 0; }

static int buffer_copy(pbrt_gpu_buffer* b, size_t offset, void* host, size_t bytes, bool up) {
    if (!b || !b->ctx) return PBRT_E_INVALID;
    pbrt_gpu_ctx* c = b->ctx;
    if (!host && bytes) return set_err(c, PBRT_E_INVALID, "NULL host pointer");
    if (!pbrtq::range_ok(b->bytes, offset, bytes)) return set_err(c, PBRT_E_INVALID, "range outside the buffer");
    HIPCHK(c, hipSetDevice(c->device));
    char* dev = (char*)b->ptr + offset;
    if (bytes) {
        if (up) HIPCHK(c, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
        else HIPCHK(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PBRT_OK;
}
int pbrt_gpu_buffer_upload(pbrt_gpu_buffer* b, size_t offset, const void* host, size_t bytes) {
    return buffer_copy(b, offset, const_cast<void*>(host), bytes, true);
}
int pbrt_gpu_buffer_download(pbrt_gpu_buffer* b, size_t offset, void* host, size_t bytes) {
    return buffer_copy(b, offset, host, bytes, false);
}
void pbrt_gpu_buffer_destroy(pbrt_gpu_buffer* b) {
    if (!b || !b->ctx) return;
    pbrt_gpu_ctx* c = b->ctx;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);   // no query still reads or writes it
    pbrtq::list_destroy(c->qbufs, b, [](void* p) { (void)hipFree(p); });
}

}  // extern "C"

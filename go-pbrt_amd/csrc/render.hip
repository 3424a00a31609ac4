// render.hip — a context's life and its frame: scene upload (pbrt_gpu_create),
// the frame's stages (render_enqueue, pbrt_gpu_synchronize; what they launch: frame_route.h),
// the film's way out. The host side of the MI355X (gfx950) library by unit:
//   context.h          what every unit below needs: HIPCHK, DevBuf, pbrt_gpu_ctx,
//                      set_err, launch_k, dev_scene, with_slot, query_blocked
//   kernel_select.hip  the selectors (kernel_select.h: arguments in, the host
//                      pointer of that instantiation out) and the launch log's names
//   frame_route.h      the rules that decide what a frame launches, pure and HIP-free
//                      (render_params.h: what they hand the kernels): the desc's check,
//                      RenderParams, the route and its refusals, the LDS layouts, the
//                      chain and path launches' arithmetic, the buffers' carving
//   render.hip         create / destroy / cancel / last_error; prepare and the frame's
//                      stages (their HIP calls; their numbers are frame_route.h's),
//                      synchronize, render; film_download, pbrt_film_to_rgba8, the
//                      group's member view
//   queries.hip        everything a context answers between frames: ray queries,
//                      camera rays, Li / DirectLighting.Li / Path.Li by steps, a
//                      frame from public pieces, the context's buffers
//   diag.hip           include/pbrt_diag.h's read-outs: k_probe, counters, mesh,
//                      schedule records, launch log, build id, ABI sizes
//   group.hip          device groups over member contexts (group.h)
//   mesh_bvh.hip       the device LBVH build of the mesh extension
// The kernels are each family's own unit (k_*.hip; declarations in
// render_kernels.h, shared types and helpers in render_common.h). A frame's:
//   k_render_exact   EXACT mode: one lane per 16-px tile. The lane replays the
//                    tile's PCG32 stream exactly as pbrt.Render's worker does
//                    (integrator.go:228-289, 311-340): pixel loop, Stratified
//                    StartPixel, samples 1..spp-1, Path.Li / DirectLighting.Li,
//                    NaN guard, FilmTile.AddSample into the tile's film slot.
//   wave pipeline    k_wf_primary (bounce 1 per pixel), k_chain_ci (the
//                    tile's RNG-offset chain), k_paths_ci or the path
//                    wavefront k_pw_* (full paths), k_film (tile films);
//                    THROUGHPUT mode: k_mb_setup instead of the chain.
//                    More lights than k_paths_ci's LDS cache holds
//                    (kMaxCachedLights) run the path wavefront.
//   camera-start route  (PBRT_KERNEL_WAVE_CAM, opt-in) the wave pipeline for
//                    renders whose camera ray belongs to the sample (n_dims 0,
//                    or 1 with a thin lens): k_chain_cam, k_paths_cam,
//                    k_film_cam; THROUGHPUT mode: k_cam_setup instead of the chain;
//                    trees beyond kLdsNodes: k_chain_cam_stack, k_paths_cam_stack.
//   k_dl_*         DirectLighting: pixel-order StartPixel + jump-ahead, one
//                    lane per sample.
//   k_merge_film     Film.MergeFilmTile (film.go:115-132): per output pixel,
//                    RGBToXYZ of every covering tile film in tile-index order.
//
// Everything is float64 with -ffp-contract=off (bit parity with the Go
// reference). The scene is a few KB and is read through the scalar/vector L1.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <mutex>
#include <vector>

#include "../../include/pbrt_gpu.h"
#include "../../include/pbrt_diag.h"
#include "../../include/pbrt_scene.h"
#include "context.h"
#include "frame_route.h"
#include "kernel_select.h"
#include "scene_tables.h"
#include "schedule.h"

using namespace pbrt;
using namespace pbrtk;


// =============================================================== C ABI
// per-slot chain clocks of the last EXACT frame: durations (the schedule's
// input), and in diagnostics builds start and end clocks (pbrt_gpu_tile_clocks)
#ifdef PBRT_CI_DIAG
constexpr int kTickPlanes = 3;   // durations, start clocks, end clocks
#else
constexpr int kTickPlanes = 1;
#endif

DevScene dev_scene(const pbrt_gpu_ctx* c, bool with_dist) {
    DevScene s;
    s.shapes = c->d_shapes.get();
    s.materials = c->d_materials.get();
    s.prims = c->d_prims.get();
    s.nodes = c->d_nodes.get();
    s.order = c->d_order.get();
    s.fprims = c->d_fprims.get();
    s.lights = c->d_lights.get();
    s.camera = c->d_camera.get();
    s.film = c->d_film.get();
    s.dist = with_dist ? c->d_dist.get() : nullptr;
    s.n_prims = c->host_scene.n_prims;
    s.n_nodes = c->host_scene.n_nodes;
    s.n_lights = c->host_scene.n_lights;
    s.use_lds_nodes = 0;
    s.n_leaves = 0;
    for (int i = 0; i < c->host_scene.n_nodes; i++) s.n_leaves += c->h_node_prims[i] > 0;
    s.mesh = c->mesh.view();
    s.groups = c->d_groups.get();
    s.gmasks = c->d_gmasks.get();
    s.n_groups = c->n_groups;
    s.cancel = c->cancel.d_flag;
    s.cancel_seen = c->cancel.d_seen.get();
    // bvh_walk_dense: culling groups over a tree of one primitive per leaf, no meshes
    s.dense_ok = c->knobs.ci_dense && s.n_groups > 0 && s.n_leaves == s.n_prims && s.mesh.n_nodes == 0 &&
                 s.n_nodes <= kLdsNodes;
    return s;
}

namespace {

// the process cache's key (schedule.h) of a schedule key on this context's scene and device
uint64_t sched_cache_key(const pbrt_gpu_ctx* c, uint64_t skey) {
    uint64_t h = fnv_bytes(c->scene_hash, &skey, sizeof(skey));
    return fnv_bytes(h, &c->facts.n_simd, sizeof(c->facts.n_simd));   // the device's size shapes the split
}

std::vector<DevNode> dev_nodes(const pbrt_scene_desc* s) {
    std::vector<DevNode> v((size_t)(s->n_nodes > 0 ? s->n_nodes : 1));
    std::memset(v.data(), 0, v.size() * sizeof(DevNode));
    for (int i = 0; i < s->n_nodes; i++) {
        const pbrt_bvh_node& n = s->nodes[i];
        for (int k = 0; k < 3; k++) {
            v[i].bmin[k] = n.bmin[k];
            v[i].bmax[k] = n.bmax[k];
        }
        v[i].offset = n.offset;
        v[i].nprims_axis = (uint32_t)n.n_prims | ((uint32_t)n.axis << 16);
    }
    return v;
}

std::vector<DevPrim> dev_prims(const pbrt_scene_desc* s) {
    std::vector<DevPrim> v((size_t)(s->n_prims > 0 ? s->n_prims : 1));
    std::memset(v.data(), 0, v.size() * sizeof(DevPrim));
    for (int i = 0; i < s->n_prims; i++) {
        const pbrt_primitive_desc& p = s->prims[i];
        v[i].shape = s->shapes[p.shape];
        v[i].prim_to_world = p.prim_to_world;
        v[i].kind = p.kind;
        v[i].material = p.material;
        v[i].prim_identity = is_identity(p.prim_to_world.m) ? 1 : 0;
        v[i].fast = xf_fast_kind(p.prim_to_world.m_inv) | xf_fast_kind(v[i].shape.object_to_world.m_inv) << 8;
    }
    return v;
}

const PcgJump& pcg_jump_table() {
    static PcgJump J = [] {
        PcgJump t;
        pcg_jump_fill(t);   // pcg_jump.h
        return t;
    }();
    return J;
}

// sizeof of the device structs frame_route.h counts in
constexpr pbrtroute::Sizes kSizes{sizeof(ChainCache), sizeof(PixelRec), sizeof(PanicRec), sizeof(RrBranches),
                                  sizeof(PwPath),     sizeof(Spec),     sizeof(RingEnt)};
static_assert(pbrtroute::kDlMaxDepthX == 2 * kDlMaxLevels, "check_render's DirectLighting depth is k_dl_samples<kX>'s");

// Static LDS of the one-wave Matte k_chain_ci of this context's tree, the 3-waves/SIMD build
// (`multi`: the several-tiles-per-wave instantiation, whose static LDS differs); 0 on failure.
size_t ci_static_lds(const pbrt_gpu_ctx* c, bool multi) {
    hipFuncAttributes fa;
    const void* f = reinterpret_cast<const void*>(
        chain_kernel(1, c->facts.n_nodes <= kLdsNodes ? 0 : 64, false, 0, false, multi));
    return hipFuncGetAttributes(&fa, f) == hipSuccess ? fa.sharedSizeBytes : 0;
}

// The path wavefront (k_pw_*) over the batch's pixel records, in chunks (pbrtroute::pw_carve).
int paths_wavefront(pbrt_gpu_ctx* c, const DevScene& sc, int64_t sb, int64_t nb) {
    const RenderParams& rp = c->rp;
    const int64_t nrec = nb * c->wb.ppt, per = rp.spp - 1;
    const int nl = sc.n_lights;
    const int sort = c->knobs.pw_sort ? 1 : 0;
    const int n_keys = std::max(1, std::min(c->facts.n_materials, kPwMaxKeys));
    const int64_t ncnt = 3 + 2 * kPwMaxKeys;
    const pbrtroute::PwCarve pw = pbrtroute::pw_carve(c->knobs, c->facts, rp, kSizes, nrec, ncnt);
    const int64_t chunk = pw.chunk;
    if (const int rc = c->d_pw.ensure(c, pw.need)) return rc;
    unsigned char* p = c->d_pw.get();
    PwPath* paths = (PwPath*)(p + pw.paths);
    PwQueues qs;
    for (int i = 0; i < 3; i++) qs.q[i] = (uint32_t*)(p + pw.q[i]);
    qs.sorted = (uint32_t*)(p + pw.sorted);
    qs.cnt = (uint32_t*)(p + pw.cnt);
    qs.cap = pw.cap;
    Spec* ldc = (Spec*)(p + pw.ldc);
    int* ldp = (int*)(p + pw.ldp);
    unsigned long long* pkey = (unsigned long long*)(p + pw.pkey);
    const unsigned G = (unsigned)std::max<int64_t>(64, (int64_t)c->facts.n_simd * 8);   // grid-stride blocks
    HIPCHK(c, hipMemsetAsync(pkey, 0xFF, (size_t)nrec * 8, c->stream));
    const bool mb = rp.mode == PBRT_MODE_THROUGHPUT;
    const bool kx = c->facts.non_matte;   // Mirror / smooth Glass / OrenNayar: the kX instantiations
    for (int64_t r0 = 0; r0 < nrec; r0 += chunk) {
        const int64_t nr = std::min(chunk, nrec - r0);
        if (per > 0) {
            HIPCHK(c, hipMemsetAsync(qs.cnt, 0, (size_t)ncnt * 4, c->stream));
            if (nl > 0)
                launch_k(c, kx ? k_pw_cache<true> : k_pw_cache<false>,
                                   dim3((unsigned)((nr * nl + kWave - 1) / kWave)), dim3(kWave), 0,
                                   c->stream, sc, c->wb, r0, nr, ldc, ldp);
            auto start = kx ? (mb ? k_pw_start<true, true> : k_pw_start<false, true>)
                            : (mb ? k_pw_start<true> : k_pw_start<false>);
            launch_k(c, start, dim3((unsigned)((nr * per + kWave - 1) / kWave)), dim3(kWave), 0, c->stream,
                               sc, rp, c->wb, sb, r0, nr, ldc, ldp, paths, qs, pkey);
            for (int pass = 0; pass + 1 < rp.max_depth; pass++) {
                launch_k(c, c->mesh_only ? k_pw_trace<true> : k_pw_trace<false>, dim3(G), dim3(kWave), 0, c->stream, sc, rp, c->wb, paths, qs, 0,
                                   n_keys, pkey);
                if (sort && n_keys > 1) {
                    launch_k(c, k_pw_scan, dim3(1), dim3(1), 0, c->stream, qs, n_keys);
                    launch_k(c, k_pw_scatter, dim3(G / 4), dim3(256), 0, c->stream, paths, qs);
                }
                launch_k(c, kx ? k_pw_shade<true> : k_pw_shade<false>, dim3(G), dim3(kWave), 0, c->stream, sc,
                                   rp, c->wb, sb, paths, qs,
                                   sort && n_keys > 1 ? 1 : 0, pkey);
                launch_k(c, c->mesh_only ? k_pw_shadow<true> : k_pw_shadow<false>, dim3(G), dim3(kWave), 0, c->stream, sc, rp, c->wb, paths, qs, pkey);
            }
        }
        launch_k(c, k_pw_panics, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, c->stream, rp, c->wb, sb, r0,
                           nr, pkey, c->d_ctr.get());
    }
    HIPCHK(c, hipGetLastError());
    return PBRT_OK;
}

// The per-batch buffers of the wave routes (pbrtroute::wave_carve sizes the batch and places the arrays).
int wave_buffers(pbrt_gpu_ctx* c) {
    size_t free_b = 0, total_b = 0, hbm_free = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) hbm_free = free_b + c->d_wave.cap();
    const pbrtroute::WaveCarve wc = pbrtroute::wave_carve(c->knobs, c->facts, c->rp, kSizes, hbm_free);
    if (const int rc = c->d_wave.ensure(c, wc.need)) return rc;
    WaveBufs& wb = c->wb;
    unsigned char* p = c->d_wave.get();
    wb.prec = (PixelRec*)(p + wc.prec);
    wb.s1d = (double*)(p + wc.s1d);
    wb.memb = (uint64_t*)(p + wc.memb);
    wb.L = (double*)(p + wc.L);
    wb.rays = (uint32_t*)(p + wc.rays);
    wb.ppanic = (PanicRec*)(p + wc.ppanic);
    wb.tile_npx = (int32_t*)(p + wc.tile_npx);
    wb.rrb = wc.rrb >= 0 ? (RrBranches*)(p + wc.rrb) : nullptr;
    wb.ppt = wc.ppt;
    wb.s1d_stride = wc.s1d_stride;
    c->wave_batch = wc.batch;
    return PBRT_OK;
}

// A frame's decisions, all of them frame_route.h's: check the desc, derive its parameters, upload
// the light distribution, choose the route, lay out the chain kernels' LDS, size the buffers.
int prepare(pbrt_gpu_ctx* c, const pbrt_render_desc* rd) {
    using pbrtroute::Route;
    const pbrt_film_desc& f = c->host_scene.film;
    const pbrtroute::Refusal bad = pbrtroute::check_render(c->facts, f, rd);
    if (bad.code != PBRT_OK) return set_err(c, bad.code, bad.text);
    RenderParams& rp = c->rp;
    rp = pbrtroute::render_params(c->facts, c->knobs, f, *rd, c->lanes_per_wave);
    pbrt_distribution_desc& dist = c->host_dist;
    std::memset(&dist, 0, sizeof(dist));
    if (rd->integrator == PBRT_INTEGRATOR_PATH) {
        int rc = pbrt_scene_light_distribution(&c->host_scene, rd->light_strategy, &dist);
        if (rc != PBRT_OK) return set_err(c, rc, "unsupported light sample strategy");
        HIPCHK(c, hipMemcpyAsync(c->d_dist.get(), &dist, sizeof(dist), hipMemcpyHostToDevice, c->stream));
    }
    const pbrtroute::Routed r = pbrtroute::route(c->kernel_req, c->facts, c->knobs, *rd, rp, dist);
    if (r.refusal.code != PBRT_OK) return set_err(c, r.refusal.code, r.refusal.text);
    c->route = r.route;
    c->mesh_only = pbrtroute::mesh_only(c->facts);
    if (c->route == Route::Cam) {
        c->lay.Lcam = pbrtroute::layout_Lcam(rp);
    } else if (c->route != Route::Serial) {
        c->lay.L = pbrtroute::layout_L(rp);
        c->lay.Lci = pbrtroute::layout_Lci(rp);
        c->tiles_per_wave = pbrtroute::tiles_per_wave(c->lanes_per_wave_set, c->lanes_per_wave);
    }
    int rc;
    if (c->route != Route::Serial && rp.n_slots > 0 && (rc = wave_buffers(c)) != PBRT_OK) return rc;
    size_t nslot = (size_t)(rp.n_slots > 0 ? rp.n_slots : 1);
    if ((rc = c->d_films.ensure(c, nslot * (size_t)(rp.slot_w * rp.slot_h * 3)))) return rc;
    if ((rc = c->d_s1d.ensure(c, nslot * (size_t)(rp.ndims > 0 ? rp.ndims : 1) * (size_t)rp.spp)))
        return rc;
    if ((rc = c->d_panics.ensure(c, nslot))) return rc;
    if ((rc = c->d_out.ensure(c, (size_t)(rp.film_w * rp.film_h * 3)))) return rc;
    return PBRT_OK;
}

}  // namespace

extern "C" {

int pbrt_gpu_create(const pbrt_scene_desc* scene, const pbrt_gpu_opts* opts, pbrt_gpu_ctx** out) {
    if (!out) return PBRT_E_INVALID;
    *out = nullptr;
    int rc = validate_scene(scene);
    if (rc != PBRT_OK) return rc;
    auto* c = new pbrt_gpu_ctx();
    c->knobs = Knobs::from_env();
    c->device = (opts && opts->device >= 0) ? opts->device : -1;
    if (opts && opts->lanes_per_wave > 0 && opts->lanes_per_wave <= 64) {
        c->lanes_per_wave = opts->lanes_per_wave;
        c->lanes_per_wave_set = true;
    }
    if (opts && (opts->occupancy == 2 || opts->occupancy == 4 || opts->occupancy == 8)) c->min_waves = opts->occupancy;
    if (opts) c->occ_req = opts->occupancy;
    if (opts && (opts->kernel < PBRT_KERNEL_AUTO || opts->kernel > PBRT_KERNEL_WAVE_CAM)) {
        delete c;
        return PBRT_E_INVALID;
    }
    if (opts) c->kernel_req = opts->kernel;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        delete c;
        return PBRT_E_HIP;
    }
    if (c->device >= 0) {
        if (hipSetDevice(c->device) != hipSuccess) { delete c; return PBRT_E_HIP; }
    } else {
        (void)hipGetDevice(&c->device);
    }
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) {
            c->facts.n_simd = 4 * prop.multiProcessorCount;
            c->facts.lds_per_block = prop.sharedMemPerBlock;
            if (prop.maxSharedMemoryPerMultiProcessor > 0) c->facts.lds_per_cu = prop.maxSharedMemoryPerMultiProcessor;
        }
    }
    std::vector<uint32_t> order;
    if (!dev_order(scene, order)) {
        delete c;
        return PBRT_E_INVALID;
    }
    c->host_scene = *scene;
    c->scene_hash = scene_content_hash(scene);
    pbrtroute::scene_facts(*scene, c->facts);
    c->h_node_prims.resize((size_t)scene->n_nodes);
    for (int i = 0; i < scene->n_nodes; i++) c->h_node_prims[i] = scene->nodes[i].n_prims;
    c->host_scene.shapes = nullptr;
    c->host_scene.materials = nullptr;
    c->host_scene.prims = nullptr;
    c->host_scene.nodes = nullptr;
    c->host_lights.assign(scene->lights, scene->lights + scene->n_lights);
    c->host_scene.lights = c->host_lights.data();
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreate(&c->ev2) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_split, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
        pbrt_gpu_destroy(c);
        return PBRT_E_HIP;
    }

    if (hipHostMalloc((void**)&c->cancel.h_flag, sizeof(int), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void**)&c->cancel.d_flag, c->cancel.h_flag, 0) != hipSuccess) {
        pbrt_gpu_destroy(c);
        return PBRT_E_HIP;
    }
    __atomic_store_n(c->cancel.h_flag, 0, __ATOMIC_SEQ_CST);
    if ((rc = c->d_shapes.upload(c, scene->shapes, scene->n_shapes)) ||
        (rc = c->d_materials.upload(c, scene->materials, scene->n_materials)) ||
        (rc = c->d_prims.upload(c, scene->prims, scene->n_prims)) ||
        (rc = c->d_nodes.upload(c, dev_nodes(scene).data(), scene->n_nodes)) ||
        (rc = c->d_order.upload(c, order.data(), order.size())) ||
        (rc = c->d_fprims.upload(c, dev_prims(scene).data(), scene->n_prims)) ||
        (rc = c->d_lights.upload(c, scene->lights, scene->n_lights)) ||
        (rc = c->d_camera.upload(c, &scene->camera, 1)) || (rc = c->d_film.upload(c, &scene->film, 1)) ||
        (rc = c->d_dist.upload(c, nullptr, 1)) ||
        (rc = c->d_ctr.upload(c, nullptr, 1)) || (rc = c->cancel.d_seen.upload(c, nullptr, 1)) ||
        (rc = c->d_jump.upload(c, &pcg_jump_table(), 1))) {
        pbrt_gpu_destroy(c);
        return rc;
    }
    {   // leaf culling groups of the LDS-staged walk
        std::vector<double> gb;
        std::vector<uint32_t> gm;
        c->n_groups = cull_groups(c->knobs.cull_group, c->knobs.cull_min, scene, order, gb, gm);
        if (!c->knobs.cull_groups) c->n_groups = 0;   // PBRT_CULL_GROUPS=0: test every leaf (A/B)
        if (c->n_groups > 0 && ((rc = c->d_groups.upload(c, gb.data(), gb.size())) ||
                                (rc = c->d_gmasks.upload(c, gm.data(), gm.size())))) {
            pbrt_gpu_destroy(c);
            return rc;
        }
    }
    if (scene->n_meshes > 0) {   // triangle meshes: LBVH built on the device (mesh_bvh.hip)
        std::string err;
        rc = mesh_bvh_build(scene, c->stream, c->mesh, err, &c->log_aux);
        if (rc != PBRT_OK) {
            pbrt_gpu_destroy(c);
            return rc;
        }
    }
    c->host_scene.meshes = nullptr;
    c->facts.mesh = c->mesh.n_nodes != 0;
    *out = c;
    return PBRT_OK;
}

namespace {
int render_enqueue(pbrt_gpu_ctx* c, const pbrt_render_desc* rd, double* film_device);
}

int pbrt_gpu_render_async_into(pbrt_gpu_ctx* c, const pbrt_render_desc* rd, double* film_device) {
    if (!c) return PBRT_E_INVALID;
    // from here on this render is the one pbrt_gpu_cancel cancels: a cancel
    // that lands while prepare() sizes and allocates the buffers is kept
    c->cancel.reset(true);
    if (rd) c->ov.last_rd = *rd;   // kept for a re-render (pbrt_gpu_synchronize)
    c->ov.last_film_device = film_device;
    const int rc = render_enqueue(c, rd, film_device);
    if (rc != PBRT_OK) c->cancel.reset(false);   // nothing was launched (or the launch failed): no render is in flight
    return rc;
}

namespace {
// ---- The frame's stages, in the order render_enqueue runs them. Each is a plain
// function over the context, the scene view and the batch.

// A tree is staged in LDS while n_nodes <= kLdsNodes (stage_nodes' own test). Beyond, it is walked
// with the [64] stack: the k_*_cam_stack kernels and the kDepth = 64 chains. Those are compiled
// with use_lds_nodes = 0 (no staged walk): select them by this test only, never for a tree the
// other kernels would stage.

// The chain launch's schedule: workgroup b runs slot order[b] (null: launch order) and records its
// chain time in ticks (null: not recorded). learned: the order comes from measured chain times.
struct Schedule {
    const uint32_t* order = nullptr;
    uint32_t* ticks = nullptr;
    bool learned = false;
};
// One batch of a wave route: the frame's tile slots [sb, sb + nb), and its chain stage's schedule.
struct Batch {
    int64_t bi, sb, nb;
    Schedule sched;
};

// Three events per batch (c->bev): before the chain, after the chain, after the paths.
int ensure_batch_events(pbrt_gpu_ctx* c) {
    c->n_batches = (int)((c->rp.n_slots + c->wave_batch - 1) / c->wave_batch);
    while ((int)c->bev.size() < 3 * c->n_batches) {
        hipEvent_t e;
        HIPCHK(c, hipEventCreate(&e));
        c->bev.push_back(e);
    }
    return PBRT_OK;
}

// The schedule of a one-batch frame's chain launch (k_chain_ci, k_chain_cam) under `key`: grows
// the tick and order buffers, takes the context's own measured order for the key or else the
// process cache's (a fresh context: another context's measured order for this scene; with
// cache_heavy_k its heavy count too), uploads it, and arms pbrt_gpu_synchronize's tick readback.
int chain_schedule(pbrt_gpu_ctx* c, uint64_t key, int64_t nb, bool cache_heavy_k, Schedule& s) {
    int rc;
    if ((rc = c->sched.d_ticks.ensure(c, (size_t)nb * kTickPlanes)) ||
        (rc = c->sched.d_slot_order.ensure(c, (size_t)nb)))
        return rc;
    auto known = [&] { return c->sched.order_key == key && (int64_t)c->sched.h_slot_order.size() == nb; };
    bool cached = false;
    SchedEntry e;
    if (!known() && c->knobs.ci_order_cache && sched_cache_get(sched_cache_key(c, key), nb, e)) {
        c->sched.h_slot_order = std::move(e.order);
        if (cache_heavy_k) c->sched.heavy_k = e.heavy_k;
        c->sched.order_key = key;
        cached = true;
    }
    if (known()) {
        c->sched.src = cached ? PBRT_SCHED_CACHED : PBRT_SCHED_LEARNED;
        HIPCHK(c, hipMemcpyAsync(c->sched.d_slot_order.get(), c->sched.h_slot_order.data(), sizeof(uint32_t) * (size_t)nb,
                                 hipMemcpyHostToDevice, c->stream));
        s.order = c->sched.d_slot_order.get();
        s.learned = true;
    }
    s.ticks = c->sched.d_ticks.get();
    c->sched.ticks_pending = true;
    c->sched.ticks_key = key;
    c->sched.ticks_n = nb;
    return PBRT_OK;
}

// The cold-frame probe: no measured order for this configuration yet, so estimate one from the
// bounce-1 records (k_tile_cost), sort the keys and write the order to d_slot_order.
int probe_order(pbrt_gpu_ctx* c, const DevScene& sc, const Batch& b) {
    int64_t npad = 2048;
    while (npad < b.nb) npad <<= 1;
    int rc;
    if ((rc = c->sched.d_cost.ensure(c, 4 * (size_t)npad)) ||
        (rc = c->sched.d_cost_keys.ensure(c, (size_t)npad)))
        return rc;
    HIPCHK(c, hipMemsetAsync(c->sched.d_cost_keys.get(), 0xFF, sizeof(uint64_t) * (size_t)npad, c->stream));
    launch_k(c, c->facts.non_matte ? k_tile_cost<true> : k_tile_cost<false>, dim3((unsigned)b.nb), dim3(kWave), 0, c->stream,
             with_slot(sc, 0), c->rp, c->wb, b.sb, b.nb, c->sched.d_cost.get(), c->sched.d_cost_keys.get());
    bitonic_sort_u64(c->sched.d_cost_keys.get(), (uint32_t)npad, c->stream, &c->log_frame);
    launch_k(c, k_order_of_keys, dim3((unsigned)((b.nb + 255) / 256)), dim3(256), 0, c->stream, c->sched.d_cost_keys.get(), b.nb,
             c->sched.d_slot_order.get());
    c->sched.probed = true;
    c->sched.src = PBRT_SCHED_PROBE;
    c->sched.cost_n = b.nb;
    return PBRT_OK;
}

// The end of a batch on both routes: the tile films (the camera route with n_dims == 0:
// k_film_cam's per-sample footprints; else k_film), then k_panic_reduce.
void launch_films(pbrt_gpu_ctx* c, const Batch& b) {
    const RenderParams& rp = c->rp;
    if (c->route == pbrtroute::Route::Cam && rp.ndims == 0)
        launch_k(c, rp.mode == PBRT_MODE_THROUGHPUT ? k_film_cam<true> : k_film_cam<false>, dim3((unsigned)b.nb),
                 dim3(kFilmThreads), 0, c->stream, c->d_film.get(), rp, c->wb, b.sb, b.nb, c->d_films.get(), c->cancel.d_seen.get(),
                 c->d_ctr.get());
    else
        launch_k(c, k_film, dim3((unsigned)b.nb), dim3(kFilmThreads), (unsigned)film_lds_bytes(rp), c->stream,
                 c->d_film.get(), rp, c->wb, b.sb, b.nb, c->d_films.get(), c->cancel.d_seen.get(), c->d_ctr.get());
    launch_k(c, k_panic_reduce, dim3((unsigned)((b.nb + 255) / 256)), dim3(256), 0, c->stream, c->wb, b.sb, b.nb,
             c->d_panics.get(), c->d_ctr.get());
}

// The camera-start route (PBRT_KERNEL_WAVE_CAM), per batch on the one stream:
// k_chain_cam (EXACT; THROUGHPUT: k_cam_setup), k_paths_cam, then the tile films
// (k_film_cam's per-sample footprints with n_dims == 0, else k_film) and
// k_panic_reduce. No kernel waits on another's progress (no k_gate). A context
// that has rendered the configuration launches the chain heaviest tile first
// (the chain times of its last frame); a cold frame runs in launch order: there
// is no bounce-1 record for k_tile_cost to probe from.
int enqueue_cam(pbrt_gpu_ctx* c, const DevScene& sc) {
    const RenderParams& rp = c->rp;
    const bool mb = rp.mode == PBRT_MODE_THROUGHPUT, stack = c->facts.n_nodes > kLdsNodes;
    int rc = ensure_batch_events(c);
    if (rc != PBRT_OK) return rc;
    c->ov.done = 0;
    c->sched.probed = false;   // this route never probes
    for (int64_t sb = 0, bi = 0; sb < rp.n_slots; sb += c->wave_batch, bi++) {
        Batch b{bi, sb, std::min<int64_t>(c->wave_batch, rp.n_slots - sb)};
        const int64_t nb = b.nb, nrec = nb * c->wb.ppt;
        HIPCHK(c, hipEventRecord(c->bev[3 * bi + 0], c->stream));
        if (mb) {
            const int64_t blocks = rp.ndims > 0 ? nrec : (nrec + kWave - 1) / kWave;
            launch_k(c, k_cam_setup, dim3((unsigned)blocks), dim3(kWave), (unsigned)c->lay.Lcam.staging, c->stream,
                     with_slot(sc, 4), rp, c->lay.Lcam, c->d_jump.get(), c->wb, sb, nb);
        } else {
            if (c->n_batches == 1 && c->knobs.ci_order) {
                // key -1: no k_chain_ci launch has this wave count. A cached entry's heavy count is the
                // chain route's: there is no split here, every slot runs 1 wave at 3 waves/SIMD
                if ((rc = chain_schedule(c, pbrtroute::schedule_key(rp, -1), nb, false, b.sched)) != PBRT_OK) return rc;
                if (kTickPlanes > 1)  // diagnostics builds read start / end clocks this kernel does not record
                    HIPCHK(c, hipMemsetAsync(c->sched.d_ticks.get(), 0, sizeof(uint32_t) * (size_t)nb * kTickPlanes, c->stream));
                c->sched.h_slot_kw.assign((size_t)nb, (uint8_t)1);
                c->sched.ci_wps = 3;
            }
            launch_k(c, stack ? k_chain_cam_stack : k_chain_cam, dim3((unsigned)nb), dim3(kWave),
                     (unsigned)c->lay.Lcam.total, c->stream, with_slot(sc, 2), rp, c->lay.Lcam, c->d_jump.get(), c->wb, sb, nb,
                     b.sched.order, b.sched.ticks);
        }
        HIPCHK(c, hipEventRecord(c->bev[3 * bi + 1], c->stream));
        if (rp.spp > 1) {
            const int pp = pbrtroute::cam_pixels_per_wave(rp.spp);
            const PathsCamKernel kern = paths_cam_kernel(pp, mb, stack);
            if (!kern) return set_err(c, PBRT_E_HIP, "no k_paths_cam instantiation for P = " + std::to_string(pp));
            launch_k(c, kern, dim3((unsigned)((nrec + pp - 1) / pp)), dim3(kWave), 0, c->stream,
                     with_slot(sc, mb ? 5 : 3), rp, c->wb, sb, nrec, c->d_ctr.get());
        }
        HIPCHK(c, hipEventRecord(c->bev[3 * bi + 2], c->stream));
        launch_films(c, b);
    }
    return PBRT_OK;
}

// k_wf_primary: bounce 1 of every pixel of the batch.
void launch_primary(pbrt_gpu_ctx* c, const DevScene& sc, const Batch& b) {
    launch_k(c, c->facts.non_matte ? k_wf_primary<true> : k_wf_primary<false>,
             dim3((unsigned)((b.nb * c->wb.ppt + kWave - 1) / kWave)), dim3(kWave), 0, c->stream, with_slot(sc, 1),
             c->rp, c->wb, b.sb, b.nb);
}

// THROUGHPUT: k_mb_setup (StartPixel + bounce 1 per pixel) instead of the chain.
void launch_mb_setup(pbrt_gpu_ctx* c, const DevScene& sc, const Batch& b) {
    launch_k(c, c->facts.non_matte ? k_mb_setup<true> : k_mb_setup<false>, dim3((unsigned)(b.nb * c->wb.ppt)), dim3(kWave),
             (unsigned)c->lay.L.total, c->stream, with_slot(sc, 4), c->rp, c->lay.L, c->d_jump.get(), c->wb, b.sb, b.nb);
}

// k_paths_ci (lane-refill paths) over n slots of the batch on stream st; ord: the slots' order,
// else slots 0 .. n - 1. mb: the THROUGHPUT instantiation (kMB) and its counter slot.
int launch_paths(pbrt_gpu_ctx* c, const DevScene& sc, const Batch& b, bool mb, const uint32_t* ord, int64_t n,
                 hipStream_t st) {
    const RenderParams& rp = c->rp;
    const int pp = pbrtroute::paths_ci_pixels(c->knobs, c->facts);
    const int sl = pbrtroute::paths_ci_s1d_lds(c->knobs, rp, pp) ? 1 : 0;
    const PathsCiKernel kern = paths_ci_kernel(pp, mb, c->facts.non_matte);
    const int lds = paths_ci_lds(pp, sl * rp.ndims * rp.spp);
    if (!kern || lds < 0)
        return set_err(c, PBRT_E_HIP, "no k_paths_ci instantiation for P = " + std::to_string(pp) +
                                          (c->facts.non_matte ? ", kX" : ""));
    const int64_t groups = pbrtroute::paths_ci_groups(c->wb.ppt, pp, n, ord != nullptr);
    launch_k(c, kern, dim3((unsigned)groups), dim3(kWave), (unsigned)lds, st, with_slot(sc, mb ? 5 : 3), rp, c->wb,
             b.sb, n * c->wb.ppt, c->d_ctr.get(), sl, ord);
    return PBRT_OK;
}

// One k_chain_ci launch of n workgroups at w waves per tile on stream st, workgroup i on slot
// ord[i] (identity if null); prog: the completion record of the overlapped path stage, or null.
// nps_allowed: the caller's leave for next-pixel speculation. pbrtroute::chain_launch chooses the
// instantiation and its numbers. Sets c->sched.ci_wps for a one-wave launch (pbrt_gpu_synchronize's
// heavy threshold reads it).
int launch_ci(pbrt_gpu_ctx* c, const DevScene& sc, const Batch& b, int w, int64_t n, const uint32_t* ord,
              hipStream_t st, uint32_t* prog, bool nps_allowed) {
    const pbrtroute::ChainLaunch l =
        pbrtroute::chain_launch(c->knobs, c->facts, c->rp, c->lay.Lci, kSizes, c->tiles_per_wave, c->mesh_only, w, n,
                                nps_allowed, [c](bool multi) { return ci_static_lds(c, multi); });
    RenderParams rpl = c->rp;
    rpl.ci_nps = l.nps;
    if (l.ci_wps) c->sched.ci_wps = l.ci_wps;
    const ChainKernel kern = chain_kernel(l.w, l.depth, l.kx, l.eu, l.window, l.multi);
    if (!kern)
        return set_err(c, PBRT_E_HIP, "no k_chain_ci instantiation for " + std::to_string(w) + " waves, walk " +
                                          std::to_string(l.depth) + (l.kx ? ", kX" : "") + (l.multi ? ", multi" : ""));
    launch_k(c, kern, dim3(l.grid), dim3(l.block), l.lds, st, with_slot(sc, 2), rpl, l.lay, c->d_jump.get(), c->wb, b.sb,
             b.nb, l.lanes_per_tile, l.ring, c->d_ctr.get(), l.per_tile ? ord : nullptr,
             l.per_tile ? b.sched.ticks : nullptr, l.stride, prog);
    return PBRT_OK;
}

using pbrtroute::Split;

// PBRT_PATHS_OVERLAP (a learned frame, one tile per workgroup): the completion-driven path stage.
//  - the heavy launch on the main stream (normal priority);
//  - the light launch on stream3 (high priority: it wins every slot that frees
//    while it has workgroups left), behind a k_gate that opens once every heavy
//    workgroup has started, so it never delays a heavy tile's start;
//  - the path stage on stream2 (normal priority): chunks of the tiles in their
//    chains' completion order (k_chain_ci's completion list), each behind a k_gate
//    that opens when its tiles' chains have ended. The chunks halve (1/2, 1/4, ...
//    of the tiles; the last 1/2^(K-1)), so most path work is queued while the
//    chains run and takes the slots they free once no chain workgroup waits.
// Without a split the one chain launch goes on stream3 (its workgroups win the slots the path
// chunks also wait for). Progress-driven, not timed (it replaces round 5's timed wait); only the
// schedule changes, never a result.
// overlap_arm: stream3 and its events (created on first use), the progress record (layout at
// kProgHead) grown and reset, and ev_split on the main stream, which every other stream waits for.
int overlap_arm(pbrt_gpu_ctx* c, int64_t nb) {
    if (!c->ov.stream3) {
        int least = 0, greatest = 0;
        HIPCHK(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(c, hipStreamCreateWithPriority(&c->ov.stream3, hipStreamNonBlocking, greatest));
        HIPCHK(c, hipEventCreateWithFlags(&c->ov.ev_l2, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ov.ev_p1, hipEventDisableTiming));
    }
    const int rc = c->ov.d_prog.ensure(c, (size_t)(nb + kProgHead));
    if (rc != PBRT_OK) return rc;
    HIPCHK(c, hipMemsetAsync(c->ov.d_prog.get(), 0, kProgHead * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->ov.d_prog.get() + kProgHead, 0xFF, sizeof(uint32_t) * (size_t)nb, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_split, c->stream));
    return PBRT_OK;
}
// the path chunks on stream2, each behind its k_gate; ev_p1 when the last is queued
int launch_path_chunks(pbrt_gpu_ctx* c, const DevScene& sc, const Batch& b) {
    HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_split, 0));
    for (int64_t s0 = 0, j = 0; s0 < b.nb; j++) {
        const int64_t e0 = pbrtroute::path_chunk_end(b.nb, s0, j, c->knobs.paths_overlap);
        launch_k(c, k_gate, dim3(1), dim3(kWave), 0, c->stream2, c->ov.d_prog.get(), (uint32_t)s0, (uint32_t)e0, c->d_ctr.get());
        const int rc = launch_paths(c, sc, b, false, c->ov.d_prog.get() + kProgHead + s0, e0 - s0, c->stream2);
        if (rc != PBRT_OK) return rc;
        s0 = e0;
    }
    HIPCHK(c, hipEventRecord(c->ov.ev_p1, c->stream2));
    return PBRT_OK;
}
// the light launch of an overlapped split on stream3, behind its k_gate; ev_l2 when it is queued.
// PBRT_GATE_HOLD: it waits for the whole path stage (ev_p1) instead of ev_split
int launch_light_gated(pbrt_gpu_ctx* c, const DevScene& sc, const Batch& b, const Split& sp) {
    HIPCHK(c, hipStreamWaitEvent(c->ov.stream3, c->knobs.gate_hold ? c->ov.ev_p1 : c->ev_split, 0));
    launch_k(c, k_gate, dim3(1), dim3(kWave), 0, c->ov.stream3, c->ov.d_prog.get(), (uint32_t)sp.heavy, (uint32_t)sp.heavy,
             c->d_ctr.get());
    const int rc = launch_ci(c, sc, b, sp.light_w, b.nb - sp.heavy, b.sched.order + sp.heavy, c->ov.stream3, c->ov.d_prog.get(), true);
    if (rc != PBRT_OK) return rc;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ov.ev_l2, c->ov.stream3));
    return PBRT_OK;
}

// The four ways of issuing the chain stage. 1: unsplit, one launch on the main stream (chain_stage).
// 2: plain split, the heavy launch on the main stream and the light one on stream2.
int chain_split(pbrt_gpu_ctx* c, const DevScene& sc, const Batch& b, const Split& sp) {
    HIPCHK(c, hipEventRecord(c->ev_split, c->stream));
    int rc = launch_ci(c, sc, b, sp.heavy_w, sp.heavy, b.sched.order, c->stream, nullptr, sp.light_kw);
    if (rc != PBRT_OK) return rc;
    HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_split, 0));
    rc = launch_ci(c, sc, b, sp.light_w, b.nb - sp.heavy, b.sched.order + sp.heavy, c->stream2, nullptr, true);
    if (rc != PBRT_OK) return rc;
    HIPCHK(c, hipEventRecord(c->ev_join, c->stream2));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    return PBRT_OK;
}
// 3: overlapped split on streams 0, 3 and 2 (after overlap_arm). PBRT_GATE_HOLD queues the path
// chunks before the light launch.
int chain_split_overlap(pbrt_gpu_ctx* c, const DevScene& sc, const Batch& b, const Split& sp) {
    int rc = launch_ci(c, sc, b, sp.heavy_w, sp.heavy, b.sched.order, c->stream, c->ov.d_prog.get(), sp.light_kw);
    if (rc != PBRT_OK) return rc;
    HIPCHK(c, hipGetLastError());   // the gates below wait for these workgroups
    rc = c->knobs.gate_hold ? launch_path_chunks(c, sc, b) : launch_light_gated(c, sc, b, sp);
    if (rc != PBRT_OK) return rc;
    rc = c->knobs.gate_hold ? launch_light_gated(c, sc, b, sp) : launch_path_chunks(c, sc, b);
    if (rc != PBRT_OK) return rc;
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ov.ev_l2, 0));
    c->ov.done = b.nb;
    return PBRT_OK;
}
// 4: unsplit with overlap: the one chain launch on stream3, the path chunks on stream2 (after overlap_arm).
int chain_unsplit_overlap(pbrt_gpu_ctx* c, const DevScene& sc, const Batch& b, int kw) {
    HIPCHK(c, hipStreamWaitEvent(c->ov.stream3, c->ev_split, 0));
    int rc = launch_ci(c, sc, b, kw, b.nb, b.sched.order, c->ov.stream3, c->ov.d_prog.get(), true);
    if (rc != PBRT_OK) return rc;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ov.ev_l2, c->ov.stream3));
    if ((rc = launch_path_chunks(c, sc, b)) != PBRT_OK) return rc;
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ov.ev_l2, 0));
    c->ov.done = b.nb;
    return PBRT_OK;
}

// The EXACT Path chain stage of a batch: k_wf_primary, the schedule, the split decision, then the
// k_chain_ci launches in one of the four ways above.
int chain_stage(pbrt_gpu_ctx* c, const DevScene& sc, Batch& b) {
    const RenderParams& rp = c->rp;
    const int G = c->tiles_per_wave;
    Schedule& s = b.sched;
    int rc;
    launch_primary(c, sc, b);
    const int kw = pbrtroute::ci_waves(c->knobs, c->facts, G, b.nb);
    if ((kw > 1 || G == 1) && c->n_batches == 1 && c->knobs.ci_order) {
        // keyed by the waves per tile; a cached entry brings its heavy count; a frame without a
        // measured order runs the cold-frame probe
        if ((rc = chain_schedule(c, pbrtroute::schedule_key(rp, kw), b.nb, true, s)) != PBRT_OK) return rc;
        c->sched.probed = false;
        if (!s.order && c->knobs.ci_probe && b.nb <= (int64_t)1 << 24) {
            if ((rc = probe_order(c, sc, b)) != PBRT_OK) return rc;
            s.order = c->sched.d_slot_order.get();
        }
    }
    const Split sp = pbrtroute::ci_split(c->knobs, c->facts, c->lay.Lci, kSizes, c->mesh_only, b.nb, kw, s.learned, G,
                                         c->sched.heavy_k, [c](bool multi) { return ci_static_lds(c, multi); });
    c->sched.last_heavy = sp.heavy;
    if (s.ticks) {   // label every slot with the waves it actually runs at
        c->sched.h_slot_kw.assign((size_t)b.nb, (uint8_t)(sp.heavy > 0 ? sp.light_w : kw));
        for (int64_t i = 0; i < sp.heavy; i++) c->sched.h_slot_kw[c->sched.h_slot_order[(size_t)i]] = (uint8_t)sp.heavy_w;
    }
    // the completion-driven path stage takes EXACT k_paths_ci (path_stage's last case) and a learned order
    const bool paths_ci_exact = !pbrtroute::paths_on_wavefront(c->knobs, c->facts);
    const bool ov_ok = c->knobs.paths_overlap > 0 && paths_ci_exact && s.learned && !c->ov.retry && c->ov.stalls < 2;
    const bool overlap = sp.heavy > 0 && ov_ok;
    // no split: the completion list needs one tile per workgroup
    const bool overlap1 = sp.heavy == 0 && ov_ok && c->knobs.paths_overlap_all && (kw > 1 || G == 1);
    if ((overlap || overlap1) && (rc = overlap_arm(c, b.nb)) != PBRT_OK) return rc;
    if (overlap1) return chain_unsplit_overlap(c, sc, b, kw);
    if (overlap) return chain_split_overlap(c, sc, b, sp);
    if (sp.heavy > 0) return chain_split(c, sc, b, sp);
    return launch_ci(c, sc, b, kw, b.nb, s.order, c->stream, nullptr, true);
}

// The path stage of a batch, after its chain stage.
int path_stage(pbrt_gpu_ctx* c, const DevScene& sc, const Batch& b) {
    const RenderParams& rp = c->rp;
    const bool mb = c->route == pbrtroute::Route::Throughput;
    if (c->route == pbrtroute::Route::DirectLighting) {
        const int64_t nrec = b.nb * c->wb.ppt;
        if (rp.spp > 1)
            launch_k(c, c->facts.non_matte ? k_dl_samples<true> : k_dl_samples<false>,
                     dim3((unsigned)std::min<int64_t>((nrec * (rp.spp - 1) + kWave - 1) / kWave, (int64_t)c->facts.n_simd * 64)),
                     dim3(kWave), 0, c->stream, with_slot(sc, 3), rp, c->wb, b.sb, nrec);
        launch_k(c, k_dl_panics, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, c->stream, rp, c->wb, b.sb, nrec,
                 c->d_ctr.get());
        return PBRT_OK;
    }
    if (pbrtroute::paths_on_wavefront(c->knobs, c->facts)) {
        if (mb) launch_mb_setup(c, sc, b);
        return paths_wavefront(c, with_slot(sc, mb ? 5 : 3), b.sb, b.nb);
    }
    if (mb) {   // setup, then lane-refill paths
        launch_mb_setup(c, sc, b);
        return launch_paths(c, sc, b, true, nullptr, b.nb, c->stream);
    }
    if (c->ov.done > 0) {   // the completion-driven path stage (stream2) ends the chain stage
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ov.ev_p1, 0));
        return PBRT_OK;
    }
    return launch_paths(c, sc, b, false, nullptr, b.nb, c->stream);
}

// The wave pipeline (DirectLighting, THROUGHPUT, EXACT Path on k_chain_ci), per batch: the chain
// stage, the path stage, the tile films.
int enqueue_wave(pbrt_gpu_ctx* c, const DevScene& sc) {
    using pbrtroute::Route;
    const RenderParams& rp = c->rp;
    int rc = ensure_batch_events(c);
    if (rc != PBRT_OK) return rc;
    for (int64_t sb = 0, bi = 0; sb < rp.n_slots; sb += c->wave_batch, bi++) {
        Batch b{bi, sb, std::min<int64_t>(c->wave_batch, rp.n_slots - sb)};
        HIPCHK(c, hipEventRecord(c->bev[3 * bi + 0], c->stream));
        c->ov.done = 0;
        if (c->route == Route::DirectLighting) {
            launch_primary(c, sc, b);
            unsigned lds = 0;
            const ChainLayout lw = pbrtroute::ci_layout(c->lay.Lci, 1, 1, lds, kSizes.chain_cache);
            launch_k(c, k_dl_setup, dim3((unsigned)b.nb), dim3(kWave), lds, c->stream, sc, rp, lw, c->d_jump.get(), c->wb,
                     sb, b.nb);
        } else if (c->route == Route::Chain) {   // (THROUGHPUT has no offset chain: every sample's stream is known up front)
            if ((rc = chain_stage(c, sc, b)) != PBRT_OK) return rc;
        }
        HIPCHK(c, hipEventRecord(c->bev[3 * bi + 1], c->stream));
        if ((rc = path_stage(c, sc, b)) != PBRT_OK) return rc;
        HIPCHK(c, hipEventRecord(c->bev[3 * bi + 2], c->stream));
        launch_films(c, b);
    }
    return PBRT_OK;
}

int render_enqueue(pbrt_gpu_ctx* c, const pbrt_render_desc* rd, double* film_device) {
    c->log_frame.clear();
    struct InFrame {   // the launches until this function returns are the frame's
        pbrt_gpu_ctx* c;
        ~InFrame() { c->in_frame = false; }
    } in_frame{c};
    c->in_frame = true;
    HIPCHK(c, hipSetDevice(c->device));
    c->t_start = std::chrono::steady_clock::now();
    int rc = prepare(c, rd);
    if (rc != PBRT_OK) return rc;
    const RenderParams& rp = c->rp;
    double* out = film_device ? film_device : c->d_out.get();
    c->film_target = out;
    c->sched.last_heavy = 0;
    c->sched.src = PBRT_SCHED_LAUNCH_ORDER;
    HIPCHK(c, hipMemsetAsync(c->d_ctr.get(), 0, sizeof(Counters), c->stream));
    HIPCHK(c, hipMemsetAsync(c->cancel.d_seen.get(), 0, sizeof(int), c->stream));
    if (rp.n_slots > 0) HIPCHK(c, hipMemsetAsync(c->d_panics.get(), 0, sizeof(PanicRec) * (size_t)rp.n_slots, c->stream));
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    if (rp.n_slots > 0) {
        DevScene sc = dev_scene(c, rd->integrator == PBRT_INTEGRATOR_PATH);
        c->last_kernel = pbrtroute::last_kernel(c->route);
        if (c->route != pbrtroute::Route::Serial) {
            if ((rc = c->route == pbrtroute::Route::Cam ? enqueue_cam(c, sc) : enqueue_wave(c, sc)) != PBRT_OK) return rc;
        } else {
            c->n_batches = 0;
            const int64_t blocks = (rp.n_slots + rp.lanes_per_wave - 1) / rp.lanes_per_wave;
            const SerialKernel kern = serial_kernel(c->min_waves);
            if (!kern)
                return set_err(c, PBRT_E_HIP, "no k_render_exact instantiation for occupancy " + std::to_string(c->min_waves));
            launch_k(c, kern, dim3((unsigned)blocks), dim3(kWave), 0, c->stream, with_slot(sc, 6), rp, c->d_films.get(),
                     c->d_s1d.get(), c->d_panics.get(), c->d_ctr.get());
        }
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    int64_t npx = rp.film_w * rp.film_h;
    launch_k(c, k_merge_film, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, c->stream, c->d_film.get(), rp,
             c->d_films.get(), out, c->cancel.d_seen.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev2, c->stream));
    c->rendered = true;
    return PBRT_OK;
}
}  // namespace

int pbrt_gpu_render_async(pbrt_gpu_ctx* c, const pbrt_render_desc* rd) {
    return pbrt_gpu_render_async_into(c, rd, nullptr);
}

int pbrt_gpu_synchronize(pbrt_gpu_ctx* c, pbrt_gpu_stats* stats) {
    if (!c) return PBRT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const hipError_t se = hipStreamSynchronize(c->stream);
    const bool cancelled = c->cancel.reset(false);   // the render has ended: its cancel flag dies with it
    HIPCHK(c, se);
    if (cancelled) {   // the kernels stopped early: the film and the schedule feedback are not valid
        c->sched.ticks_pending = false;
        c->rendered = false;
        if (stats) {
            std::memset(stats, 0, sizeof(*stats));
            stats->kernel = c->last_kernel;
            stats->total_ms =
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c->t_start).count();
        }
        return set_err(c, PBRT_E_CANCELLED, "cancelled by pbrt_gpu_cancel");
    }
    Counters ctr;
    HIPCHK(c, hipMemcpy(&ctr, c->d_ctr.get(), sizeof(ctr), hipMemcpyDeviceToHost));
    if (ctr.gate_stall) {
        // the completion-driven path stage's gates saw the chains stand still
        // (k_gate): the film misses path work. Render the frame again with the path
        // stage after the chains; the chains replay the same streams, so the
        // result is the one an overlapped frame gives.
        if (++c->ov.stalls == 2)
            std::fprintf(stderr, "pbrt: k_gate stalled twice (kernels serialised across streams, e.g. by a "
                                 "counter-collecting profiler): the path stage now runs after the chains\n");
        c->ov.retry = true;
        const int rr = render_enqueue(c, &c->ov.last_rd, c->ov.last_film_device);
        c->ov.retry = false;
        if (rr != PBRT_OK) return rr;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(&ctr, c->d_ctr.get(), sizeof(ctr), hipMemcpyDeviceToHost));
        if (ctr.gate_stall) return set_err(c, PBRT_E_HIP, "k_gate stalled without the overlap");
    } else if (c->ov.done > 0) {
        c->ov.stalls = 0;
    }
    float ms = 0, ms_merge = 0;
    (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
    (void)hipEventElapsedTime(&ms_merge, c->ev1, c->ev2);
    int rc = PBRT_OK;
    pbrt_gpu_stats st;
    std::memset(&st, 0, sizeof(st));
    st.tiles_rendered = (uint64_t)c->rp.n_slots;
    st.camera_samples = ctr.camera_samples;
    st.paths_traced = ctr.paths;
    st.kernel_ms = ms;
    st.merge_ms = ms_merge;
    st.kernel = c->last_kernel;
    st.batches = c->n_batches;
    st.rays_closest = ctr.closest_rays;
    st.rays_shadow = ctr.shadow_rays;
    for (int b = 0; b < c->n_batches; b++) {
        float a = 0, p = 0;
        (void)hipEventElapsedTime(&a, c->bev[3 * b + 0], c->bev[3 * b + 1]);
        (void)hipEventElapsedTime(&p, c->bev[3 * b + 1], c->bev[3 * b + 2]);
        st.chain_ms += a;
        st.paths_ms += p;
    }
    if (c->sched.ticks_pending) {   // heaviest-first slot order for the next frame of this configuration
        c->sched.ticks_pending = false;
        std::vector<uint32_t> t((size_t)c->sched.ticks_n);
        HIPCHK(c, hipMemcpy(t.data(), c->sched.d_ticks.get(), sizeof(uint32_t) * t.size(), hipMemcpyDeviceToHost));
        c->sched.h_last_ticks = t;   // pbrt_gpu_tile_ticks
        if (kTickPlanes > 1) {   // diagnostics builds: start and end clocks (pbrt_gpu_tile_clocks)
            c->sched.h_tick_clocks.resize(2 * t.size());
            HIPCHK(c, hipMemcpy(c->sched.h_tick_clocks.data(), c->sched.d_ticks.get() + t.size(), sizeof(uint32_t) * 2 * t.size(),
                                hipMemcpyDeviceToHost));
        }
        c->sched.heavy_k = learn_order(t, c->sched.h_slot_kw, c->sched.ci_wps, c->facts.n_simd, c->knobs.ci_heavy,
                                       c->sched.h_slot_order);   // schedule.h
        c->sched.order_key = c->sched.ticks_key;
        if (c->knobs.ci_order_cache) sched_cache_put(sched_cache_key(c, c->sched.ticks_key), c->sched.h_slot_order, c->sched.heavy_k);
    }
    if (ctr.any_panic) {
        std::vector<PanicRec> pr((size_t)c->rp.n_slots);
        HIPCHK(c, hipMemcpy(pr.data(), c->d_panics.get(), sizeof(PanicRec) * pr.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < pr.size(); i++) {
            if (pr[i].kind == 0) continue;
            st.panic_kind = pr[i].kind;
            st.panic_tile = (int32_t)(c->rp.tile_begin + (int64_t)i * c->rp.tile_stride);
            st.panic_pixel_x = pr[i].px;
            st.panic_pixel_y = pr[i].py;
            st.panic_sample = pr[i].sample;
            st.panic_bounce = pr[i].bounce;
            break;
        }
        if (st.panic_kind == -1) {
            rc = set_err(c, PBRT_E_UNSUPPORTED, "unsupported material");
            st.panic_kind = 0;
        } else {
            rc = set_err(c, PBRT_E_REF_PANIC, "the Go reference panics on this input");
        }
    }
    st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c->t_start).count();
    if (stats) *stats = st;
    return rc;
}

int pbrt_gpu_render(pbrt_gpu_ctx* c, const pbrt_render_desc* rd, double* film_xyz, pbrt_gpu_stats* stats) {
    if (!c) return PBRT_E_INVALID;
    int rc = pbrt_gpu_render_async(c, rd);
    if (rc != PBRT_OK) return rc;
    rc = pbrt_gpu_synchronize(c, stats);
    if (rc != PBRT_OK) return rc;
    if (film_xyz) return pbrt_gpu_film_download(c, film_xyz);
    return PBRT_OK;
}

double* pbrt_gpu_film_device(pbrt_gpu_ctx* c) { return c ? c->d_out.get() : nullptr; }
void* pbrt_gpu_stream(pbrt_gpu_ctx* c) { return c ? (void*)c->stream : nullptr; }

int pbrt_gpu_film_download(pbrt_gpu_ctx* c, double* film_xyz) {
    if (!c || !film_xyz || !c->rendered) return PBRT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(film_xyz, c->film_target ? c->film_target : c->d_out.get(),
                        sizeof(double) * (size_t)(c->rp.film_w * c->rp.film_h * 3),
                        hipMemcpyDeviceToHost));
    return PBRT_OK;
}

void pbrt_gpu_cancel(pbrt_gpu_ctx* c) {
    if (!c) return;
    std::lock_guard<std::mutex> lk(c->cancel.mu);
    if (!c->cancel.in_flight) return;   // nothing to cancel: no render is in flight
    c->cancel.req = true;
    __atomic_store_n(c->cancel.h_flag, 1, __ATOMIC_SEQ_CST);
}
const char* pbrt_gpu_last_error(const pbrt_gpu_ctx* c) { return c ? c->err.c_str() : "null context"; }

void pbrt_gpu_destroy(pbrt_gpu_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (hipStream_t st : {c->stream, c->stream2, c->ov.stream3})
        if (st) (void)hipStreamSynchronize(st);
    // the caller's buffers that are still alive (the streams are idle by now)
    pbrtq::list_free_all(c->qbufs, [](void* p) { (void)hipFree(p); });
    mesh_bvh_free(c->mesh);
    for (hipEvent_t e : c->bev) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev2) (void)hipEventDestroy(c->ev2);
    if (c->ev_split) (void)hipEventDestroy(c->ev_split);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    for (hipEvent_t e : {c->ov.ev_l2, c->ov.ev_p1})
        if (e) (void)hipEventDestroy(e);
    if (c->ov.stream3) {
        (void)hipStreamSynchronize(c->ov.stream3);
        (void)hipStreamDestroy(c->ov.stream3);
    }
    if (c->stream2) {
        (void)hipStreamSynchronize(c->stream2);
        (void)hipStreamDestroy(c->stream2);
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->cancel.h_flag) (void)hipHostFree(c->cancel.h_flag);
    delete c;   // every DevBuf frees its allocation
}

}  // extern "C"

// what a device group (group.hip) reads of a member after its frame
pbrtk::GroupMemberView pbrt_group_member_view(const pbrt_gpu_ctx* c) {
    return pbrtk::GroupMemberView{c->device, c->d_films.get(), c->d_film.get(), &c->host_scene.film, c->rp};
}

extern "C" {

// film.go:142-179 WriteImage pixel conversion
int pbrt_film_to_rgba8(const double* film, int64_t w, int64_t h, uint8_t* rgba) {
    if (!film || !rgba || w <= 0 || h <= 0) return PBRT_E_INVALID;
    for (int64_t i = 0; i < w * h; i++) {
        for (int c = 0; c < 3; c++)
            rgba[i * 4 + c] = (uint8_t)(gomath::to_int(gomath::clamp(film[i * 3 + c], 0, 1) * 255) & 0xFF);
        rgba[i * 4 + 3] = 255;
    }
    return PBRT_OK;
}

}  // extern "C"

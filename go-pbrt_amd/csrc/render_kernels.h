// render_kernels.h — declarations of the kernels, for the host units (render.hip,
// queries.hip, kernel_select.hip, group.hip). Each kernel is defined (and its
// template instantiations made) in its own translation unit; the launch goes
// through the host stub that unit emits.
#pragma once

#include "film_query.h"
#include "group.h"
#include "render_common.h"

namespace pbrtk {

template <int kMinWaves>
__global__ void k_render_exact(DevScene sc, RenderParams rp, double* __restrict__ films, double* __restrict__ s1d_scratch, PanicRec* __restrict__ panics, Counters* __restrict__ ctr);
template <int P, bool kMB = false, bool kX = false>
__global__ void k_paths_ci(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr, int s1d_lds, const uint32_t* __restrict__ order);
template <bool kX = false>
__global__ void k_pw_cache(DevScene sc, WaveBufs wb, int64_t rec0, int64_t nrec, Spec* __restrict__ ldc, int* __restrict__ ldp);
template <bool kMB, bool kX = false>
__global__ void k_pw_start(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t rec0, int64_t nrec, const Spec* __restrict__ ldc, const int* __restrict__ ldp, PwPath* __restrict__ paths, PwQueues qs, unsigned long long* __restrict__ pkey);
template <bool kMeshOnly = false>
__global__ void k_pw_trace(DevScene sc, RenderParams rp, WaveBufs wb, PwPath* __restrict__ paths, PwQueues qs, int cin, int n_keys, unsigned long long* __restrict__ pkey);
__global__ void k_pw_scan(PwQueues qs, int n_keys);
__global__ void k_pw_scatter(const PwPath* __restrict__ paths, PwQueues qs);
template <bool kX = false>
__global__ void k_pw_shade(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, PwPath* __restrict__ paths, PwQueues qs, int sorted, unsigned long long* __restrict__ pkey);
template <bool kMeshOnly = false>
__global__ void k_pw_shadow(DevScene sc, RenderParams rp, WaveBufs wb, PwPath* __restrict__ paths, PwQueues qs, unsigned long long* __restrict__ pkey);
__global__ void k_pw_panics(RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t rec0, int64_t nrec, const unsigned long long* __restrict__ pkey, Counters* __restrict__ ctr);
template <bool kX = false>
__global__ void k_mb_setup(DevScene sc, RenderParams rp, ChainLayout lay, const PcgJump* __restrict__ jump, WaveBufs wb, int64_t slot_base, int64_t nslots_batch);
__global__ void k_film(const pbrt_film_desc* __restrict__ film_desc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nslots_batch, double* __restrict__ films, const int* __restrict__ cancel_seen, Counters* __restrict__ ctr);
__global__ void k_panic_reduce(WaveBufs wb, int64_t slot_base, int64_t nslots_batch, PanicRec* __restrict__ panics, Counters* __restrict__ ctr);
template <bool kX = false>
__global__ void k_wf_primary(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nb);
__global__ void k_dl_setup(DevScene sc, RenderParams rp, ChainLayout lay, const PcgJump* __restrict__ jump, WaveBufs wb, int64_t slot_base, int64_t nb);
template <bool kX = false>
__global__ void k_dl_samples(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec);
__global__ void k_dl_panics(RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr);
template <bool kX = false>
__global__ void k_tile_cost(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nb, float* __restrict__ feat, uint64_t* __restrict__ keys);
__global__ void k_order_of_keys(const uint64_t* __restrict__ keys, int64_t nb, uint32_t* __restrict__ order);
__global__ void k_gate(const uint32_t* __restrict__ prog, uint32_t b, uint32_t e, Counters* __restrict__ ctr);
template <int kW, int kDepth = 0, bool kX = false, int kEu = 0, bool kSpWin = false, bool kMulti = false>
__global__ void k_chain_ci(DevScene sc, RenderParams rp, ChainLayout lay, const PcgJump* __restrict__ jump, WaveBufs wb, int64_t slot_base, int64_t nslots_batch, int lanes_per_tile, int ring_size, Counters* __restrict__ ctr, const uint32_t* __restrict__ order, uint32_t* __restrict__ ticks, int cstride, uint32_t* __restrict__ prog);
// the camera-start wave route (PBRT_KERNEL_WAVE_CAM): k_chain_c.hip, k_paths_c.hip
__global__ void k_chain_cam(DevScene sc, RenderParams rp, ChainLayout lay, const PcgJump* __restrict__ jump, WaveBufs wb, int64_t slot_base, int64_t nslots_batch, const uint32_t* __restrict__ order, uint32_t* __restrict__ ticks);
__global__ void k_cam_setup(DevScene sc, RenderParams rp, ChainLayout lay, const PcgJump* __restrict__ jump, WaveBufs wb, int64_t slot_base, int64_t nslots_batch);
template <int P, bool kMB>
__global__ void k_paths_cam(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr);
// (trees beyond kLdsNodes: the same kernels with the [64] traversal stack in LDS)
__global__ void k_chain_cam_stack(DevScene sc, RenderParams rp, ChainLayout lay, const PcgJump* __restrict__ jump, WaveBufs wb, int64_t slot_base, int64_t nslots_batch, const uint32_t* __restrict__ order, uint32_t* __restrict__ ticks);
template <int P, bool kMB>
__global__ void k_paths_cam_stack(DevScene sc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nrec, Counters* __restrict__ ctr);
template <bool kMB>
__global__ void k_film_cam(const pbrt_film_desc* __restrict__ film_desc, RenderParams rp, WaveBufs wb, int64_t slot_base, int64_t nslots_batch, double* __restrict__ films, const int* __restrict__ cancel_seen, Counters* __restrict__ ctr);
__global__ void k_merge_film(const pbrt_film_desc* __restrict__ film_desc, RenderParams rp, const double* __restrict__ films, double* __restrict__ out, const int* __restrict__ cancel_seen);
__global__ void k_merge_film_group(const pbrt_film_desc* __restrict__ film_desc, RenderParams rp, pbrtgroup::GroupMap gm, GroupFilms films, double* __restrict__ out);
__global__ void k_intersect(DevScene sc, int64_t n, const double* __restrict__ rays, double* __restrict__ out, int any_hit);
template <bool kAny, bool kMeshOnly>
__global__ void k_query_hit(DevScene sc, int64_t n, pbrt_ray_soa rays, pbrt_hit_soa hits, QueryRec* __restrict__ rec);
template <bool kAny>
__global__ void k_query_hit_staged(DevScene sc, int64_t n, pbrt_ray_soa rays, pbrt_hit_soa hits, QueryRec* __restrict__ rec);
__global__ void k_query_camera(const pbrt_camera_desc* __restrict__ cam, pbrt_camera_rays_desc d, pbrt_ray_soa_out out);
// batched Integrator.Li over device arrays (pbrt_gpu_li_device): k_li.hip
template <bool kX, int kDepth>
__global__ void k_li(DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_radiance_soa out, QueryRec* __restrict__ rec);
// batched DirectLighting.Li over device arrays (pbrt_gpu_direct_li_device): k_li_direct.hip
template <bool kX, int kDepth>
__global__ void k_li_direct(DevScene sc, int max_depth, int strategy, int nlev, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_radiance_soa out, QueryRec* __restrict__ rec, double* __restrict__ lev);
// Path.Li one iteration at a time over device path state (pbrt_gpu_path_begin_device, pbrt_gpu_path_step_device): k_path_step.hip
__global__ void k_path_begin(int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_path_soa p);
template <bool kX, int kDepth>
__global__ void k_path_step(DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_path_soa p, pbrt_path_queue in, pbrt_path_queue out, pbrt_path_step_soa st, QueryRec* __restrict__ rec);
// a frame from public pieces (pbrt_gpu_frame_samples_device, pbrt_gpu_film_add_device, pbrt_gpu_film_rgba8_device): k_film_q.hip
__global__ void k_frame_samples(const pbrt_camera_desc* __restrict__ cam, pbrtfilm::Layout lay, int64_t px_begin, int ns, int64_t n, pbrt_frame_samples_soa out);
template <bool kLds>
__global__ void k_film_add_tiles(const pbrt_film_desc* __restrict__ film_desc, RenderParams rp, pbrtfilm::Layout lay, int64_t tile_begin, int ns, pbrt_film_samples_soa in, double* __restrict__ films);
__global__ void k_film_add_merge(const pbrt_film_desc* __restrict__ film_desc, RenderParams rp, int64_t tile_begin, int64_t tile_end, int64_t row0, int64_t rows, int clear, const double* __restrict__ films, double* __restrict__ out);
__global__ void k_film_rgba8(const double* __restrict__ film, int64_t n, uint32_t* __restrict__ rgba);
// the same pieces under sampler.Stratified (pbrt_gpu_frame_samples_stratified_device, pbrt_gpu_li_stratified_device): k_strat.hip
__global__ void k_strat_pixels(const pbrt_camera_desc* __restrict__ cam, RenderParams rp, ChainLayout lay, const PcgJump* __restrict__ jump, pbrtfilm::Layout fl, int64_t px_begin, int64_t npx, pbrt_frame_samples_soa out, pbrt_strat_samples_soa so);
template <bool kX, int kDepth>
__global__ void k_li_strat(DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_radiance_soa out, pbrt_strat_soa st, QueryRec* __restrict__ rec);

}  // namespace pbrtk

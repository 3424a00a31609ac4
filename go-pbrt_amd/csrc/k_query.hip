// k_query.hip — device-resident ray queries (pbrt_gpu_intersect[_p]_device,
// pbrt_gpu_camera_rays_device): k_query_hit, k_query_camera; and the diagnostic
// k_query_hit_staged (pbrt_diag_intersect[_p]_staged_device)
#pragma clang fp contract(off)

#include "render_common.h"

namespace pbrtk {

// BVH.Intersect / IntersectP (bvh.go:659-765) over SoA arrays in device memory:
// lane i of the grid reads element i of each ray array (unit stride, 512 B per
// wave and array) and writes element i of each output the caller asked for
// (hits.* other than hit may be null; uniform branches). The traversal is
// k_intersect's, bvh_traverse with the nodes read from memory, so the values
// are the same bits. Blocks of four waves: bvh_walk_analytic indexes its stack
// by lane with stride kStackStride, so every wave owns a 64 * kStackStride
// region of its own; the mesh-only walk has no stack and the kernel no LDS.
// A ray on which the reference panics is written as a miss and recorded:
// rec->panics counts them, rec->first keeps the smallest (index << 8 | kind).
template <bool kAny, bool kMeshOnly>
__device__ __forceinline__ void query_hit_lane(const DevScene& sc, int64_t n, const pbrt_ray_soa& rays,
                                               const pbrt_hit_soa& hits, QueryRec* __restrict__ rec) {
    uint16_t* stack = nullptr;
    if constexpr (!kMeshOnly) {
        __shared__ uint16_t stack_lds[(kQueryBlock / kWave) * 64 * kStackStride];
        stack = stack_lds + (threadIdx.x / kWave) * (64 * kStackStride) + (threadIdx.x % kWave);
    }
    const int64_t i = (int64_t)blockIdx.x * kQueryBlock + threadIdx.x;
    if (i >= n) return;
    const double tmax0 = rays.tmax ? rays.tmax[i] : kInf;
    Ray r{V3{rays.ox[i], rays.oy[i], rays.oz[i]}, V3{rays.dx[i], rays.dy[i], rays.dz[i]}, tmax0, 0};
    int panic = 0;
    if (kAny) {
        const bool h = bvh_traverse<true, 4, kMeshOnly>(sc, r, nullptr, stack, panic);
        hits.hit[i] = (h && !panic) ? 1 : 0;
    } else {
        SI si;
        si.p = si.n = V3{0, 0, 0};
        si.prim = -1;
        bool h = bvh_traverse<false, 4, kMeshOnly>(sc, r, &si, stack, panic);
        if (panic) {   // a miss, whatever the walk had found before
            h = false;
            r.tmax = tmax0;
            si.p = si.n = V3{0, 0, 0};
        }
        hits.hit[i] = h ? 1 : 0;
        if (hits.t_max) hits.t_max[i] = r.tmax;
        if (hits.prim) hits.prim[i] = h ? si.prim : -1;
        if (hits.px) hits.px[i] = si.p.x;
        if (hits.py) hits.py[i] = si.p.y;
        if (hits.pz) hits.pz[i] = si.p.z;
        if (hits.nx) hits.nx[i] = si.n.x;
        if (hits.ny) hits.ny[i] = si.n.y;
        if (hits.nz) hits.nz[i] = si.n.z;
    }
    if (panic) query_panic(rec, i, panic);
}

template <bool kAny, bool kMeshOnly>
__global__ __launch_bounds__(kQueryBlock) void k_query_hit(DevScene sc, int64_t n, pbrt_ray_soa rays, pbrt_hit_soa hits,
                                                          QueryRec* __restrict__ rec) {
    query_hit_lane<kAny, kMeshOnly>(sc, n, rays, hits, rec);
}

// Diagnostic (include/pbrt_diag.h): k_query_hit<kAny, false> over a tree the
// render kernels stage in LDS. stage_nodes first, by every thread of the block
// (it holds a __syncthreads(), so before the i >= n return), and bvh_walk_analytic
// takes its use_lds_nodes branches: the leaf-preorder scan, with the context's
// culling groups if it has any. The host launches it on trees of at most
// kLdsNodes nodes only (beyond them stage_nodes stages nothing and this is k_query_hit).
template <bool kAny>
__global__ __launch_bounds__(kQueryBlock) void k_query_hit_staged(DevScene sc, int64_t n, pbrt_ray_soa rays,
                                                                 pbrt_hit_soa hits, QueryRec* __restrict__ rec) {
    stage_nodes(sc);
    query_hit_lane<kAny, false>(sc, n, rays, hits, rec);
}

// PerspectiveCamera.GenerateRay (camera.go:192-242) for every pixel of a window,
// in raster order: camera_ray as the render kernels call it.
__global__ __launch_bounds__(kQueryBlock) void k_query_camera(const pbrt_camera_desc* __restrict__ cam,
                                                             pbrt_camera_rays_desc d, pbrt_ray_soa_out out) {
    const int64_t w = d.x1 - d.x0;
    const int64_t i = (int64_t)blockIdx.x * kQueryBlock + threadIdx.x;
    if (i >= w * (d.y1 - d.y0)) return;
    const int64_t x = d.x0 + i % w, y = d.y0 + i / w;
    const Ray r = camera_ray(*cam, (double)x + d.film_dx, (double)y + d.film_dy, d.time_u, V2{d.lens_u, d.lens_v});
    out.ox[i] = r.o.x; out.oy[i] = r.o.y; out.oz[i] = r.o.z;
    out.dx[i] = r.d.x; out.dy[i] = r.d.y; out.dz[i] = r.d.z;
    if (out.tmax) out.tmax[i] = r.tmax;
}

template __global__ void k_query_hit<false, false>(DevScene sc, int64_t n, pbrt_ray_soa rays, pbrt_hit_soa hits, QueryRec* __restrict__ rec);
template __global__ void k_query_hit<true, false>(DevScene sc, int64_t n, pbrt_ray_soa rays, pbrt_hit_soa hits, QueryRec* __restrict__ rec);
template __global__ void k_query_hit<false, true>(DevScene sc, int64_t n, pbrt_ray_soa rays, pbrt_hit_soa hits, QueryRec* __restrict__ rec);
template __global__ void k_query_hit<true, true>(DevScene sc, int64_t n, pbrt_ray_soa rays, pbrt_hit_soa hits, QueryRec* __restrict__ rec);
template __global__ void k_query_hit_staged<false>(DevScene sc, int64_t n, pbrt_ray_soa rays, pbrt_hit_soa hits, QueryRec* __restrict__ rec);
template __global__ void k_query_hit_staged<true>(DevScene sc, int64_t n, pbrt_ray_soa rays, pbrt_hit_soa hits, QueryRec* __restrict__ rec);

}  // namespace pbrtk

// diag.hip — the diagnostics of include/pbrt_diag.h that read a context or the
// library and render nothing: the device math probe (k_probe), the counters of
// the last frame, the mesh LBVH, the chain schedule's records, the launch log,
// the counter symbols of the diagnostics builds, the build id and the ABI sizes.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/pbrt_diag.h"
#include "context.h"
#include "kernel_select.h"
#include "schedule.h"

using namespace pbrt;
using namespace pbrtk;

namespace {
__global__ void k_probe(int op, const double* __restrict__ in, int64_t n, int in_stride, double* __restrict__ out,
                        int out_stride) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* a = in + i * in_stride;
    double* o = out + i * out_stride;
    switch (op) {
        case PBRT_PROBE_SIN: o[0] = gomath::sin(a[0]); break;
        case PBRT_PROBE_COS: o[0] = gomath::cos(a[0]); break;
        case PBRT_PROBE_TAN: o[0] = gomath::tan(a[0]); break;
        case PBRT_PROBE_ATAN: o[0] = gomath::atan(a[0]); break;
        case PBRT_PROBE_ATAN2: o[0] = gomath::atan2(a[0], a[1]); break;
        case PBRT_PROBE_ASIN: o[0] = gomath::asin(a[0]); break;
        case PBRT_PROBE_ACOS: o[0] = gomath::acos(a[0]); break;
        case PBRT_PROBE_SQRT: o[0] = gomath::sqrt(a[0]); break;
        case PBRT_PROBE_DIV: o[0] = a[0] / a[1]; break;
        case PBRT_PROBE_NEXTAFTER: o[0] = gomath::nextafter(a[0], a[1]); break;
        case PBRT_PROBE_MAX: o[0] = gomath::max(a[0], a[1]); break;
        case PBRT_PROBE_MIN: o[0] = gomath::min(a[0], a[1]); break;
        case PBRT_PROBE_OFFSET_RAY_ORIGIN: {
            V3 r = offset_ray_origin(load3(a), load3(a + 3), load3(a + 6), load3(a + 9));
            o[0] = r.x; o[1] = r.y; o[2] = r.z;
            break;
        }
        case PBRT_PROBE_EFLOAT_ADD: {
            int panic = 0;
            EF r = ef_add(ef_new(a[0], a[1], panic), ef_new(a[2], a[3], panic), panic);
            o[0] = r.v; o[1] = r.lo; o[2] = r.hi; o[3] = panic;
            break;
        }
        case PBRT_PROBE_TRANSFORM_RAY: {
            pbrt_matrix4x4 m;
            for (int k = 0; k < 16; k++) m.m[k / 4][k % 4] = a[k];
            Ray r{load3(a + 16), load3(a + 19), gomath::kInf, 0};
            Ray w = xf_ray(m, r, nullptr, nullptr);
            o[0] = w.o.x; o[1] = w.o.y; o[2] = w.o.z; o[3] = w.d.x; o[4] = w.d.y; o[5] = w.d.z;
            break;
        }
        case PBRT_PROBE_SPAWN_RAY_TO: {
            V3 p0 = load3(a), e0 = load3(a + 3), n0 = load3(a + 6), p1 = load3(a + 9), e1 = load3(a + 12),
               n1 = load3(a + 15);
            V3 origin = offset_ray_origin(p0, e0, n0, p1 - p0);
            V3 target = offset_ray_origin(p1, e1, n1, origin - p1);
            V3 d = target - origin;
            o[0] = p0.x; o[1] = p0.y; o[2] = p0.z; o[3] = d.x; o[4] = d.y; o[5] = d.z; o[6] = 1 - 0.0001;
            break;
        }
        case PBRT_PROBE_PCG: {
            Pcg r;
            pcg_seed(r, (uint64_t)a[0]);
            for (int k = 0; k < out_stride; k++) o[k] = pcg_float(r);
            break;
        }
        case PBRT_PROBE_MIN_NONAN: o[0] = gomath::min_nonan(a[0], a[1]); break;
        case PBRT_PROBE_MAX_NONAN: o[0] = gomath::max_nonan(a[0], a[1]); break;
        case PBRT_PROBE_EFLOAT_MUL:
        case PBRT_PROBE_EFLOAT_DIV: {
            int panic = 0;
            EF x = ef_new(a[0], a[1], panic), y = ef_new(a[2], a[3], panic);
            EF r = op == PBRT_PROBE_EFLOAT_MUL ? ef_mul(x, y, panic) : ef_div(x, y, panic);
            o[0] = r.v; o[1] = r.lo; o[2] = r.hi; o[3] = panic;
            break;
        }
        case PBRT_PROBE_NEXT_FLOAT_UP: o[0] = gomath::next_up(a[0]); break;
        case PBRT_PROBE_NEXT_FLOAT_DOWN: o[0] = gomath::next_down(a[0]); break;
        case PBRT_PROBE_SINCOS: {
            double s, c;
            gomath::sincos(a[0], s, c);
            o[0] = s; o[1] = c;
            break;
        }
        case PBRT_PROBE_CONCENTRIC_DISK: {
            V2 d = concentric_sample_disk(V2{a[0], a[1]});
            o[0] = d.x; o[1] = d.y;
            break;
        }
        default: o[0] = gomath::nan();
    }
}
const KernelName kDiagKernelNames[] = {PBRT_KERNEL_NAME(k_probe)};
}  // namespace

const KernelName* pbrtk::diag_kernel_names(size_t* n) {
    *n = sizeof(kDiagKernelNames) / sizeof(kDiagKernelNames[0]);
    return kDiagKernelNames;
}

extern "C" int pbrt_gpu_probe(int device, int op, const double* in, size_t n, int in_stride, double* out,
                              int out_stride) {
    if (!in || !out || in_stride <= 0 || out_stride <= 0) return PBRT_E_INVALID;
    if ((op == PBRT_PROBE_SINCOS || op == PBRT_PROBE_CONCENTRIC_DISK) && out_stride < 2) return PBRT_E_INVALID;
    if (op == PBRT_PROBE_CONCENTRIC_DISK && in_stride < 2) return PBRT_E_INVALID;
    if (n == 0) return PBRT_OK;
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return PBRT_E_HIP;
    DevBuf<double> in_buf, out_buf;
    if (in_buf.ensure(nullptr, n * in_stride) != PBRT_OK || out_buf.ensure(nullptr, n * out_stride) != PBRT_OK)
        return PBRT_E_HIP;
    double *d_in = in_buf.get(), *d_out = out_buf.get();
    hipError_t e = hipMemcpy(d_in, in, sizeof(double) * n * in_stride, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_logged(nullptr, 0, k_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, d_in, (int64_t)n,
                           in_stride, d_out, out_stride);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out, sizeof(double) * n * out_stride, hipMemcpyDeviceToHost);
    return e == hipSuccess ? PBRT_OK : PBRT_E_HIP;
}

extern "C" int pbrt_gpu_counters(pbrt_gpu_ctx* c, uint64_t* out, int n) {
    if (!c || !out) return PBRT_E_INVALID;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return PBRT_E_HIP;
    Counters ctr;
    if (hipMemcpy(&ctr, c->d_ctr.get(), sizeof(ctr), hipMemcpyDeviceToHost) != hipSuccess) return PBRT_E_HIP;
    const uint64_t v[kNumCounters] = {ctr.paths,    ctr.camera_samples, ctr.closest_rays, ctr.shadow_rays,
                                      (uint64_t)ctr.any_panic, ctr.windows, ctr.phase[0], ctr.phase[1],
                                      ctr.phase[2], ctr.phase[3], ctr.phase[4], ctr.phase[5],
                                      ctr.phase[6], ctr.phase[7]};
    for (int i = 0; i < n && i < kNumCounters; i++)
        out[i] = i < 14 ? v[i] : i < 78 ? (uint64_t)ctr.dhist[i - 14] : i == 78 ? ctr.busy : i == 79 ? ctr.nps_issued
                                                                                                   : ctr.odd_d;
    return kNumCounters;
}

extern "C" int pbrt_gpu_mesh_info(pbrt_gpu_ctx* c, double* out, int n) {
    if (!c || !out) return -PBRT_E_INVALID;
    const double v[] = {(double)c->mesh.n_tris, (double)c->mesh.n_nodes, (double)c->mesh.depth, c->mesh.build_ms,
                        (double)c->mesh.n_meshes, (double)PBRT_MESH_WIDE};
    const int m = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < m; i++) out[i] = v[i];
    return m;
}
extern "C" int pbrt_gpu_mesh_counters(uint64_t* out, int n, int reset) {
#ifdef PBRT_MESH_COUNT
    unsigned long long h[kMeshCountSlots * 6];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_mesh_count), sizeof(h)) != hipSuccess) return -PBRT_E_HIP;
    for (int i = 0; i < n && i < kMeshCountSlots * 6; i++) out[i] = h[i];
    if (reset) {
        std::memset(h, 0, sizeof(h));
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_mesh_count), h, sizeof(h)) != hipSuccess) return -PBRT_E_HIP;
    }
    return kMeshCountSlots * 6;
#else
    (void)out; (void)n; (void)reset;
    return 0;
#endif
}

extern "C" int pbrt_gpu_mesh_download(pbrt_gpu_ctx* c, void* nodes, int32_t* gid, float* tris) {
    if (!c) return PBRT_E_INVALID;
    if (hipSetDevice(c->device) != hipSuccess) return PBRT_E_HIP;
    const size_t nn = mesh_node_bytes(c->mesh.n_nodes), nt = (size_t)c->mesh.n_tris;
    if (nodes && nn && hipMemcpy(nodes, c->mesh.nodes, nn, hipMemcpyDeviceToHost) != hipSuccess)
        return PBRT_E_HIP;
    if (gid && nt && hipMemcpy(gid, c->mesh.gid, nt * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return PBRT_E_HIP;
    if (tris && nt && hipMemcpy(tris, c->mesh.tris, nt * 9 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
        return PBRT_E_HIP;
    return PBRT_OK;
}

extern "C" int64_t pbrt_gpu_tile_clocks(pbrt_gpu_ctx* c, uint32_t* start, uint32_t* end, int64_t n) {
    if (!c) return -PBRT_E_INVALID;
    const int64_t m = (int64_t)c->sched.h_tick_clocks.size() / 2;
    for (int64_t i = 0; i < m && i < n; i++) {
        if (start) start[i] = c->sched.h_tick_clocks[(size_t)i];
        if (end) end[i] = c->sched.h_tick_clocks[(size_t)(m + i)];
    }
    return m;
}

extern "C" int64_t pbrt_gpu_tile_ticks(pbrt_gpu_ctx* c, uint32_t* out, int64_t n, int64_t* heavy) {
    if (!c) return -PBRT_E_INVALID;
    if (heavy) *heavy = c->sched.last_heavy;
    const int64_t m = (int64_t)c->sched.h_last_ticks.size();
    for (int64_t i = 0; out && i < n && i < m; i++) out[i] = c->sched.h_last_ticks[(size_t)i];
    return m;
}

extern "C" void pbrt_gpu_schedule_cache_clear(void) {
    sched_cache_clear();
}

extern "C" int64_t pbrt_gpu_overlap_slots(pbrt_gpu_ctx* c) {
    if (!c) return -PBRT_E_INVALID;
    return c->ov.done;
}

// the launch log (pbrt_diag.h); the names by host function pointer: kernel_select.hip
extern "C" int64_t pbrt_gpu_launch_log(pbrt_gpu_ctx* c, int which, pbrt_launch_rec* out, int64_t n, uint64_t* overflow) {
    if (!c || (which != PBRT_LAUNCHES_FRAME && which != PBRT_LAUNCHES_OUTSIDE)) return -PBRT_E_INVALID;
    const LaunchLog& log = which == PBRT_LAUNCHES_FRAME ? c->log_frame : c->log_aux;
    if (overflow) *overflow = log.overflow;
    const int64_t m = (int64_t)log.recs.size();
    if (out && n > 0 && hipSetDevice(c->device) != hipSuccess) return -PBRT_E_HIP;
    for (int64_t i = 0; out && i < n && i < m; i++) {
        const LaunchRec& r = log.recs[(size_t)i];
        pbrt_launch_rec& o = out[i];
        o.name = kernel_name_of(r.fn);
        o.fn = r.fn;
        for (int k = 0; k < 3; k++) {
            o.grid[k] = r.grid[k];
            o.block[k] = r.block[k];
        }
        o.lds_dynamic = r.lds;
        hipFuncAttributes fa;
        o.lds_static = hipFuncGetAttributes(&fa, r.fn) == hipSuccess ? (uint32_t)fa.sharedSizeBytes : 0xFFFFFFFFu;
        o.stream = r.stream;
        o.pad0 = 0;
    }
    return m;
}

extern "C" int64_t pbrt_gpu_lds_per_block(pbrt_gpu_ctx* c) { return c ? (int64_t)c->facts.lds_per_block : -PBRT_E_INVALID; }

extern "C" int pbrt_gpu_schedule_source(pbrt_gpu_ctx* c) {
    if (!c) return -PBRT_E_INVALID;
    return c->sched.src;
}

extern "C" int64_t pbrt_gpu_tile_costs(pbrt_gpu_ctx* c, float* out, int64_t n) {
    if (!c) return -PBRT_E_INVALID;
    if (!c->sched.probed || !c->sched.d_cost.get()) return 0;
    if (out && n > 0) {
        const int64_t m = std::min<int64_t>(n, c->sched.cost_n);
        if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(out, c->sched.d_cost.get(), sizeof(float) * 4 * (size_t)m, hipMemcpyDeviceToHost) != hipSuccess)
            return -PBRT_E_HIP;
    }
    return c->sched.cost_n;
}

// Region cycles of trajectory steps (PBRT_STEP_TIMING builds only; else zeros):
// [0] loop top / light-sample draws, [1] closest-hit traversal + interaction,
// [2] BSDF setup, [3] light sampling (full paths), [4] BSDF sample + spawn + RR.
extern "C" int pbrt_gpu_step_cycles(uint64_t* out, int n, int reset) {
#ifdef PBRT_STEP_TIMING
    unsigned long long h[8];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_step_cycles), sizeof(h)) != hipSuccess) return PBRT_E_HIP;
    for (int i = 0; i < n && i < 8; i++) out[i] = h[i];
    if (reset) {
        std::memset(h, 0, sizeof(h));
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_step_cycles), h, sizeof(h)) != hipSuccess) return PBRT_E_HIP;
    }
#else
    for (int i = 0; i < n && i < 8; i++) out[i] = 0;
    (void)reset;
#endif
    return 8;
}

#ifndef PBRT_BUILD_ID
#define PBRT_BUILD_ID "unknown"
#endif
extern "C" const char* pbrt_gpu_build_id(void) { return PBRT_BUILD_ID; }

extern "C" int pbrt_abi_sizes(size_t* out, int n) {
    const size_t s[] = {sizeof(pbrt_matrix4x4),   sizeof(pbrt_transform),    sizeof(pbrt_shape_desc),
                        sizeof(pbrt_material_desc), sizeof(pbrt_primitive_desc), sizeof(pbrt_bvh_node),
                        sizeof(pbrt_light_desc),  sizeof(pbrt_camera_desc),  sizeof(pbrt_film_desc),
                        sizeof(pbrt_distribution_desc), sizeof(pbrt_scene_desc), sizeof(pbrt_render_desc),
                        sizeof(pbrt_gpu_stats),   sizeof(pbrt_ray_soa),      sizeof(pbrt_hit_soa),
                        sizeof(pbrt_gpu_opts),    sizeof(pbrt_mesh_desc)};
    int m = (int)(sizeof(s) / sizeof(s[0]));
    for (int i = 0; i < n && i < m; i++) out[i] = s[i];
    return m;
}

// path_query.h — the host side of pbrt_gpu_path_begin_device and
// pbrt_gpu_path_step_device (include/pbrt_gpu.h) that needs no device: the
// argument checks, the queue rules and the grid of k_path_begin / k_path_step.
// What the desc and the scene refuse, the light distributions served and the
// choice of the instantiation are the li query's (li_query.h: check_supported,
// check_distribution, kernel_args), used as they are.
// Plain C++ with no dependency on HIP: queries.hip passes in what it knows of
// the context, and tests/path_query_check.cpp compiles this header on its own.
#pragma once

#include <cstddef>
#include <cstdint>

#include "li_query.h"

namespace pbrtpath {

constexpr int kBeginBlock = 256;               // threads of a k_path_begin workgroup, one path each
constexpr int kSlice = pbrtli::kLiRays;        // queue entries of one k_path_step workgroup (one wave, one staged tree)
constexpr int kBytesPerPath = 141;             // pbrt_path_soa's arrays; 133 without tmax
constexpr int kBytesPerPathNoTmax = kBytesPerPath - 8;

// every pointer of the state is required, but tmax
inline bool state_complete(const pbrt_path_soa& p) {
    return p.ox && p.oy && p.oz && p.dx && p.dy && p.dz && p.lr && p.lg && p.lb && p.br && p.bg && p.bb && p.eta_scale &&
           p.state && p.inc && p.draws && p.rays && p.bounces && p.status;
}

// A queue that is given names both of its arrays; in and out share neither.
inline bool queue_complete(const pbrt_path_queue* q) { return !q || (q->index && q->count); }
inline bool queues_alias(const pbrt_path_queue* in, const pbrt_path_queue* out) {
    if (!in || !out) return false;
    return in == out || in->index == out->index || in->count == out->count;
}

// PBRT_E_INVALID's conditions of path_begin, in the header's order; `why` names the first.
inline int check_begin(bool ctx_ok, const pbrt_ray_soa* rays, const pbrt_rng_soa* rng, size_t n, const pbrt_path_soa* paths,
                       bool in_flight, const char** why) {
    auto bad = [&](const char* m) {
        *why = m;
        return (int)PBRT_E_INVALID;
    };
    if (!ctx_ok) return bad("null context");
    if (!rays) return bad("rays is NULL");
    if (!pbrtli::rays_complete(*rays)) return bad("a ray array is NULL");
    if (!rng) return bad("rng is NULL");
    if (!pbrtli::rng_complete(*rng)) return bad("an rng array is NULL");
    if (!paths) return bad("paths is NULL");
    if (!state_complete(*paths)) return bad("a path state array is NULL");
    if (n > (size_t)INT32_MAX) return bad("more than 2^31 - 1 paths in one call");
    if (in_flight) return bad("a render is in flight on this context");
    *why = "";
    return PBRT_OK;
}

// PBRT_E_INVALID's conditions of path_step (step and its pointers are all optional)
inline int check_step(bool ctx_ok, const pbrt_li_desc* d, const pbrt_path_soa* paths, const pbrt_path_queue* in,
                      const pbrt_path_queue* out, size_t n, bool in_flight, const char** why) {
    auto bad = [&](const char* m) {
        *why = m;
        return (int)PBRT_E_INVALID;
    };
    if (!ctx_ok) return bad("null context");
    if (!d) return bad("the li desc is NULL");
    if (!paths) return bad("paths is NULL");
    if (!state_complete(*paths)) return bad("a path state array is NULL");
    if (!queue_complete(in)) return bad("the in queue's index or count is NULL");
    if (!queue_complete(out)) return bad("the out queue's index or count is NULL");
    if (queues_alias(in, out)) return bad("the in and out queues alias");
    if (n > (size_t)INT32_MAX) return bad("more than 2^31 - 1 paths in one call");
    if (d->max_depth < 1) return bad("max_depth < 1");
    if (d->reserved != 0) return bad("reserved must be 0");
    if (in_flight) return bad("a render is in flight on this context");
    *why = "";
    return PBRT_OK;
}

// Workgroups of k_path_begin: kBeginBlock paths each.
inline uint32_t begin_grid(size_t n) { return (uint32_t)((n + kBeginBlock - 1) / kBeginBlock); }

// The k_path_step launch: the instantiation by pbrtli::kernel_args' rule; one
// wave a workgroup, which stages the tree once for kSlice entries of the queue.
// The grid covers n entries, the queue's upper bound: *in->count is known on
// the device only, and a workgroup whose slice starts beyond it exits before it
// stages anything.
inline pbrtli::KernelArgs step_args(bool non_matte, int n_nodes, bool mesh, size_t n, int lds_nodes) {
    pbrtli::KernelArgs a = pbrtli::kernel_args(non_matte, n_nodes, mesh, n, lds_nodes);
    a.grid = (uint32_t)((n + kSlice - 1) / kSlice);
    return a;
}

}  // namespace pbrtpath

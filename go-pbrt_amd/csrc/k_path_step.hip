// k_path_step.hip — Path.Li one iteration at a time over path state resident on
// the device (pbrt_gpu_path_begin_device, pbrt_gpu_path_step_device):
// k_path_begin, k_path_step
#pragma clang fp contract(off)

#include "render_common.h"
#include "path_query.h"

namespace pbrtk {

// path_step's State of k_path_step: PathState without the radiance sum, which an
// iteration only adds to, once, as its last statement; the term is kept instead
// (kTapAdded) and the sum stays in memory until the iteration is over. note_hit
// writes the interaction to the caller's arrays where it is found, so none of
// it is held across the rest of the iteration.
constexpr uint32_t kTapAdded = 1u, kTapHit = 2u;
struct PathStateTap {
    Spec beta;
    Ray ray;
    double eta_scale;
    int bounces;
    int first;
    uint32_t rays;
    Spec added;
    uint32_t flags;
    int64_t i;                        // the path's index
    const pbrt_path_step_soa* step;   // (the kernel's argument)
};
__device__ __forceinline__ void add_L(PathStateTap& s, Spec v) {
    s.added = v;
    s.flags |= kTapAdded;
}
__device__ __forceinline__ void add_rays(PathStateTap& s, uint32_t v) { s.rays += v; }
__device__ __forceinline__ constexpr bool caller_eta(const PathStateTap&) { return true; }   // pbrt_path_soa's eta_scale
__device__ __forceinline__ void note_hit(PathStateTap& s, const DevScene& sc, const SI& si) {
    s.flags |= kTapHit;
    const pbrt_hit_soa& h = s.step->hit;
    const int64_t i = s.i;
    if (h.hit) h.hit[i] = 1;
    if (h.t_max) h.t_max[i] = s.ray.tmax;
    if (h.prim) h.prim[i] = si.prim;
    if (h.px) h.px[i] = si.p.x;
    if (h.py) h.py[i] = si.p.y;
    if (h.pz) h.pz[i] = si.p.z;
    if (h.nx) h.nx[i] = si.n.x;
    if (h.ny) h.ny[i] = si.n.y;
    if (h.nz) h.nz[i] = si.n.z;
    if (s.step->material)   // compute_bsdf's choice
        s.step->material[i] = si.prim < sc.n_prims ? sc.prims[si.prim].material
                                                   : sc.mesh.mesh_mat[tri_mesh(sc, si.prim - sc.n_prims)];
}

// The state k_li gives a lane that takes ray i: one path a thread.
__global__ __launch_bounds__(pbrtpath::kBeginBlock) void k_path_begin(int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng,
                                                                      pbrt_path_soa p) {
    const int64_t i = (int64_t)blockIdx.x * pbrtpath::kBeginBlock + threadIdx.x;
    if (i >= n) return;
    p.ox[i] = rays.ox[i]; p.oy[i] = rays.oy[i]; p.oz[i] = rays.oz[i];
    p.dx[i] = rays.dx[i]; p.dy[i] = rays.dy[i]; p.dz[i] = rays.dz[i];
    if (p.tmax) p.tmax[i] = rays.tmax ? rays.tmax[i] : kInf;
    p.lr[i] = 0.0; p.lg[i] = 0.0; p.lb[i] = 0.0;
    p.br[i] = 1.0; p.bg[i] = 1.0; p.bb[i] = 1.0;
    p.eta_scale[i] = 1.0;
    p.state[i] = rng.state[i];
    const_cast<uint64_t*>(p.inc)[i] = rng.inc[i];
    p.draws[i] = 0;
    p.rays[i] = 0;
    p.bounces[i] = 0;
    p.status[i] = PBRT_PATH_ALIVE;
}

// One iteration of Path.Li's loop, path_step<2, kX, true> as k_li runs it, for
// every covered path that is PBRT_PATH_ALIVE. A workgroup is one wave and owns
// the kSlice queue entries from blockIdx.x * kSlice on (in.index NULL: the paths
// of those indices), so the tree is staged once (stage_nodes) for up to kSlice
// paths, walked 64 at a time; a workgroup whose slice starts at or beyond
// *in.count exits before it stages anything. A lane gathers its path's state by
// index, steps it in registers and scatters back what the iteration changed: a
// path's values depend on its state only. The survivors of each 64 go to the out
// queue with one atomic a wave: ballot, popcount, lane 0 adds, the base is
// broadcast, each survivor stores at base + its rank.
// kDepth and the stack: k_li's. An index outside [0, n) is skipped.
template <bool kX, int kDepth>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(kPathsWaves, 8))) void k_path_step(
    DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_path_soa p, pbrt_path_queue in, pbrt_path_queue out,
    pbrt_path_step_soa st, QueryRec* __restrict__ rec) {
    __shared__ uint16_t stack_lds[kDepth > 0 ? kDepth * kStackStride : 1];
    const int64_t e0 = (int64_t)blockIdx.x * pbrtpath::kSlice;
    int64_t cnt = n;
    if (in.count) {
        const int64_t c = (int64_t)*in.count;
        cnt = c < n ? c : n;
    }
    if (e0 >= cnt) return;   // (the whole workgroup: nothing staged)
    // (kDepth > 0: launched on trees beyond kLdsNodes only, which stage_nodes leaves alone)
    if (kDepth > 0) sc.use_lds_nodes = 0;
    else stage_nodes(sc);
    const int lane = threadIdx.x;
    const int T = (int)(cnt - e0 < (int64_t)pbrtpath::kSlice ? cnt - e0 : (int64_t)pbrtpath::kSlice);
    const unsigned long long lt_mask = (1ULL << lane) - 1ULL;
    NoCache none;   // (never read: no code is generated for it)
    const SpecSampler ss{nullptr, 1, 0, nullptr};
    for (int t0 = 0; t0 < T; t0 += kWave) {   // uniform
        const int t = t0 + lane;
        int64_t i = -1;
        if (t < T) {
            i = in.index ? (int64_t)in.index[e0 + t] : e0 + t;
            if (i >= n) i = -1;
        }
        bool alive = false;
        if (i >= 0 && p.status[i] == PBRT_PATH_ALIVE) {
            Cursor c;
            c.rng.state = p.state[i];
            c.rng.inc = p.inc[i];
            c.draws = p.draws[i];
            c.cur1d = 0;
            c.cur2d = 0;
            c.k = -1;
            c.kdep = 0;
            c.rri = -1;
            c.rrn = 0;
            PathStateTap ps;
            const double tmax0 = p.tmax ? p.tmax[i] : kInf;
            ps.ray = Ray{V3{p.ox[i], p.oy[i], p.oz[i]}, V3{p.dx[i], p.dy[i], p.dz[i]}, tmax0, 0.0};
            ps.beta = Spec{p.br[i], p.bg[i], p.bb[i]};
            ps.eta_scale = p.eta_scale[i];
            ps.bounces = p.bounces[i];
            ps.first = 0;
            ps.rays = p.rays[i];
            ps.added = spec(0);
            ps.flags = 0;
            ps.i = i;
            ps.step = &st;
            int pnc = 0, bnc = 1;
            const bool done = path_step<2, kX, true>(sc, none, ss, c, ps, max_depth, rr_threshold,
                                                     kDepth > 0 ? stack_lds + lane : nullptr, pnc, bnc);
            alive = !done;
            p.state[i] = c.rng.state;
            p.draws[i] = c.draws;
            p.rays[i] = ps.rays;
            p.bounces[i] = ps.bounces;
            p.status[i] = done ? (pnc ? PBRT_PATH_PANICKED : PBRT_PATH_ENDED) : PBRT_PATH_ALIVE;
            Spec added = spec(0);
            if (done && pnc) {   // as k_li reports such a ray
                p.lr[i] = 0.0;
                p.lg[i] = 0.0;
                p.lb[i] = 0.0;
                query_panic(rec, i, pnc);
            } else if (ps.flags & kTapAdded) {
                added = ps.added;
                p.lr[i] = p.lr[i] + added.r;
                p.lg[i] = p.lg[i] + added.g;
                p.lb[i] = p.lb[i] + added.b;
            }
            if (alive) {   // the scatter's ray and throughput
                p.ox[i] = ps.ray.o.x; p.oy[i] = ps.ray.o.y; p.oz[i] = ps.ray.o.z;
                p.dx[i] = ps.ray.d.x; p.dy[i] = ps.ray.d.y; p.dz[i] = ps.ray.d.z;
                if (p.tmax) p.tmax[i] = ps.ray.tmax;
                p.br[i] = ps.beta.r; p.bg[i] = ps.beta.g; p.bb[i] = ps.beta.b;
                p.eta_scale[i] = ps.eta_scale;
            }
            if (!(ps.flags & kTapHit)) {   // a miss, as k_query_hit writes it
                const pbrt_hit_soa& h = st.hit;
                if (h.hit) h.hit[i] = 0;
                if (h.t_max) h.t_max[i] = tmax0;
                if (h.prim) h.prim[i] = -1;
                if (h.px) h.px[i] = 0.0;
                if (h.py) h.py[i] = 0.0;
                if (h.pz) h.pz[i] = 0.0;
                if (h.nx) h.nx[i] = 0.0;
                if (h.ny) h.ny[i] = 0.0;
                if (h.nz) h.nz[i] = 0.0;
                if (st.material) st.material[i] = -1;
            }
            if (st.ar) st.ar[i] = added.r;
            if (st.ag) st.ag[i] = added.g;
            if (st.ab) st.ab[i] = added.b;
        }
        if (out.index) {
            const unsigned long long m = __ballot(alive);
            if (m) {   // uniform
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(out.count, (uint32_t)__popcll(m));
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                const int64_t pos = (int64_t)base + __popcll(m & lt_mask);
                if (alive && pos < n) out.index[pos] = (int32_t)i;
            }
        }
    }
}

template __global__ void k_path_step<false, 0>(DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_path_soa p, pbrt_path_queue in, pbrt_path_queue out, pbrt_path_step_soa st, QueryRec* __restrict__ rec);
template __global__ void k_path_step<true, 0>(DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_path_soa p, pbrt_path_queue in, pbrt_path_queue out, pbrt_path_step_soa st, QueryRec* __restrict__ rec);
template __global__ void k_path_step<false, 64>(DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_path_soa p, pbrt_path_queue in, pbrt_path_queue out, pbrt_path_step_soa st, QueryRec* __restrict__ rec);
template __global__ void k_path_step<true, 64>(DevScene sc, int max_depth, double rr_threshold, int64_t n, pbrt_path_soa p, pbrt_path_queue in, pbrt_path_queue out, pbrt_path_step_soa st, QueryRec* __restrict__ rec);

}  // namespace pbrtk

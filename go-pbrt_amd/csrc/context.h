// context.h — what every host unit (render.hip, queries.hip, diag.hip) needs of
// a context: the error macro, the owner of a device allocation, the context
// itself, and the few functions every entry point calls. Host only.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pbrt_gpu.h"
#include "frame_route.h"
#include "knobs.h"
#include "query_buffers.h"
#include "render_common.h"

#pragma GCC visibility push(hidden)   // the units' own: not among the library's exported symbols
inline int set_err(pbrt_gpu_ctx* c, int code, const std::string& m);
#pragma GCC visibility pop
#define HIPCHK(ctx, call)                                                                            \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return set_err(ctx, PBRT_E_HIP, std::string(#call ": ") + hipGetErrorString(e_));      \
    } while (0)

// The one owner of a device allocation: freed with its owner (the context, or a
// scope). Errors go to the context `c` (null outside one).
template <class T>
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
        return *this;
    }
    ~DevBuf() { release(); }
    T* get() const { return p_; }
    size_t cap() const { return cap_; }   // elements it has room for
    // room for n elements: kept if it has them, else freed and allocated anew (the contents are lost)
    int ensure(pbrt_gpu_ctx* c, size_t n) {
        if (cap_ >= n && p_) return PBRT_OK;
        release();
        HIPCHK(c, hipMalloc((void**)&p_, sizeof(T) * (n ? n : 1)));
        cap_ = n;
        return PBRT_OK;
    }
    // a fresh allocation of n elements (an empty array keeps a valid pointer), filled from src unless null
    int upload(pbrt_gpu_ctx* c, const T* src, size_t n) {
        if (n == 0) n = 1;
        release();
        HIPCHK(c, hipMalloc((void**)&p_, sizeof(T) * n));
        cap_ = n;
        if (src) HIPCHK(c, hipMemcpy(p_, src, sizeof(T) * n, hipMemcpyHostToDevice));
        return PBRT_OK;
    }

  private:
    void release() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    T* p_ = nullptr;
    size_t cap_ = 0;   // elements
};

struct pbrt_gpu_ctx {
    pbrtk::Knobs knobs;
    int device = 0;
    pbrtroute::Facts facts;   // what the frame's rules read of the scene and the device (pbrt_gpu_create)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    // heavy/light split of k_chain_ci: the heaviest tiles with 4 waves each on
    // the main stream, the rest on stream2, concurrently
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_split = nullptr, ev_join = nullptr;
    // PBRT_PATHS_OVERLAP: a high-priority stream for the light chain launch, the
    // events of the completion-driven path stage, and k_chain_ci's progress record
    // (layout at kProgHead)
    struct {
        hipStream_t stream3 = nullptr;
        hipEvent_t ev_l2 = nullptr, ev_p1 = nullptr;
        int64_t done = 0;                // slots whose path stage was launched beside the chains
        DevBuf<uint32_t> d_prog;
        // a frame whose k_gate saw the chains stand still (a dispatcher that serialises
        // kernels across streams) is rendered again without the overlap; two such
        // frames in a row turn the overlap off for the context
        pbrt_render_desc last_rd{};
        double* last_film_device = nullptr;
        int stalls = 0;
        bool retry = false;
    } ov;
    pbrtk::MeshBuild mesh;          // triangle meshes + their LBVH (extension)
    // k_chain_ci heaviest-first schedule: per-slot chain time of the last
    // EXACT frame (wall_clock64 ticks) and the slot order derived from it
    struct {
        int64_t heavy_k = 0;                 // slots at the front of h_slot_order that get 4 waves
        int ci_wps = 2;                      // waves/SIMD of the last one-wave k_chain_ci launch (3 or 2)
        int64_t last_heavy = 0;              // heavy slots of the last EXACT launch (0: no split)
        std::vector<uint32_t> h_last_ticks;  // per-slot chain ticks of the last EXACT frame
        std::vector<uint8_t> h_slot_kw;      // waves per tile each slot ran with in the last frame
        DevBuf<uint32_t> d_ticks;            // [kTickPlanes][slots] (render.hip)
        std::vector<uint32_t> h_tick_clocks; // diagnostics builds: [start | end] clocks of the last frame
        DevBuf<uint32_t> d_slot_order;
        std::vector<uint32_t> h_slot_order;
        uint64_t order_key = 0, ticks_key = 0;
        int64_t ticks_n = 0;
        bool ticks_pending = false;
        int src = 0;                         // schedule of the last EXACT frame: PBRT_SCHED_* (pbrt_diag.h)
        // cold-frame schedule (k_tile_cost): per-slot features and sort keys
        DevBuf<float> d_cost;
        DevBuf<uint64_t> d_cost_keys;
        int64_t cost_n = 0;
        bool probed = false;                 // the last EXACT frame ran the cost probe
    } sched;
    uint64_t scene_hash = 0;         // content hash of the scene (process-wide schedule cache)
    double* film_target = nullptr;   // caller buffer of the last render_async_into
    int lanes_per_wave = 64;
    bool lanes_per_wave_set = false;
    int min_waves = 1;      // amdgpu_waves_per_eu variant of k_render_exact
    int occ_req = 0;        // opts.occupancy as given (0 = each kernel's default)
    int kernel_req = PBRT_KERNEL_AUTO;
    int last_kernel = 0;    // stats.kernel of the last frame (pbrtroute::last_kernel of its route)
    DevBuf<pbrtk::PcgJump> d_jump;
    pbrt_distribution_desc host_dist;
    // the last frame's route (frame_route.h) and what it fixes for every launch: whether the scene
    // is triangle meshes only, and the dynamic-LDS layouts of k_mb_setup (L), k_chain_ci /
    // k_dl_setup (Lci) and k_chain_cam / k_cam_setup (Lcam)
    pbrtroute::Route route = pbrtroute::Route::Serial;
    bool mesh_only = false;
    struct {
        pbrtk::ChainLayout L{}, Lci{}, Lcam{};
    } lay;
    // wave-parallel path (k_wf_primary, k_chain_ci, k_paths_ci / k_pw_*, k_film)
    DevBuf<unsigned char> d_wave;      // per-batch pixel records, stratified values, RNG states, L
    int64_t wave_batch = 0;            // tile slots per batch
    int tiles_per_wave = 1;            // k_chain_ci lane groups per wave (64 / lanes per tile)
    std::vector<hipEvent_t> bev;       // per batch: before the chain, after the chain, after the paths
    int n_batches = 0;
    pbrtk::WaveBufs wb{};
    // device scene
    DevBuf<pbrt_shape_desc> d_shapes;
    DevBuf<pbrt_material_desc> d_materials;
    DevBuf<pbrt_primitive_desc> d_prims;
    DevBuf<pbrtk::DevNode> d_nodes;
    DevBuf<uint32_t> d_order;        // [8][n_nodes] preorder visit tables, then [8][n_nodes] leaf lists (dev_order)
    DevBuf<double> d_groups;         // leaf culling groups (cull_groups)
    DevBuf<uint32_t> d_gmasks;
    int n_groups = 0;
    std::vector<int> h_node_prims;   // nPrimitives per node (leaf count for DevScene)
    DevBuf<pbrtk::DevPrim> d_fprims;
    DevBuf<pbrt_light_desc> d_lights;
    DevBuf<pbrt_camera_desc> d_camera;
    DevBuf<pbrt_film_desc> d_film;
    DevBuf<pbrt_distribution_desc> d_dist;
    pbrt_scene_desc host_scene;   // counts + film/camera (pointer fields are not kept)
    std::vector<pbrt_light_desc> host_lights;
    // per-render buffers (grown on demand)
    DevBuf<double> d_films;
    DevBuf<double> d_s1d;
    DevBuf<pbrtk::PanicRec> d_panics;
    DevBuf<pbrtk::Counters> d_ctr;
    // path wavefront (k_pw_*, PBRT_PATHS_WF=1): path records, queues, counters,
    // bounce-1 light estimates, per-pixel panic keys (grown on demand)
    DevBuf<unsigned char> d_pw;
    DevBuf<double> d_out;
    // last render
    pbrtk::RenderParams rp{};
    bool rendered = false;
    // cancellation (pbrt_gpu_cancel): a flag in fine-grained host memory the
    // kernels poll; it belongs to the render in flight (render_async entry to
    // synchronize) and is cleared when that render ends, so a cancel never
    // outlives its render and never reaches the next one
    struct {
        std::mutex mu;
        bool in_flight = false;
        bool req = false;
        int* h_flag = nullptr;   // hipHostMalloc (coherent, mapped)
        int* d_flag = nullptr;   // its device address
        DevBuf<int> d_seen;      // device-memory copy the kernels publish (reset per render)
        // A render begins (in_flight_now) or has ended: the flag is cleared either
        // way. Returns whether the render that was in flight had been cancelled.
        bool reset(bool in_flight_now) {
            std::lock_guard<std::mutex> lk(mu);
            const bool cancelled = in_flight && req;
            in_flight = in_flight_now;
            req = false;
            __atomic_store_n(h_flag, 0, __ATOMIC_SEQ_CST);
            return cancelled;
        }
    } cancel;
    // device-resident queries: the buffers the context owns (pbrt_gpu_buffer;
    // whatever is left is freed by pbrt_gpu_destroy) and the panic record of
    // the queries since the last pbrt_gpu_query_status (allocated by the first)
    pbrtq::BufferList qbufs;
    DevBuf<pbrtk::QueryRec> d_qrec;
    // pbrt_gpu_li_device: the light distribution of the strategy last queried, in a buffer of the
    // query's own (a frame uploads its strategy's to d_dist), uploaded when the strategy changes
    struct {
        DevBuf<pbrt_distribution_desc> d_dist;
        pbrt_distribution_desc host_dist;
        int strategy = 0;   // the strategy d_dist holds (0: none yet)
    } li;
    // pbrt_gpu_direct_li_device: the level records of k_li_direct<true, *>, [workgroup][level][field][lane]
    // (grown on demand; sized by the capped grid and max_depth, direct_li_query.h)
    DevBuf<double> d_dli_levels;
    // pbrt_gpu_film_add_device: the tile films of a call's tile range (grown on demand)
    DevBuf<double> d_fq_films;
    // every kernel launch of the context (pbrt_gpu_launch_log): the last frame's
    // (cleared by render_enqueue) and those outside a frame (LBVH build, queries)
    pbrtk::LaunchLog log_frame, log_aux;
    bool in_frame = false;
    std::string err;
    std::chrono::steady_clock::time_point t_start;
};

#pragma GCC visibility push(hidden)

inline int set_err(pbrt_gpu_ctx* c, int code, const std::string& m) {
    if (c) c->err = m;
    return code;
}

// Every launch of a context: the record (launch_log.h), then hipLaunchKernelGGL.
template <class... P, class... A>
inline void launch_k(pbrt_gpu_ctx* c, void (*kern)(P...), dim3 grid, dim3 block, unsigned lds, hipStream_t st, A&&... args) {
    const int sid = st == c->stream ? 0 : st == c->stream2 ? 2 : 3;
    pbrtk::launch_logged(c->in_frame ? &c->log_frame : &c->log_aux, sid, kern, grid, block, lds, st, std::forward<A>(args)...);
}

// the scene view a kernel reads (render.hip); with_dist: with the frame's light distribution
pbrtk::DevScene dev_scene(const pbrt_gpu_ctx* c, bool with_dist);

// The scene view a launch passes, tagged with its kernel's counter set for
// the mesh-traversal counting build (PBRT_MESH_COUNT; ignored otherwise):
// 1 k_wf_primary, 2 k_chain_ci, 3 k_paths_ci / k_pw_* EXACT, 4 k_mb_setup,
// 5 k_paths_ci / k_pw_* THROUGHPUT, 6 k_render_exact, 7 k_intersect.
inline pbrtk::DevScene with_slot(pbrtk::DevScene s, int slot) {
    s.mesh.count_slot = slot;
    return s;
}

// A query may go on the stream only between frames: a frame in flight owns the
// context's counters and buffers, and its kernels may be waiting on one another
// across the context's streams.
inline bool query_blocked(pbrt_gpu_ctx* c) {
    std::lock_guard<std::mutex> lk(c->cancel.mu);
    return c->cancel.in_flight;
}

#pragma GCC visibility pop

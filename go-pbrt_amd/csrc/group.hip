// group.hip — device groups (pbrt_gpu_group, include/pbrt_gpu.h): one scene on
// several GPUs, one frame, one film.
//
// A group is N single-context renderers (members) and a merge. The caller's
// tiles are split over the members by group_map.h; every member renders its
// share through pbrt_gpu_render_async_into / pbrt_gpu_synchronize, unchanged,
// and keeps its tile films in its device memory. When every member's
// synchronize has returned, k_merge_film_group (k_group.hip) on the leader
// (member 0) adds all tile films in tile-index order, reading them over peer
// access or from a staging copy on the leader.
//
// Threads: one worker per distinct device and frame (the current HIP device is
// per thread, and a member's enqueue and synchronize block in places). A worker
// runs its device's members strictly one after the other: a context's path
// stage waits on the progress of chains on another of its own streams (k_gate),
// so two contexts competing for one GPU's hardware queues could starve each
// other into the stall re-render. Nothing here waits on the device for another
// member's kernel; the merge is launched after the host has seen every member
// end (its synchronize also ran any stall re-render, so the tile films are final).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pbrt_gpu.h"
#include "render_kernels.h"

using pbrtk::GroupFilms;
using pbrtk::GroupMemberView;
using pbrtk::RenderParams;

struct pbrt_gpu_group {
    int n = 0;
    pbrt_gpu_ctx* m[PBRT_GROUP_MAX] = {};
    int dev[PBRT_GROUP_MAX] = {};
    bool staged[PBRT_GROUP_MAX] = {};   // the merge reads this member's films from d_stage (no peer access, or PBRT_GROUP_STAGE=1)
    // on the leader's device
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double* d_out = nullptr;
    size_t out_cap = 0;
    double* d_stage[PBRT_GROUP_MAX] = {};
    size_t stage_cap[PBRT_GROUP_MAX] = {};
    // the frame in flight
    pbrt_render_desc rd{};
    pbrtgroup::GroupMap map{};
    double* target = nullptr;          // caller's film buffer on the leader (render_async), else d_out
    std::vector<std::thread> workers;
    bool pending = false;              // render_async without its synchronize yet
    int rc[PBRT_GROUP_MAX] = {};
    pbrt_gpu_stats st[PBRT_GROUP_MAX] = {};
    std::chrono::steady_clock::time_point t_start;
    // cancellation: belongs to the frame in flight, as a context's does
    std::mutex mu;
    bool in_flight = false;
    std::atomic<bool> cancel_req{false};
    // last frame
    bool rendered = false;
    int64_t film_doubles = 0;
    std::string err;
};

namespace {

int group_err(pbrt_gpu_group* g, int code, const std::string& m) {
    if (g) g->err = m;
    return code;
}
#define GROUP_HIPCHK(grp, call)                                                                          \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return group_err(grp, PBRT_E_HIP, std::string("group: " #call ": ") + hipGetErrorString(e_)); \
    } while (0)

std::string member_name(const pbrt_gpu_group* g, int i) {
    return "member " + std::to_string(i) + " (device " + std::to_string(g->dev[i]) + ")";
}

// one device's members, one after the other
void run_members(pbrt_gpu_group* g, std::vector<int> members) {
    bool dead = false;   // a member's HIP error: the device's remaining members are not started
    for (int i : members) {
        std::memset(&g->st[i], 0, sizeof(g->st[i]));
        if (dead) {
            g->rc[i] = PBRT_E_HIP;
            continue;
        }
        if (g->cancel_req.load()) {
            g->rc[i] = PBRT_E_CANCELLED;
            continue;
        }
        pbrt_render_desc rd = g->rd;
        pbrtgroup::group_member_tiles(g->map, i, rd.tile_begin, rd.tile_end, rd.tile_stride);
        int rc = pbrt_gpu_render_async_into(g->m[i], &rd, nullptr);
        if (rc == PBRT_OK) {
            // a cancel that came before this member's render was in flight did not reach it
            if (g->cancel_req.load()) pbrt_gpu_cancel(g->m[i]);
            rc = pbrt_gpu_synchronize(g->m[i], &g->st[i]);
        }
        g->rc[i] = rc;
        dead = rc == PBRT_E_HIP;
    }
}

void join_workers(pbrt_gpu_group* g) {
    for (std::thread& t : g->workers)
        if (t.joinable()) t.join();
    g->workers.clear();
}

template <class T>
int group_ensure(pbrt_gpu_group* g, T** buf, size_t* cap, size_t n) {
    if (*cap >= n && *buf) return PBRT_OK;
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    GROUP_HIPCHK(g, hipMalloc((void**)buf, sizeof(T) * (n ? n : 1)));
    *cap = n;
    return PBRT_OK;
}

// every member's frame has ended without error, panic or cancel: merge on the leader
int merge_films(pbrt_gpu_group* g, float& merge_ms) {
    GROUP_HIPCHK(g, hipSetDevice(g->dev[0]));
    const GroupMemberView lead = pbrt_group_member_view(g->m[0]);
    RenderParams rp = lead.rp;
    {   // the split was made before the leader laid out its frame: both must see the same tile grid
        const pbrtgroup::GroupMap chk = pbrtgroup::group_map_make(rp.ntx * rp.nty, g->rd.tile_begin, g->rd.tile_end,
                                                                  g->rd.tile_stride, g->n);
        if (chk.begin != g->map.begin || chk.end != g->map.end || chk.stride != g->map.stride ||
            chk.n_tiles != g->map.n_tiles)
            return group_err(g, PBRT_E_INVALID, "group: tile grid differs from the leader's");
    }
    rp.tile_begin = g->map.begin;
    rp.tile_stride = g->map.stride;
    rp.n_slots = g->map.n_tiles;
    const size_t slot_doubles = (size_t)(rp.slot_w * rp.slot_h * 3);
    g->film_doubles = rp.film_w * rp.film_h * 3;
    int rc = PBRT_OK;
    if (!g->target && (rc = group_ensure(g, &g->d_out, &g->out_cap, (size_t)g->film_doubles))) return rc;
    double* out = g->target ? g->target : g->d_out;
    GroupFilms films;
    GROUP_HIPCHK(g, hipEventRecord(g->ev0, g->stream));
    for (int i = 0; i < PBRT_GROUP_MAX; i++) films.p[i] = nullptr;
    for (int i = 0; i < g->n; i++) {
        const GroupMemberView v = pbrt_group_member_view(g->m[i]);
        const int64_t slots = pbrtgroup::group_member_slots(g->map, i);
        if (v.rp.n_slots != slots || v.rp.slot_w != rp.slot_w || v.rp.slot_h != rp.slot_h)
            return group_err(g, PBRT_E_INVALID, "group: " + member_name(g, i) + " rendered another tile subset");
        films.p[i] = v.d_films;
        if (!g->staged[i] || slots == 0) continue;
        const size_t nd = (size_t)slots * slot_doubles;
        if ((rc = group_ensure(g, &g->d_stage[i], &g->stage_cap[i], nd))) return rc;
        if (g->dev[i] == g->dev[0])
            GROUP_HIPCHK(g, hipMemcpyAsync(g->d_stage[i], v.d_films, nd * sizeof(double), hipMemcpyDeviceToDevice,
                                           g->stream));
        else
            GROUP_HIPCHK(g, hipMemcpyPeerAsync(g->d_stage[i], g->dev[0], v.d_films, g->dev[i], nd * sizeof(double),
                                               g->stream));
        films.p[i] = g->d_stage[i];
    }
    const int64_t npx = rp.film_w * rp.film_h;
    if (npx > 0) {
        hipLaunchKernelGGL(pbrtk::k_merge_film_group, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, g->stream,
                           lead.d_film, rp, g->map, films, out);
        GROUP_HIPCHK(g, hipGetLastError());
    }
    GROUP_HIPCHK(g, hipEventRecord(g->ev1, g->stream));
    GROUP_HIPCHK(g, hipStreamSynchronize(g->stream));
    (void)hipEventElapsedTime(&merge_ms, g->ev0, g->ev1);
    return PBRT_OK;
}

}  // namespace

extern "C" {

int pbrt_gpu_group_create(const pbrt_scene_desc* scene, const pbrt_gpu_opts* opts, const int32_t* devices,
                          int32_t n_devices, pbrt_gpu_group** out) {
    if (!out) return PBRT_E_INVALID;
    *out = nullptr;
    if (!scene || !devices || n_devices < 1 || n_devices > PBRT_GROUP_MAX) return PBRT_E_INVALID;
    for (int i = 0; i < n_devices; i++)
        if (devices[i] < 0) return PBRT_E_INVALID;
    auto* g = new pbrt_gpu_group();
    g->n = n_devices;
    // PBRT_GROUP_STAGE=1: every member but the leader is merged from a staging copy
    // (the path taken where peer access is refused); read once, here
    const char* e = getenv("PBRT_GROUP_STAGE");
    const bool stage_all = e && atoi(e) != 0;
    int rc = PBRT_OK;
    for (int i = 0; i < n_devices && rc == PBRT_OK; i++) {
        pbrt_gpu_opts o;
        std::memset(&o, 0, sizeof(o));
        if (opts) o = *opts;
        o.device = g->dev[i] = devices[i];
        rc = pbrt_gpu_create(scene, &o, &g->m[i]);
    }
    if (rc == PBRT_OK && hipSetDevice(g->dev[0]) != hipSuccess) rc = PBRT_E_HIP;
    for (int i = 1; i < n_devices && rc == PBRT_OK; i++) {
        g->staged[i] = stage_all;
        if (stage_all || g->dev[i] == g->dev[0]) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, g->dev[0], g->dev[i]) != hipSuccess) can = 0;
        if (can) {
            const hipError_t pe = hipDeviceEnablePeerAccess(g->dev[i], 0);
            if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) can = 0;
        }
        (void)hipGetLastError();   // "already enabled" and a refusal are both handled: clear the sticky error
        g->staged[i] = !can;
    }
    if (rc == PBRT_OK &&
        (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess ||
         hipEventCreate(&g->ev0) != hipSuccess || hipEventCreate(&g->ev1) != hipSuccess))
        rc = PBRT_E_HIP;
    if (rc != PBRT_OK) {
        pbrt_gpu_group_destroy(g);
        return rc;
    }
    *out = g;
    return PBRT_OK;
}

int pbrt_gpu_group_render_async(pbrt_gpu_group* g, const pbrt_render_desc* rd, double* film_device) {
    if (!g) return PBRT_E_INVALID;
    if (g->pending) return group_err(g, PBRT_E_INVALID, "group: the previous frame was not synchronized");
    if (!rd) return group_err(g, PBRT_E_INVALID, "group: null render desc");
    if (rd->tile_size <= 0) return group_err(g, PBRT_E_INVALID, "group: bad tile size");
    {
        std::lock_guard<std::mutex> lk(g->mu);
        g->in_flight = true;
        g->cancel_req.store(false);
    }
    g->t_start = std::chrono::steady_clock::now();
    g->rd = *rd;
    g->target = film_device;
    g->rendered = false;
    const pbrt_film_desc& f = *pbrt_group_member_view(g->m[0]).host_film;
    const int64_t ntx = (f.crop_max_x - f.crop_min_x + rd->tile_size - 1) / rd->tile_size;
    const int64_t nty = (f.crop_max_y - f.crop_min_y + rd->tile_size - 1) / rd->tile_size;
    g->map = pbrtgroup::group_map_make(ntx * nty, rd->tile_begin, rd->tile_end, rd->tile_stride, g->n);
    bool taken[PBRT_GROUP_MAX] = {};
    g->pending = true;
    for (int i = 0; i < g->n; i++) {
        if (taken[i]) continue;
        std::vector<int> members;
        for (int j = i; j < g->n; j++)
            if (g->dev[j] == g->dev[i]) {
                members.push_back(j);
                taken[j] = true;
            }
        g->workers.emplace_back(run_members, g, std::move(members));
    }
    return PBRT_OK;
}

int pbrt_gpu_group_synchronize(pbrt_gpu_group* g, pbrt_gpu_stats* stats) {
    if (!g) return PBRT_E_INVALID;
    if (!g->pending) return group_err(g, PBRT_E_INVALID, "group: no frame in flight");
    join_workers(g);
    g->pending = false;
    {   // the frame's members have ended: its cancel dies with it
        std::lock_guard<std::mutex> lk(g->mu);
        g->in_flight = false;
        g->cancel_req.store(false);
    }
    pbrt_gpu_stats st;
    std::memset(&st, 0, sizeof(st));
    int rc = PBRT_OK;
    bool cancelled = false;
    int panic_of = -1;
    for (int i = 0; i < g->n; i++) {
        const pbrt_gpu_stats& s = g->st[i];
        st.tiles_rendered += s.tiles_rendered;
        st.camera_samples += s.camera_samples;
        st.paths_traced += s.paths_traced;
        st.rays_closest += s.rays_closest;
        st.rays_shadow += s.rays_shadow;
        st.kernel_ms = std::max(st.kernel_ms, s.kernel_ms);
        st.chain_ms = std::max(st.chain_ms, s.chain_ms);
        st.paths_ms = std::max(st.paths_ms, s.paths_ms);
        st.batches = std::max(st.batches, s.batches);
        if (!st.kernel && s.tiles_rendered) st.kernel = s.kernel;
        if (g->rc[i] == PBRT_E_CANCELLED) {
            cancelled = true;
        } else if (g->rc[i] == PBRT_E_REF_PANIC) {
            if (panic_of < 0 || s.panic_tile < g->st[panic_of].panic_tile) panic_of = i;
        } else if (g->rc[i] != PBRT_OK && rc == PBRT_OK) {   // a member's error is the group's
            rc = group_err(g, g->rc[i], member_name(g, i) + ": " + pbrt_gpu_last_error(g->m[i]));
        }
    }
    if (!st.kernel) st.kernel = g->st[0].kernel;
    if (rc == PBRT_OK && cancelled) {
        std::memset(&st, 0, sizeof(st));
        rc = group_err(g, PBRT_E_CANCELLED, "cancelled by pbrt_gpu_group_cancel");
    } else if (rc == PBRT_OK && panic_of >= 0) {
        const pbrt_gpu_stats& s = g->st[panic_of];
        st.panic_kind = s.panic_kind;
        st.panic_tile = s.panic_tile;
        st.panic_pixel_x = s.panic_pixel_x;
        st.panic_pixel_y = s.panic_pixel_y;
        st.panic_sample = s.panic_sample;
        st.panic_bounce = s.panic_bounce;
        rc = group_err(g, PBRT_E_REF_PANIC, member_name(g, panic_of) + ": the Go reference panics on this input");
    } else if (rc == PBRT_OK) {
        float ms = 0;
        rc = merge_films(g, ms);
        st.merge_ms = ms;
        g->rendered = rc == PBRT_OK;
    }
    st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g->t_start).count();
    if (stats) *stats = st;
    return rc;
}

int pbrt_gpu_group_render(pbrt_gpu_group* g, const pbrt_render_desc* rd, double* film_xyz, pbrt_gpu_stats* stats) {
    if (!g) return PBRT_E_INVALID;
    int rc = pbrt_gpu_group_render_async(g, rd, nullptr);
    if (rc != PBRT_OK) return rc;
    rc = pbrt_gpu_group_synchronize(g, stats);
    if (rc != PBRT_OK) return rc;
    if (film_xyz) return pbrt_gpu_group_film_download(g, film_xyz);
    return PBRT_OK;
}

double* pbrt_gpu_group_film_device(pbrt_gpu_group* g) { return g ? (g->target ? g->target : g->d_out) : nullptr; }

int pbrt_gpu_group_film_download(pbrt_gpu_group* g, double* film_xyz) {
    if (!g || !film_xyz || !g->rendered || g->pending) return PBRT_E_INVALID;
    GROUP_HIPCHK(g, hipSetDevice(g->dev[0]));
    GROUP_HIPCHK(g, hipMemcpy(film_xyz, g->target ? g->target : g->d_out, sizeof(double) * (size_t)g->film_doubles,
                              hipMemcpyDeviceToHost));
    return PBRT_OK;
}

int pbrt_gpu_group_size(const pbrt_gpu_group* g) { return g ? g->n : 0; }

pbrt_gpu_ctx* pbrt_gpu_group_member(pbrt_gpu_group* g, int i) { return g && i >= 0 && i < g->n ? g->m[i] : nullptr; }

int pbrt_gpu_group_member_stats(pbrt_gpu_group* g, int i, pbrt_gpu_stats* stats) {
    if (!g || !stats || i < 0 || i >= g->n || g->pending) return PBRT_E_INVALID;
    *stats = g->st[i];
    return PBRT_OK;
}

void pbrt_gpu_group_cancel(pbrt_gpu_group* g) {
    if (!g) return;
    std::lock_guard<std::mutex> lk(g->mu);
    if (!g->in_flight) return;   // nothing to cancel: no frame is in flight
    // the flag first: a worker that enqueues a member after this sees it, and a
    // member already in flight takes the call below
    g->cancel_req.store(true);
    for (int i = 0; i < g->n; i++) pbrt_gpu_cancel(g->m[i]);
}

const char* pbrt_gpu_group_last_error(const pbrt_gpu_group* g) { return g ? g->err.c_str() : "null group"; }

void pbrt_gpu_group_destroy(pbrt_gpu_group* g) {
    if (!g) return;
    if (g->pending) {   // a frame nobody waited for: end it
        pbrt_gpu_group_cancel(g);
        join_workers(g);
    }
    if (g->stream) {
        (void)hipSetDevice(g->dev[0]);
        (void)hipStreamSynchronize(g->stream);
    }
    for (int i = 0; i < g->n; i++)
        if (g->m[i]) pbrt_gpu_destroy(g->m[i]);
    if (g->stream || g->d_out) (void)hipSetDevice(g->dev[0]);
    for (double* b : g->d_stage)
        if (b) (void)hipFree(b);
    if (g->d_out) (void)hipFree(g->d_out);
    if (g->ev0) (void)hipEventDestroy(g->ev0);
    if (g->ev1) (void)hipEventDestroy(g->ev1);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
}

}  // extern "C"

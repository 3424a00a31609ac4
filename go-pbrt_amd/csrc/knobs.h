// knobs.h — the experiment knobs of a context and their parsing from the
// environment. No HIP: tests/host_tables_check.cpp compiles this header on its own.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace pbrt {

// Experiment knobs (environment), read ONCE when a context is created
// (pbrt_gpu_create), never per launch; defaults are the measured best.
struct Knobs {
    int ci_waves = 0;          // PBRT_CI_WAVES = 1, 2, 4, 8 (0: by tile count)
    int ci_stride = 0;         // PBRT_CI_STRIDE = 1, 2 (0: 2 at one wave per tile, else 1)
    int ci_heavy_waves = 4;    // PBRT_CI_HEAVY_WAVES = 4, 8
    bool ci_light_kw = false;  // PBRT_CI_LIGHT_KW=1: a multi-wave shard's split runs its light tiles at the
                               // shard's waves per tile (not 1), the heavy ones at PBRT_CI_HEAVY_WAVES
    int ci_split8 = 32;        // PBRT_CI_SPLIT8=K: a learned multi-wave Matte shard that fits the wave slots
                               // (no split otherwise: 1/8 of B) runs its K heaviest tiles (at most 1/16 of
                               // them) at 8 waves beside the rest at its waves per tile; 0: off
    int ci_eu = 0;             // PBRT_CI_EU = 2 / 3: the one-wave Matte chain's build (waves/SIMD its registers
                               // are budgeted for); 0: by the workgroup's LDS (ci_eu3_fits)
    int64_t ci_heavy = -1;     // PBRT_CI_HEAVY = K forces the heavy tile count (tests)
    bool ci_split = true;      // PBRT_CI_SPLIT=0
    bool ci_order = true;      // PBRT_CI_ORDER=0
    bool ci_probe = true;      // PBRT_CI_PROBE=0
    bool ci_order_cache = true;// PBRT_CI_ORDER_CACHE=0
    bool sp_window = true;     // PBRT_SP_WINDOW=0: the lane-0 StartPixel replay instead of the windowed one
    int ci_scap = -1;          // PBRT_CI_SCAP=Z: k_chain_ci's statistical speculation cap at Z/10 sigmas (0: off;
                               // -1: the kernel's default, 1.5 sigma for mesh scenes; multi-wave tiles with
                               // next-pixel speculation always use 3)
    int ci_nps = 8;            // PBRT_CI_NPS=K: next-pixel speculation in multi-wave k_chain_ci tiles from K
                               // samples before a pixel's end (0: off)
    int paths_overlap = 5;     // PBRT_PATHS_OVERLAP=K: a split frame's path stage runs in K chunks of the
                               // tiles in their chains' completion order, each released when its tiles'
                               // chains have ended (render_enqueue; 0: off, the path stage after the chains)
    bool paths_overlap_all = true;    // PBRT_PATHS_OVERLAP_ALL=0: the completion-driven path stage only for
                               // split frames (measured on: C 5056 -> 4603 ms, G 495 -> 472 ms, the
                               // N=8 shards' max 128.6 -> 119.7 ms)
    bool gate_hold = false;    // PBRT_GATE_HOLD=1 (tests): the light chain launch waits for the path stage,
                               // as a dispatcher that serialises kernels across streams may order them;
                               // k_gate's stall exit and the re-render recover the frame
    bool paths_s1d_lds = false;// PBRT_PATHS_S1D=lds
    int paths_ci = -1;         // PBRT_PATHS_CI = 0, 2, 4, 8 (-1: auto)
    int paths_wf = -1;         // PBRT_PATHS_WF = 0 / 1 (-1: mesh scenes)
    bool pw_sort = false;      // PBRT_PW_SORT=1
    double pw_gb = 24.0;       // PBRT_PW_GB
    double wave_buffer_gb = 0; // PBRT_WAVE_BUFFER_GB (0: min(96 GB, half the free HBM))
    bool ci_dense = false;     // PBRT_CI_DENSE=1 (builds with -DPBRT_CI_DENSE_WALK): k_chain_ci's closest hit by
                               // bvh_walk_dense (bit-exact; slower on B)
    int cull_group = 4;        // PBRT_CULL_GROUP: leaves per culling group
    int cull_min = 2;          // PBRT_CULL_MIN
    bool cull_groups = true;   // PBRT_CULL_GROUPS=0
    bool film_add_lds = true;  // PBRT_FILM_ADD=direct: pbrt_gpu_film_add_device's tile films by the direct gather
                               // (k_film_add_tiles<false>) where the LDS-staged one would run
    int direct_li_grid = 8192; // PBRT_DIRECT_LI_GRID=K: pbrt_gpu_direct_li_device's grid cap, 1 .. 65536 workgroups of
                               // one wave, each striding over the work lists beyond; it bounds the kX kernels'
                               // level records (direct_li_query.h). Measured on 2 M rays: 2048 is 7 % (Matte)
                               // and 10 % (kX) slower, 16384 and more level
    static Knobs from_env() {
        Knobs k;
        auto ival = [](const char* n, int& out) { if (const char* e = getenv(n)) out = atoi(e); };
        if (const char* e = getenv("PBRT_CI_WAVES")) {
            const int v = atoi(e);
            if (v == 1 || v == 2 || v == 4 || v == 8) k.ci_waves = v;
        }
        if (const char* e = getenv("PBRT_CI_STRIDE")) {
            const int v = atoi(e);
            if (v == 1 || v == 2) k.ci_stride = v;
        }
        if (const char* e = getenv("PBRT_CI_HEAVY_WAVES")) k.ci_heavy_waves = atoi(e) == 8 ? 8 : 4;
        if (const char* e = getenv("PBRT_CI_LIGHT_KW")) k.ci_light_kw = atoi(e) != 0;
        if (const char* e = getenv("PBRT_CI_SPLIT8")) k.ci_split8 = std::max(0, atoi(e));
        if (const char* e = getenv("PBRT_CI_EU")) k.ci_eu = (atoi(e) == 2 || atoi(e) == 3) ? atoi(e) : 0;
        if (const char* e = getenv("PBRT_CI_HEAVY")) k.ci_heavy = (int64_t)atoll(e);
        if (const char* e = getenv("PBRT_CI_SPLIT")) k.ci_split = atoi(e) != 0;
        if (const char* e = getenv("PBRT_CI_DENSE")) k.ci_dense = atoi(e) != 0;
        if (const char* e = getenv("PBRT_CI_ORDER")) k.ci_order = atoi(e) != 0;
        if (const char* e = getenv("PBRT_CI_PROBE")) k.ci_probe = atoi(e) != 0;
        if (const char* e = getenv("PBRT_CI_ORDER_CACHE")) k.ci_order_cache = atoi(e) != 0;
        if (const char* e = getenv("PBRT_SP_WINDOW")) k.sp_window = atoi(e) != 0;
        if (const char* e = getenv("PBRT_CI_NPS")) k.ci_nps = std::max(0, atoi(e));
        if (const char* e = getenv("PBRT_CI_SCAP")) k.ci_scap = std::max(-1, atoi(e));
        if (const char* e = getenv("PBRT_PATHS_OVERLAP")) k.paths_overlap = std::min(std::max(0, atoi(e)), 16);
        if (const char* e = getenv("PBRT_PATHS_OVERLAP_ALL")) k.paths_overlap_all = atoi(e) != 0;
        if (const char* e = getenv("PBRT_GATE_HOLD")) k.gate_hold = atoi(e) != 0;
        if (const char* e = getenv("PBRT_PATHS_S1D")) k.paths_s1d_lds = std::strcmp(e, "lds") == 0;
        if (const char* e = getenv("PBRT_PATHS_CI")) {
            const int v = atoi(e);
            if (v == 0 || v == 2 || v == 4 || v == 8) k.paths_ci = v;
        }
        if (const char* e = getenv("PBRT_PATHS_WF")) k.paths_wf = atoi(e) == 1 ? 1 : 0;
        if (const char* e = getenv("PBRT_PW_SORT")) k.pw_sort = atoi(e) == 1;
        if (const char* e = getenv("PBRT_PW_GB")) k.pw_gb = atof(e) > 0 ? atof(e) : k.pw_gb;
        if (const char* e = getenv("PBRT_WAVE_BUFFER_GB")) k.wave_buffer_gb = atof(e) > 0 ? atof(e) : 0;
        if (const char* e = getenv("PBRT_CULL_GROUP")) k.cull_group = std::max(2, atoi(e));
        if (const char* e = getenv("PBRT_CULL_MIN")) k.cull_min = std::max(0, atoi(e));
        int cg = 1;
        ival("PBRT_CULL_GROUPS", cg);
        k.cull_groups = cg != 0;
        if (const char* e = getenv("PBRT_FILM_ADD")) k.film_add_lds = std::strcmp(e, "direct") != 0;
        if (const char* e = getenv("PBRT_DIRECT_LI_GRID")) k.direct_li_grid = std::min(std::max(1, atoi(e)), 65536);
        return k;
    }
};

}  // namespace pbrt

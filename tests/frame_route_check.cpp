// tests/frame_route_check.cpp — host check of the rules that decide what a frame launches
// (go-pbrt_amd/csrc/frame_route.h, render_params.h). Built alone, no HIP, under ASan + UBSan
// (tests/test_frame_route_host.py). Every property is held against brute force written here or
// against a recorded value: the refusal texts are the parent commit's, the launches are lines of
// profiles/frame_route/launches_parent.json (tools/dump_launch_logs.py on one MI355X), the static
// LDS is profiles/frame_route/kernel_resources_parent.json's.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../go-pbrt_amd/csrc/frame_route.h"

using namespace pbrtroute;

static long g_checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        g_checks++;                                                              \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)
#define CHECK_STR(got, want)                                                                              \
    do {                                                                                                  \
        g_checks++;                                                                                       \
        const std::string g_ = (got), w_ = (want);                                                        \
        if (g_ != w_) {                                                                                   \
            std::fprintf(stderr, "FAIL %s:%d:\n  got  %s\n  want %s\n", __FILE__, __LINE__, g_.c_str(), w_.c_str()); \
            std::exit(1);                                                                                 \
        }                                                                                                 \
    } while (0)
static void section(const char* name) {
    std::printf("ok %s %ld\n", name, g_checks);
    g_checks = 0;
}

// sizeof of the device structs (gfx950 build of the parent commit)
static const Sizes kSz{408, 416, 32, 40, 320, 24, 16};   // ChainCache PixelRec PanicRec RrBranches PwPath Spec RingEnt
// static LDS of k_chain_ci<1, depth, false, 0, false, multi> (kernel_resources_parent.json)
static size_t static_lds_of(int depth, bool multi) {
    return depth == 0 ? (multi ? 6784 : 6560) : (multi ? 14960 : 14736);
}

static pbrt_film_desc film(int64_t w, int64_t h, double r = 1.0) {
    pbrt_film_desc f{};
    f.res_x = w;
    f.res_y = h;
    f.crop_max_x = w;
    f.crop_max_y = h;
    f.filter_radius_x = f.filter_radius_y = r;
    return f;
}
static pbrt_render_desc desc(int sx, int sy, int n_dims = 4, bool jitter = false, int max_depth = 10) {
    pbrt_render_desc rd{};
    rd.sampler_x = sx;
    rd.sampler_y = sy;
    rd.jitter = jitter;
    rd.n_dims = n_dims;
    rd.integrator = PBRT_INTEGRATOR_PATH;
    rd.max_depth = max_depth;
    rd.light_strategy = 1;
    rd.dl_strategy = PBRT_DL_UNIFORM_SAMPLE_ALL;
    rd.rr_threshold = 1.0;
    rd.tile_size = 16;
    rd.tile_stride = 1;
    return rd;
}
static Facts matte_facts(int n_nodes = 45, int n_lights = 4) {   // the README scene on an MI355X
    Facts f;
    f.n_prims = (n_nodes + 1) / 2;
    f.n_nodes = n_nodes;
    f.n_lights = n_lights;
    f.n_materials = 22;
    f.n_simd = 1024;
    f.lds_per_block = 65536;
    f.lds_per_cu = 160 * 1024;
    return f;
}
static pbrt_distribution_desc uniform_dist(int n) {
    pbrt_distribution_desc d{};
    d.count = n;
    for (int i = 0; i < n; i++) d.func[i] = 1.0;
    d.func_int = n > 0 ? 1.0 : 0.0;
    return d;
}

// ---------------------------------------------------------------- layouts
struct Region {
    int off;
    int64_t bytes;
};
// every offset 16-byte aligned, the regions in order without overlap, `end` the aligned end of the last
static void check_regions(const std::vector<Region>& r, int64_t end) {
    int64_t at = 0;
    for (const Region& x : r) {
        CHECK(x.off % 16 == 0);
        CHECK(x.off >= at);       // disjoint from everything before it
        CHECK(x.off - at < 16);   // and no hole beyond the alignment
        at = x.off + x.bytes;
    }
    CHECK(end == ((at + 15) & ~int64_t(15)));
}
static int64_t vbuf_bytes(const RenderParams& rp) {   // sp_vbuf_bytes, restated
    if (rp.sp_window) return (((int64_t)rp.ndims * rp.spp * 2 + 15) / 16) * 16 + 256 * 4;
    return rp.sp_serial ? 4 : (int64_t)rp.sp_draws * 4;
}
static void check_layouts() {
    const Knobs k;
    int lci_branch[3][2] = {};   // [values staged | picks only | serial][staging <= / > PBRT_CI_STAGE_KB]
    for (int nd : {0, 1, 2, 5})
        for (int s : {1, 2, 8, 16, 32, 64})   // spp 1, 4, 64, 256, 1024, 4096
            for (bool jitter : {false, true}) {
                const Facts f = matte_facts();
                const pbrt_render_desc rd = desc(s, s, nd, jitter);
                const RenderParams rp = render_params(f, k, film(64, 64), rd, 64);
                const int64_t n = rp.spp, v8 = nd * n * 8, v2 = nd * n * 2, vb = vbuf_bytes(rp);
                CHECK(vb == sp_vbuf_bytes(rp));
                if ((int64_t)nd * n <= 8192) {   // (beyond: no wave route, the layouts are never built)
                    const ChainLayout L = layout_L(rp);
                    check_regions({{L.s1d, v8}, {L.other, v2}, {L.sbuf, 64 * 8}, {L.dbuf, 64 * 4}, {L.vbuf, vb}}, L.total);
                    CHECK(L.ring == 0 && L.staging == 0 && L.pcs == 0);

                    const ChainLayout C = layout_Lci(rp);
                    const int64_t full = ((v8 + 15) & ~15) + ((v2 + 15) & ~15) + ((vb + 15) & ~15);
                    const bool big = full > PBRT_CI_STAGE_KB * 1024;
                    if (rp.sp_serial && !rp.sp_window) {   // the serial StartPixel: nothing but a 16-byte scratch
                        check_regions({{C.other, 16}, {C.vbuf, vb}}, C.staging);
                        CHECK(C.s1d == -1);
                        lci_branch[2][big]++;
                    } else if (rp.sp_window || big) {
                        check_regions({{C.other, v2}, {C.vbuf, vb}}, C.staging);
                        CHECK(C.s1d == -1);
                        lci_branch[1][big]++;
                    } else {
                        check_regions({{C.s1d, v8}, {C.other, v2}, {C.vbuf, vb}}, C.staging);
                        lci_branch[0][big]++;
                    }
                    CHECK(C.ring == C.staging && C.total == C.staging + kCiRingBytes && C.sbuf == 0 && C.dbuf == 0);
                }
                if (nd <= 1) {
                    const ChainLayout M = layout_Lcam(rp);
                    std::vector<Region> r;
                    if (!rp.sp_serial && nd > 0) r.push_back({M.s1d, v8});
                    else CHECK(M.s1d == -1);
                    r.push_back({M.other, rp.sp_serial ? 16 : v2 + 16});
                    r.push_back({M.vbuf, rp.sp_serial ? 4 : vb});
                    check_regions(r, M.staging);
                    CHECK(M.ring == 0 && M.total == std::max(M.staging, kCiRingBytes));
                }
            }
    // values staged / picks only: below the stage limit and (picks only: by size) above it; serial: both sides
    // by the size the staging would have had
    CHECK(lci_branch[0][0] > 0 && lci_branch[0][1] == 0);
    CHECK(lci_branch[1][0] > 0 && lci_branch[2][0] > 0 && lci_branch[2][1] > 0);
    {   // the size branch exactly at the limit: 5 dims of 81 spp stage 8192 bytes (values 3248, picks 816, draws 4128)
        Facts f = matte_facts();
        RenderParams rp = render_params(f, k, film(64, 64), desc(9, 9, 5), 64);
        rp.sp_draws = 1032;   // (a draw count the sampler itself does not reach: the rule reads the bytes alone)
        CHECK(!rp.sp_serial && !rp.sp_window);
        CHECK(layout_Lci(rp).s1d == 0 && layout_Lci(rp).staging == 8192);
        rp.sp_draws = 1033;   // 4 bytes more: one more 16-byte granule, past the limit
        CHECK(layout_Lci(rp).s1d == -1 && layout_Lci(rp).staging == 816 + 4144);
        lci_branch[1][1]++;
    }
    CHECK(lci_branch[1][1] > 0);

    // ci_layout over a base
    const RenderParams rp = render_params(matte_facts(), k, film(64, 64), desc(10, 10), 64);   // 100 spp: values, picks and draws staged, more than one ring
    const ChainLayout base = layout_Lci(rp);
    CHECK(base.staging > kCiRingBytes);
    for (int w : {1, 2, 4, 8})
        for (int G : {1, 2, 4}) {
            if (w > 1 && G > 1) continue;
            unsigned lds = 0;
            const ChainLayout l = ci_layout(base, w, G, lds, kSz.chain_cache);
            if (G == 1) {   // the ring aliases the staging
                CHECK(l.ring == 0 && l.pcs >= std::max(base.staging, w * kCiRingBytes) && l.pcs - std::max(base.staging, w * kCiRingBytes) < 16);
            } else {        // the ring after the staging
                CHECK(l.ring == base.staging && l.pcs >= l.ring + w * kCiRingBytes && l.pcs - (l.ring + w * kCiRingBytes) < 16);
            }
            CHECK(l.pcs % 16 == 0 && l.total == l.pcs + 2 * G * 408 && lds == (unsigned)l.total);
            CHECK(l.s1d == base.s1d && l.other == base.other && l.vbuf == base.vbuf && l.staging == base.staging);
            if (w > 1) {   // next-pixel speculation: two rings after the staging
                const ChainLayout p = ci_layout(base, w, 1, lds, kSz.chain_cache, true);
                CHECK(p.ring % 16 == 0 && p.ring >= base.staging && p.ring - base.staging < 16);
                CHECK(p.pcs == p.ring + 2 * w * kCiRingBytes && p.total == p.pcs + 2 * 408 && lds == (unsigned)p.total);
            }
        }
    section("layouts");
}

// ---------------------------------------------------------------- render_params
static void check_render_params() {
    const Knobs k;
    const Facts f = matte_facts();
    const pbrt_film_desc fd = film(45, 30, 1.5);   // 3 x 2 tiles
    const int64_t total = 6;
    for (int64_t begin : {(int64_t)-1, (int64_t)0, (int64_t)1, total - 1, total, total + 1})
        for (int64_t end : {(int64_t)-1, (int64_t)0, (int64_t)1, total - 1, total, total + 1})
            for (int64_t stride : {(int64_t)0, (int64_t)1, (int64_t)2, total - 1, total, total + 1, (int64_t)100}) {
                pbrt_render_desc rd = desc(2, 2);
                rd.tile_begin = begin;
                rd.tile_end = end;
                rd.tile_stride = stride;
                const RenderParams rp = render_params(f, k, fd, rd, 64);
                const int64_t b = std::max<int64_t>(begin, 0), e = end > 0 && end < total ? end : total,
                              st = stride > 0 ? stride : 1;
                int64_t count = 0;
                for (int64_t t = b; t < e; t += st) count++;
                CHECK(rp.n_slots == count && rp.tile_begin == b && rp.tile_stride == st);
                CHECK(rp.ntx == 3 && rp.nty == 2 && rp.film_w == 45 && rp.film_h == 30);
                CHECK(rp.slot_w == 16 + 2 * 2 && rp.slot_h == 16 + 2 * 2 && rp.spp == 4 && rp.lanes_per_wave == 64);
            }
    // sp_serial: raw draws V = E + 64 + E / 8 over E = ndims * (s1 + s2) events; serial above PBRT_SP_SERIAL_KB
    // of them. ndims 1 without jitter: E = 2 n, V = 2 n + 64 + n / 4: 4096 bytes at n = 426.67: 20 x 21 = 420
    // (V = 1009, 4036 B) stays, 6 x 71 = 426 (V 1022, 4088 B) stays, 7 x 61 = 427 (V 1024, 4096 B) stays,
    // 4 x 107 = 428 (V 1027, 4108 B) is serial
    auto params = [&](int sx, int sy, int nd, bool jitter, const Facts& ff, const Knobs& kk) {
        return render_params(ff, kk, film(16, 16), desc(sx, sy, nd, jitter), 64);
    };
    for (int n : {420, 426, 427, 428, 429}) {
        const RenderParams rp = params(1, n, 1, false, f, k);
        const int64_t V = 2 * n + 64 + (2 * n) / 8;
        CHECK(rp.sp_events == 2 * n && rp.sp_draws == V);
        CHECK(rp.sp_serial == (V * 4 > PBRT_SP_SERIAL_KB * 1024));
    }
    CHECK(params(1, 427, 1, false, f, k).sp_serial == 0 && params(1, 428, 1, false, f, k).sp_serial == 1);
    // sp_window: serial, no jitter, and ndims * n * 4 + 1024 <= PBRT_SP_WINDOW_KB * 1024: ndims 4: n <= 320
    CHECK(params(1, 320, 4, false, f, k).sp_window == 1 && params(1, 321, 4, false, f, k).sp_window == 0);
    CHECK(params(1, 320, 4, false, f, k).sp_serial == 1 && params(1, 321, 4, false, f, k).sp_serial == 1);
    CHECK(params(1, 320, 4, true, f, k).sp_window == 0);   // jitter
    CHECK(params(1, 8, 4, false, f, k).sp_window == 0);    // the wave StartPixel fits: not serial
    {
        Knobs off;
        off.sp_window = false;
        Facts kx = f, deep = f, mesh = f;
        kx.non_matte = true;
        deep.n_nodes = kLdsNodes + 1;
        mesh.mesh = true;
        CHECK(params(1, 320, 4, false, f, off).sp_window == 0 && params(1, 320, 4, false, kx, k).sp_window == 0);
        CHECK(params(1, 320, 4, false, deep, k).sp_window == 0 && params(1, 320, 4, false, mesh, k).sp_window == 0);
        deep.n_nodes = kLdsNodes;
        CHECK(params(1, 320, 4, false, deep, k).sp_window == 1);
    }
    {   // jitter: s1 = 2 n, s2 = 3 n
        const RenderParams rp = params(2, 2, 3, true, f, k);
        CHECK(rp.sp_events == 3 * (8 + 12) && rp.sp_draws == 60 + 64 + 7 && rp.jitter == 1 && rp.xs == 2 && rp.ys == 2);
    }
    {
        Knobs kk;
        kk.ci_scap = 15;
        CHECK(params(2, 2, 4, false, f, kk).ci_scap == 15 && params(2, 2, 4, false, f, kk).ci_nps == 0);
    }
    section("render_params");
}

// ---------------------------------------------------------------- check_render and the route
static void refused(const Refusal& r, int code, const char* text) {
    CHECK(r.code == code);
    CHECK_STR(r.text, text);
}
static void check_route() {
    const Knobs k;
    const Facts f = matte_facts();
    const pbrt_film_desc fd = film(64, 64);
    // check_render: one case per rule, in the rules' order (texts: the parent commit's prepare())
    {
        Facts kx = f;
        kx.non_matte = true;
        pbrt_render_desc rd = desc(2, 2);
        refused(check_render(f, fd, nullptr), PBRT_E_INVALID, "null render desc");
        CHECK(check_render(f, fd, &rd).code == PBRT_OK && check_render(f, fd, &rd).text.empty());
        auto with = [&](auto set) {
            pbrt_render_desc d = desc(2, 2);
            set(d);
            return d;
        };
        pbrt_render_desc d;
        for (auto set : {+[](pbrt_render_desc& x) { x.tile_size = 0; }, +[](pbrt_render_desc& x) { x.sampler_x = 0; },
                         +[](pbrt_render_desc& x) { x.sampler_y = -1; }, +[](pbrt_render_desc& x) { x.n_dims = -1; },
                         +[](pbrt_render_desc& x) { x.n_dims = 65; }}) {
            d = with(set);
            refused(check_render(f, fd, &d), PBRT_E_INVALID, "bad sampler / tile size");
        }
        d = with([](pbrt_render_desc& x) { x.n_dims = 64; });
        CHECK(check_render(f, fd, &d).code == PBRT_OK);
        d = with([](pbrt_render_desc& x) { x.sampler_x = 1024, x.sampler_y = 1025; });
        refused(check_render(f, fd, &d), PBRT_E_INVALID, "spp too large");
        d = with([](pbrt_render_desc& x) { x.sampler_x = 1024, x.sampler_y = 1024; });
        CHECK(check_render(f, fd, &d).code == PBRT_OK);
        d = with([](pbrt_render_desc& x) { x.integrator = 3; });
        refused(check_render(f, fd, &d), PBRT_E_UNSUPPORTED, "unknown integrator");
        d = with([](pbrt_render_desc& x) { x.integrator = PBRT_INTEGRATOR_DIRECT_LIGHTING, x.dl_strategy = 3; });
        refused(check_render(f, fd, &d), PBRT_E_UNSUPPORTED, "unknown DirectLighting strategy");
        d = with([](pbrt_render_desc& x) { x.dl_strategy = 3; });   // a Path render does not read it
        CHECK(check_render(f, fd, &d).code == PBRT_OK);
        d = with([](pbrt_render_desc& x) { x.mode = 2; });
        refused(check_render(f, fd, &d), PBRT_E_INVALID, "unknown mode");
        for (double r : {0.0, -1.0, 16.0}) {
            refused(check_render(f, film(64, 64, r), &rd), PBRT_E_UNSUPPORTED, "filter radius must be in (0, tile_size)");
            pbrt_film_desc fy = film(64, 64);
            fy.filter_radius_y = r;
            refused(check_render(f, fy, &rd), PBRT_E_UNSUPPORTED, "filter radius must be in (0, tile_size)");
        }
        CHECK(check_render(f, film(64, 64, 15.5), &rd).code == PBRT_OK);
        d = with([](pbrt_render_desc& x) { x.flags = PBRT_FLAG_PANIC_FIDELITY; });
        refused(check_render(kx, fd, &d), PBRT_E_UNSUPPORTED, "panic fidelity covers Matte scenes only");
        CHECK(check_render(f, fd, &d).code == PBRT_OK);
        d = with([](pbrt_render_desc& x) { x.integrator = PBRT_INTEGRATOR_DIRECT_LIGHTING, x.max_depth = 65; });
        refused(check_render(kx, fd, &d), PBRT_E_UNSUPPORTED, "DirectLighting through glass: maxDepth must be <= 64");
        CHECK(check_render(f, fd, &d).code == PBRT_OK);
        d.max_depth = 64;
        CHECK(check_render(kx, fd, &d).code == PBRT_OK);
    }

    const pbrt_distribution_desc dist = uniform_dist(4);
    auto go = [&](int req, const Facts& ff, const pbrt_render_desc& rd, const pbrt_distribution_desc& d,
                  const pbrt_film_desc& fl) { return route(req, ff, k, rd, render_params(ff, k, fl, rd, 64), d); };
#define routed(req, ff, rd, want)                                                      \
    do {                                                                               \
        const Routed r_ = go(req, ff, rd, dist, fd);                                   \
        CHECK(r_.refusal.code == PBRT_OK && r_.refusal.text.empty() && r_.route == want); \
    } while (0)
    const char* const kWave_ = "render not eligible for the wave-parallel kernels";
    const std::string kCam = "render not eligible for the camera-start wave kernels: ";
    pbrt_render_desc path = desc(2, 2), tp = desc(2, 2), dl = desc(2, 2), cam = desc(2, 2, 0);
    tp.mode = PBRT_MODE_THROUGHPUT;
    dl.integrator = PBRT_INTEGRATOR_DIRECT_LIGHTING;
    // every route, and the kernel each reports
    routed(PBRT_KERNEL_AUTO, f, path, Route::Chain);
    routed(PBRT_KERNEL_WAVE, f, path, Route::Chain);
    routed(PBRT_KERNEL_WAVEFRONT, f, path, Route::Chain);
    routed(PBRT_KERNEL_WAVE_CI, f, path, Route::Chain);
    routed(PBRT_KERNEL_AUTO, f, tp, Route::Throughput);
    routed(PBRT_KERNEL_WAVE_CI, f, tp, Route::Throughput);
    routed(PBRT_KERNEL_AUTO, f, dl, Route::DirectLighting);
    routed(PBRT_KERNEL_WAVE_DL, f, dl, Route::DirectLighting);
    routed(PBRT_KERNEL_SERIAL, f, path, Route::Serial);
    routed(PBRT_KERNEL_SERIAL, f, dl, Route::Serial);
    routed(PBRT_KERNEL_WAVE_CAM, f, cam, Route::Cam);
    routed(PBRT_KERNEL_AUTO, f, cam, Route::Serial);   // the camera-start route is opt-in
    {
        pbrt_render_desc cam_tp = cam;
        cam_tp.mode = PBRT_MODE_THROUGHPUT;
        routed(PBRT_KERNEL_WAVE_CAM, f, cam_tp, Route::Cam);
        pbrt_render_desc dl_tp = dl;
        dl_tp.mode = PBRT_MODE_THROUGHPUT;
        routed(PBRT_KERNEL_AUTO, f, dl_tp, Route::DirectLighting);
    }
    CHECK(last_kernel(Route::Serial) == PBRT_KERNEL_SERIAL && last_kernel(Route::Chain) == PBRT_KERNEL_WAVE_CI);
    CHECK(last_kernel(Route::Throughput) == PBRT_KERNEL_WAVE && last_kernel(Route::DirectLighting) == PBRT_KERNEL_WAVE_DL);
    CHECK(last_kernel(Route::Cam) == PBRT_KERNEL_WAVE_CAM);
    // every request against a render no wave kernel takes (rough glass)
    {
        Facts rough = f;
        rough.non_matte = rough.rough_glass = true;
        routed(PBRT_KERNEL_AUTO, rough, path, Route::Serial);
        routed(PBRT_KERNEL_SERIAL, rough, path, Route::Serial);
        for (int req : {PBRT_KERNEL_WAVE, PBRT_KERNEL_WAVEFRONT, PBRT_KERNEL_WAVE_CI})
            refused(go(req, rough, path, dist, fd).refusal, PBRT_E_UNSUPPORTED, kWave_);
        refused(go(PBRT_KERNEL_WAVE_DL, rough, dl, dist, fd).refusal, PBRT_E_UNSUPPORTED,
                "render not eligible for the DirectLighting wave kernels");
        refused(go(PBRT_KERNEL_WAVE_CAM, rough, cam, dist, fd).refusal, PBRT_E_UNSUPPORTED,
                (kCam + "Mirror / Glass / OrenNayar materials").c_str());
    }
    // the DirectLighting requests
    for (int req : {PBRT_KERNEL_WAVE, PBRT_KERNEL_WAVEFRONT, PBRT_KERNEL_WAVE_CI})
        refused(go(req, f, dl, dist, fd).refusal, PBRT_E_UNSUPPORTED, "DirectLighting runs on the serial or the k_dl_* kernels");
    refused(go(PBRT_KERNEL_WAVE_DL, f, path, dist, fd).refusal, PBRT_E_UNSUPPORTED,
            "render not eligible for the DirectLighting wave kernels");
    // the wave pipeline's own conditions: AUTO falls back to the serial kernel, WAVE_CI is refused
    auto not_wave = [&](const Facts& ff, const pbrt_render_desc& rd, const pbrt_distribution_desc& d,
                        const pbrt_film_desc& fl) {
        const Routed a = go(PBRT_KERNEL_AUTO, ff, rd, d, fl);
        CHECK(a.refusal.code == PBRT_OK && a.route == Route::Serial);
        refused(go(PBRT_KERNEL_WAVE_CI, ff, rd, d, fl).refusal, PBRT_E_UNSUPPORTED, kWave_);
    };
    pbrt_distribution_desc zero = dist;
    zero.func[2] = 0;
    pbrt_distribution_desc none = dist;
    none.func_int = 0;
    Facts lens = f, kx = f, small_lds = f, mesh = f, dark = f;
    lens.lens_radius = 0.3;
    kx.non_matte = true;
    small_lds.lds_per_block = 8192;
    mesh.mesh = true;
    dark.n_lights = 0;
    {
        pbrt_render_desc d = path;
        d.flags = PBRT_FLAG_PANIC_FIDELITY;
        not_wave(f, d, dist, fd);
        d = path, d.max_depth = 2049;
        not_wave(f, d, dist, fd);
        d.max_depth = 2048;
        routed(PBRT_KERNEL_WAVE_CI, f, d, Route::Chain);
        not_wave(f, desc(2, 2, 0), dist, fd);      // the camera ray belongs to the sample
        not_wave(lens, desc(2, 2, 1), dist, fd);   // pLens is drawn per sample
        routed(PBRT_KERNEL_WAVE_CI, f, desc(2, 2, 1), Route::Chain);   // a pinhole: pLens unused
        not_wave(f, path, zero, fd);
        not_wave(f, path, none, fd);
        routed(PBRT_KERNEL_WAVE_CI, dark, path, Route::Chain);   // no lights: the distribution is not read
        not_wave(small_lds, path, dist, fd);
        // (a device whose LDS holds k_film's run at any spp, so that the rules after it decide)
        Facts roomy = f;
        roomy.lds_per_block = 1 << 20;
        not_wave(f, desc(64, 64, 1), dist, fd);           // k_film's run of 4095 samples: 107880 bytes
        routed(PBRT_KERNEL_WAVE_CI, roomy, desc(64, 64, 1), Route::Chain);
        not_wave(roomy, desc(64, 65, 1), dist, fd);       // spp > 4096
        not_wave(roomy, desc(32, 65, 4), dist, fd);       // ndims * spp > 8192
        // L.total <= 48 KB: 10 bytes per value, 768 of window buffers, 16 of draws
        routed(PBRT_KERNEL_WAVE_CI, roomy, desc(48, 50, 2), Route::Chain);   // 4800 values: 48784
        not_wave(roomy, desc(49, 50, 2), dist, fd);                          // 4900 values: 49792
        // DirectLighting: the camera ray per pixel; the zero-pdf rule and maxDepth 2048 are Path's
        pbrt_render_desc d0 = dl, d1 = dl;
        d0.n_dims = 0, d1.n_dims = 1;
        CHECK(go(PBRT_KERNEL_AUTO, f, d0, dist, fd).route == Route::Serial);
        CHECK(go(PBRT_KERNEL_AUTO, lens, d1, dist, fd).route == Route::Serial);
        CHECK(go(PBRT_KERNEL_AUTO, f, d1, dist, fd).route == Route::DirectLighting);
        pbrt_render_desc deep = dl;
        deep.max_depth = 4000;
        CHECK(go(PBRT_KERNEL_AUTO, f, deep, zero, fd).route == Route::DirectLighting);
        deep.max_depth = 65;
        CHECK(go(PBRT_KERNEL_AUTO, kx, deep, dist, fd).route == Route::Serial);
        // kX with k_paths_ci at 2 pixels per wave has no instantiation
        Knobs p2;
        p2.paths_ci = 2;
        CHECK(route(PBRT_KERNEL_AUTO, kx, p2, path, render_params(kx, p2, fd, path, 64), dist).route == Route::Serial);
        CHECK(route(PBRT_KERNEL_AUTO, f, p2, path, render_params(f, p2, fd, path, 64), dist).route == Route::Chain);
        p2.paths_wf = 1;
        CHECK(route(PBRT_KERNEL_AUTO, kx, p2, path, render_params(kx, p2, fd, path, 64), dist).route == Route::Chain);
        routed(PBRT_KERNEL_AUTO, kx, path, Route::Chain);
    }
    // the camera route's reasons, each first in its order
    auto cam_no = [&](const Facts& ff, const pbrt_render_desc& rd, const pbrt_distribution_desc& d, const char* why) {
        refused(go(PBRT_KERNEL_WAVE_CAM, ff, rd, d, fd).refusal, PBRT_E_UNSUPPORTED, (kCam + why).c_str());
    };
    {
        pbrt_render_desc d = cam;
        d.flags = PBRT_FLAG_PANIC_FIDELITY;
        d.integrator = PBRT_INTEGRATOR_DIRECT_LIGHTING;   // (also fails the next rule: the first decides)
        cam_no(f, d, dist, "panic fidelity runs on the serial kernel");
        d = cam, d.integrator = PBRT_INTEGRATOR_DIRECT_LIGHTING, d.max_depth = 4000;
        cam_no(f, d, dist, "Path integrator only (DirectLighting is out of scope)");
        d = cam, d.max_depth = 2049, d.n_dims = 2;
        cam_no(f, d, dist, "maxDepth > 2048");
        cam_no(kx, desc(2, 2, 2), dist, "n_dims >= 2: the camera ray is the pixel's (the wave_ci route)");
        cam_no(kx, desc(2, 2, 1), dist, "n_dims == 1 with a pinhole: the camera ray is the pixel's (the wave_ci route)");
        Facts kx_mesh = kx;
        kx_mesh.mesh = true;
        cam_no(kx_mesh, cam, zero, "Mirror / Glass / OrenNayar materials");
        cam_no(mesh, cam, zero, "triangle meshes");
        cam_no(small_lds, desc(64, 65, 0), zero, "a light with pdf 0");
        cam_no(small_lds, desc(64, 65, 0), dist, "the tile film does not fit LDS");
        Facts roomy = f, roomy_lens = lens;
        roomy.lds_per_block = roomy_lens.lds_per_block = 1 << 20;
        cam_no(roomy, desc(64, 65, 0), dist, "more than 4096 samples per pixel");
        cam_no(roomy_lens, desc(91, 91, 1), dist, "more than 4096 samples per pixel");   // 8281 values
        routed(PBRT_KERNEL_WAVE_CAM, roomy, desc(64, 64, 0), Route::Cam);
        routed(PBRT_KERNEL_WAVE_CAM, lens, desc(2, 2, 1), Route::Cam);
        routed(PBRT_KERNEL_WAVE_CAM, dark, cam, Route::Cam);
        Facts deep = f;
        deep.n_nodes = 181;   // any tree
        routed(PBRT_KERNEL_WAVE_CAM, deep, cam, Route::Cam);
    }
    {   // scene_facts
        pbrt_material_desc m[3] = {};
        m[0].type = PBRT_MAT_MATTE;
        m[1].type = PBRT_MAT_MATTE;
        m[2].type = PBRT_MAT_MATTE;
        pbrt_scene_desc s{};
        s.materials = m;
        s.n_materials = 3;
        s.n_prims = 7, s.n_nodes = 13, s.n_lights = 2;
        s.camera.lens_radius = 0.25;
        Facts g;
        g.n_simd = 96;
        scene_facts(s, g);
        CHECK(!g.non_matte && !g.rough_glass && g.n_prims == 7 && g.n_nodes == 13 && g.n_lights == 2 && g.n_materials == 3);
        CHECK(g.lens_radius == 0.25 && g.n_simd == 96 && !g.mesh);
        m[1].sigma = 30;   // OrenNayar
        scene_facts(s, g);
        CHECK(g.non_matte && !g.rough_glass);
        m[1].sigma = -5;   // clamps to 0: Lambertian
        scene_facts(s, g);
        CHECK(!g.non_matte);
        m[2].type = PBRT_MAT_GLASS;
        scene_facts(s, g);
        CHECK(g.non_matte && !g.rough_glass);
        m[2].v_roughness = 0.1;
        scene_facts(s, g);
        CHECK(g.non_matte && g.rough_glass);
        Facts mo;
        mo.mesh = true;
        CHECK(mesh_only(mo));
        mo.n_prims = 1;
        CHECK(!mesh_only(mo));
        mo.n_prims = 0, mo.non_matte = true;
        CHECK(!mesh_only(mo));
        mo.non_matte = false, mo.mesh = false;
        CHECK(!mesh_only(mo));
    }
#undef routed
    section("route");
}

// ---------------------------------------------------------------- ci_waves, ci_stride, ci_split
static void check_chain_rules() {
    Knobs k;
    Facts f = matte_facts();
    f.n_simd = 96;   // slots = 192
    const int64_t slots = 192;
    CHECK(ci_waves(k, f, 1, slots) == 4 && ci_waves(k, f, 1, slots + 1) == 2);
    CHECK(ci_waves(k, f, 1, 2 * slots) == 2 && ci_waves(k, f, 1, 2 * slots + 1) == 1);
    CHECK(ci_waves(k, f, 1, 1) == 4 && ci_waves(k, f, 2, 1) == 1 && ci_waves(k, f, 4, slots) == 1);
    {
        Knobs w8 = k;
        w8.ci_waves = 8;
        Facts kx = f;
        kx.non_matte = true;
        CHECK(ci_waves(w8, f, 1, 100000) == 8 && ci_waves(w8, kx, 1, 100000) == 4 && ci_waves(w8, f, 4, 5) == 8);
        w8.ci_waves = 2;
        CHECK(ci_waves(w8, kx, 1, 1) == 2);
        CHECK(ci_heavy_waves(k, f) == 4 && ci_heavy_waves(k, kx) == 4);
        w8.ci_heavy_waves = 8;
        CHECK(ci_heavy_waves(w8, f) == 8 && ci_heavy_waves(w8, kx) == 4);
    }
    CHECK(ci_stride(k, 1) == 2 && ci_stride(k, 2) == 1 && ci_stride(k, 8) == 1);
    {
        Knobs s = k;
        s.ci_stride = 1;
        CHECK(ci_stride(s, 1) == 1 && ci_stride(s, 4) == 1);
        s.ci_stride = 2;
        CHECK(ci_stride(s, 1) == 2 && ci_stride(s, 4) == 2);
    }
    CHECK(tiles_per_wave(false, 2) == 1 && tiles_per_wave(true, 1) == 1 && tiles_per_wave(true, 2) == 2);
    CHECK(tiles_per_wave(true, 4) == 4 && tiles_per_wave(true, 3) == 1 && tiles_per_wave(true, 8) == 1 && tiles_per_wave(true, 64) == 1);
    // ci_eu3_fits: 12 workgroups on the CU's LDS
    CHECK(ci_eu3_fits(f, 6560, 7093) && !ci_eu3_fits(f, 6560, 7094) && !ci_eu3_fits(f, 0, 0));   // 163840 / 12 = 13653.3

    const RenderParams rp = render_params(f, k, film(64, 64), desc(2, 2), 64);
    const ChainLayout Lci = layout_Lci(rp);
    int asked = 0;
    auto stat = [&](bool multi) {
        asked++;
        return static_lds_of(0, multi);
    };
    auto split = [&](const Knobs& kk, const Facts& ff, bool mo, int64_t nb, int kw, bool learned, int G, int64_t heavy_k) {
        return ci_split(kk, ff, Lci, kSz, mo, nb, kw, learned, G, heavy_k, stat);
    };
    Facts kx = f;
    kx.non_matte = true;
    // 1: a multi-wave shard beyond n_simd tiles: the learned heavy count at 4 waves, the rest at 1
    Split s = split(k, f, false, 97, 2, true, 1, 10);
    CHECK(s.heavy == 10 && s.heavy_w == 4 && s.light_w == 1 && !s.light_kw);
    CHECK(asked == 0);   // the static LDS is asked for the one-GPU rule alone
    s = split(k, f, false, 97, 2, false, 1, 10);   // not learned
    CHECK(s.heavy == 0);
    s = split(k, f, false, 97, 2, true, 2, 10);    // several tiles per wave
    CHECK(s.heavy == 0);
    {
        Knobs off = k;
        off.ci_split = false;
        CHECK(split(off, f, false, 97, 2, true, 1, 10).heavy == 0 && split(off, f, false, 96, 2, true, 1, 10).heavy == 0);
        Knobs lkw = k;
        lkw.ci_light_kw = true;
        s = split(lkw, f, false, 97, 2, true, 1, 10);
        CHECK(s.heavy == 10 && s.light_kw && s.light_w == 2 && s.heavy_w == 4);
        s = split(lkw, f, false, 2000, 1, true, 1, 10);   // one wave per tile: nothing to keep
        CHECK(!s.light_kw && s.light_w == 1);
    }
    // 2: one GPU (kw == 1): only the 3-wave Matte analytic chain splits
    s = split(k, f, false, 2000, 1, true, 1, 7);
    CHECK(s.heavy == 7 && s.heavy_w == 4 && s.light_w == 1 && asked > 0);
    CHECK(split(k, kx, false, 2000, 1, true, 1, 7).heavy == 0);   // kX
    Facts mesh = f;
    mesh.mesh = true, mesh.n_prims = 0;
    CHECK(split(k, mesh, true, 2000, 1, true, 1, 7).heavy == 0);   // mesh only
    {   // a workgroup whose LDS leaves fewer than 12 on a CU (the 2-wave build): no split
        auto fat = [&](bool) { return (size_t)14736; };
        CHECK(ci_split(k, f, Lci, kSz, false, 2000, 1, true, 1, 7, fat).heavy == 0);
    }
    // 3: the override (learned frames of one tile per workgroup), kX and mesh-only included
    {
        Knobs o = k;
        o.ci_heavy = 3;
        CHECK(split(o, f, false, 50, 4, true, 1, 10).heavy == 3 && split(o, kx, false, 2000, 1, true, 1, 0).heavy == 3);
        CHECK(split(o, mesh, true, 2000, 1, true, 1, 0).heavy == 3);
        CHECK(split(o, f, false, 50, 4, false, 1, 10).heavy == 0 && split(o, f, false, 50, 1, true, 2, 10).heavy == 0);
        CHECK(split(o, f, false, 3, 4, true, 1, 10).heavy == 0);    // heavy >= nb: nothing left for the light launch
        CHECK(split(o, f, false, 4, 4, true, 1, 10).heavy == 3);
        o.ci_heavy = 0;   // forced to none: the 8-wave split stays off too
        CHECK(split(o, f, false, 64, 4, true, 1, 10).heavy == 0);
        o.ci_heavy = 100;
        CHECK(split(o, f, false, 50, 4, true, 1, 10).heavy == 0);   // min(100, nb) == nb
    }
    // 4: a multi-wave Matte shard within n_simd tiles: PBRT_CI_SPLIT8 tiles, at most nb / 16, at 8 waves
    s = split(k, f, false, 96, 4, true, 1, 50);
    CHECK(s.heavy == 6 && s.heavy_w == 8 && s.light_w == 4 && s.light_kw);   // 96 / 16 caps the 32
    {
        Facts wide = f;
        wide.n_simd = 1024;
        s = split(k, wide, false, 1020, 4, true, 1, 50);
        CHECK(s.heavy == 32 && s.heavy_w == 8 && s.light_w == 4);   // 1020 / 16 = 63: the knob's 32
        CHECK(split(k, wide, false, 16, 2, true, 1, 0).heavy == 1 && split(k, wide, false, 15, 2, true, 1, 0).heavy == 0);
    }
    CHECK(split(k, kx, false, 96, 4, true, 1, 50).heavy == 0 && split(k, mesh, true, 96, 4, true, 1, 50).heavy == 0);
    CHECK(split(k, f, false, 96, 4, false, 1, 50).heavy == 0);
    {
        Knobs off = k;
        off.ci_split8 = 0;
        CHECK(split(off, f, false, 96, 4, true, 1, 50).heavy == 0);
    }
    // path chunks: they partition [0, nb) in order; K chunks, or fewer when nb runs out
    for (int64_t nb : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)6, (int64_t)16, (int64_t)17, (int64_t)1000, (int64_t)8160})
        for (int K = 1; K <= 16; K++) {
            int64_t s0 = 0, j = 0;
            while (s0 < nb) {
                const int64_t e0 = path_chunk_end(nb, s0, j, K);
                CHECK(e0 > s0 && e0 <= nb);
                if (j + 1 < K && nb - s0 >= 2) CHECK(e0 - s0 == (nb - s0) / 2);   // halving
                s0 = e0;
                j++;
            }
            CHECK(s0 == nb && j <= K);
            int64_t want = 0;   // chunks: one per halving while tiles remain, K at the most
            for (int64_t left = nb; left > 0 && want < K; want++) left -= want + 1 == K ? left : std::max<int64_t>(1, left / 2);
            CHECK(j == want);
        }
    // paths_ci_pixels and the path stage's choice
    {
        Facts l = f;
        CHECK(paths_ci_pixels(k, l) == 8);   // 4 lights
        l.n_lights = 8;
        CHECK(paths_ci_pixels(k, l) == 8);
        l.n_lights = 9;
        CHECK(paths_ci_pixels(k, l) == 4);
        l.n_lights = 16;
        CHECK(paths_ci_pixels(k, l) == 4);
        l.n_lights = 17;
        CHECK(paths_ci_pixels(k, l) == 0 && paths_on_wavefront(k, l));
        l.n_lights = 0;
        CHECK(paths_ci_pixels(k, l) == 8);
        l.n_nodes = kLdsNodes + 1;
        CHECK(paths_ci_pixels(k, l) == 0);
        Knobs p = k;
        p.paths_ci = 2;
        l = f;
        l.n_lights = 16;
        CHECK(paths_ci_pixels(p, l) == 2);
        l.n_lights = 17;   // kMaxCachedLights holds whatever the wave would
        CHECK(paths_ci_pixels(p, l) == 0);
        p.paths_ci = 8;
        l.n_lights = 9;
        CHECK(paths_ci_pixels(p, l) == 0);
        p.paths_ci = 0;
        CHECK(paths_ci_pixels(p, f) == 0 && paths_on_wavefront(p, f));
        CHECK(!paths_wf_enabled(k, f) && paths_wf_enabled(k, mesh) && !paths_on_wavefront(k, f));
        p = k, p.paths_wf = 0;
        CHECK(!paths_wf_enabled(p, mesh));
        p.paths_wf = 1;
        CHECK(paths_wf_enabled(p, f) && paths_on_wavefront(p, f));
        p = k;
        CHECK(!paths_ci_s1d_lds(p, rp, 8));
        p.paths_s1d_lds = true;
        CHECK(paths_ci_s1d_lds(p, rp, 8));   // 8 * 4 * 4 * 8 bytes
        const RenderParams r64 = render_params(f, k, film(64, 64), desc(8, 8), 64);
        CHECK(paths_ci_s1d_lds(p, r64, 8) && !paths_ci_s1d_lds(p, render_params(f, k, film(64, 64), desc(8, 9), 64), 8));
        CHECK(cam_pixels_per_wave(1) == 64 && cam_pixels_per_wave(8) == 64 && cam_pixels_per_wave(9) == 16);
        CHECK(cam_pixels_per_wave(32) == 16 && cam_pixels_per_wave(33) == 4 && cam_pixels_per_wave(4096) == 4);
        CHECK(paths_ci_groups(256, 8, 6, false) == 192 && paths_ci_groups(256, 8, 6, true) == 192);
        CHECK(paths_ci_groups(9, 4, 3, false) == 7 && paths_ci_groups(9, 4, 3, true) == 9);   // pp need not divide ppt
    }
    // the buffers: arrays in order, 256-byte aligned, disjoint, `need` their end
    {
        Facts g = f;
        for (bool kxs : {false, true}) {
            g.non_matte = kxs;
            const RenderParams r = render_params(g, k, film(45, 30), desc(3, 3), 64);
            Knobs small = k;
            for (double gb : {0.0, 1e-6, 0.001}) {
                small.wave_buffer_gb = gb;
                const WaveCarve c = wave_carve(small, g, r, kSz, gb == 0 ? (size_t)1 << 30 : 0);
                const int64_t ppt = 256, n = 9, nd = 4;
                const int64_t bytes[8] = {ppt * 416, ppt * nd * n * 8, ppt * n * 8, ppt * n * 24, ppt * n * 4, ppt * 32, 4,
                                          kxs ? 1024 * 40 : 0};
                int64_t per_tile = 0;
                for (int64_t b : bytes) per_tile += (b + 255) / 256 * 256;
                const double budget = gb > 0 ? gb : 0.5;   // half of the 1 GiB free
                const int64_t want = std::min<int64_t>(6, std::max<int64_t>(1, (int64_t)(budget * 1073741824.0) / per_tile));
                CHECK(c.batch == want && c.need == (size_t)(want * per_tile) && c.ppt == ppt && c.s1d_stride == nd * n);
                const int64_t offs[8] = {c.prec, c.s1d, c.memb, c.L, c.rays, c.ppanic, c.tile_npx, c.rrb};
                int64_t at = 0;
                for (int i = 0; i < 8; i++) {
                    if (i == 7 && !kxs) {
                        CHECK(offs[i] < 0);
                        continue;
                    }
                    CHECK(offs[i] == at && offs[i] % 256 == 0);
                    at += c.batch * ((bytes[i] + 255) / 256 * 256);
                }
                CHECK((size_t)at == c.need);
            }
        }
        const RenderParams r = render_params(f, k, film(45, 30), desc(3, 3), 64);
        CHECK(wave_carve(k, f, r, kSz, 0).batch == 6);   // 96 GB holds every slot
        const RenderParams none = render_params(f, k, film(45, 30), [] { pbrt_render_desc d = desc(3, 3); d.tile_begin = 9; return d; }(), 64);
        CHECK(none.n_slots == 0 && wave_carve(k, f, none, kSz, 0).batch == 1);
        // the path wavefront
        for (double gb : {24.0, 1e-5})
            for (int sx : {1, 3}) {
                Knobs p = k;
                p.pw_gb = gb;
                const RenderParams q = render_params(f, k, film(45, 30), desc(sx, sx), 64);
                const int64_t nrec = 6 * 256, per = q.spp - 1, nl = 4;
                const PwCarve c = pw_carve(p, f, q, kSz, nrec, 131);
                int64_t chunk = nrec;
                if (per > 0) chunk = std::min<int64_t>(nrec, std::max<int64_t>(1, (int64_t)(gb * 1073741824.0) / ((320 + 16) * per)));
                CHECK(c.chunk == chunk && c.cap == std::max<int64_t>(1, chunk * std::max<int64_t>(per, 1)));
                if (gb < 1) CHECK(per == 0 || c.chunk < nrec);
                const int64_t offs[9] = {c.paths, c.q[0], c.q[1], c.q[2], c.sorted, c.cnt, c.ldc, c.ldp, c.pkey};
                const int64_t bytes[9] = {c.cap * 320, c.cap * 4, c.cap * 4, c.cap * 4, c.cap * 4, 131 * 4,
                                          chunk * nl * 24, chunk * nl * 4, nrec * 8};
                int64_t at = 0;
                for (int i = 0; i < 9; i++) {
                    CHECK(offs[i] == at && at % 256 == 0);
                    at += (bytes[i] + 255) / 256 * 256;
                }
                CHECK((size_t)at == c.need);
            }
        Facts dark = f;
        dark.n_lights = 0;   // the light arrays keep one entry per pixel
        const PwCarve c = pw_carve(k, dark, render_params(dark, k, film(16, 16), desc(2, 2), 64), kSz, 256, 131);
        CHECK(c.ldp - c.ldc == 256 * 24 && c.pkey - c.ldp == 256 * 4);
    }
    CHECK(schedule_key(rp, 1) != schedule_key(rp, 2) && schedule_key(rp, 4) == schedule_key(rp, 4));
    section("chain_rules");
}

// ---------------------------------------------------------------- recorded launches
// The chain and path launches of a frame as render.hip's stages issue them, spelled as the launch
// log spells them (tools/dump_launch_logs.py, without the stream): kernel<template arguments>
// [grid x block] lds <dynamic LDS>. k_paths_ci's dynamic LDS is sizeof arithmetic over its kernel's
// types (paths_group_lds, not a rule of frame_route.h): its lines end at the block.
struct Frame {
    Facts f;
    Knobs k;
    pbrt_film_desc film;
    pbrt_render_desc rd;
    int req = PBRT_KERNEL_AUTO;
    int lanes_per_wave = 0;   // opts.lanes_per_wave (0: unset)
};
static const char* tf(bool b) { return b ? "true" : "false"; }
static std::vector<std::string> launches(const Frame& c, bool learned, int64_t heavy_k) {
    const Facts& f = c.f;
    const Knobs& k = c.k;
    CHECK(check_render(f, c.film, &c.rd).code == PBRT_OK);
    const RenderParams rp = render_params(f, k, c.film, c.rd, c.lanes_per_wave ? c.lanes_per_wave : 64);
    const pbrt_distribution_desc dist = uniform_dist(f.n_lights);
    const Routed r = route(c.req, f, k, c.rd, rp, dist);
    CHECK(r.refusal.code == PBRT_OK);
    const bool mb = rp.mode == PBRT_MODE_THROUGHPUT, mo = mesh_only(f);
    const int depth = f.n_nodes <= kLdsNodes ? 0 : 64;
    auto stat = [&](bool multi) { return static_lds_of(depth, multi); };
    const int64_t nb = rp.n_slots, ppt = rp.tile_size * rp.tile_size, nrec = nb * ppt;
    std::vector<std::string> out;
    auto line = [&](const std::string& name, int64_t grid, int block, int64_t lds) {
        out.push_back(name + " [" + std::to_string(grid) + " x " + std::to_string(block) + "]" +
                      (lds >= 0 ? " lds " + std::to_string(lds) : ""));
    };
    if (r.route == Route::Cam) {
        const ChainLayout L = layout_Lcam(rp);
        const bool stack = f.n_nodes > kLdsNodes;
        if (mb) line("k_cam_setup", rp.ndims > 0 ? nrec : (nrec + 63) / 64, 64, L.staging);
        else line(stack ? "k_chain_cam_stack" : "k_chain_cam", nb, 64, L.total);
        const int pp = cam_pixels_per_wave(rp.spp);
        if (rp.spp > 1)
            line(std::string(stack ? "k_paths_cam_stack<" : "k_paths_cam<") + std::to_string(pp) + ", " + tf(mb) + ">",
                 (nrec + pp - 1) / pp, 64, 0);
        return out;
    }
    CHECK(r.route != Route::Serial);
    const ChainLayout Lci = layout_Lci(rp);
    const int G = tiles_per_wave(c.lanes_per_wave != 0, c.lanes_per_wave);
    auto chain = [&](int w, int64_t n, bool nps_allowed) {
        const ChainLaunch l = chain_launch(k, f, rp, Lci, kSz, G, mo, w, n, nps_allowed, stat);
        line("k_chain_ci<" + std::to_string(l.w) + ", " + std::to_string(l.depth) + ", " + tf(l.kx) + ", " +
                 std::to_string(l.eu) + ", " + tf(l.window) + ", " + tf(l.multi) + ">",
             l.grid, (int)l.block, l.lds);
        CHECK(l.ring == (int)(l.w * 4096 / 16 / l.Gc) && l.lanes_per_tile * l.Gc == (int)l.block && l.per_tile == (l.Gc == 1));
        CHECK(l.lay.total == (int)l.lds && l.stride == (w > 1 ? 1 : 2));
        return l;
    };
    auto paths = [&](int64_t n, bool ordered) {
        const int pp = paths_ci_pixels(k, f);
        line("k_paths_ci<" + std::to_string(pp) + ", " + tf(mb) + ", " + tf(f.non_matte) + ">",
             paths_ci_groups(ppt, pp, n, ordered), 64, -1);
    };
    if (r.route == Route::DirectLighting) {
        unsigned lds = 0;
        (void)ci_layout(Lci, 1, 1, lds, kSz.chain_cache);
        line("k_dl_setup", nb, 64, lds);
        return out;
    }
    if (r.route == Route::Throughput) {
        line(f.non_matte ? "k_mb_setup<true>" : "k_mb_setup<false>", nrec, 64, layout_L(rp).total);
        if (!paths_on_wavefront(k, f)) paths(nb, false);
        return out;
    }
    const int kw = ci_waves(k, f, G, nb);
    const Split sp = ci_split(k, f, Lci, kSz, mo, nb, kw, learned, G, heavy_k, stat);
    if (sp.heavy > 0) {
        chain(sp.heavy_w, sp.heavy, sp.light_kw);
        chain(sp.light_w, nb - sp.heavy, true);
    } else {
        chain(kw, nb, true);
    }
    if (paths_on_wavefront(k, f)) return out;
    const bool ov = k.paths_overlap > 0 && learned && (sp.heavy > 0 || (k.paths_overlap_all && (kw > 1 || G == 1)));
    if (!ov) {
        paths(nb, false);
        return out;
    }
    for (int64_t s0 = 0, j = 0; s0 < nb; j++) {
        const int64_t e0 = path_chunk_end(nb, s0, j, k.paths_overlap);
        paths(e0 - s0, true);
        s0 = e0;
    }
    return out;
}
static void expect(const Frame& c, bool learned, int64_t heavy_k, std::vector<std::string> want) {
    const std::vector<std::string> got = launches(c, learned, heavy_k);
    CHECK(got.size() == want.size());
    for (size_t i = 0; i < got.size(); i++) CHECK_STR(got[i], want[i]);
}
static Frame frame(const Facts& f, int w, int h, const pbrt_render_desc& rd) { return Frame{f, Knobs{}, film(w, h), rd}; }

static void check_recorded() {
    // the scenes of tests/kernel_cases.py and tests/edge_routes.py, as pbrt_gpu_create sees them
    const Facts readme = matte_facts();
    Facts glass = matte_facts(49), mesh = matte_facts(0), spheres = matte_facts(181, 2), crowd = matte_facts(73, 3),
          small_kx = matte_facts(13, 3), lens = matte_facts(73, 3);
    glass.non_matte = true;
    mesh.n_prims = 0, mesh.mesh = true, mesh.n_materials = 1;
    small_kx.non_matte = true;
    lens.lens_radius = 0.3;
    const pbrt_render_desc s22 = desc(2, 2), s33 = desc(3, 3);
    pbrt_render_desc tp = s22;
    tp.mode = PBRT_MODE_THROUGHPUT;
    Frame c;

    // ci_w1_eu3: the Matte 1-wave chain; the learned frame's paths in halving chunks
    c = frame(readme, 45, 30, s22);
    c.k.ci_waves = 1, c.k.ci_eu = 3;
    expect(c, false, 0, {"k_chain_ci<1, 0, false, 0, false, false> [6 x 64] lds 4912", "k_paths_ci<8, false, false> [192 x 64]"});
    expect(c, true, 0, {"k_chain_ci<1, 0, false, 0, false, false> [6 x 64] lds 4912", "k_paths_ci<8, false, false> [96 x 64]",
                        "k_paths_ci<8, false, false> [32 x 64]", "k_paths_ci<8, false, false> [32 x 64]",
                        "k_paths_ci<8, false, false> [32 x 64]"});
    // ci_w1_eu2, ci_w4, ci_w8
    c.k.ci_eu = 2;
    expect(c, false, 0, {"k_chain_ci<1, 0, false, 2, false, false> [6 x 64] lds 4912", "k_paths_ci<8, false, false> [192 x 64]"});
    c.k.ci_eu = 0, c.k.ci_waves = 4;
    expect(c, false, 0, {"k_chain_ci<4, 0, false, 0, false, false> [6 x 256] lds 34144", "k_paths_ci<8, false, false> [192 x 64]"});
    c.k.ci_waves = 8;
    expect(c, false, 0, {"k_chain_ci<8, 0, false, 0, false, false> [6 x 512] lds 66912", "k_paths_ci<8, false, false> [192 x 64]"});
    // kx_w1, kx_w2, kx_w4_p4 (kX: the one-wave chain is the per-lane code)
    c = frame(glass, 48, 32, s22);
    c.k.ci_waves = 1;
    expect(c, false, 0, {"k_chain_ci<1, 0, true, 0, false, true> [6 x 64] lds 4912", "k_paths_ci<8, false, true> [192 x 64]"});
    c.k.ci_waves = 2;
    expect(c, false, 0, {"k_chain_ci<2, 0, true, 0, false, false> [6 x 128] lds 9008", "k_paths_ci<8, false, true> [192 x 64]"});
    c.k.ci_waves = 4, c.k.paths_ci = 4;
    expect(c, true, 0, {"k_chain_ci<4, 0, true, 0, false, false> [6 x 256] lds 17200", "k_paths_ci<4, false, true> [192 x 64]",
                        "k_paths_ci<4, false, true> [64 x 64]", "k_paths_ci<4, false, true> [64 x 64]",
                        "k_paths_ci<4, false, true> [64 x 64]"});
    // mesh_w1, mesh_w4 (mesh only: no analytic walk; the paths on the wavefront)
    c = frame(mesh, 48, 32, s22);
    c.k.ci_waves = 1;
    expect(c, false, 0, {"k_chain_ci<1, -1, false, 0, false, false> [6 x 64] lds 4912"});
    c.k.ci_waves = 4;
    expect(c, true, 0, {"k_chain_ci<4, -1, false, 0, false, false> [6 x 256] lds 34144"});
    // multi_mesh (lanes_per_wave 4)
    c = frame(mesh, 48, 32, s22);
    c.lanes_per_wave = 4;
    expect(c, false, 0, {"k_chain_ci<1, -1, false, 0, false, true> [2 x 64] lds 7920"});
    // stack_w1_eu2, stack_w2 and stack_w1_auto (a stack tree; its static LDS leaves no room for the 3-wave build)
    c = frame(spheres, 64, 48, s22);
    c.k.ci_waves = 1, c.k.ci_eu = 2;
    expect(c, false, 0, {"k_chain_ci<1, 64, false, 2, false, false> [12 x 64] lds 4912"});
    c.k.ci_eu = 3;
    expect(c, false, 0, {"k_chain_ci<1, 64, false, 0, false, false> [12 x 64] lds 4912"});
    c.k.ci_eu = 0;
    expect(c, true, 0, {"k_chain_ci<1, 64, false, 2, false, false> [12 x 64] lds 4912"});
    c.k.ci_waves = 2;
    expect(c, false, 0, {"k_chain_ci<2, 64, false, 0, false, false> [12 x 128] lds 17760"});
    // edge_matte: the default waves of 6 tiles on 1024 SIMDs
    c = frame(crowd, 48, 32, desc(2, 2, 4, false, 5));
    expect(c, true, 0, {"k_chain_ci<4, 64, false, 0, false, false> [6 x 256] lds 34144"});
    // edge_small_kx_lanes_per_wave2, multi_eu2 (lanes_per_wave 4, 9 tiles), multi_eu3 (2)
    c = frame(small_kx, 48, 32, desc(2, 2, 4, false, 5));
    c.lanes_per_wave = 2;
    expect(c, true, 0, {"k_chain_ci<1, 0, true, 0, false, true> [3 x 64] lds 6288", "k_paths_ci<8, false, true> [192 x 64]"});
    c = frame(readme, 45, 46, s22);
    c.lanes_per_wave = 4, c.k.ci_eu = 2;
    expect(c, true, 0, {"k_chain_ci<1, 0, false, 2, false, true> [3 x 64] lds 7920", "k_paths_ci<8, false, false> [288 x 64]"});
    c.lanes_per_wave = 2, c.k.ci_eu = 3;
    expect(c, false, 0, {"k_chain_ci<1, 0, false, 0, false, true> [5 x 64] lds 6288", "k_paths_ci<8, false, false> [288 x 64]"});
    // split_heavy4, split_heavy8
    c = frame(readme, 45, 30, s33);
    c.k.ci_waves = 1, c.k.ci_eu = 3, c.k.ci_heavy = 2;
    expect(c, false, 0, {"k_chain_ci<1, 0, false, 0, false, false> [6 x 64] lds 4912", "k_paths_ci<8, false, false> [192 x 64]"});
    expect(c, true, 2, {"k_chain_ci<4, 0, false, 0, false, false> [2 x 256] lds 17200",
                        "k_chain_ci<1, 0, false, 0, false, false> [4 x 64] lds 4912", "k_paths_ci<8, false, false> [96 x 64]",
                        "k_paths_ci<8, false, false> [32 x 64]", "k_paths_ci<8, false, false> [32 x 64]",
                        "k_paths_ci<8, false, false> [32 x 64]"});
    c.k.paths_overlap = 0;   // split_heavy4_paths_overlap0
    expect(c, true, 2, {"k_chain_ci<4, 0, false, 0, false, false> [2 x 256] lds 17200",
                        "k_chain_ci<1, 0, false, 0, false, false> [4 x 64] lds 4912", "k_paths_ci<8, false, false> [192 x 64]"});
    c.k.paths_overlap = 5, c.k.ci_waves = 2, c.k.ci_heavy_waves = 8;
    expect(c, false, 0, {"k_chain_ci<2, 0, false, 0, false, false> [6 x 128] lds 18160", "k_paths_ci<8, false, false> [192 x 64]"});
    expect(c, true, 2, {"k_chain_ci<8, 0, false, 0, false, false> [2 x 512] lds 33584",
                        "k_chain_ci<1, 0, false, 0, false, false> [4 x 64] lds 4912", "k_paths_ci<8, false, false> [96 x 64]",
                        "k_paths_ci<8, false, false> [32 x 64]", "k_paths_ci<8, false, false> [32 x 64]",
                        "k_paths_ci<8, false, false> [32 x 64]"});
    // shard_w2_split8 and shard_w2_split8_off: 16 tiles at 2 waves within the wave slots
    c = frame(readme, 64, 64, s22);
    c.k.ci_waves = 2;
    expect(c, false, 0, {"k_chain_ci<2, 0, false, 0, false, false> [16 x 128] lds 17760", "k_paths_ci<8, false, false> [512 x 64]"});
    expect(c, true, 0, {"k_chain_ci<8, 0, false, 0, false, false> [1 x 512] lds 66912",
                        "k_chain_ci<2, 0, false, 0, false, false> [15 x 128] lds 17760", "k_paths_ci<8, false, false> [256 x 64]",
                        "k_paths_ci<8, false, false> [128 x 64]", "k_paths_ci<8, false, false> [64 x 64]",
                        "k_paths_ci<8, false, false> [32 x 64]", "k_paths_ci<8, false, false> [32 x 64]"});
    c.k.ci_split8 = 0;
    expect(c, true, 0, {"k_chain_ci<2, 0, false, 0, false, false> [16 x 128] lds 17760", "k_paths_ci<8, false, false> [256 x 64]",
                        "k_paths_ci<8, false, false> [128 x 64]", "k_paths_ci<8, false, false> [64 x 64]",
                        "k_paths_ci<8, false, false> [32 x 64]", "k_paths_ci<8, false, false> [32 x 64]"});
    // spwin_w1_eu3, spwin_w4 (121 spp without jitter: the windowed StartPixel), multi_spwin_eu2
    c = frame(readme, 16, 16, desc(11, 11, 4, false, 3));
    c.k.ci_waves = 1, c.k.ci_eu = 3;
    expect(c, true, 0, {"k_chain_ci<1, 0, false, 0, true, false> [1 x 64] lds 4912", "k_paths_ci<8, false, false> [32 x 64]"});
    c.k.ci_eu = 0, c.k.ci_waves = 4;
    expect(c, false, 0, {"k_chain_ci<4, 0, false, 0, true, false> [1 x 256] lds 36560", "k_paths_ci<8, false, false> [32 x 64]"});
    c.k.ci_waves = 0, c.k.ci_eu = 2, c.lanes_per_wave = 2;
    expect(c, false, 0, {"k_chain_ci<1, 0, false, 2, true, true> [1 x 64] lds 8704", "k_paths_ci<8, false, false> [32 x 64]"});
    // spp256_w1: 256 spp (config C's sampler), the build by the LDS rule
    c = frame(readme, 16, 16, desc(16, 16, 4, false, 3));
    c.k.ci_waves = 1;
    expect(c, false, 0, {"k_chain_ci<1, 0, false, 0, true, false> [1 x 64] lds 5936", "k_paths_ci<8, false, false> [32 x 64]"});
    // paths_p4 (12 lights), paths_p2
    c = frame(matte_facts(45, 12), 32, 32, s22);
    expect(c, true, 0, {"k_chain_ci<4, 0, false, 0, false, false> [4 x 256] lds 34144", "k_paths_ci<4, false, false> [128 x 64]",
                        "k_paths_ci<4, false, false> [64 x 64]", "k_paths_ci<4, false, false> [64 x 64]"});
    c = frame(readme, 45, 30, s22);
    c.k.paths_ci = 2;
    expect(c, false, 0, {"k_chain_ci<4, 0, false, 0, false, false> [6 x 256] lds 34144", "k_paths_ci<2, false, false> [768 x 64]"});
    // THROUGHPUT: tp_p8, tp_kx_p4, pw_tp_sort
    c = frame(readme, 45, 30, tp);
    expect(c, false, 0, {"k_mb_setup<false> [1536 x 64] lds 1328", "k_paths_ci<8, true, false> [192 x 64]"});
    c.k.paths_wf = 1;
    expect(c, false, 0, {"k_mb_setup<false> [1536 x 64] lds 1328"});
    c = frame(glass, 48, 32, tp);
    c.k.paths_ci = 4;
    expect(c, true, 0, {"k_mb_setup<true> [1536 x 64] lds 1328", "k_paths_ci<4, true, true> [384 x 64]"});
    // dl_matte's k_dl_setup (edge_dl_matte: 6 tiles)
    {
        pbrt_render_desc dl = desc(2, 2, 4, false, 5);
        dl.integrator = PBRT_INTEGRATOR_DIRECT_LIGHTING;
        expect(frame(crowd, 48, 32, dl), false, 0, {"k_dl_setup [6 x 64] lds 4912"});
    }
    // the camera route: cam_p64, cam_p16, cam_p4, cam_tp_p16 (n_dims 0), edge_cam_lens (n_dims 1), cam_stack_tp_p4
    auto cam = [&](const Facts& f, int w, int h, pbrt_render_desc rd, bool mb) {
        if (mb) rd.mode = PBRT_MODE_THROUGHPUT;
        Frame x = frame(f, w, h, rd);
        x.req = PBRT_KERNEL_WAVE_CAM;
        return x;
    };
    expect(cam(readme, 32, 32, desc(2, 2, 0, false, 5), false), true, 0,
           {"k_chain_cam [4 x 64] lds 4096", "k_paths_cam<64, false> [16 x 64] lds 0"});
    expect(cam(readme, 32, 32, desc(3, 3, 0, false, 5), false), false, 0,
           {"k_chain_cam [4 x 64] lds 4096", "k_paths_cam<16, false> [64 x 64] lds 0"});
    expect(cam(readme, 16, 16, desc(6, 6, 0, false, 5), false), false, 0,
           {"k_chain_cam [1 x 64] lds 4096", "k_paths_cam<4, false> [64 x 64] lds 0"});
    expect(cam(readme, 32, 32, desc(3, 3, 0, false, 5), true), false, 0,
           {"k_cam_setup [16 x 64] lds 272", "k_paths_cam<16, true> [64 x 64] lds 0"});
    expect(cam(lens, 48, 32, desc(2, 2, 1, false, 5), false), true, 0,
           {"k_chain_cam_stack [6 x 64] lds 4096", "k_paths_cam_stack<64, false> [24 x 64] lds 0"});
    expect(cam(crowd, 16, 16, desc(6, 6, 0, false, 5), true), false, 0,
           {"k_cam_setup [4 x 64] lds 272", "k_paths_cam_stack<4, true> [64 x 64] lds 0"});
    section("recorded");
}

int main() {
    check_layouts();
    check_render_params();
    check_route();
    check_chain_rules();
    check_recorded();
    return 0;
}

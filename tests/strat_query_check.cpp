// tests/strat_query_check.cpp — host check of go-pbrt_amd/csrc/strat_query.h (the
// host side of pbrt_gpu_frame_samples_stratified_device and
// pbrt_gpu_li_stratified_device), with no device:
//   - every PBRT_E_INVALID and PBRT_E_UNSUPPORTED case of both calls, each alone on
//     otherwise valid arguments, with its text; the order where two hold;
//   - the pixel (= table) counts of tile ranges against a literal enumeration on
//     ragged films: 45 x 30 at tile 16, 17 x 5 at tile 4, one 16 x 16 tile;
//   - the cursors and the PCG32 draws after the camera sample for n_dims 0 .. 5,
//     against a literal replay of GetCameraSample's three requests;
//   - the StartPixel form and LDS carve of the plan for the shapes the GPU tests
//     run (buffered, serial, windowed), and the k_li_strat instantiation.
// No pointer is dereferenced by the checks. Compiled with
// -fsanitize=address,undefined and run by tests/test_strat_query_host.py. Prints
// one "case <name> <status> <reason>" line per case, "count ..." / "cursor ..." /
// "plan ..." / "kernel ..." lines, and "checks=.. bad=..".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../go-pbrt_amd/csrc/strat_query.h"

using namespace pbrtstrat;

static long g_checks = 0, g_bad = 0;

static void expect(bool ok, const char* what) {
    g_checks++;
    if (!ok) {
        g_bad++;
        std::printf("FAILED %s\n", what);
    }
}

static pbrt_film_desc film_of(int w, int h, double radius = 1.0) {
    pbrt_film_desc f;
    std::memset(&f, 0, sizeof(f));
    f.res_x = w;
    f.res_y = h;
    f.crop_max_x = w;
    f.crop_max_y = h;
    f.filter_radius_x = f.filter_radius_y = radius;
    return f;
}

struct Args {
    double a[16];
    uint64_t s[2];
    int32_t i[4];
    pbrt_film_desc f;
    pbrt_frame_desc d;
    pbrt_strat_sampler_desc sm;
    pbrt_frame_samples_soa out;
    pbrt_strat_samples_soa so;
    pbrt_li_desc ld;
    pbrt_ray_soa rays;
    pbrt_rng_soa rng;
    pbrt_radiance_soa rad;
    pbrt_strat_soa st;
    Args() {
        f = film_of(45, 30);
        d = pbrt_frame_desc{16, 3, 0, 6, 0, 0};
        sm = pbrt_strat_sampler_desc{2, 2, 4, 0, 0};
        out = pbrt_frame_samples_soa{a, a + 1, a + 2, a + 3, a + 4, a + 5, nullptr, a + 6, a + 7, s, s + 1, nullptr, nullptr};
        so = pbrt_strat_samples_soa{i, i + 1, a + 8};
        ld = pbrt_li_desc{PBRT_INTEGRATOR_PATH, 5, PBRT_LIGHT_STRATEGY_UNIFORM, 0, 1.0};
        rays = pbrt_ray_soa{a, a + 1, a + 2, a + 3, a + 4, a + 5, nullptr};
        rng = pbrt_rng_soa{s, s + 1};
        rad = pbrt_radiance_soa{a + 9, a + 10, a + 11, nullptr, nullptr, nullptr};
        st = pbrt_strat_soa{a + 8, i, i + 1, 1350, 4, 4, 1, 2, 0};
    }
};

static void report(const char* name, int rc, const char* why, int want, const char* word) {
    std::printf("case %s %d %s\n", name, rc, why ? why : "(null)");
    expect(rc == want, name);
    expect(why != nullptr && (rc == PBRT_OK) == (why[0] == 0), "a refusal names its reason");
    expect(!word || (why && std::strstr(why, word)), "the reason's text");
}

// frame_samples_stratified as queries.hip calls the header: the arguments, then the refusals
static int samples_call(const Args& g, bool ctx_ok, const pbrt_frame_desc* d, const pbrt_strat_sampler_desc* sm,
                        const pbrt_frame_samples_soa* out, const pbrt_strat_samples_soa* so, bool in_flight, int64_t* n,
                        const char** why, const pbrtroute::Facts& facts = pbrtroute::Facts()) {
    if (int rc = check_samples_args(ctx_ok, ctx_ok ? &g.f : nullptr, d, sm, out, so, in_flight, n, why)) return rc;
    return check_samples_supported(facts, pbrt::Knobs(), g.f, *d, *sm, why);
}
static void samples_case(const char* name, const Args& g, int want, const char* word = nullptr, bool ctx_ok = true,
                         bool in_flight = false, bool null_desc = false, bool null_sampler = false, bool null_out = false,
                         bool null_strat = false) {
    const char* why = nullptr;
    int64_t n = -1;
    const int rc = samples_call(g, ctx_ok, null_desc ? nullptr : &g.d, null_sampler ? nullptr : &g.sm,
                                null_out ? nullptr : &g.out, null_strat ? nullptr : &g.so, in_flight, &n, &why);
    report(name, rc, why, want, word);
}
static void li_case(const char* name, const Args& g, int want, const char* word = nullptr, bool ctx_ok = true,
                    bool in_flight = false, bool null_strat = false, size_t n = 4) {
    const char* why = nullptr;
    const int rc = check_li_args(ctx_ok, &g.ld, &g.rays, &g.rng, n, &g.rad, null_strat ? nullptr : &g.st, in_flight, &why);
    report(name, rc, why, want, word);
}

// the pixels of the tiles [b, e) of a w x h film at tile size ts, one by one
static int64_t enumerate_pixels(int w, int h, int ts, int64_t b, int64_t e) {
    const int ntx = (w + ts - 1) / ts;
    int64_t n = 0;
    for (int64_t t = b; t < e; t++) {
        const int x0 = (int)(t % ntx) * ts, y0 = (int)(t / ntx) * ts;
        for (int y = y0; y < y0 + ts && y < h; y++)
            for (int x = x0; x < x0 + ts && x < w; x++) n++;
    }
    return n;
}

int main() {
    const int INV = PBRT_E_INVALID, UNS = PBRT_E_UNSUPPORTED;
    Args g;

    // ---- pbrt_gpu_frame_samples_stratified_device
    samples_case("samples_valid", g, PBRT_OK);
    samples_case("samples_null_ctx", g, INV, "null context", false);
    samples_case("samples_null_desc", g, INV, "frame desc", true, false, true);
    samples_case("samples_null_sampler", g, INV, "sampler desc is NULL", true, false, false, true);
    samples_case("samples_null_out", g, INV, "out is NULL", true, false, false, false, true);
    samples_case("samples_null_strat", g, INV, "strat is NULL", true, false, false, false, false, true);
    samples_case("samples_in_flight", g, INV, "in flight", true, true);
    { Args h; h.d.tile_size = 0; samples_case("samples_tile_size_0", h, INV, "tile_size"); }
    { Args h; h.d.ns = 0; h.sm.sampler_x = h.sm.sampler_y = 1; samples_case("samples_ns_0", h, INV, "ns < 1"); }
    { Args h; h.d.flags = PBRT_FILM_ADD_CLEAR; samples_case("samples_clear_flag", h, INV, "flags"); }
    { Args h; h.d.reserved = 1; samples_case("samples_frame_reserved", h, INV, "reserved"); }
    { Args h; h.d.tile_end = 7; samples_case("samples_end_past_the_film", h, INV, "tile range"); }
    { Args h; h.d.tile_begin = -1; samples_case("samples_begin_negative", h, INV, "tile range"); }
    { Args h; h.sm.sampler_x = 0; samples_case("samples_sampler_x_0", h, INV, "sampler_x"); }
    { Args h; h.sm.sampler_y = -2; samples_case("samples_sampler_y_negative", h, INV, "sampler_y"); }
    { Args h; h.sm.reserved = 3; samples_case("samples_sampler_reserved", h, INV, "sampler's reserved"); }
    { Args h; h.d.ns = 4; samples_case("samples_ns_is_spp", h, INV, "ns != sampler_x * sampler_y - 1"); }
    { Args h; h.d.ns = 2; samples_case("samples_ns_short", h, INV, "ns != sampler_x * sampler_y - 1"); }
    { Args h; h.sm.sampler_x = h.sm.sampler_y = 65536; samples_case("samples_spp_2_32", h, INV, "ns != "); }
    { Args h; h.out.oz = nullptr; samples_case("samples_null_ray_array", h, INV, "ray array"); }
    { Args h; h.out.pfilm_y = nullptr; samples_case("samples_null_pfilm", h, INV, "pfilm"); }
    { Args h; h.out.state = nullptr; samples_case("samples_null_state", h, INV, "rng array"); }
    { Args h; h.so.k = nullptr; samples_case("samples_null_k", h, INV, "sample index array"); }
    { Args h; h.so.table = nullptr; samples_case("samples_null_table", h, INV, "sample index array"); }
    { Args h; h.so.s1d = nullptr; samples_case("samples_null_s1d", h, INV, "table array"); }
    { Args h; h.d.tile_begin = h.d.tile_end = 3; samples_case("samples_valid_empty", h, PBRT_OK); }
    { Args h; h.sm.jitter = 1; h.sm.n_dims = 1; samples_case("samples_valid_jitter", h, PBRT_OK); }
    {   // the order: the frame's own cases first, a render in flight among them; then the sampler; then the pointers
        Args h;
        h.sm.sampler_x = 0;
        h.so.k = nullptr;
        samples_case("samples_order_in_flight_first", h, INV, "in flight", true, true);
        samples_case("samples_order_sampler_before_pointers", h, INV, "sampler_x");
        h.d.tile_size = 0;
        samples_case("samples_order_frame_first", h, INV, "tile_size");
    }
    // PBRT_E_UNSUPPORTED
    { Args h; h.sm.n_dims = 0; samples_case("samples_n_dims_0", h, UNS, "n_dims < 1"); }
    { Args h; h.sm.n_dims = -1; samples_case("samples_n_dims_negative", h, UNS, "n_dims < 1"); }
    { Args h; h.d.tile_size = 257; h.d.tile_end = 1; samples_case("samples_tile_257", h, UNS, "256"); }
    {
        Args h;
        h.sm.sampler_x = 4097; h.sm.sampler_y = 1; h.sm.n_dims = 1; h.d.ns = 4096; h.d.tile_end = 1;
        samples_case("samples_spp_4097", h, UNS, "4096 samples");
        h.sm.sampler_x = 64; h.sm.sampler_y = 64; h.d.ns = 4095;
        samples_case("samples_spp_4096", h, PBRT_OK);
        h.sm.n_dims = 2;
        samples_case("samples_lds_beyond_48k", h, UNS, "48 KB");   // 2 x 4096 values: 64 KB cannot be staged
    }
    {
        Args h;
        h.sm.sampler_x = 64; h.sm.sampler_y = 64; h.sm.n_dims = 3; h.d.ns = 4095; h.d.tile_end = 1;
        samples_case("samples_n_dims_times_spp", h, UNS, "n_dims * spp > 8192");
    }

    // ---- pbrt_gpu_li_stratified_device
    li_case("li_valid", g, PBRT_OK);
    li_case("li_valid_n0", g, PBRT_OK, nullptr, true, false, false, 0);
    li_case("li_null_ctx", g, INV, "null context", false);
    li_case("li_in_flight", g, INV, "in flight", true, true);
    li_case("li_null_strat", g, INV, "strat is NULL", true, false, true);
    li_case("li_n_2_31", g, INV, "2^31", true, false, false, (size_t)INT32_MAX + 1);
    { Args h; h.ld.reserved = 1; li_case("li_desc_reserved", h, INV, "reserved must be 0"); }
    { Args h; h.ld.max_depth = 0; li_case("li_depth_0", h, INV, "max_depth"); }
    { Args h; h.rays.dx = nullptr; li_case("li_null_ray_array", h, INV, "ray array"); }
    { Args h; h.rad.g = nullptr; li_case("li_null_radiance", h, INV, "radiance array"); }
    { Args h; h.st.reserved = 2; li_case("li_strat_reserved", h, INV, "strat's reserved"); }
    { Args h; h.st.n_dims = -1; h.st.first_1d = h.st.first_2d = 0; li_case("li_n_dims_negative", h, INV, "n_dims < 0"); }
    { Args h; h.st.first_1d = 5; li_case("li_first_1d_beyond", h, INV, "cursor"); }
    { Args h; h.st.first_1d = -1; li_case("li_first_1d_negative", h, INV, "cursor"); }
    { Args h; h.st.first_2d = 5; li_case("li_first_2d_beyond", h, INV, "cursor"); }
    { Args h; h.st.first_2d = -1; li_case("li_first_2d_negative", h, INV, "cursor"); }
    { Args h; h.st.s1d = nullptr; li_case("li_null_s1d", h, INV, "table array"); }
    { Args h; h.st.table = nullptr; li_case("li_null_table", h, INV, "sample index array"); }
    { Args h; h.st.k = nullptr; li_case("li_null_k", h, INV, "sample index array"); }
    { Args h; h.st.spp = 0; li_case("li_spp_0", h, INV, "spp < 1"); }
    { Args h; h.st.n_tables = 0; li_case("li_n_tables_0", h, INV, "n_tables < 1"); }
    { Args h; h.st.first_1d = h.st.first_2d = 4; li_case("li_valid_cursors_at_n_dims", h, PBRT_OK); }
    { Args h; h.st.first_1d = h.st.first_2d = 0; li_case("li_valid_cursors_at_0", h, PBRT_OK); }
    {   // n_dims 0: nothing of the tables is read or required
        Args h;
        h.st = pbrt_strat_soa{nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0};
        li_case("li_valid_n_dims_0", h, PBRT_OK);
        h.st.first_2d = 1;
        li_case("li_n_dims_0_cursor_1", h, INV, "cursor");
    }
    {   // the order: li_device's cases (the render in flight last of them) before the strat block's
        Args h;
        h.st.reserved = 1;
        li_case("li_order_in_flight_before_strat", h, INV, "in flight", true, true);
        h.ld.reserved = 1;
        li_case("li_order_desc_first", h, INV, "reserved must be 0");
    }
    {   // the desc's refusals are li_query.h's own function: called by queries.hip, stated once
        const char* why = nullptr;
        pbrt_li_desc d = g.ld;
        d.integrator = PBRT_INTEGRATOR_DIRECT_LIGHTING;
        int rc = pbrtli::check_supported(d, false, &why);
        report("li_direct_lighting", rc, why, UNS, "Path integrator only");
        rc = pbrtli::check_supported(g.ld, true, &why);
        report("li_rough_glass", rc, why, UNS, "rough glass");
    }

    // ---- the pixel and table counts on ragged films
    struct FilmCase { int w, h, ts; };
    for (const FilmCase fc : {FilmCase{45, 30, 16}, FilmCase{17, 5, 4}, FilmCase{16, 16, 16}}) {
        const pbrt_film_desc f = film_of(fc.w, fc.h);
        const int64_t nt = (int64_t)((fc.w + fc.ts - 1) / fc.ts) * ((fc.h + fc.ts - 1) / fc.ts);
        for (int64_t b = 0; b <= nt; b++)
            for (int64_t e = b; e <= nt; e++) {
                const pbrt_frame_desc d{fc.ts, 3, b, e, 0, 0};
                const int64_t want = enumerate_pixels(fc.w, fc.h, fc.ts, b, e);
                expect(pixel_count(f, d) == want, "pixel_count is the enumeration");
                Args h;
                h.f = f;
                h.d = d;
                const char* why = nullptr;
                int64_t n = -1;
                expect(samples_call(h, true, &h.d, &h.sm, &h.out, &h.so, false, &n, &why) == PBRT_OK && n == want * 3,
                       "the sample count is pixels * ns");
            }
        const pbrt_frame_desc all{fc.ts, 3, 0, nt, 0, 0};
        std::printf("count %dx%d tile %d -> %lld pixels\n", fc.w, fc.h, fc.ts, (long long)pixel_count(f, all));
        expect(pixel_count(f, all) == (int64_t)fc.w * fc.h, "the whole film");
    }
    expect(table_doubles(g.sm) == 16 && table_doubles(pbrt_strat_sampler_desc{8, 8, 4, 0, 0}) == 256, "table_doubles");

    // ---- the cursors and the draws after the camera sample: pFilm (Get2D), pLens (Get2D), time (Get1D)
    for (int nd = 0; nd <= 5; nd++) {
        int c1 = 0, c2 = 0;
        uint32_t draws = 0;
        for (int req = 0; req < 2; req++) {
            if (c2 < nd) c2++;
            else draws += 2;
        }
        if (c1 < nd) c1++;
        else draws += 1;
        const Cursors c = cursors_after_camera(nd);
        std::printf("cursor %d -> %d %d draws %u\n", nd, c.first_1d, c.first_2d, camera_draws(nd));
        expect(c.first_1d == c1 && c.first_2d == c2 && camera_draws(nd) == draws, "the camera sample's cursors and draws");
    }
    expect(camera_draws(0) == 5 && camera_draws(1) == 2 && camera_draws(2) == 0, "5, 2, 0 draws");

    // ---- the StartPixel form and the LDS carve (render_params / layout_L of the same sampler)
    struct PlanCase { const char* name; int sx, sy, nd, jitter, form; bool non_matte; };
    for (const PlanCase pc : {PlanCase{"s2x2_nd4", 2, 2, 4, 0, 0, false}, PlanCase{"s3x3_nd1_jitter", 3, 3, 1, 1, 0, false},
                              PlanCase{"s1x2_nd2", 1, 2, 2, 0, 0, false}, PlanCase{"s8x8_nd4", 8, 8, 4, 0, 0, false},
                              PlanCase{"s11x11_nd4_windowed", 11, 11, 4, 0, 2, false},
                              PlanCase{"s11x11_nd4_kx_serial", 11, 11, 4, 0, 1, true},
                              PlanCase{"s6x6_nd4_jitter_buffered", 6, 6, 4, 1, 0, false},
                              PlanCase{"s7x7_nd4_jitter_serial", 7, 7, 4, 1, 1, false}}) {
        pbrtroute::Facts facts;
        facts.non_matte = pc.non_matte;
        const pbrt_strat_sampler_desc sm{pc.sx, pc.sy, pc.nd, pc.jitter, 0};
        const pbrt_frame_desc d{16, pc.sx * pc.sy - 1, 0, 1, 0, 0};
        const Plan p = plan(facts, pbrt::Knobs(), g.f, d, sm);
        const int n = pc.sx * pc.sy, s1 = pc.jitter ? 2 * n : n, s2 = pc.jitter ? 3 * n : n;
        std::printf("plan %s form %d events %d draws %d lds %d\n", pc.name, start_pixel_form(p.rp), p.rp.sp_events,
                    p.rp.sp_draws, p.lay.total);
        expect(start_pixel_form(p.rp) == pc.form, pc.name);
        expect(p.rp.spp == n && p.rp.ndims == pc.nd && p.rp.jitter == pc.jitter && p.rp.xs == pc.sx && p.rp.ys == pc.sy,
               "the sampler reaches the RenderParams");
        expect(p.rp.sp_events == pc.nd * (s1 + s2), "StartPixel's events");
        expect((p.rp.sp_serial != 0) == ((int64_t)p.rp.sp_draws * 4 > PBRT_SP_SERIAL_KB * 1024), "the sp_serial threshold");
        // the carve holds what start_pixel_wave touches: the values, the picks, the form's draw area
        expect(p.lay.s1d == 0 && p.lay.other >= pc.nd * n * 8 && p.lay.vbuf >= p.lay.other + pc.nd * n * 2 &&
                   p.lay.total >= p.lay.vbuf + (int)pbrtk::sp_vbuf_bytes(p.rp) && p.lay.total <= kMaxLds,
               "layout_L's carve");
    }

    // ---- the k_li_strat instantiation: k_li's rule
    for (int nm = 0; nm < 2; nm++)
        for (int nodes : {1, 64, 65, 121}) {
            const pbrtli::KernelArgs ka = kernel_args(nm != 0, nodes, false, 1000, 64), kl = pbrtli::kernel_args(nm != 0, nodes, false, 1000, 64);
            std::printf("kernel %d %d -> %d %d %u\n", nm, nodes, (int)ka.kx, ka.depth, ka.grid);
            expect(ka.kx == (nm != 0) && ka.depth == (nodes > 64 ? 64 : 0) && ka.grid == 4, "kX, kDepth and the grid");
            expect(ka.kx == kl.kx && ka.depth == kl.depth && ka.grid == kl.grid, "k_li's choice");
        }
    std::printf("checks=%ld bad=%ld\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}

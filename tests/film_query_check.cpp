// tests/film_query_check.cpp — host check of go-pbrt_amd/csrc/film_query.h, the
// frame layout and the argument checks of pbrt_gpu_frame_samples_device,
// pbrt_gpu_film_add_device and pbrt_gpu_film_rgba8_device, with no device:
//   - the layout against a literal enumeration (tiles in index order, pixels
//     row-major in their tile) on films whose size is a multiple of the tile,
//     ragged in x, in y and in both, cropped, of one tile and of one pixel:
//     pixels_before of every tile, locate of every pixel, pixels_in of every
//     range, the scratch size and the rows a range can reach;
//   - every PBRT_E_INVALID case of include/pbrt_gpu.h, each alone on otherwise
//     valid arguments, and the order of the checks where two conditions hold;
//   - every PBRT_E_UNSUPPORTED case, and which gather kernel a film gets.
// No pointer is dereferenced. Compiled with -fsanitize=address,undefined and
// run by tests/test_film_query_host.py. Without arguments it prints one
// "case <name> <status> <reason>" line per case and "checks=.. bad=..". With
// `layout res_x res_y min_x min_y max_x max_y tile_size` it prints the layout
// of that film instead: "tiles N", one "tile t pixels_before" line per tile
// and one "px g tile pi x y" line per pixel, for the test to compare with
// tests/li_reference.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../go-pbrt_amd/csrc/film_query.h"

using namespace pbrtfilm;

static long g_checks = 0, g_bad = 0;

static void expect(bool ok, const char* what) {
    g_checks++;
    if (!ok) {
        g_bad++;
        std::printf("FAILED %s\n", what);
    }
}

static pbrt_film_desc film_of(int64_t rx, int64_t ry, int64_t x0, int64_t y0, int64_t x1, int64_t y1, double radius) {
    pbrt_film_desc f;
    std::memset(&f, 0, sizeof(f));
    f.res_x = rx;
    f.res_y = ry;
    f.crop_min_x = x0;
    f.crop_min_y = y0;
    f.crop_max_x = x1;
    f.crop_max_y = y1;
    f.filter_radius_x = f.filter_radius_y = radius;
    f.max_sample_luminance = 1.0;
    return f;
}

// integrator.go:316-325, literally
static void tile_box(const pbrt_film_desc& f, int64_t ts, int64_t t, int64_t b[4]) {
    const int64_t w = f.crop_max_x - f.crop_min_x, ntx = (w + ts - 1) / ts;
    b[0] = f.crop_min_x + (t % ntx) * ts;
    b[1] = f.crop_min_y + (t / ntx) * ts;
    b[2] = b[0] + ts < f.crop_max_x ? b[0] + ts : f.crop_max_x;
    b[3] = b[1] + ts < f.crop_max_y ? b[1] + ts : f.crop_max_y;
}

static void layout_case(const pbrt_film_desc& f, int64_t ts) {
    const Layout l = layout(f, ts);
    const int64_t nt = num_tiles(l);
    std::vector<int64_t> before((size_t)nt + 1);
    int64_t g = 0;
    for (int64_t t = 0; t < nt; t++) {
        int64_t b[4];
        tile_box(f, ts, t, b);
        before[(size_t)t] = g;
        expect(pixels_before(l, t) == g, "pixels_before");
        for (int64_t y = b[1]; y < b[3]; y++)
            for (int64_t x = b[0]; x < b[2]; x++, g++) {
                const Where w = locate(l, g);
                expect(w.tile == t && w.pi == (y - b[1]) * (b[2] - b[0]) + (x - b[0]) && w.px == x && w.py == y, "locate");
            }
    }
    before[(size_t)nt] = g;
    expect(g == l.w * l.h && pixels_before(l, nt) == g && pixels_before(l, nt + 5) == g, "the whole film");
    const int64_t step = nt > 48 ? nt / 24 : 1;   // every range of a small film, a grid of them on a large one
    for (int64_t b = 0; b <= nt; b += step)
        for (int64_t e = 0; e <= nt; e += step) {
            expect(pixels_in(l, b, e) == (b < e ? before[(size_t)e] - before[(size_t)b] : 0), "pixels_in");
            // the rows a range reaches hold every film pixel of its tiles' films
            if (b < e) {
                const Rows r = rows_touched(l, f, b, e, false);
                const int64_t reach = (int64_t)(f.filter_radius_y + 0.5);
                for (int64_t t = b; t < e; t++) {
                    int64_t tb[4];
                    tile_box(f, ts, t, tb);
                    int64_t y0 = tb[1] - reach - f.crop_min_y, y1 = tb[3] + reach - f.crop_min_y;
                    if (y0 < 0) y0 = 0;
                    if (y1 > l.h) y1 = l.h;
                    expect(r.y0 <= y0 && y1 <= r.y1 && 0 <= r.y0 && r.y1 <= l.h, "rows_touched holds the tile films");
                }
                const Rows all = rows_touched(l, f, b, e, true);
                expect(all.y0 == 0 && all.y1 == l.h, "clear writes every row");
            }
        }
    const Rows none = rows_touched(l, f, 3, 3, false), cleared = rows_touched(l, f, 3, 3, true);
    expect(none.y1 - none.y0 == 0 && cleared.y0 == 0 && cleared.y1 == l.h, "an empty range touches nothing, or clears");
    const int64_t sw = slot_extent(ts, f.filter_radius_x), sh = slot_extent(ts, f.filter_radius_y);
    expect(sw >= ts + 2 * (int64_t)(f.filter_radius_x + 0.5), "a slot holds the widest tile film");
    expect(scratch_doubles(f, ts, 1, 1) == 0 && scratch_doubles(f, ts, 0, nt) == (size_t)(nt * sw * sh * 3), "scratch");
}

static void print_layout(int argc, char** argv) {
    if (argc != 9) std::exit(2);
    int64_t v[7];
    for (int i = 0; i < 7; i++) v[i] = std::atoll(argv[2 + i]);
    const pbrt_film_desc f = film_of(v[0], v[1], v[2], v[3], v[4], v[5], 1.0);
    const Layout l = layout(f, v[6]);
    std::printf("tiles %lld\n", (long long)num_tiles(l));
    for (int64_t t = 0; t <= num_tiles(l); t++) std::printf("tile %lld %lld\n", (long long)t, (long long)pixels_before(l, t));
    for (int64_t g = 0; g < l.w * l.h; g++) {
        const Where w = locate(l, g);
        std::printf("px %lld %lld %lld %lld %lld\n", (long long)g, (long long)w.tile, (long long)w.pi, (long long)w.px,
                    (long long)w.py);
    }
}

static int frame_case(const char* name, bool ctx_ok, const pbrt_film_desc* f, const pbrt_frame_desc* d, int32_t flags_ok,
                      bool in_flight, int want, int64_t want_count = -1) {
    const char* why = nullptr;
    int64_t n = -7;
    int rc = check_frame(ctx_ok, f, d, flags_ok, in_flight, &n, &why);
    if (rc == PBRT_OK) rc = check_frame_supported(*f, *d, flags_ok != 0, &why);
    std::printf("case %s %d %s\n", name, rc, why ? why : "(null)");
    expect(rc == want, name);
    expect(why != nullptr && (rc == PBRT_OK) == (why[0] == 0), "a refusal names its reason");
    if (rc != PBRT_OK && rc != PBRT_E_UNSUPPORTED) expect(n == 0, "a refused desc counts nothing");
    if (want_count >= 0) expect(n == want_count, "the count");
    return rc;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "layout") == 0) {
        print_layout(argc, argv);
        return 0;
    }
    const int INV = PBRT_E_INVALID, UNS = PBRT_E_UNSUPPORTED, CLR = PBRT_FILM_ADD_CLEAR;
    // ---- the layout
    const pbrt_film_desc films[] = {
        film_of(32, 32, 0, 0, 32, 32, 1.0),   film_of(40, 24, 0, 0, 40, 24, 1.0),  film_of(45, 30, 0, 0, 45, 30, 2.7),
        film_of(80, 48, 0, 0, 80, 48, 0.5),   film_of(64, 40, 16, 4, 51, 36, 1.5), film_of(7, 5, 0, 0, 7, 5, 1.0),
        film_of(1, 1, 0, 0, 1, 1, 0.5),       film_of(64, 40, 63, 39, 64, 40, 1.0), film_of(33, 17, 1, 0, 33, 17, 1.0),
    };
    for (const pbrt_film_desc& f : films)
        for (int64_t ts : {1, 2, 5, 8, 13, 16, 64, 256}) layout_case(f, ts);

    // ---- PBRT_E_INVALID of the frame calls
    const pbrt_film_desc f = films[1];   // 40 x 24: 3 x 2 tiles of 16
    const pbrt_frame_desc ok{16, 2, 0, 6, 0, 0};
    auto with = [&](auto set) {
        pbrt_frame_desc d = ok;
        set(d);
        return d;
    };
    frame_case("valid", true, &f, &ok, 0, false, PBRT_OK, 40 * 24 * 2);
    pbrt_frame_desc d = with([](pbrt_frame_desc& q) { q.tile_begin = 2; q.tile_end = 3; });
    frame_case("valid_single_tile", true, &f, &d, 0, false, PBRT_OK, 8 * 16 * 2);
    d = with([](pbrt_frame_desc& q) { q.tile_begin = 4; q.tile_end = 4; });
    frame_case("valid_empty", true, &f, &d, 0, false, PBRT_OK, 0);
    d = with([](pbrt_frame_desc& q) { q.tile_begin = 6; q.tile_end = 6; });
    frame_case("valid_empty_at_end", true, &f, &d, 0, false, PBRT_OK, 0);
    d = with([&](pbrt_frame_desc& q) { q.flags = CLR; });
    frame_case("valid_clear", true, &f, &d, CLR, false, PBRT_OK, 40 * 24 * 2);
    d = with([](pbrt_frame_desc& q) { q.tile_size = 256; q.tile_end = 1; q.ns = (1 << 20) - 1; });
    frame_case("valid_largest", true, &f, &d, CLR, false, PBRT_OK, (int64_t)40 * 24 * ((1 << 20) - 1));
    frame_case("null_ctx", false, nullptr, &ok, 0, false, INV);
    frame_case("null_desc", true, &f, nullptr, 0, false, INV);
    d = with([](pbrt_frame_desc& q) { q.tile_size = 0; });
    frame_case("tile_size_0", true, &f, &d, 0, false, INV);
    d = with([](pbrt_frame_desc& q) { q.tile_size = -16; });
    frame_case("tile_size_negative", true, &f, &d, 0, false, INV);
    d = with([](pbrt_frame_desc& q) { q.ns = 0; });
    frame_case("ns_0", true, &f, &d, 0, false, INV);
    d = with([](pbrt_frame_desc& q) { q.ns = -1; });
    frame_case("ns_negative", true, &f, &d, 0, false, INV);
    d = with([&](pbrt_frame_desc& q) { q.flags = CLR; });
    frame_case("samples_clear_flag", true, &f, &d, 0, false, INV);
    d = with([](pbrt_frame_desc& q) { q.flags = 2; });
    frame_case("unknown_flag", true, &f, &d, CLR, false, INV);
    d = with([](pbrt_frame_desc& q) { q.reserved = 1; });
    frame_case("reserved", true, &f, &d, 0, false, INV);
    d = with([](pbrt_frame_desc& q) { q.tile_begin = -1; });
    frame_case("begin_negative", true, &f, &d, 0, false, INV);
    d = with([](pbrt_frame_desc& q) { q.tile_begin = 4; q.tile_end = 3; });
    frame_case("end_before_begin", true, &f, &d, 0, false, INV);
    d = with([](pbrt_frame_desc& q) { q.tile_end = 7; });
    frame_case("end_past_the_film", true, &f, &d, 0, false, INV);
    {   // 1920 x 1080 at 1200 samples a pixel: 2.49e9 elements
        const pbrt_film_desc hd = film_of(1920, 1080, 0, 0, 1920, 1080, 1.0);
        pbrt_frame_desc q{16, 1200, 0, 120 * 68, 0, 0};
        frame_case("more_than_2_31", true, &hd, &q, 0, false, INV);
        q.tile_end = 120;   // one tile row
        frame_case("valid_one_row_of_1080p", true, &hd, &q, 0, false, PBRT_OK, (int64_t)1920 * 16 * 1200);
    }
    frame_case("in_flight", true, &f, &ok, 0, true, INV);
    d = with([](pbrt_frame_desc& q) { q.tile_begin = 4; q.tile_end = 4; });
    frame_case("in_flight_empty", true, &f, &d, 0, true, INV);
    {   // the order: a NULL context first, a render in flight last
        const char* why = nullptr;
        int64_t n = 0;
        pbrt_frame_desc q = with([](pbrt_frame_desc& z) { z.ns = 0; });
        expect(check_frame(false, nullptr, nullptr, 0, true, &n, &why) == INV && std::strstr(why, "context"), "context first");
        expect(check_frame(true, &f, &q, 0, true, &n, &why) == INV && std::strstr(why, "ns"), "in flight last");
    }
    // ---- PBRT_E_UNSUPPORTED
    d = with([](pbrt_frame_desc& q) { q.tile_size = 257; q.tile_end = 1; });
    frame_case("tile_size_257", true, &f, &d, 0, false, UNS);
    d = with([](pbrt_frame_desc& q) { q.ns = 1 << 20; });
    frame_case("ns_2_20", true, &f, &d, 0, false, UNS);
    d = with([](pbrt_frame_desc& q) { q.ns = 1 << 20; });
    frame_case("ns_2_20_in_flight", true, &f, &d, 0, true, INV);
    {
        pbrt_film_desc wide = f;
        wide.filter_radius_x = 16.0;   // the tile film of tile 0 would reach tile 2
        frame_case("radius_is_the_tile", true, &wide, &ok, CLR, false, UNS);
        frame_case("samples_ignore_the_filter", true, &wide, &ok, 0, false, PBRT_OK);
        wide.filter_radius_x = 15.99;
        frame_case("radius_below_the_tile", true, &wide, &ok, CLR, false, PBRT_OK);
        wide.filter_radius_x = 1.0;
        wide.filter_radius_y = 0.0;
        frame_case("radius_0", true, &wide, &ok, CLR, false, UNS);
        wide.filter_radius_y = -1.0;
        frame_case("radius_negative", true, &wide, &ok, CLR, false, UNS);
        wide.filter_radius_y = __builtin_nan("");
        frame_case("radius_nan", true, &wide, &ok, CLR, false, UNS);
        pbrt_frame_desc t8 = with([](pbrt_frame_desc& q) { q.tile_size = 8; q.tile_end = 15; });
        wide.filter_radius_y = 8.5;
        frame_case("radius_beyond_a_tile_of_8", true, &wide, &t8, CLR, false, UNS);
    }
    // ---- the pointer checks
    {
        double a[16];
        uint64_t s[2];
        int32_t p[2];
        const char* why = nullptr;
        auto pcase = [&](const char* name, int rc, int want) {
            std::printf("case %s %d %s\n", name, rc, why ? why : "(null)");
            expect(rc == want, name);
            expect(why != nullptr && (rc == PBRT_OK) == (why[0] == 0), "a refusal names its reason");
        };
        const pbrt_frame_samples_soa so{a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7, a + 8, s, s + 1, p, p + 1};
        pcase("samples_valid", check_samples_out(&so, &why), PBRT_OK);
        pbrt_frame_samples_soa q = so;
        q.tmax = nullptr;
        q.px = q.py = nullptr;
        pcase("samples_valid_without_optional", check_samples_out(&q, &why), PBRT_OK);
        pcase("samples_null_out", check_samples_out(nullptr, &why), INV);
#define NULL_FIELD(S, BASE, FIELD, CHECK) \
    {                                       \
        S z = BASE;                         \
        z.FIELD = nullptr;                  \
        pcase(#S "_null_" #FIELD, CHECK, INV); \
    }
        NULL_FIELD(pbrt_frame_samples_soa, so, ox, check_samples_out(&z, &why))
        NULL_FIELD(pbrt_frame_samples_soa, so, oy, check_samples_out(&z, &why))
        NULL_FIELD(pbrt_frame_samples_soa, so, oz, check_samples_out(&z, &why))
        NULL_FIELD(pbrt_frame_samples_soa, so, dx, check_samples_out(&z, &why))
        NULL_FIELD(pbrt_frame_samples_soa, so, dy, check_samples_out(&z, &why))
        NULL_FIELD(pbrt_frame_samples_soa, so, dz, check_samples_out(&z, &why))
        NULL_FIELD(pbrt_frame_samples_soa, so, pfilm_x, check_samples_out(&z, &why))
        NULL_FIELD(pbrt_frame_samples_soa, so, pfilm_y, check_samples_out(&z, &why))
        NULL_FIELD(pbrt_frame_samples_soa, so, state, check_samples_out(&z, &why))
        NULL_FIELD(pbrt_frame_samples_soa, so, inc, check_samples_out(&z, &why))
        const pbrt_film_samples_soa fi{a, a + 1, a + 2, a + 3, a + 4};
        pcase("film_valid", check_film_in(&fi, a + 5, &why), PBRT_OK);
        pcase("film_null_samples", check_film_in(nullptr, a + 5, &why), INV);
        pcase("film_null_film", check_film_in(&fi, nullptr, &why), INV);
        NULL_FIELD(pbrt_film_samples_soa, fi, pfilm_x, check_film_in(&z, a + 5, &why))
        NULL_FIELD(pbrt_film_samples_soa, fi, pfilm_y, check_film_in(&z, a + 5, &why))
        NULL_FIELD(pbrt_film_samples_soa, fi, r, check_film_in(&z, a + 5, &why))
        NULL_FIELD(pbrt_film_samples_soa, fi, g, check_film_in(&z, a + 5, &why))
        NULL_FIELD(pbrt_film_samples_soa, fi, b, check_film_in(&z, a + 5, &why))
#undef NULL_FIELD
        alignas(8) uint8_t bytes[16];
        pcase("rgba8_valid", check_rgba8(true, a, 40, 24, bytes, false, &why), PBRT_OK);
        pcase("rgba8_null_ctx", check_rgba8(false, a, 40, 24, bytes, false, &why), INV);
        pcase("rgba8_null_film", check_rgba8(true, nullptr, 40, 24, bytes, false, &why), INV);
        pcase("rgba8_null_rgba", check_rgba8(true, a, 40, 24, nullptr, false, &why), INV);
        pcase("rgba8_misaligned_rgba", check_rgba8(true, a, 40, 24, bytes + 2, false, &why), INV);
        pcase("rgba8_misaligned_film", check_rgba8(true, (const double*)(bytes + 4), 40, 24, bytes, false, &why), INV);
        pcase("rgba8_w_0", check_rgba8(true, a, 0, 24, bytes, false, &why), INV);
        pcase("rgba8_h_negative", check_rgba8(true, a, 40, -1, bytes, false, &why), INV);
        pcase("rgba8_2_31_pixels", check_rgba8(true, a, 65536, 32768, bytes, false, &why), INV);
        pcase("rgba8_valid_largest", check_rgba8(true, a, INT32_MAX, 1, bytes, false, &why), PBRT_OK);
        pcase("rgba8_huge", check_rgba8(true, a, INT64_MAX, INT64_MAX, bytes, false, &why), INV);
        pcase("rgba8_in_flight", check_rgba8(true, a, 40, 24, bytes, true, &why), INV);
    }
    // ---- the gather kernel of a film: the LDS-staged one up to 512 tile-film pixels
    expect(lds_gather(true, films[1], 16) && !lds_gather(false, films[1], 16), "the knob");
    expect(lds_gather(true, films[2], 16), "radius 2.7 at tile 16: 22 x 22");
    {
        pbrt_film_desc r3 = films[1];
        r3.filter_radius_x = r3.filter_radius_y = 3.0;   // 24 x 24
        expect(!lds_gather(true, r3, 16) && lds_gather(true, r3, 8), "radius 3 at tile 16 is beyond, at tile 8 inside");
        expect(!lds_gather(true, films[1], 32), "tile 32");
    }
    std::printf("checks=%ld bad=%ld\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}

// tests/direct_li_query_check.cpp — host check of pbrt_gpu_direct_li_device's
// argument checks, refusals, kernel choice and level-record size
// (go-pbrt_amd/csrc/direct_li_query.h), with no device:
//   - every PBRT_E_INVALID case of include/pbrt_gpu.h, each alone on otherwise
//     valid arguments, in the header's order, and the order of the checks where
//     two conditions hold (a NULL context first, a render in flight last);
//   - every PBRT_E_UNSUPPORTED case: an unknown dl_strategy, rough glass,
//     max_depth > 64 on a scene with Mirror / Glass / OrenNayar; any max_depth on
//     a Matte-only scene passes;
//   - the kernel-argument table over (non_matte, n_nodes, mesh), the grid capped
//     and clamped;
//   - levels(max_depth) against a literal count of the reference's recursion, and
//     the storage size at max_depth 1, 2, 3, 63, 64 and at the grid cap.
// The ray pointers are never dereferenced. Compiled with
// -fsanitize=address,undefined and run by tests/test_direct_li_host.py. Prints
// one "case <name> <status> <reason>" line per case, one "kernel ..." line per
// row of the table, one "levels ..." / "bytes ..." line per size, and
// "checks=.. bad=..".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../go-pbrt_amd/csrc/direct_li_query.h"

using namespace pbrtdli;

static long g_checks = 0, g_bad = 0;

static void expect(bool ok, const char* what) {
    g_checks++;
    if (!ok) {
        g_bad++;
        std::printf("FAILED %s\n", what);
    }
}

struct Args {
    double a[8];
    uint64_t s[2];
    double o[3];
    pbrt_direct_li_desc d;
    pbrt_ray_soa rays;
    pbrt_rng_soa rng;
    pbrt_radiance_soa out;
    Args() {
        d = pbrt_direct_li_desc{5, PBRT_DL_UNIFORM_SAMPLE_ALL, {0, 0}};
        rays = pbrt_ray_soa{a, a + 1, a + 2, a + 3, a + 4, a + 5, nullptr};
        rng = pbrt_rng_soa{s, s + 1};
        out = pbrt_radiance_soa{o, o + 1, o + 2, nullptr, nullptr, nullptr};
    }
};

static int invalid_case(const char* name, bool ctx_ok, const pbrt_direct_li_desc* d, const pbrt_ray_soa* rays,
                        const pbrt_rng_soa* rng, size_t n, const pbrt_radiance_soa* out, bool in_flight, int want) {
    const char* why = nullptr;
    const int rc = check_args(ctx_ok, d, rays, rng, n, out, in_flight, &why);
    std::printf("case %s %d %s\n", name, rc, why ? why : "(null)");
    expect(rc == want, name);
    expect(why != nullptr && (rc == PBRT_OK) == (why[0] == 0), "a refusal names its reason");
    return rc;
}

// the reference's recursion, literally: Li(depth) pushes a level where depth + 1 < max_depth and
// SpecularTransmit recurses at depth + 2 (directlighting.go:95-101, integrator.go:383-422)
static int levels_literal(int max_depth) {
    int n = 0;
    for (int depth = 0; depth + 1 < max_depth && n < kMaxLevels; depth += 2) n++;
    return n;
}

int main() {
    Args g;
    const int INV = PBRT_E_INVALID, UNS = PBRT_E_UNSUPPORTED;
    invalid_case("valid", true, &g.d, &g.rays, &g.rng, 4, &g.out, false, PBRT_OK);
    invalid_case("valid_n0", true, &g.d, &g.rays, &g.rng, 0, &g.out, false, PBRT_OK);
    invalid_case("valid_nmax", true, &g.d, &g.rays, &g.rng, (size_t)INT32_MAX, &g.out, false, PBRT_OK);
    invalid_case("null_ctx", false, &g.d, &g.rays, &g.rng, 4, &g.out, false, INV);
    invalid_case("null_desc", true, nullptr, &g.rays, &g.rng, 4, &g.out, false, INV);
    invalid_case("null_rays", true, &g.d, nullptr, &g.rng, 4, &g.out, false, INV);
    invalid_case("null_rng", true, &g.d, &g.rays, nullptr, 4, &g.out, false, INV);
    invalid_case("null_out", true, &g.d, &g.rays, &g.rng, 4, nullptr, false, INV);
    const char* ray_names[6] = {"null_ox", "null_oy", "null_oz", "null_dx", "null_dy", "null_dz"};
    for (int k = 0; k < 6; k++) {
        Args h;
        const double** p[6] = {&h.rays.ox, &h.rays.oy, &h.rays.oz, &h.rays.dx, &h.rays.dy, &h.rays.dz};
        *p[k] = nullptr;
        invalid_case(ray_names[k], true, &h.d, &h.rays, &h.rng, 4, &h.out, false, INV);
    }
    {
        Args h;
        h.rays.tmax = h.a + 6;   // tmax is optional either way
        invalid_case("with_tmax", true, &h.d, &h.rays, &h.rng, 4, &h.out, false, PBRT_OK);
    }
    {
        Args h;
        h.rng.state = nullptr;
        invalid_case("null_state", true, &h.d, &h.rays, &h.rng, 4, &h.out, false, INV);
        Args h2;
        h2.rng.inc = nullptr;
        invalid_case("null_inc", true, &h2.d, &h2.rays, &h2.rng, 4, &h2.out, false, INV);
    }
    const char* out_names[3] = {"null_r", "null_g", "null_b"};
    for (int k = 0; k < 3; k++) {
        Args h;
        double** p[3] = {&h.out.r, &h.out.g, &h.out.b};
        *p[k] = nullptr;
        invalid_case(out_names[k], true, &h.d, &h.rays, &h.rng, 4, &h.out, false, INV);
    }
    invalid_case("n_2_31", true, &g.d, &g.rays, &g.rng, (size_t)INT32_MAX + 1, &g.out, false, INV);
    invalid_case("n_huge", true, &g.d, &g.rays, &g.rng, SIZE_MAX, &g.out, false, INV);
    {
        Args h;
        h.d.max_depth = 0;
        invalid_case("depth_0", true, &h.d, &h.rays, &h.rng, 4, &h.out, false, INV);
        h.d.max_depth = -3;
        invalid_case("depth_negative", true, &h.d, &h.rays, &h.rng, 4, &h.out, false, INV);
        Args h2;
        h2.d.reserved[0] = 1;
        invalid_case("reserved_0", true, &h2.d, &h2.rays, &h2.rng, 4, &h2.out, false, INV);
        Args h3;
        h3.d.reserved[1] = -1;
        invalid_case("reserved_1", true, &h3.d, &h3.rays, &h3.rng, 4, &h3.out, false, INV);
    }
    invalid_case("in_flight", true, &g.d, &g.rays, &g.rng, 4, &g.out, true, INV);
    invalid_case("in_flight_n0", true, &g.d, &g.rays, &g.rng, 0, &g.out, true, INV);
    {   // the order: a NULL context before anything is read, the render in flight last
        const char* why = nullptr;
        expect(check_args(false, nullptr, nullptr, nullptr, SIZE_MAX, nullptr, true, &why) == INV &&
                   !std::strcmp(why, "null context"), "null context first");
        Args h;
        h.d.reserved[1] = 7;
        expect(check_args(true, &h.d, &h.rays, &h.rng, 4, &h.out, true, &why) == INV &&
                   !std::strcmp(why, "reserved must be 0"), "the desc before the render in flight");
        h.d.max_depth = 0;
        expect(check_args(true, &h.d, &h.rays, &h.rng, 4, &h.out, true, &why) == INV &&
                   !std::strcmp(why, "max_depth < 1"), "max_depth before reserved");
        expect(check_args(true, &h.d, &h.rays, &h.rng, SIZE_MAX, &h.out, true, &why) == INV &&
                   !std::strcmp(why, "more than 2^31 - 1 rays in one query"), "n before the desc's fields");
    }

    // ---- PBRT_E_UNSUPPORTED
    auto unsupported_case = [&](const char* name, pbrt_direct_li_desc d, bool rough, bool non_matte, int want,
                                const char* word) {
        const char* why = nullptr;
        const int rc = check_supported(d, rough, non_matte, &why);
        std::printf("case %s %d %s\n", name, rc, why ? why : "(null)");
        expect(rc == want, name);
        expect(why != nullptr && (rc == PBRT_OK) == (why[0] == 0), "a refusal names its reason");
        expect(why != nullptr && std::strstr(why, word) != nullptr, "the reason holds its word");
    };
    pbrt_direct_li_desc d = g.d;
    unsupported_case("supported", d, false, false, PBRT_OK, "");
    unsupported_case("supported_kx", d, false, true, PBRT_OK, "");
    d.dl_strategy = PBRT_DL_UNIFORM_SAMPLE_ONE;
    unsupported_case("sample_one", d, false, true, PBRT_OK, "");
    d.dl_strategy = 0;
    unsupported_case("strategy_0", d, false, false, UNS, "strategy");
    d.dl_strategy = 3;
    unsupported_case("strategy_3", d, false, true, UNS, "strategy");
    unsupported_case("rough_glass", g.d, true, true, UNS, "rough glass");
    d = g.d;
    d.max_depth = 64;
    unsupported_case("kx_depth_64", d, false, true, PBRT_OK, "");
    d.max_depth = 65;
    unsupported_case("kx_depth_65", d, false, true, UNS, "64");
    unsupported_case("matte_depth_65", d, false, false, PBRT_OK, "");
    d.max_depth = INT32_MAX;
    unsupported_case("matte_depth_max", d, false, false, PBRT_OK, "");
    unsupported_case("kx_depth_max", d, false, true, UNS, "64");
    {   // the order: the strategy, then rough glass, then the depth
        const char* why = nullptr;
        pbrt_direct_li_desc e{65, 3, {0, 0}};
        expect(check_supported(e, true, true, &why) == UNS && std::strstr(why, "strategy"), "the strategy first");
        e.dl_strategy = PBRT_DL_UNIFORM_SAMPLE_ALL;
        expect(check_supported(e, true, true, &why) == UNS && std::strstr(why, "rough glass"), "rough glass second");
    }

    // ---- the kernel-argument table
    const int kLds = 64;
    for (int nm = 0; nm < 2; nm++)
        for (int mesh = 0; mesh < 2; mesh++)
            for (int nodes : {0, 1, 63, 64, 65, 121, 100000}) {
                const KernelArgs ka = kernel_args(nm != 0, nodes, mesh != 0, 1000, kLds, 2048, 5);
                std::printf("kernel %d %d %d -> %d %d %u %d %zu\n", nm, nodes, mesh, (int)ka.kx, ka.depth, ka.grid,
                            ka.levels, ka.level_doubles);
                expect(ka.kx == (nm != 0), "kX is the scene's non_matte");
                expect(ka.depth == (nodes > kLds ? 64 : 0), "kDepth 64 beyond the LDS-staged trees, else 0");
                expect(ka.grid == 4, "1000 rays: 4 waves of 256");
                expect(ka.levels == (nm ? 2 : 0), "two levels at max_depth 5, none without kX");
                expect(ka.level_doubles == (nm ? (size_t)4 * 2 * 7 * 64 : 0), "kX false carries no level storage");
            }
    // the grid: the work lists of n, capped; the cap clamped to 1 .. kGridCapMax
    const size_t ns[] = {1, 255, 256, 257, 511, 512, 513, 1000, 2073600, (size_t)INT32_MAX};
    for (size_t n : ns)
        for (int cap : {-5, 0, 1, 2, 3, 2048, kGridCapMax, kGridCapMax + 1, INT32_MAX}) {
            const KernelArgs ka = kernel_args(true, 45, false, n, kLds, cap, 64);
            const uint64_t lists = (n + kRays - 1) / kRays;
            const uint64_t c = cap < 1 ? 1 : cap > kGridCapMax ? kGridCapMax : (uint64_t)cap;
            std::printf("grid %zu cap %d -> %u\n", n, cap, ka.grid);
            expect(ka.grid == (lists < c ? lists : c) && ka.grid >= 1, "the grid is the lists of n, capped");
            expect(ka.level_doubles == (size_t)ka.grid * 32 * 7 * 64, "32 levels of 7 doubles a lane at max_depth 64");
        }

    // ---- levels and the storage size
    for (int md = 1; md <= 200; md++) expect(levels(md) == levels_literal(md), "levels(max_depth) is the recursion's count");
    expect(levels(0) == 0 && levels(-7) == 0 && levels(INT32_MAX) == kMaxLevels, "levels outside the served depths");
    const int want_levels[][2] = {{1, 0}, {2, 1}, {3, 1}, {63, 31}, {64, 32}};
    for (const auto& wl : want_levels) {
        std::printf("levels %d -> %d\n", wl[0], levels(wl[0]));
        expect(levels(wl[0]) == wl[1], "levels at max_depth 1, 2, 3, 63, 64");
        for (uint32_t grid : {1u, 2u, 2048u, (uint32_t)kGridCapMax}) {
            const size_t bytes = level_doubles(grid, wl[0]) * sizeof(double);
            std::printf("bytes grid %u max_depth %d -> %zu\n", grid, wl[0], bytes);
            expect(bytes == (size_t)grid * (size_t)wl[1] * 64 * 56, "grid * levels * 64 lanes * 56 B");
        }
    }
    expect(level_doubles(kGridCapMax, 64) * sizeof(double) == (size_t)65536 * 32 * 64 * 56, "the size at the grid cap");
    {   // n far beyond the cap adds nothing: the records are bounded independently of n
        const KernelArgs a = kernel_args(true, 45, false, (size_t)2048 * kRays, kLds, 2048, 10);
        const KernelArgs b = kernel_args(true, 45, false, (size_t)INT32_MAX, kLds, 2048, 10);
        expect(a.grid == 2048 && b.grid == 2048 && a.level_doubles == b.level_doubles, "bounded independently of n");
    }
    expect(kRays == 256 && kMaxLevels == 32 && kMaxDepthX == 64 && kRecDoubles * sizeof(double) == 56 &&
               kWaveLanes == 64, "the constants of the contract");
    std::printf("checks=%ld bad=%ld\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}

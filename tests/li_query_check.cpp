// tests/li_query_check.cpp — host check of pbrt_gpu_li_device's argument checks
// and kernel choice (go-pbrt_amd/csrc/li_query.h), with no device:
//   - every PBRT_E_INVALID case of include/pbrt_gpu.h, each alone on otherwise
//     valid arguments, and that the valid arguments pass; the order of the
//     checks where two conditions hold (a NULL context first, a render in
//     flight last);
//   - every PBRT_E_UNSUPPORTED case: the integrator, max_depth > 2048, an unknown
//     light strategy, rough glass, and a distribution that mixes lights of pdf 0
//     with others (one func 0, a negative, a NaN, a zero integral over nonzero
//     entries, more entries than lights); the reference's all-zero Power
//     distribution and a scene without lights pass;
//   - the kernel-argument table over (non_matte, n_nodes, mesh) and the grid for
//     n around the multiples of kLiRays and at 2^31 - 1.
// The ray pointers are never dereferenced. Compiled with
// -fsanitize=address,undefined and run by tests/test_li_host.py. Prints one
// "case <name> <status> <reason>" line per case, one "kernel ..." line per row of
// the table, and "checks=.. bad=..".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../go-pbrt_amd/csrc/li_query.h"

using namespace pbrtli;

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
    pbrt_li_desc d;
    pbrt_ray_soa rays;
    pbrt_rng_soa rng;
    pbrt_radiance_soa out;
    Args() {
        d = pbrt_li_desc{PBRT_INTEGRATOR_PATH, 5, PBRT_LIGHT_STRATEGY_UNIFORM, 0, 1.0};
        rays = pbrt_ray_soa{a, a + 1, a + 2, a + 3, a + 4, a + 5, nullptr};
        rng = pbrt_rng_soa{s, s + 1};
        out = pbrt_radiance_soa{o, o + 1, o + 2, nullptr, nullptr, nullptr};
    }
};

static int invalid_case(const char* name, bool ctx_ok, const Args& g, const pbrt_li_desc* d, const pbrt_ray_soa* rays,
                        const pbrt_rng_soa* rng, size_t n, const pbrt_radiance_soa* out, bool in_flight, int want) {
    (void)g;
    const char* why = nullptr;
    const int rc = check_args(ctx_ok, d, rays, rng, n, out, in_flight, &why);
    std::printf("case %s %d %s\n", name, rc, why ? why : "(null)");
    expect(rc == want, name);
    expect(why != nullptr && (rc == PBRT_OK) == (why[0] == 0), "a refusal names its reason");
    return rc;
}

int main() {
    Args g;
    const int INV = PBRT_E_INVALID, UNS = PBRT_E_UNSUPPORTED;
    invalid_case("valid", true, g, &g.d, &g.rays, &g.rng, 4, &g.out, false, PBRT_OK);
    invalid_case("valid_n0", true, g, &g.d, &g.rays, &g.rng, 0, &g.out, false, PBRT_OK);
    invalid_case("valid_nmax", true, g, &g.d, &g.rays, &g.rng, (size_t)INT32_MAX, &g.out, false, PBRT_OK);
    invalid_case("null_ctx", false, g, &g.d, &g.rays, &g.rng, 4, &g.out, false, INV);
    invalid_case("null_desc", true, g, nullptr, &g.rays, &g.rng, 4, &g.out, false, INV);
    invalid_case("null_rays", true, g, &g.d, nullptr, &g.rng, 4, &g.out, false, INV);
    invalid_case("null_rng", true, g, &g.d, &g.rays, nullptr, 4, &g.out, false, INV);
    invalid_case("null_out", true, g, &g.d, &g.rays, &g.rng, 4, nullptr, false, INV);
    const char* ray_names[6] = {"null_ox", "null_oy", "null_oz", "null_dx", "null_dy", "null_dz"};
    for (int k = 0; k < 6; k++) {
        Args h;
        const double** p[6] = {&h.rays.ox, &h.rays.oy, &h.rays.oz, &h.rays.dx, &h.rays.dy, &h.rays.dz};
        *p[k] = nullptr;
        invalid_case(ray_names[k], true, h, &h.d, &h.rays, &h.rng, 4, &h.out, false, INV);
    }
    {
        Args h;
        h.rays.tmax = h.a + 6;   // tmax is optional either way
        invalid_case("with_tmax", true, h, &h.d, &h.rays, &h.rng, 4, &h.out, false, PBRT_OK);
    }
    {
        Args h;
        h.rng.state = nullptr;
        invalid_case("null_state", true, h, &h.d, &h.rays, &h.rng, 4, &h.out, false, INV);
        Args h2;
        h2.rng.inc = nullptr;
        invalid_case("null_inc", true, h2, &h2.d, &h2.rays, &h2.rng, 4, &h2.out, false, INV);
    }
    const char* out_names[3] = {"null_r", "null_g", "null_b"};
    for (int k = 0; k < 3; k++) {
        Args h;
        double** p[3] = {&h.out.r, &h.out.g, &h.out.b};
        *p[k] = nullptr;
        invalid_case(out_names[k], true, h, &h.d, &h.rays, &h.rng, 4, &h.out, false, INV);
    }
    invalid_case("n_2_31", true, g, &g.d, &g.rays, &g.rng, (size_t)INT32_MAX + 1, &g.out, false, INV);
    invalid_case("n_huge", true, g, &g.d, &g.rays, &g.rng, SIZE_MAX, &g.out, false, INV);
    {
        Args h;
        h.d.max_depth = 0;
        invalid_case("depth_0", true, h, &h.d, &h.rays, &h.rng, 4, &h.out, false, INV);
        h.d.max_depth = -3;
        invalid_case("depth_negative", true, h, &h.d, &h.rays, &h.rng, 4, &h.out, false, INV);
        Args h2;
        h2.d.reserved = 1;
        invalid_case("reserved", true, h2, &h2.d, &h2.rays, &h2.rng, 4, &h2.out, false, INV);
    }
    invalid_case("in_flight", true, g, &g.d, &g.rays, &g.rng, 4, &g.out, true, INV);
    invalid_case("in_flight_n0", true, g, &g.d, &g.rays, &g.rng, 0, &g.out, true, INV);
    {   // the order: a NULL context before anything is read, the render in flight last
        const char* why = nullptr;
        expect(check_args(false, nullptr, nullptr, nullptr, SIZE_MAX, nullptr, true, &why) == INV &&
                   !std::strcmp(why, "null context"), "null context first");
        Args h;
        h.d.reserved = 7;
        expect(check_args(true, &h.d, &h.rays, &h.rng, 4, &h.out, true, &why) == INV &&
                   !std::strcmp(why, "reserved must be 0"), "the desc before the render in flight");
    }

    // ---- PBRT_E_UNSUPPORTED
    auto unsupported_case = [&](const char* name, pbrt_li_desc d, bool rough, int want) {
        const char* why = nullptr;
        const int rc = check_supported(d, rough, &why);
        std::printf("case %s %d %s\n", name, rc, why ? why : "(null)");
        expect(rc == want, name);
        expect(why != nullptr && (rc == PBRT_OK) == (why[0] == 0), "a refusal names its reason");
    };
    pbrt_li_desc d = g.d;
    unsupported_case("supported", d, false, PBRT_OK);
    d.max_depth = 2048;
    unsupported_case("depth_2048", d, false, PBRT_OK);
    d.max_depth = 2049;
    unsupported_case("depth_2049", d, false, UNS);
    d = g.d;
    d.integrator = PBRT_INTEGRATOR_DIRECT_LIGHTING;
    unsupported_case("direct_lighting", d, false, UNS);
    d.integrator = 0;
    unsupported_case("integrator_0", d, false, UNS);
    d = g.d;
    d.light_strategy = PBRT_LIGHT_STRATEGY_POWER;
    unsupported_case("power_strategy", d, false, PBRT_OK);
    d.light_strategy = 3;
    unsupported_case("strategy_3", d, false, UNS);
    unsupported_case("rough_glass", g.d, true, UNS);

    auto dist_case = [&](const char* name, int n_lights, const double* func, int count, double func_int, int want) {
        const char* why = nullptr;
        const int rc = check_distribution(n_lights, func, count, func_int, &why);
        std::printf("case %s %d %s\n", name, rc, why ? why : "(null)");
        expect(rc == want, name);
        expect(why != nullptr && (rc == PBRT_OK) == (why[0] == 0), "a refusal names its reason");
    };
    const double uniform4[4] = {1, 1, 1, 1}, power8[8] = {0, 0, 0, 0, 0, 0, 0, 0}, one_zero[4] = {1, 0, 1, 1},
                 with_nan[4] = {1, 1, std::nan(""), 1}, negative[4] = {1, 1, -1, 1};
    dist_case("dist_uniform", 4, uniform4, 4, 1.0, PBRT_OK);
    dist_case("dist_power_all_zero", 4, power8, 8, 0.0, PBRT_OK);   // the reference's Power: 2n values of Y() == 0
    dist_case("dist_zero_integral_nonzero_entry", 4, one_zero, 4, 0.0, UNS);
    dist_case("dist_more_entries_than_lights", 2, uniform4, 4, 1.0, UNS);
    dist_case("dist_one_zero", 4, one_zero, 4, 0.75, UNS);
    dist_case("dist_nan", 4, with_nan, 4, 1.0, UNS);
    dist_case("dist_negative", 4, negative, 4, 0.5, UNS);
    dist_case("dist_nan_integral", 4, uniform4, 4, std::nan(""), UNS);
    dist_case("dist_no_lights", 0, power8, 0, 0.0, PBRT_OK);

    // ---- the kernel-argument table
    const int kLds = 64;
    for (int nm = 0; nm < 2; nm++)
        for (int mesh = 0; mesh < 2; mesh++)
            for (int nodes : {0, 1, 63, 64, 65, 121, 100000}) {
                const KernelArgs ka = kernel_args(nm != 0, nodes, mesh != 0, 1000, kLds);
                std::printf("kernel %d %d %d -> %d %d %u\n", nm, nodes, mesh, (int)ka.kx, ka.depth, ka.grid);
                expect(ka.kx == (nm != 0), "kX is the scene's non_matte");
                expect(ka.depth == (nodes > kLds ? 64 : 0), "kDepth 64 beyond the LDS-staged trees, else 0");
                expect(ka.grid == 4, "1000 rays: 4 waves of 256");
            }
    const size_t ns[] = {1, 255, 256, 257, 511, 512, 513, 1000, 2073600, (size_t)INT32_MAX};
    for (size_t n : ns) {
        const KernelArgs ka = kernel_args(false, 45, false, n, kLds);
        std::printf("grid %zu -> %u\n", n, ka.grid);
        expect((uint64_t)ka.grid * kLiRays >= n && ((uint64_t)ka.grid - 1) * kLiRays < n, "the grid covers n and no more");
    }
    expect(kLiRays == 256 && kLiMaxDepth == 2048, "the constants of the contract");
    std::printf("checks=%ld bad=%ld\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}

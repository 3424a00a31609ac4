// tests/path_query_check.cpp — host check of pbrt_gpu_path_begin_device's and
// pbrt_gpu_path_step_device's argument checks, queue rules and grids
// (go-pbrt_amd/csrc/path_query.h), with no device:
//   - every PBRT_E_INVALID case of include/pbrt_gpu.h, each alone on otherwise
//     valid arguments, and that the valid arguments pass (tmax NULL, queues
//     given or not); a NULL context first, a render in flight last;
//   - the queue rules: a queue that is given names both arrays; in and out
//     alias when they are one struct or share an index or a count array;
//   - the desc's refusals are the li query's (check_supported, as it is);
//   - the grids: begin_grid in blocks of kBeginBlock, step_args' instantiation
//     by pbrtli::kernel_args' rule and its grid in slices of kSlice, for n around
//     the multiples and at 2^31 - 1; the bytes per path.
// No pointer is dereferenced. Compiled with -fsanitize=address,undefined and run
// by tests/test_path_step_host.py. Prints one "case <name> <status> <reason>"
// line per case, one "kernel ..." line per row, and "checks=.. bad=..".
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <string_view>

#include "../go-pbrt_amd/csrc/path_query.h"

using namespace pbrtpath;

static long g_checks = 0, g_bad = 0;

static void expect(bool ok, const char* what) {
    g_checks++;
    if (!ok) {
        g_bad++;
        std::printf("FAILED %s\n", what);
    }
}

struct Args {
    double a[16];
    uint64_t s[2];
    uint32_t u[4];
    int32_t i[4];
    uint8_t b[1];
    pbrt_li_desc d;
    pbrt_ray_soa rays;
    pbrt_rng_soa rng;
    pbrt_path_soa p;
    pbrt_path_queue qa, qb;
    Args() {
        d = pbrt_li_desc{PBRT_INTEGRATOR_PATH, 5, PBRT_LIGHT_STRATEGY_UNIFORM, 0, 1.0};
        rays = pbrt_ray_soa{a, a + 1, a + 2, a + 3, a + 4, a + 5, nullptr};
        rng = pbrt_rng_soa{s, s + 1};
        p = pbrt_path_soa{a, a + 1, a + 2, a + 3, a + 4, a + 5, nullptr, a + 7, a + 8, a + 9, a + 10, a + 11, a + 12, a + 13,
                          s, s + 1, u, u + 1, i, b};
        qa = pbrt_path_queue{i + 1, u + 2};
        qb = pbrt_path_queue{i + 2, u + 3};
    }
};

static void report(const char* name, int rc, const char* why, int want) {
    std::printf("case %s %d %s\n", name, rc, why ? why : "(null)");
    expect(rc == want, name);
    expect(why != nullptr && (rc == PBRT_OK) == (why[0] == 0), "a refusal names its reason");
}
static void begin_case(const char* name, bool ctx_ok, const pbrt_ray_soa* rays, const pbrt_rng_soa* rng, size_t n,
                       const pbrt_path_soa* p, bool in_flight, int want) {
    const char* why = nullptr;
    const int rc = check_begin(ctx_ok, rays, rng, n, p, in_flight, &why);
    report(name, rc, why, want);
}
static void step_case(const char* name, bool ctx_ok, const pbrt_li_desc* d, const pbrt_path_soa* p,
                      const pbrt_path_queue* in, const pbrt_path_queue* out, size_t n, bool in_flight, int want) {
    const char* why = nullptr;
    const int rc = check_step(ctx_ok, d, p, in, out, n, in_flight, &why);
    report(name, rc, why, want);
}

int main() {
    Args g;
    const int INV = PBRT_E_INVALID, UNS = PBRT_E_UNSUPPORTED;
    const size_t NMAX = (size_t)INT32_MAX;

    // ---- begin
    begin_case("begin_valid", true, &g.rays, &g.rng, 4, &g.p, false, PBRT_OK);
    begin_case("begin_valid_n0", true, &g.rays, &g.rng, 0, &g.p, false, PBRT_OK);
    begin_case("begin_valid_nmax", true, &g.rays, &g.rng, NMAX, &g.p, false, PBRT_OK);
    {
        Args t;
        t.p.tmax = t.a + 6;
        t.rays.tmax = t.a + 6;
        begin_case("begin_with_tmax", true, &t.rays, &t.rng, 4, &t.p, false, PBRT_OK);
    }
    begin_case("begin_null_ctx", false, &g.rays, &g.rng, 4, &g.p, false, INV);
    begin_case("begin_null_rays", true, nullptr, &g.rng, 4, &g.p, false, INV);
    begin_case("begin_null_rng", true, &g.rays, nullptr, 4, &g.p, false, INV);
    begin_case("begin_null_paths", true, &g.rays, &g.rng, 4, nullptr, false, INV);
    begin_case("begin_n_2_31", true, &g.rays, &g.rng, NMAX + 1, &g.p, false, INV);
    begin_case("begin_in_flight", true, &g.rays, &g.rng, 4, &g.p, true, INV);
    begin_case("begin_in_flight_n0", true, &g.rays, &g.rng, 0, &g.p, true, INV);
    {
        const char* names[] = {"ox", "oy", "oz", "dx", "dy", "dz"};
        const double* pbrt_ray_soa::*const rm[] = {&pbrt_ray_soa::ox, &pbrt_ray_soa::oy, &pbrt_ray_soa::oz,
                                                   &pbrt_ray_soa::dx, &pbrt_ray_soa::dy, &pbrt_ray_soa::dz};
        for (int k = 0; k < 6; k++) {
            Args t;
            t.rays.*rm[k] = nullptr;
            char nm[32];
            std::snprintf(nm, sizeof nm, "begin_null_ray_%s", names[k]);
            begin_case(nm, true, &t.rays, &t.rng, 4, &t.p, false, INV);
        }
        Args t;
        t.rng.state = nullptr;
        begin_case("begin_null_rng_state", true, &t.rays, &t.rng, 4, &t.p, false, INV);
        Args v;
        v.rng.inc = nullptr;
        begin_case("begin_null_rng_inc", true, &v.rays, &v.rng, 4, &v.p, false, INV);
    }
    {   // the order: a NULL context before everything, a render in flight after everything
        const char* why = nullptr;
        check_begin(false, nullptr, nullptr, NMAX + 1, nullptr, true, &why);
        expect(why && std::string_view(why) == "null context", "begin: the context is checked first");
        check_begin(true, &g.rays, &g.rng, NMAX + 1, &g.p, true, &why);
        expect(why && std::string_view(why).find("2^31") != std::string_view::npos, "begin: in flight is checked last");
    }

    // ---- step
    step_case("step_valid", true, &g.d, &g.p, nullptr, nullptr, 4, false, PBRT_OK);
    step_case("step_valid_n0", true, &g.d, &g.p, nullptr, nullptr, 0, false, PBRT_OK);
    step_case("step_valid_nmax", true, &g.d, &g.p, nullptr, nullptr, NMAX, false, PBRT_OK);
    step_case("step_valid_in", true, &g.d, &g.p, &g.qa, nullptr, 4, false, PBRT_OK);
    step_case("step_valid_out", true, &g.d, &g.p, nullptr, &g.qa, 4, false, PBRT_OK);
    step_case("step_valid_in_out", true, &g.d, &g.p, &g.qa, &g.qb, 4, false, PBRT_OK);
    step_case("step_null_ctx", false, &g.d, &g.p, nullptr, nullptr, 4, false, INV);
    step_case("step_null_desc", true, nullptr, &g.p, nullptr, nullptr, 4, false, INV);
    step_case("step_null_paths", true, &g.d, nullptr, nullptr, nullptr, 4, false, INV);
    step_case("step_n_2_31", true, &g.d, &g.p, nullptr, nullptr, NMAX + 1, false, INV);
    step_case("step_in_flight", true, &g.d, &g.p, &g.qa, &g.qb, 4, true, INV);
    step_case("step_in_flight_n0", true, &g.d, &g.p, nullptr, nullptr, 0, true, INV);
    {
        Args t;
        t.d.max_depth = 0;
        step_case("step_depth_0", true, &t.d, &t.p, nullptr, nullptr, 4, false, INV);
        t.d.max_depth = -3;
        step_case("step_depth_negative", true, &t.d, &t.p, nullptr, nullptr, 4, false, INV);
        Args v;
        v.d.reserved = 1;
        step_case("step_reserved", true, &v.d, &v.p, nullptr, nullptr, 4, false, INV);
    }
    {   // every state pointer but tmax is required, by both calls
        const char* names[] = {"ox", "oy", "oz", "dx", "dy", "dz", "tmax", "lr", "lg", "lb", "br", "bg", "bb", "eta_scale"};
        double* pbrt_path_soa::*const pm[] = {&pbrt_path_soa::ox, &pbrt_path_soa::oy, &pbrt_path_soa::oz, &pbrt_path_soa::dx,
                                              &pbrt_path_soa::dy, &pbrt_path_soa::dz, &pbrt_path_soa::tmax, &pbrt_path_soa::lr,
                                              &pbrt_path_soa::lg, &pbrt_path_soa::lb, &pbrt_path_soa::br, &pbrt_path_soa::bg,
                                              &pbrt_path_soa::bb, &pbrt_path_soa::eta_scale};
        for (int k = 0; k < 14; k++) {
            if (k == 6) continue;
            Args t;
            t.p.*pm[k] = nullptr;
            char nm[40];
            std::snprintf(nm, sizeof nm, "step_null_state_%s", names[k]);
            step_case(nm, true, &t.d, &t.p, nullptr, nullptr, 4, false, INV);
            std::snprintf(nm, sizeof nm, "begin_null_state_%s", names[k]);
            begin_case(nm, true, &t.rays, &t.rng, 4, &t.p, false, INV);
        }
        for (int k = 0; k < 6; k++) {
            Args t;
            const char* nm_s[] = {"state", "inc", "draws", "rays", "bounces", "status"};
            switch (k) {
            case 0: t.p.state = nullptr; break;
            case 1: t.p.inc = nullptr; break;
            case 2: t.p.draws = nullptr; break;
            case 3: t.p.rays = nullptr; break;
            case 4: t.p.bounces = nullptr; break;
            default: t.p.status = nullptr; break;
            }
            char nm[40];
            std::snprintf(nm, sizeof nm, "step_null_state_%s", nm_s[k]);
            step_case(nm, true, &t.d, &t.p, nullptr, nullptr, 4, false, INV);
            std::snprintf(nm, sizeof nm, "begin_null_state_%s", nm_s[k]);
            begin_case(nm, true, &t.rays, &t.rng, 4, &t.p, false, INV);
        }
    }
    {   // the queue rules
        Args t;
        pbrt_path_queue no_index{nullptr, t.u + 2}, no_count{t.i + 1, nullptr};
        step_case("step_in_null_index", true, &t.d, &t.p, &no_index, nullptr, 4, false, INV);
        step_case("step_in_null_count", true, &t.d, &t.p, &no_count, nullptr, 4, false, INV);
        step_case("step_out_null_index", true, &t.d, &t.p, nullptr, &no_index, 4, false, INV);
        step_case("step_out_null_count", true, &t.d, &t.p, nullptr, &no_count, 4, false, INV);
        step_case("step_alias_same_struct", true, &t.d, &t.p, &t.qa, &t.qa, 4, false, INV);
        pbrt_path_queue copy = t.qa, same_index{t.qa.index, t.qb.count}, same_count{t.qb.index, t.qa.count};
        step_case("step_alias_copy", true, &t.d, &t.p, &t.qa, &copy, 4, false, INV);
        step_case("step_alias_index", true, &t.d, &t.p, &t.qa, &same_index, 4, false, INV);
        step_case("step_alias_count", true, &t.d, &t.p, &t.qa, &same_count, 4, false, INV);
        expect(!queues_alias(nullptr, &t.qa) && !queues_alias(&t.qa, nullptr) && !queues_alias(&t.qa, &t.qb), "no alias");
        expect(queue_complete(nullptr) && queue_complete(&t.qa) && !queue_complete(&no_index), "queue_complete");
    }
    {   // the order of step's checks
        const char* why = nullptr;
        check_step(false, nullptr, nullptr, nullptr, nullptr, NMAX + 1, true, &why);
        expect(why && std::string_view(why) == "null context", "step: the context is checked first");
        Args t;
        t.d.reserved = 2;
        check_step(true, &t.d, &t.p, nullptr, nullptr, 4, true, &why);
        expect(why && std::string_view(why).find("reserved") != std::string_view::npos, "step: in flight is checked last");
    }

    // ---- the desc's refusals are the li query's
    {
        const char* why = nullptr;
        pbrt_li_desc d = g.d;
        auto sup = [&](const char* name, const pbrt_li_desc& dd, bool rough, int want) {
            const int rc = pbrtli::check_supported(dd, rough, &why);
            report(name, rc, why, want);
        };
        sup("supported", d, false, PBRT_OK);
        sup("rough_glass", d, true, UNS);
        d.integrator = PBRT_INTEGRATOR_DIRECT_LIGHTING;
        sup("direct_lighting", d, false, UNS);
        d = g.d;
        d.max_depth = 2049;
        sup("depth_2049", d, false, UNS);
        d.max_depth = 2048;
        sup("depth_2048", d, false, PBRT_OK);
        d = g.d;
        d.light_strategy = 3;
        sup("strategy_3", d, false, UNS);
    }

    // ---- grids and the instantiation
    expect(kSlice >= pbrtli::kLiRays && kSlice % 64 == 0, "a slice amortises the staging over at least kLiRays entries");
    expect(kBytesPerPath == 6 * 8 + 8 + 3 * 8 + 3 * 8 + 8 + 8 + 8 + 4 + 4 + 4 + 1 && kBytesPerPath == 141 &&
               kBytesPerPathNoTmax == 133,
           "bytes per path");
    expect(begin_grid(0) == 0 && begin_grid(1) == 1 && begin_grid(256) == 1 && begin_grid(257) == 2 &&
               begin_grid(NMAX) == (uint32_t)((NMAX + 255) / 256),
           "begin_grid");
    for (int non_matte = 0; non_matte < 2; non_matte++)
        for (int mesh = 0; mesh < 2; mesh++)
            for (int nodes : {0, 1, 63, 64, 65, 121, 100000}) {
                const pbrtli::KernelArgs li = pbrtli::kernel_args(non_matte != 0, nodes, mesh != 0, 1000, 64);
                const pbrtli::KernelArgs a = step_args(non_matte != 0, nodes, mesh != 0, 1000, 64);
                std::printf("kernel non_matte=%d mesh=%d nodes=%d -> kx=%d depth=%d grid=%u\n", non_matte, mesh, nodes,
                            (int)a.kx, a.depth, a.grid);
                expect(a.kx == li.kx && a.depth == li.depth, "the instantiation is k_li's");
                expect(a.kx == (non_matte != 0) && a.depth == (nodes > 64 ? 64 : 0), "kx and depth");
                expect(a.grid == (1000 + kSlice - 1) / kSlice, "grid of 1000");
            }
    for (size_t n : {(size_t)1, (size_t)kSlice - 1, (size_t)kSlice, (size_t)kSlice + 1, (size_t)10 * kSlice, NMAX}) {
        const pbrtli::KernelArgs a = step_args(false, 10, false, n, 64);
        expect((uint64_t)a.grid * kSlice >= n && ((uint64_t)a.grid - 1) * kSlice < n, "the grid covers n and no slice more");
    }

    std::printf("checks=%ld bad=%ld\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}

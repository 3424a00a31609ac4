// k_li_direct.hip — batched DirectLighting.Li over ray and RNG arrays resident on
// the device (pbrt_gpu_direct_li_device): k_li_direct
#pragma clang fp contract(off)

#include "render_common.h"
#include "direct_li_query.h"

namespace pbrtk {

static_assert(pbrtdli::kMaxLevels == kDlMaxLevels, "the host's level bound is direct_li's");
static_assert(pbrtdli::kWaveLanes == kWave, "the level records are laid out per wave");

// k_li's wave structure around the loop of direct_li (pbrt_path.h, fidelity
// false): one wave per workgroup; a work list is the kLiRays rays from
// list * kLiRays on; an idle lane takes the next ray of the list by its rank in
// the idle ballot (so a refill's loads are contiguous) and starts
// DirectLighting.Li at depth 0 from the caller's ray and PCG32 stream.
// sampler.RandomSampler: no dimension is stratified (SpecSampler n_dims 0, Cursor
// k = -1), every value is a draw. The grid is capped by the host
// (pbrtdli::kernel_args): a workgroup strides over the work lists.
//
// One loop iteration is one level of every live lane: the closest hit, the BSDF,
// UniformSampleAllLights or UniformSampleOneLight without a distribution (with
// its > 10 panic), and where depth + 1 < max_depth the two Get2D of
// SpecularReflect / SpecularTransmit. A level that refracts through smooth glass
// (spec_trans_sample, local-frame wi, SURVEY #7) stores its record -- own
// radiance, f, |wi.ns| / pdf -- and spawns the ray of depth + 2 (#23); a lane
// whose ray ends folds its records innermost first, as the reference's returns
// do (L_k = own_k + (f_k * L_k+1) * w_k: never a running throughput), writes the
// value and becomes idle, so the refill stays useful where the levels per ray
// range from 1 to 33.
//
// The level records (kX only; without a SPEC_PAIR BSDF spec_trans_sample is black
// and no level is ever pushed, so kX = false carries none) live in global
// memory, `lev`, as [workgroup][level][field][lane]: a wave's store of one field
// of one level is 512 contiguous bytes, and a lane only ever reads what it
// wrote. They are indexed at run time, which as private arrays would be scratch.
// A lane's record count is its depth / 2; it is bounded by `nlev`, the levels
// the host sized the buffer for (pbrtdli::levels(max_depth) <= kDlMaxLevels).
// Every lane of a work list is idle before the next list starts, so successive
// lists of a workgroup reuse its records.
//
// A ray's values depend on its ray and stream only, never on its lane.
// kDepth as k_li's. A panicking ray is written as L = 0 (its optional outputs as
// they stand) and recorded as k_query_hit records its own. Li leaves a NaN
// radiance alone.
template <bool kX, int kDepth>
__global__ __launch_bounds__(kWave) void k_li_direct(DevScene sc, int max_depth, int strategy, int nlev, int64_t n,
                                                     pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_radiance_soa out,
                                                     QueryRec* __restrict__ rec, double* __restrict__ lev) {
    __shared__ uint16_t stack_lds[kDepth > 0 ? kDepth * kStackStride : 1];
    // (kDepth > 0: launched on trees beyond kLdsNodes only, which stage_nodes leaves alone)
    if (kDepth > 0) sc.use_lds_nodes = 0;
    else stage_nodes(sc);
    const int lane = threadIdx.x;
    uint16_t* const stack = kDepth > 0 ? stack_lds + lane : nullptr;
    const unsigned long long lt_mask = (1ULL << lane) - 1ULL;
    constexpr size_t kField = kWave, kLevel = pbrtdli::kRecDoubles * kWave;
    double* const my = kX ? lev + (size_t)blockIdx.x * (size_t)nlev * kLevel + lane : nullptr;
    const SpecSampler ss{nullptr, 1, 0, nullptr};
    const int nl = sc.n_lights;
    const int64_t nlists = (n + pbrtli::kLiRays - 1) / pbrtli::kLiRays;
    for (int64_t list = blockIdx.x; list < nlists; list += gridDim.x) {
        const int64_t i0 = list * pbrtli::kLiRays;
        const int T = (int)(n - i0 < (int64_t)pbrtli::kLiRays ? n - i0 : (int64_t)pbrtli::kLiRays);   // > 0
        int base = 0;
        int w = -1;
        Cursor c;
        c.rri = -1;
        c.rrn = 0;
        Ray ray;
        int levels = 0;        // records pushed: the level runs at depth 2 * levels
        uint64_t shadow = 0;   // visibility rays traced
        for (;;) {
            const bool idle = w < 0;
            const unsigned long long m = __ballot(idle);
            if (idle) {
                const int t = base + __popcll(m & lt_mask);
                if (t < T) {
                    const int64_t i = i0 + t;
                    w = t;
                    c.rng.state = rng.state[i];
                    c.rng.inc = rng.inc[i];
                    c.draws = 0;
                    c.cur1d = 0;
                    c.cur2d = 0;
                    c.k = -1;
                    c.kdep = 0;
                    ray = Ray{V3{rays.ox[i], rays.oy[i], rays.oz[i]}, V3{rays.dx[i], rays.dy[i], rays.dz[i]},
                              rays.tmax ? rays.tmax[i] : kInf, 0.0};
                    levels = 0;
                    shadow = 0;
                }
            }
            base += __popcll(m);
            if (!__any(w >= 0)) {
                if (base >= T) break;
                continue;
            }
            if (w >= 0) {
                // ---- one level of DirectLighting.Li (directlighting.go:62-104) at depth 2 * levels
                Spec L = spec(0);
                int panic = 0;
                bool ended = true;
                do {
                    SI si;
                    if (!bvh_traverse<false>(sc, ray, &si, stack, panic)) {
                        for (int i = 0; i < nl; i++) L = L + spec(0);
                        break;
                    }
                    if (panic) break;
                    BSDF b;
                    BSDFX x;   // Mirror: F and Pdf are 0 and SpecularReflect / Transmit match no lobe
                    if ((kX ? compute_bsdf_x(sc, si, b, x, false) : compute_bsdf(sc, si, b)) < 0) {
                        panic = -1;
                        break;
                    }
                    L = L + spec(0);   // si.Le(si.Wo): no primitive carries an area light
                    if (nl > 0) {
                        if (strategy == PBRT_DL_UNIFORM_SAMPLE_ALL) {   // integrator.go:23-46
                            Spec acc = spec(0);
                            for (int j = 0; j < nl && !panic; j++) {
                                const V2 ul = c_get2d(c, ss);
                                c_get2d(c, ss);   // uScattering: only the MIS half reads it
                                if constexpr (kX)
                                    acc = acc + estimate_direct_x(sc, stack, panic, si, b, x, j, ul, &shadow);
                                else
                                    acc = acc + estimate_direct(sc, stack, panic, si, b, j, ul, &shadow);
                            }
                            if (panic) break;
                            L = L + acc;
                        } else {   // UniformSampleOneLight with no distribution (integrator.go:48-77)
                            const int ln =
                                (int)gomath::to_int(gomath::min(c_get1d(c, ss) * (double)nl, (double)(nl - 1)));
                            const V2 ul = c_get2d(c, ss);
                            c_get2d(c, ss);
                            Spec s1;
                            if constexpr (kX) s1 = estimate_direct_x(sc, stack, panic, si, b, x, ln, ul, &shadow);
                            else s1 = estimate_direct(sc, stack, panic, si, b, ln, ul, &shadow);
                            if (!panic && max_component(s1) > 10) panic = PBRT_PANIC_LD_GT_10;
                            if (panic) break;
                            L = L + s1;
                        }
                    }
                    if (!(2 * levels + 1 < max_depth)) break;
                    c_get2d(c, ss);   // SpecularReflect (integrator.go:352-355): black
                    L = L + spec(0);
                    const V2 u = c_get2d(c, ss);   // SpecularTransmit (integrator.go:383-385)
                    if constexpr (kX) {
                        V3 wi;
                        double pdf;
                        const Spec f = spec_trans_sample(b, x, si.wo, u, wi, pdf);
                        const double adn = absdot(wi, si.sn);
                        if (!(pdf > 0 && !is_black(f) && adn != 0.0) || levels == kDlMaxLevels || levels >= nlev) {
                            L = L + spec(0);
                            break;
                        }
                        double* const r = my + (size_t)levels * kLevel;
                        r[0 * kField] = L.r;
                        r[1 * kField] = L.g;
                        r[2 * kField] = L.b;
                        r[3 * kField] = f.r;
                        r[4 * kField] = f.g;
                        r[5 * kField] = f.b;
                        r[6 * kField] = adn / pdf;
                        levels++;
                        // SpawnRay (interaction.go:68-77) with the local-frame wi
                        ray.o = offset_ray_origin(si.p, si.perr, si.n, wi);
                        ray.d = wi;
                        ray.tmax = kInf;
                        ray.time = si.time;
                        ended = false;
                    } else {
                        (void)u;   // a Lambertian-only BSDF has no SpecularTransmission
                        L = L + spec(0);
                    }
                } while (false);
                if (ended) {
                    const int64_t i = i0 + w;
                    const uint32_t closest = (uint32_t)levels + 1u;   // one closest-hit query per level
                    if (panic) {
                        L = spec(0);
                    } else if constexpr (kX) {
                        for (int q = levels - 1; q >= 0; q--) {
                            const double* const r = my + (size_t)q * kLevel;
                            const Spec own{r[0 * kField], r[1 * kField], r[2 * kField]};
                            const Spec f{r[3 * kField], r[4 * kField], r[5 * kField]};
                            L = own + smuls(smul(f, L), r[6 * kField]);
                        }
                    }
                    out.r[i] = L.r;
                    out.g[i] = L.g;
                    out.b[i] = L.b;
                    if (out.state) out.state[i] = c.rng.state;
                    if (out.draws) out.draws[i] = c.draws;
                    if (out.rays) out.rays[i] = closest * kRayClosest + (uint32_t)shadow * kRayShadow;
                    if (panic) query_panic(rec, i, panic);
                    w = -1;
                }
            }
        }
    }
}

template __global__ void k_li_direct<false, 0>(DevScene sc, int max_depth, int strategy, int nlev, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_radiance_soa out, QueryRec* __restrict__ rec, double* __restrict__ lev);
template __global__ void k_li_direct<true, 0>(DevScene sc, int max_depth, int strategy, int nlev, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_radiance_soa out, QueryRec* __restrict__ rec, double* __restrict__ lev);
template __global__ void k_li_direct<false, 64>(DevScene sc, int max_depth, int strategy, int nlev, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_radiance_soa out, QueryRec* __restrict__ rec, double* __restrict__ lev);
template __global__ void k_li_direct<true, 64>(DevScene sc, int max_depth, int strategy, int nlev, int64_t n, pbrt_ray_soa rays, pbrt_rng_soa rng, pbrt_radiance_soa out, QueryRec* __restrict__ rec, double* __restrict__ lev);

}  // namespace pbrtk

// pcg_jump.h — PCG32 jump-ahead: the tables and the helpers that position a
// state at an offset of its stream. Plain C++: host and device, no other header
// of the project, so the arithmetic is also checked as a stand-alone host
// program (tests/pcg_steps_check.cpp).
//
// One LCG step is s' = M * s + inc, so n steps are the affine map
// s -> a_n * s + inc * b_n (mod 2^64) with a_n = M^n and b_n = 1 + M + ... +
// M^(n-1); the map of m steps followed by k steps is (a_k a_m, a_k b_m + b_k).
// Everything is integer arithmetic mod 2^64: whichever maps a state is
// advanced through, it is the state n literal steps would have produced.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define PBRT_PCG_HD __host__ __device__ __forceinline__
#else
#define PBRT_PCG_HD inline
#endif

namespace pbrt {

constexpr uint64_t kPcgMult = 0x5851f42d4c957f2dULL;   // rng.go:36-42
constexpr int kPcgNear = 128;   // step[]: offsets 0 .. kPcgNear - 1 in one map
constexpr int kPcgMid = 8;      // mid[]: multiples of kPcgNear below kPcgNear * kPcgMid

struct PcgStep {   // the map of a fixed number of steps: s -> a * s + inc * b
    uint64_t a, b;
};
struct PcgJump {
    // state after 2^i steps = a[i] * state + inc * b[i]
    uint64_t a[64];
    uint64_t b[64];
    // step[k]: k steps; mid[j]: kPcgNear * j steps (16-byte pairs: one load each)
    alignas(16) PcgStep step[kPcgNear];
    PcgStep mid[kPcgMid];
};

PBRT_PCG_HD void pcg_jump_fill(PcgJump& t) {
    uint64_t a = kPcgMult, b = 1;   // one step: s' = a*s + inc*1
    for (int i = 0; i < 64; i++) {
        t.a[i] = a;
        t.b[i] = b;
        b = b * (a + 1);   // two applications of the 2^i jump
        a = a * a;
    }
    PcgStep m{1, 0};   // no step
    for (int k = 0; k < kPcgNear * kPcgMid; k++) {
        if (k < kPcgNear) t.step[k] = m;
        if (k % kPcgNear == 0) t.mid[k / kPcgNear] = m;
        m.a = m.a * kPcgMult;       // one more step after the k so far
        m.b = m.b * kPcgMult + 1;
    }
}

// the generic jump: one map per set bit of n
PBRT_PCG_HD uint64_t pcg_advance(const PcgJump& J, uint64_t s, uint64_t inc, uint64_t n) {
    for (int i = 0; n; ++i, n >>= 1)
        if (n & 1) s = J.a[i] * s + inc * J.b[i];
    return s;
}
// k < kPcgNear steps: one 16-byte load, one map
PBRT_PCG_HD uint64_t pcg_step(const PcgJump& J, uint64_t s, uint64_t inc, uint32_t k) {
    const PcgStep m = J.step[k];
    return m.a * s + inc * m.b;
}
// n steps where n is usually small: one map below kPcgNear, two below
// kPcgNear * kPcgMid (a multi-wave tile's idle lanes reach 2 * 511), else the
// generic jump
PBRT_PCG_HD uint64_t pcg_advance_near(const PcgJump& J, uint64_t s, uint64_t inc, uint64_t n) {
    if (n < (uint64_t)kPcgNear) return pcg_step(J, s, inc, (uint32_t)n);
    if (n < (uint64_t)(kPcgNear * kPcgMid)) {
        const PcgStep m = J.mid[n / kPcgNear];
        return pcg_step(J, m.a * s + inc * m.b, inc, (uint32_t)(n % kPcgNear));
    }
    return pcg_advance(J, s, inc, n);
}

// k <= kPcgSkipMax steps with compile-time maps (a trajectory's unused draws)
constexpr int kPcgSkipMax = 5;
constexpr PcgStep pcg_const_map(int k) {
    PcgStep m{1, 0};
    for (int i = 0; i < k; i++) {
        m.a = m.a * kPcgMult;
        m.b = m.b * kPcgMult + 1;
    }
    return m;
}
PBRT_PCG_HD uint64_t pcg_skip(uint64_t s, uint64_t inc, int k) {
    constexpr PcgStep m1 = pcg_const_map(1), m2 = pcg_const_map(2), m3 = pcg_const_map(3), m4 = pcg_const_map(4),
                      m5 = pcg_const_map(5);
    switch (k) {
    case 0: return s;
    case 1: return m1.a * s + inc * m1.b;
    case 2: return m2.a * s + inc * m2.b;
    case 3: return m3.a * s + inc * m3.b;
    case 4: return m4.a * s + inc * m4.b;
    default: return m5.a * s + inc * m5.b;
    }
}

}  // namespace pbrt

// pcg_steps_check.cpp — go-pbrt_amd/csrc/pcg_jump.h as a stand-alone host
// program (tests/test_pcg_steps_host.py builds it with ASan + UBSan). It checks
//   1. the step and mid tables against literal LCG steps,
//   2. pcg_advance_near against pcg_advance (and both against literal steps),
//   3. the state k_chain_ci carries at `nxt` through issues and resets, and the
//      lanes' table steps from it, against pcg_advance from the origin,
//   4. pcg_skip against k literal steps, k = 0..5.
// Prints one "ok <name> <checks>" line per part; any mismatch prints FAIL and exits 1.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../go-pbrt_amd/csrc/pcg_jump.h"

using namespace pbrt;

static uint64_t rnd_state = 0x9e3779b97f4a7c15ULL;
static uint64_t rnd() {   // splitmix64
    uint64_t z = (rnd_state += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
static uint64_t literal(uint64_t s, uint64_t inc, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) s = s * kPcgMult + inc;
    return s;
}
static void fail(const char* what, uint64_t a, uint64_t b) {
    std::printf("FAIL %s %llu %llu\n", what, (unsigned long long)a, (unsigned long long)b);
    std::exit(1);
}

int main() {
    static_assert(sizeof(PcgStep) == 16, "one 16-byte load per map");
    static_assert(offsetof(PcgJump, step) % 16 == 0 && offsetof(PcgJump, mid) % 16 == 0, "aligned pairs");
    auto Jp = std::make_unique<PcgJump>();   // on the heap: ASan sees an index past a table
    pcg_jump_fill(*Jp);
    const PcgJump& J = *Jp;
    long checks = 0;

    // 1. step[k], mid[j] == k, 128 j literal steps
    for (int i = 0; i < 300; i++) {
        const uint64_t s0 = rnd(), inc = rnd() | 1;
        uint64_t s = s0;
        for (int k = 0; k < kPcgNear * kPcgMid; k++) {
            if (k < kPcgNear && pcg_step(J, s0, inc, (uint32_t)k) != s) fail("step", (uint64_t)i, (uint64_t)k);
            if (k % kPcgNear == 0) {
                const PcgStep m = J.mid[k / kPcgNear];
                if (m.a * s0 + inc * m.b != s) fail("mid", (uint64_t)i, (uint64_t)k);
            }
            s = s * kPcgMult + inc;
            checks++;
        }
    }
    std::printf("ok tables %ld\n", checks);

    // 2. pcg_advance_near == pcg_advance == literal steps
    checks = 0;
    for (int i = 0; i < 64; i++) {
        const uint64_t s0 = rnd(), inc = rnd() | 1;
        uint64_t ns[] = {0, 1, 126, 127, 128, 129, 255, 1023, 1024, 1025, (1ull << 20) + 3, rnd() % 5000, rnd() % 200000};
        for (uint64_t n : ns) {
            if (i >= 4 && n > 100000) continue;   // (the long literal loops a few times only)
            const uint64_t want = literal(s0, inc, n);
            if (pcg_advance(J, s0, inc, n) != want) fail("advance", (uint64_t)i, n);
            if (pcg_advance_near(J, s0, inc, n) != want) fail("advance_near", (uint64_t)i, n);
            checks++;
        }
        // far jumps: no literal loop, the two helpers against each other
        const uint64_t far = rnd();
        if (pcg_advance_near(J, s0, inc, far) != pcg_advance(J, s0, inc, far)) fail("advance_near far", (uint64_t)i, far);
        checks++;
    }
    std::printf("ok advance_near %ld\n", checks);

    // 3. the carried state. Offsets count from the origin state s0; the model
    // keeps what the kernel keeps: head, nxt and Sn (the state at nxt).
    checks = 0;
    long resets_far = 0, resets_near = 0, issues_far = 0;
    for (int run = 0; run < 8; run++) {
        const uint64_t s0 = rnd(), inc = rnd() | 1;
        const uint32_t cs = (run & 1) ? 2u : 1u;
        uint64_t head = 0, nxt = 0, Sn = s0;
        for (int op = 0; op < 4000; op++) {
            if (rnd() % 3) {   // issue: `waves` waves of 64 lanes, m candidates in rank order
                const int waves = 1 << (rnd() % 4);
                const uint32_t m = (uint32_t)(rnd() % (uint64_t)(64 * waves + 1));
                for (int w = 0; w < waves; w++) {   // a wave's base, its lanes one table step from it
                    const uint32_t r0 = (uint32_t)(rnd() % (uint64_t)(m + 1));
                    const uint64_t wS = pcg_advance_near(J, Sn, inc, (uint64_t)cs * r0);
                    const uint32_t r = (uint32_t)(rnd() % 64);
                    const uint64_t st = pcg_step(J, wS, inc, cs * r);
                    if (st != pcg_advance(J, s0, inc, nxt + (uint64_t)cs * (r0 + r))) fail("lane", (uint64_t)op, r);
                    checks++;
                }
                if ((uint64_t)cs * m >= (uint64_t)kPcgNear * kPcgMid) issues_far++;
                Sn = pcg_advance_near(J, Sn, inc, (uint64_t)cs * m);
                nxt += (uint64_t)cs * m;
            } else {   // the walk passes an entry at eo in [head, nxt] with draw count d
                const uint64_t eo = head + (nxt > head ? rnd() % (nxt - head + 1) : 0);
                const uint64_t est = pcg_advance(J, s0, inc, eo);   // what its issue wrote
                const uint32_t d = (rnd() % 8 == 0) ? (uint32_t)(128 + rnd() % 1200) : (uint32_t)(rnd() % 128);
                head = eo + d;
                if (nxt < head || (cs == 2u && ((nxt ^ head) & 1u))) {
                    nxt = head;
                    Sn = pcg_advance_near(J, est, inc, (uint64_t)d);
                    (d >= (uint32_t)kPcgNear ? resets_far : resets_near)++;
                }
            }
            if (Sn != pcg_advance(J, s0, inc, nxt)) fail("carried", (uint64_t)run, (uint64_t)op);
            checks++;
        }
    }
    if (resets_far < 50 || resets_near < 50 || issues_far < 1) fail("coverage", (uint64_t)resets_far, (uint64_t)resets_near);
    std::printf("ok carried %ld resets_near %ld resets_far %ld issues_far %ld\n", checks, resets_near, resets_far, issues_far);

    // 4. the constant maps of a trajectory's unused draws
    checks = 0;
    for (int i = 0; i < 300; i++) {
        const uint64_t s0 = rnd(), inc = rnd() | 1;
        for (int k = 0; k <= kPcgSkipMax; k++) {
            if (pcg_skip(s0, inc, k) != literal(s0, inc, (uint64_t)k)) fail("skip", (uint64_t)i, (uint64_t)k);
            checks++;
        }
    }
    std::printf("ok skip %ld\n", checks);
    return 0;
}

// wave_cam_check.cpp — go-pbrt_amd/csrc/cam_sample.h as a stand-alone host
// program (tests/test_wave_cam_host.py builds it with ASan + UBSan): for each
// seed and n_dims it prints the CameraSample drawn at the start of the stream
// Sampler.Clone(seed) opens (rng.go:28-34), doubles as their bit patterns:
//   seed n_dims draws time_drawn film_x film_y lens_x lens_y time_u next
// where `next` is the stream's next raw draw after the camera sample.
#include <cstdio>
#include <cstring>

#include "../go-pbrt_amd/csrc/cam_sample.h"

static unsigned long long bits(double v) {
    unsigned long long u;
    static_assert(sizeof(u) == sizeof(v), "fp64");
    std::memcpy(&u, &v, sizeof(u));
    return u;
}

int main() {
    const uint64_t seeds[] = {0, 1, 7};
    for (uint64_t seed : seeds) {
        for (int nd = 0; nd <= 3; nd++) {
            // NewRNGWithSeed / SetSequence (rng.go:28-34)
            const uint64_t inc = (seed << 1) | 1;
            uint64_t state = 0;
            pbrtcam::pcg32_next(state, inc);
            state += 0x853c49e6748fea9bULL;
            pbrtcam::pcg32_next(state, inc);
            const pbrtcam::CamSample s = pbrtcam::cam_sample(state, inc, nd);
            if (s.draws != pbrtcam::cam_draws(nd)) return 1;
            const uint32_t next = pbrtcam::pcg32_next(state, inc);
            std::printf("%llu %d %u %d %llx %llx %llx %llx %llx %u\n", (unsigned long long)seed, nd, s.draws, s.time_drawn,
                        bits(s.film_x), bits(s.film_y), bits(s.lens_x), bits(s.lens_y), bits(s.time_u), next);
        }
    }
    return 0;
}

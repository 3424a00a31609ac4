// cam_sample.h — a sample's CameraSample where the camera ray belongs to the
// sample, not to the pixel (the camera-start wave route, k_chain_cam /
// k_paths_cam / k_film_cam). Plain C++: host and device, no other header of the
// project, so the mapping is also checked as a stand-alone host program
// (tests/wave_cam_check.cpp).
//
// GetCameraSample (pkg/sampler/sampler.go:75-80) asks for pFilm = pixel +
// Get2D, pLens = Get2D, time = Get1D, in that order. A request below
// nSampledDimensions is stratified (pixel.go:60-80: a 2D value is (0,0),
// ledger #3; a 1D value is the pixel's shuffled s1d[dim][k]); one beyond it is
// drawn from the tile's PCG32 stream:
//
//   n_dims   pFilm offset        pLens          time             draws
//   0        draws 0, 1          draws 2, 3     draw 4           5
//   1        (0,0)               draws 0, 1     s1d[0][k]        2
//   >= 2     (0,0)               (0,0)          s1d[0][k]        0
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define PBRT_CAM_HD __host__ __device__ __forceinline__
#else
#define PBRT_CAM_HD inline
#endif

namespace pbrtcam {

struct CamSample {
    double film_x, film_y;   // pFilm - pixel
    double lens_x, lens_y;   // pLens
    double time_u;           // the time value when it is a draw (time_drawn), else 0: the caller's s1d[0][k]
    uint32_t draws;          // PCG32 draws consumed
    int time_drawn;
};

// PCG32 (pkg/pbrt/rng.go:36-42; the (rot + 1) & 31 rotation is ledger #1)
PBRT_CAM_HD uint32_t pcg32_next(uint64_t& state, uint64_t inc) {
    const uint64_t old = state;
    state = old * 0x5851f42d4c957f2dULL + inc;
    const uint32_t xs = (uint32_t)(((old >> 18) ^ old) >> 27);
    const uint32_t rot = (uint32_t)(old >> 59);
    return (xs >> rot) | (xs << ((rot + 1u) & 31u));
}
// rng.go:55-57 UniformFloat64
PBRT_CAM_HD double pcg32_float(uint64_t& state, uint64_t inc) {
    const double v = (double)pcg32_next(state, inc) * 2.3283064365386963e-10;
    const double one_minus_eps = 0x1.fffffffffffffp-1;
    return v < one_minus_eps ? v : one_minus_eps;
}

// PCG32 draws of a CameraSample
PBRT_CAM_HD uint32_t cam_draws(int n_dims) { return n_dims <= 0 ? 5u : n_dims == 1 ? 2u : 0u; }

// The CameraSample drawn at `state` (advanced past its draws) of the stream `inc`
PBRT_CAM_HD CamSample cam_sample(uint64_t& state, uint64_t inc, int n_dims) {
    CamSample s{0.0, 0.0, 0.0, 0.0, 0.0, 0u, 0};
    if (n_dims <= 0) {
        s.film_x = pcg32_float(state, inc);
        s.film_y = pcg32_float(state, inc);
    }
    if (n_dims <= 1) {
        s.lens_x = pcg32_float(state, inc);
        s.lens_y = pcg32_float(state, inc);
    }
    if (n_dims <= 0) {
        s.time_u = pcg32_float(state, inc);
        s.time_drawn = 1;
    }
    s.draws = cam_draws(n_dims);
    return s;
}

}  // namespace pbrtcam

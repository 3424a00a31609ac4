// tests/li_mb_check.cpp — mb_state (go-pbrt_amd/csrc/pbrt_path.h) printed from the header
// itself, for tests/test_li_host.py: a host-only compile of the device header
// (hipcc --cuda-host-only; mb_mix and mb_state are __host__ __device__).
// One "tile pi s state" line per triple.
#include <cstdio>

#include "../go-pbrt_amd/csrc/pbrt_path.h"

int main() {
    const unsigned long long v[] = {0, 1, 2, 5, 255, 256, 8159, 1ull << 32, ~0ull};
    for (unsigned long long t : v)
        for (unsigned long long p : v)
            for (unsigned long long s : v)
                std::printf("%llu %llu %llu %llu\n", t, p, s, (unsigned long long)pbrt::mb_state(t, p, s));
    return 0;
}

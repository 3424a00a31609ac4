// tests/gomath_once_check.cpp — the one-evaluation forms of Go's trig routines
// (go-pbrt_amd/csrc/gomath.h: sincos, satan with one xatan, asin with one division
// and one satan, atan with one satan) and concentric_sample_disk with one division
// and one sincos (go-pbrt_amd/csrc/pbrt_path.h) against the branch-per-range forms
// they replace, carried here verbatim (namespace was). A stand-alone program for
// tests/test_gomath_once.py: a host-only compile of the device header (hipcc
// --cuda-host-only) under ASan + UBSan. Every comparison is on the IEEE bits, NaN
// as a class. One "ok <name> <comparisons>" line per group; the first mismatches
// are printed and the exit status is 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../go-pbrt_amd/csrc/pbrt_path.h"

// ------------------------------------------------------------------ reference
// The routines as they were before the one-evaluation forms (src/math/sin.go,
// atan.go, asin.go, atan2.go as a scalar CPU runs them: one branch per range).
namespace was {
using gomath::kPi;
using gomath::is_nan;
using gomath::is_inf;
using gomath::nan;
using gomath::abs;
using gomath::copysign;
using gomath::signbit;
using gomath::kInf;

constexpr double PI4A = 7.85398125648498535156e-1;
constexpr double PI4B = 3.77489470793079817668e-8;
constexpr double PI4C = 2.69515142907905952645e-15;
constexpr double FOUR_OVER_PI = 1.27323954473516268615;

inline double sin_poly(double z, double zz) {
    return z + z * zz * ((((((1.58962301576546568060e-10 * zz) + -2.50507477628578072866e-8) * zz +
                            2.75573136213857245213e-6) * zz + -1.98412698295895385996e-4) * zz +
                          8.33333333332211858878e-3) * zz + -1.66666666666666307295e-1);
}
inline double cos_poly(double zz) {
    return 1.0 - 0.5 * zz +
           zz * zz * ((((((-1.13585365213876817300e-11 * zz) + 2.08757008419747316778e-9) * zz +
                         -2.75573141792967388112e-7) * zz + 2.48015872888517045348e-5) * zz +
                       -1.38888888888730564116e-3) * zz + 4.16666666666665929218e-2);
}
inline double reduce(double x, uint64_t& j) {
    j = (uint64_t)(x * FOUR_OVER_PI);
    double y = (double)j;
    if (j & 1) { j++; y++; }
    j &= 7;
    return ((x - y * PI4A) - y * PI4B) - y * PI4C;
}
inline double cos(double x) {
    if (is_nan(x) || is_inf(x)) return nan();
    bool sign = false;
    x = abs(x);
    uint64_t j;
    double z = reduce(x, j);
    if (j > 3) { j -= 4; sign = !sign; }
    if (j > 1) sign = !sign;
    double zz = z * z;
    double y = (j == 1 || j == 2) ? sin_poly(z, zz) : cos_poly(zz);
    return sign ? -y : y;
}
inline double sin(double x) {
    if (x == 0 || is_nan(x)) return x;
    if (is_inf(x)) return nan();
    bool sign = false;
    if (x < 0) { x = -x; sign = true; }
    uint64_t j;
    double z = reduce(x, j);
    if (j > 3) { sign = !sign; j -= 4; }
    double zz = z * z;
    double y = (j == 1 || j == 2) ? cos_poly(zz) : sin_poly(z, zz);
    return sign ? -y : y;
}
inline double xatan(double x) {
    double z = x * x;
    z = z * ((((-8.750608600031904122785e-01 * z + -1.615753718733365076637e+01) * z +
               -7.500855792314704667340e+01) * z + -1.228866684490136173410e+02) * z +
             -6.485021904942025371773e+01) /
        (((((z + 2.485846490142306297962e+01) * z + 1.650270098316988542046e+02) * z +
           4.328810604912902668951e+02) * z + 4.853903996359136964868e+02) * z +
         1.945506571482613964425e+02);
    return x * z + x;
}
inline double satan(double x) {
    constexpr double Morebits = 6.123233995736765886130e-17;
    if (x <= 0.66) return xatan(x);
    if (x > 2.41421356237309504880) return kPi / 2 - xatan(1 / x) + Morebits;
    return kPi / 4 + xatan((x - 1) / (x + 1)) + 0.5 * Morebits;
}
inline double atan(double x) {
    if (x == 0) return x;
    return x > 0 ? satan(x) : -satan(-x);
}
inline double atan2(double y, double x) {
    if (is_nan(y) || is_nan(x)) return nan();
    if (y == 0) return (x >= 0 && !signbit(x)) ? copysign(0, y) : copysign(kPi, y);
    if (x == 0) return copysign(kPi / 2, y);
    if (is_inf(x)) {
        if (x == kInf) return is_inf(y) ? copysign(kPi / 4, y) : copysign(0, y);
        return is_inf(y) ? copysign(2.35619449019234492884698253745962716, y) : copysign(kPi, y);
    }
    if (is_inf(y)) return copysign(kPi / 2, y);
    double q = atan(y / x);
    if (x < 0) return q <= 0 ? q + kPi : q - kPi;
    return q;
}
inline double asin(double x) {
    if (x == 0) return x;
    bool sign = false;
    if (x < 0) { x = -x; sign = true; }
    if (x > 1) return nan();
    double t = __builtin_sqrt(1 - x * x);
    t = (x > 0.7) ? kPi / 2 - satan(t / x) : satan(x / t);
    return sign ? -t : t;
}
inline double acos(double x) { return kPi / 2 - asin(x); }

// sampling.go:173-198 as pbrt_path.h had it
inline pbrt::V2 concentric_sample_disk(pbrt::V2 u) {
    pbrt::V2 uo{u.x * 2.0 - 1, u.y * 2.0 - 1};
    if (uo.x == 0 && uo.y == 0) return pbrt::V2{0, 0};
    double theta, r;
    if (gomath::abs(uo.x) > gomath::abs(uo.y)) {
        r = uo.x;
        theta = (gomath::kPi / 4.0) * (uo.y / uo.x);
    } else {
        r = uo.y;
        theta = (gomath::kPi / 2.0) - (gomath::kPi / 4.0) * (uo.x / uo.y);
    }
    return pbrt::V2{was::cos(theta) * r, was::sin(theta) * r};
}
}  // namespace was

// ------------------------------------------------------------------- harness
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() {   // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double rnd01() { return (double)(rnd64() >> 11) * (1.0 / 9007199254740992.0); }
static double rnd_sym(double a) { return (2 * rnd01() - 1) * a; }
static double from_u(uint64_t u) { double d; std::memcpy(&d, &u, 8); return d; }
static uint64_t to_u(double d) { uint64_t u; std::memcpy(&u, &d, 8); return u; }
// ±2^e with e uniform in [lo, hi) and a random mantissa
static double rnd_log(int lo, int hi) {
    const int e = lo + (int)(rnd64() % (uint64_t)(hi - lo));
    const double m = 1 + rnd01();
    const double v = __builtin_ldexp(m, e);
    return (rnd64() & 1) ? -v : v;
}

static long g_bad = 0;
static bool same(double a, double b) { return (a != a && b != b) || to_u(a) == to_u(b); }
static void expect(const char* what, double x, double y, double got, double want) {
    if (same(got, want)) return;
    if (g_bad++ < 20)
        std::printf("MISMATCH %s(%.17g [%016llx], %.17g): got %016llx want %016llx\n", what, x,
                    (unsigned long long)to_u(x), y, (unsigned long long)to_u(got), (unsigned long long)to_u(want));
}

static void around(std::vector<double>& v, double c, int ulps) {
    for (int s = -1; s <= 1; s += 2) {
        const uint64_t u = to_u(s * c);
        for (int k = -ulps; k <= ulps; k++) v.push_back(from_u(u + (uint64_t)(int64_t)k));
    }
}

static std::vector<double> special_values() {
    std::vector<double> v = {0.0, -0.0, 1.0, -1.0, gomath::nan(), from_u(0xFFF8000000000001ull), gomath::kInf,
                             -gomath::kInf};
    for (double one : {1.0, -1.0}) {
        v.push_back(from_u(to_u(one) + 1));   // the next doubles beyond and inside ±1
        v.push_back(from_u(to_u(one) - 1));
    }
    for (uint64_t sign : {0ull, 1ull << 63}) {
        v.push_back(from_u(sign | 1));                        // the smallest denormal
        v.push_back(from_u(sign | 0x000FFFFFFFFFFFFFull));    // the largest denormal
        v.push_back(from_u(sign | 0x0010000000000000ull));    // the smallest normal
        v.push_back(from_u(sign | 0x7FEFFFFFFFFFFFFFull));    // the largest finite
    }
    // the range thresholds of satan and asin ...
    for (double t : {0.66, 0.7, 2.41421356237309504880}) around(v, t, 8);
    // ... and the arguments of asin whose ratio x / t (below 0.7) or t / x (above) meets satan's 0.66
    const double h = __builtin_sqrt(1 + 0.66 * 0.66);
    for (double t : {0.66 / h, 1 / h}) around(v, t, 64);
    return v;
}

template <class F, class R>
static long run1(const char* name, F f, R ref, const std::vector<double>& xs) {
    for (double x : xs) expect(name, x, 0, f(x), ref(x));
    return (long)xs.size();
}

static void sincos_check(double x, long& n) {
    double s, c;
    gomath::sincos(x, s, c);
    expect("sincos.sin", x, 0, s, was::sin(x));
    expect("sincos.cos", x, 0, c, was::cos(x));
    expect("sin", x, 0, gomath::sin(x), was::sin(x));   // sin and cos themselves stay as they were
    expect("cos", x, 0, gomath::cos(x), was::cos(x));
    n += 4;
}

int main(int argc, char** argv) {
    // the random counts of the full run; a smaller first argument divides them (for a quick look)
    const long scale = argc > 1 ? std::atol(argv[1]) : 1;
    const long n_rand = 10000000 / scale, n_bits = 1000000 / scale;
    const std::vector<double> sp = special_values();

    {   // asin, acos: [-1, 1], and everything else is NaN
        long n = 0;
        n += run1("asin", gomath::asin, was::asin, sp);
        n += run1("acos", gomath::acos, was::acos, sp);
        for (long i = 0; i < n_rand; i++) {
            const double x = (i & 3) == 3 ? rnd_log(-1074, 1) : rnd_sym(1.0);
            expect("asin", x, 0, gomath::asin(x), was::asin(x));
            expect("acos", x, 0, gomath::acos(x), was::acos(x));
        }
        for (long i = 0; i < n_bits; i++) {
            const double x = from_u(rnd64());
            expect("asin", x, 0, gomath::asin(x), was::asin(x));
            expect("acos", x, 0, gomath::acos(x), was::acos(x));
        }
        n += 2 * (n_rand + n_bits);
        if (!g_bad) std::printf("ok asin_acos %ld\n", n);
    }
    {   // atan: the whole line
        long n = run1("atan", gomath::atan, was::atan, sp);
        for (long i = 0; i < n_rand; i++) {
            const double x = (i & 1) ? rnd_log(-1074, 1024) : rnd_sym(4.0);
            expect("atan", x, 0, gomath::atan(x), was::atan(x));
        }
        for (long i = 0; i < n_bits; i++) {
            const double x = from_u(rnd64());
            expect("atan", x, 0, gomath::atan(x), was::atan(x));
        }
        n += n_rand + n_bits;
        if (!g_bad) std::printf("ok atan %ld\n", n);
    }
    {   // atan2: every pair of special values, then random pairs
        long n = 0;
        for (double y : sp)
            for (double x : sp) expect("atan2", y, x, gomath::atan2(y, x), was::atan2(y, x)), n++;
        for (long i = 0; i < n_rand; i++) {
            const bool wide = (i & 1) != 0;
            const double y = wide ? rnd_log(-1074, 1024) : rnd_sym(4.0), x = wide ? rnd_log(-1074, 1024) : rnd_sym(4.0);
            expect("atan2", y, x, gomath::atan2(y, x), was::atan2(y, x));
        }
        for (long i = 0; i < n_bits; i++) {
            const double y = from_u(rnd64()), x = from_u(rnd64());
            expect("atan2", y, x, gomath::atan2(y, x), was::atan2(y, x));
        }
        n += n_rand + n_bits;
        if (!g_bad) std::printf("ok atan2 %ld\n", n);
    }
    {   // sincos: octant boundaries k * Pi/4, arguments up to 2^40, every bit pattern class
        long n = 0;
        std::vector<double> v = sp;
        for (int k = 0; k <= 16; k++) around(v, k * (gomath::kPi / 4), 8);
        for (int e = 30; e <= 40; e++) around(v, __builtin_ldexp(1.0, e), 8);
        for (double x : v) sincos_check(x, n);
        for (long i = 0; i < n_rand; i++) sincos_check((i & 1) ? rnd_log(-1074, 40) : rnd_sym(8 * gomath::kPi), n);
        // beyond 2^64 * Pi/4 the reduction's uint64 conversion is out of range: both forms make the same
        // conversion of the same product, so the patterns are compared all the same
        for (long i = 0; i < n_bits; i++) sincos_check(from_u(rnd64()), n);
        if (!g_bad) std::printf("ok sincos %ld\n", n);
    }
    {   // concentric_sample_disk: a 1024 x 1024 grid of u, the diagonals |ux| == |uy| and the centre
        long n = 0;
        auto disk = [&](double ux, double uy) {
            const pbrt::V2 got = pbrt::concentric_sample_disk(pbrt::V2{ux, uy});
            const pbrt::V2 want = was::concentric_sample_disk(pbrt::V2{ux, uy});
            expect("disk.x", ux, uy, got.x, want.x);
            expect("disk.y", ux, uy, got.y, want.y);
            n += 2;
        };
        for (int i = 0; i < 1024; i++)
            for (int j = 0; j < 1024; j++) disk(i / 1023.0, j / 1023.0);
        for (int i = 0; i <= 1024; i++) {   // dyadic u: 2 u - 1 and 1 - u are exact, so |ux| == |uy| exactly
            const double u = i / 1024.0;
            disk(u, u);
            disk(u, 1 - u);
        }
        disk(0.5, 0.5);
        for (double a : {0.0, -0.0, 0.5, 1.0, gomath::nan(), gomath::kInf})
            for (double b : {0.0, 0.5, gomath::kOneMinusEpsilon, gomath::nan(), -gomath::kInf}) disk(a, b), disk(b, a);
        if (!g_bad) std::printf("ok concentric_disk %ld\n", n);
    }
    if (g_bad) std::printf("FAILED: %ld mismatches\n", g_bad);
    return g_bad ? 1 : 0;
}

"""The one-evaluation forms of Go's trig routines, checked without a GPU.

go-pbrt_amd/csrc/gomath.h evaluates Sin and Cos of one argument together
(sincos), xatan once per satan, and one division and one satan per asin;
pbrt_path.h's concentric_sample_disk holds one division and one sincos. A wave
whose lanes fall into different ranges then runs each expensive part once; every
lane still performs exactly the operations Go performs for its argument.

tests/gomath_once_check.cpp carries the branch-per-range forms verbatim and
requires the IEEE bits (NaN as a class) of asin, acos, atan, atan2 and sincos to
be theirs on: ±0, ±1 and their neighbours, NaN, ±Inf, the smallest and largest
denormals, ±8 ulps around 0.66, 0.7 and Tan(3*Pi/8), ±8 ulps around k * Pi/4 for
k = 0..16 and around 2^30..2^40, 10^7 random arguments per routine over its
domain and 10^6 random 64-bit patterns; and of concentric_sample_disk on a
1024 x 1024 grid of u, the diagonals |ux| == |uy| and the centre.

Built as a host-only compile of the device header under ASan + UBSan. The
float-cast-overflow check alone is off: beyond 2^64 * Pi/4 the Cody-Waite
reduction's uint64 conversion is out of range in Go's routine and in both forms
here alike (the hot path's arguments are below 2 * Pi), and the random bit
patterns go there.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_one_evaluation_trig_is_bit_identical_to_the_branching_forms(tmp_path):
    exe = tmp_path / "gmo"
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-g", "-ffp-contract=off",
                    "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize=float-cast-overflow", "-fno-sanitize-recover=all", "-static-libsan",
                    "-o", str(exe), os.path.join(REPO, "tests", "gomath_once_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [ln[:2] for ln in lines] == [["ok", "asin_acos"], ["ok", "atan"], ["ok", "atan2"], ["ok", "sincos"],
                                        ["ok", "concentric_disk"]]
    checks = {ln[1]: int(ln[2]) for ln in lines}
    # 10^7 random arguments and 10^6 bit patterns per routine (asin and acos share theirs; sincos
    # compares its two outputs and sin, cos themselves); the grid, 2 x 1025 diagonal points, the centre
    assert checks["asin_acos"] > 2 * 11_000_000 and checks["atan"] > 11_000_000 and checks["atan2"] > 11_000_000
    assert checks["sincos"] > 4 * 11_000_000
    assert checks["concentric_disk"] > 2 * (1024 * 1024 + 2 * 1025 + 1)

"""The host side of pbrt_gpu_li_device without a GPU.

- go-pbrt_amd/csrc/li_query.h (the argument checks, the refusals and the kernel
  choice) as a stand-alone program under ASan + UBSan: tests/li_query_check.cpp.
- tests/li_reference.py, the restatements the GPU tests rely on, each against an
  independent source: its PCG32 against the golden streams of tests/golden/golden.json
  and the oracle's floats; its advance against literal steps; its mb_state against the
  values tests/li_mb_check.cpp prints from go-pbrt_amd/csrc/pbrt_path.h itself (the
  header compiles on the host with hipcc --cuda-host-only, so no copy of the
  splitmix chain is needed); its camera draws against cam_sample.h's table; and
  the pFilm offsets the GPU tests draw (some are exactly 0: see that test).
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np

import li_reference as R
import oracle_lib as O
import pbrtgpu as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GOLDEN = json.load(open(os.path.join(REPO, "tests", "golden", "golden.json")))


def test_li_query_header_under_sanitizers(tmp_path):
    exe = tmp_path / "lqc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(REPO, "tests", "li_query_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"checks=(\d+) bad=(\d+)", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) > 150
    cases = {ln.split()[1]: int(ln.split()[2]) for ln in r.stdout.splitlines() if ln.startswith("case ")}
    invalid = {"null_ctx", "null_desc", "null_rays", "null_rng", "null_out", "null_ox", "null_oy", "null_oz", "null_dx",
               "null_dy", "null_dz", "null_state", "null_inc", "null_r", "null_g", "null_b", "n_2_31", "n_huge",
               "depth_0", "depth_negative", "reserved", "in_flight", "in_flight_n0"}
    unsupported = {"depth_2049", "direct_lighting", "integrator_0", "strategy_3", "rough_glass", "dist_one_zero",
                   "dist_nan", "dist_negative", "dist_nan_integral", "dist_zero_integral_nonzero_entry",
                   "dist_more_entries_than_lights"}
    assert {k for k, v in cases.items() if v == G.abi.PBRT_E_INVALID} == invalid
    assert {k for k, v in cases.items() if v == G.abi.PBRT_E_UNSUPPORTED} == unsupported
    assert {k for k, v in cases.items() if v == 0} == {"valid", "valid_n0", "valid_nmax", "with_tmax", "supported",
                                                       "depth_2048", "power_strategy", "dist_uniform",
                                                       "dist_power_all_zero", "dist_no_lights"}
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("kernel ")]
    assert len(rows) == 2 * 2 * 7


def test_selector_has_the_four_kernels_the_table_can_ask_for():
    """li_kernel (kernel_select.hip) by its launch-log names; null for what is not compiled."""
    for kx in (0, 1):
        for depth in (0, 64):
            assert G.kernel_choice("k_li", kx, depth) == f"k_li<{'true' if kx else 'false'}, {depth}>"
    assert G.kernel_choice("k_li", 0, 32) is None and G.kernel_choice("k_li", 1, -1) is None
    assert {n for n in G.kernel_names() if n.startswith("k_li<")} == \
        {"k_li<false, 0>", "k_li<true, 0>", "k_li<false, 64>", "k_li<true, 64>"}


def test_pcg32_is_the_golden_stream():
    for seed, want in GOLDEN["pcg32_first16"].items():
        # NewRNGWithSeed / SetSequence (rng.go:28-34): state 0, one step, + the constant, one step
        inc = R.pcg_inc_of(int(seed))
        st, _ = R.pcg_next(np.zeros(1, np.uint64), inc)
        with np.errstate(over="ignore"):
            st = st + np.uint64(0x853c49e6748fea9b)
        st, _ = R.pcg_next(st, inc)
        got, st0 = [], st
        for _ in range(16):
            st, v = R.pcg_next(st, inc)
            got.append(int(v[0]))
        assert got == want, seed
        fl = (C.c_double * 16)()
        O.lib().oracle_pcg_floats(int(seed), 16, fl)
        st = st0
        for i in range(16):
            st, f = R.pcg_float(st, inc)
            assert f[0] == fl[i], (seed, i)
        # advance: k literal steps, per element
        ks = np.array([0, 1, 2, 7, 16])
        adv = R.pcg_advance(np.repeat(st0, ks.size), np.repeat(inc, ks.size), ks)
        for k, a in zip(ks, adv):
            s = st0
            for _ in range(k):
                s, _ = R.pcg_next(s, inc)
            assert a == s[0], (seed, k)


def test_mb_state_is_the_headers(tmp_path):
    exe = tmp_path / "mbc"
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-o", str(exe),
                    os.path.join(REPO, "tests", "li_mb_check.cpp")], check=True, capture_output=True)
    rows = np.array([[int(v) for v in ln.split()] for ln in
                     subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()],
                    dtype=np.uint64)
    assert rows.shape == (9 ** 3, 4)
    assert np.array_equal(R.mb_state(rows[:, 0], rows[:, 1], rows[:, 2]), rows[:, 3])
    assert len(set(rows[:, 3].tolist())) > 700   # (t ^ pi collisions aside, the states differ)


def test_samples_follow_the_reference_order_and_the_camera_table():
    scene = G.Scene.readme(40, 24)   # 3 x 2 tiles of 16, the last column 8 wide (the Scene owns the descriptor)
    film = scene.desc.film
    s = R.samples(film, 3)
    assert len(s.k) == 40 * 24 * 2 and set(s.k.tolist()) == {1, 2}
    assert R.num_tiles(film, 16) == 6 and R.tile_bounds(film, 16, 2) == (32, 0, 40, 16)
    assert s.tile[0] == 0 and s.tile[-1] == 5 and (np.diff(s.tile) >= 0).all()
    last = s.tile == 2
    assert s.pi[last].max() == 8 * 16 - 1 and s.px[last].min() == 32 and s.px[last].max() == 39
    assert np.array_equal(s.pi[last][:4], [0, 0, 1, 1]) and np.array_equal(s.px[last][:6], [32, 32, 33, 33, 34, 34])
    # cam_sample.h, n_dims = 0: draws 0, 1 pFilm, 2, 3 pLens, 4 the time; Li starts five steps on
    assert np.array_equal(R.pcg_advance(s.start, s.inc, 5), s.state)
    st, fx = R.pcg_float(s.start, s.inc)
    assert np.array_equal(fx, s.film_x)
    st = R.pcg_advance(s.start, s.inc, 4)
    _, tu = R.pcg_float(st, s.inc)
    assert np.array_equal(tu, s.time_u)
    assert np.array_equal(s.inc, 2 * s.tile.astype(np.uint64) + np.uint64(1))
    for v in (s.film_x, s.film_y, s.lens_u, s.lens_v, s.time_u):
        assert (v >= 0).all() and (v < 1).all()


def test_drawn_film_offsets_that_are_exactly_zero():
    """The issue asked for an assertion that no drawn pFilm offset of the GPU cases is exactly 0.
    With their fixed seeds that does not hold, and cannot: the reference's PCG32, with its
    (rot + 1) & 31 rotation (SURVEY #1), returns 0 about once in 150 draws (the golden stream
    of seed 0 holds one at index 12). Counted here for every film size tests/test_gpu_li.py
    uses: README 40x24 draws 14 zero x offsets and 13 zero y offsets among its 1920 samples.
    A zero offset puts pFilm on the pixel's corner, where both camera_ray callers compute
    (double)x + 0.0; those samples are part of the film comparison like any other, so the
    cases cover them. What is asserted is therefore the range, and that the corner case is
    present in the README case."""
    import test_gpu_li as T
    for name, case in T.CASES.items():
        scene = case.scene()   # (owns the descriptor)
        film = scene.desc.film
        s = R.samples(film, T.SPP)
        for v in (s.film_x, s.film_y):
            assert (v >= 0).all() and (v < 1).all(), name
        print(name, "zero offsets: x", int((s.film_x == 0).sum()), "y", int((s.film_y == 0).sum()), "of", len(s.k))
        assert film.res_x <= 48 and film.res_y <= 32, name
        if name == "readme40x24":
            assert ((s.film_x == 0).sum(), (s.film_y == 0).sum(), len(s.k)) == (14, 13, 1920)


def test_film_of_one_sample_is_its_footprint():
    """film(): a sample at pixel (5, 3) + (0.25, 0.75) with radius 1 reaches the film pixels
    x in {4, 5}, y in {3, 4} with the filter table's weights; RGBToXYZ of the sum."""
    scene = G.Scene.readme(40, 24)
    f = scene.desc.film
    assert (f.filter_radius_x, f.filter_radius_y) == (1.0, 1.0) and not 0.0 > f.max_sample_luminance
    one = R.Samples(*[np.array([v]) for v in (0, 3 * 16 + 5, 1, 5, 3, 1, 0, 0.25, 0.75, 0.5, 0.5, 0.0, 0)])
    out = R.film(f, one, np.array([[1.0, 2.0, 4.0]]))
    ys, xs = np.nonzero(out[..., 1])
    assert sorted(set(xs.tolist())) == [4, 5] and sorted(set(ys.tolist())) == [3, 4]
    table = np.array(list(f.filter_table))
    dx, dy = 5.25 - 0.5, 3.75 - 0.5
    for y in (3, 4):
        for x in (4, 5):
            w = table[int(abs((y - dy) * 16.0)) * 16 + int(abs((x - dx) * 16.0))]
            want = 0.212671 * (1.0 * w) + 0.715160 * (2.0 * w) + 0.072169 * (4.0 * w)
            assert out[y, x, 1] == want
    nan = R.film(f, one, np.array([[np.nan, 2.0, 4.0]]))   # integrator.go:256-262
    assert np.array_equal(nan, R.film(f, one, np.array([[0.1, 0.1, 0.1]])))

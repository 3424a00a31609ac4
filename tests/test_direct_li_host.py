"""The host side of pbrt_gpu_direct_li_device without a GPU.

- go-pbrt_amd/csrc/direct_li_query.h (the argument checks, the refusals, the kernel
  choice, the capped grid and the size of the level records) as a stand-alone program
  under ASan + UBSan: tests/direct_li_query_check.cpp.
- The ctypes mirror of pbrt_direct_li_desc against the header, the exported symbols,
  and the wrapper's buffer checks.
- The kernel names and the selector.
- The preconditions of tests/test_gpu_direct_li.py's cases, on the oracle alone: the
  cases recurse as deep as they are meant to (so the GPU tests cannot pass vacuously),
  every oracle render the GPU tests compare with returns 0 and a finite film, and the
  Matte cases trace exactly one closest-hit ray per path.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pbrtgpu as G
import test_gpu_direct_li as T
from pbrtgpu import abi
from test_query_abi import FakeRenderer, fake

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = abi.PBRT_E_INVALID


def test_direct_li_query_header_under_sanitizers(tmp_path):
    exe = tmp_path / "dlqc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(REPO, "tests", "direct_li_query_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"checks=(\d+) bad=(\d+)", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) > 500
    cases = {ln.split()[1]: int(ln.split()[2]) for ln in r.stdout.splitlines() if ln.startswith("case ")}
    invalid = {"null_ctx", "null_desc", "null_rays", "null_rng", "null_out", "null_ox", "null_oy", "null_oz", "null_dx",
               "null_dy", "null_dz", "null_state", "null_inc", "null_r", "null_g", "null_b", "n_2_31", "n_huge",
               "depth_0", "depth_negative", "reserved_0", "reserved_1", "in_flight", "in_flight_n0"}
    unsupported = {"strategy_0", "strategy_3", "rough_glass", "kx_depth_65", "kx_depth_max"}
    assert {k for k, v in cases.items() if v == abi.PBRT_E_INVALID} == invalid
    assert {k for k, v in cases.items() if v == abi.PBRT_E_UNSUPPORTED} == unsupported
    assert {k for k, v in cases.items() if v == 0} == {"valid", "valid_n0", "valid_nmax", "with_tmax", "supported",
                                                       "supported_kx", "sample_one", "kx_depth_64", "matte_depth_65",
                                                       "matte_depth_max"}
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("kernel ")]) == 2 * 2 * 7
    levels = dict(tuple(int(v) for v in ln.split()[1::2]) for ln in r.stdout.splitlines() if ln.startswith("levels "))
    assert levels == {1: 0, 2: 1, 3: 1, 63: 31, 64: 32}
    sizes = {(int(p[2]), int(p[4])): int(p[6]) for p in (ln.split() for ln in r.stdout.splitlines())
             if p and p[0] == "bytes"}
    assert sizes[(2048, 64)] == 2048 * 32 * 64 * 56 and sizes[(65536, 64)] == 65536 * 32 * 64 * 56
    assert sizes[(2048, 1)] == 0 and sizes[(1, 2)] == sizes[(1, 3)] == 64 * 56 and sizes[(2, 63)] == 2 * 31 * 64 * 56


def test_the_symbols_are_exported_and_the_struct_is_the_headers(tmp_path):
    L = G.lib()
    assert abi.DIRECT_LI_SYMBOLS == ("pbrt_gpu_direct_li_device", "pbrt_gpu_direct_li_scratch_bytes")
    for name in abi.DIRECT_LI_SYMBOLS:
        assert hasattr(L, name), name
    assert len(L.pbrt_gpu_direct_li_device.argtypes) == 6
    hdr = open(os.path.join(REPO, "include", "pbrt_gpu.h")).read()
    assert re.search(r"int pbrt_gpu_direct_li_device\(pbrt_gpu_ctx\* ctx, const pbrt_direct_li_desc\* desc", hdr)
    fields = ("max_depth", "dl_strategy", "reserved")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pbrt_gpu.h"\nint main(void) {\n'
                   '    printf("size %zu\\n", sizeof(pbrt_direct_li_desc));\n' +
                   "".join(f'    printf("{f} %zu\\n", offsetof(pbrt_direct_li_desc, {f}));\n' for f in fields) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o", str(exe),
                    str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(abi.DirectLiDesc) == 16
    assert tuple(f for f, _ in abi.DirectLiDesc._fields_) == fields
    for f in fields:
        assert int(got[f]) == getattr(abi.DirectLiDesc, f).offset, f
    d = abi.direct_li_desc()
    assert (d.max_depth, d.dl_strategy, tuple(d.reserved)) == (5, abi.PBRT_DL_UNIFORM_SAMPLE_ALL, (0, 0))
    d = abi.direct_li_desc(7, abi.PBRT_DL_UNIFORM_SAMPLE_ONE, (3, 4))
    assert (d.max_depth, d.dl_strategy, tuple(d.reserved)) == (7, 2, (3, 4))


def test_null_context_is_invalid_with_no_device():
    L = G.lib()
    n = 4
    cols = [np.zeros(n) for _ in range(7)]
    rays = abi.RaySoA(*[c.ctypes.data_as(C.POINTER(C.c_double)) for c in cols])
    st, inc = np.zeros(n, np.uint64), np.ones(n, np.uint64)
    rng = abi.RngSoA(st.ctypes.data_as(C.POINTER(C.c_uint64)), inc.ctypes.data_as(C.POINTER(C.c_uint64)))
    rgb = [np.full(n, 7.0) for _ in range(3)]
    out = abi.RadianceSoA(*[c.ctypes.data_as(C.POINTER(C.c_double)) for c in rgb])
    d = abi.direct_li_desc()
    assert L.pbrt_gpu_direct_li_device(None, C.byref(d), C.byref(rays), C.byref(rng), n, C.byref(out)) == INVALID
    assert L.pbrt_gpu_direct_li_device(None, None, None, None, 0, None) == INVALID
    assert L.pbrt_gpu_direct_li_scratch_bytes(None) == 0
    assert all((c == 7.0).all() for c in rgb)   # never dereferenced


class FakeDirectLi(FakeRenderer):
    """A Renderer whose direct_li_device stops at its buffer check (no context behind it)."""
    direct_li_device = G.Renderer.direct_li_device
    h = None


def test_direct_li_device_checks_its_buffers_before_the_library():
    r, other = FakeDirectLi(), FakeDirectLi()

    def bufs(**bad):
        rays = {k: fake(r, 10) for k in G.RAY_KEYS}
        rng = {k: fake(r, 10, np.uint64) for k in G.RNG_KEYS}
        out = {k: fake(r, 10, dt) for k, dt in G.LI_DTYPES.items()}
        for k, b in bad.items():
            (rays if k in rays else rng if k in rng else out)[k] = b
        return rays, rng, out

    cases = {
        "state of the wrong type": dict(state=fake(r, 10, np.float64)),
        "r of the wrong type": dict(r=fake(r, 10, np.uint64)),
        "rays of the wrong type": dict(rays=fake(r, 10, np.int32)),
        "a short ray buffer": dict(dz=fake(r, 9)),
        "a short rng buffer": dict(inc=fake(r, 9, np.uint64)),
        "a short optional output": dict(draws=fake(r, 9, np.uint32)),
        "another renderer's": dict(g=fake(other, 10)),
        "not a buffer": dict(r=np.zeros(10)),
    }
    for what, bad in cases.items():
        rays, rng, out = bufs(**bad)
        with pytest.raises(G.PbrtError) as e:
            r.direct_li_device(rays, rng, 10, out)
        assert e.value.code == INVALID, what
    rays, rng, out = bufs()
    for bad_call in (lambda: r.direct_li_device(rays, rng, 11, out),
                     lambda: r.direct_li_device(rays, rng, 10, {k: v for k, v in out.items() if k != "b"}),
                     lambda: r.direct_li_device(rays, {"inc": rng["inc"]}, 10, out),
                     lambda: r.direct_li_device(rays, rng, 10, dict(out, alpha=out["r"]))):
        with pytest.raises(G.PbrtError) as e:
            bad_call()
        assert e.value.code == INVALID


def test_selector_has_the_four_kernels_and_k_li_keeps_its_four():
    for kx in (0, 1):
        for depth in (0, 64):
            assert G.kernel_choice("k_li_direct", kx, depth) == f"k_li_direct<{'true' if kx else 'false'}, {depth}>"
    assert G.kernel_choice("k_li_direct", 0, 32) is None and G.kernel_choice("k_li_direct", 1) is None
    assert {n for n in G.kernel_names() if n.startswith("k_li_direct<")} == \
        {"k_li_direct<false, 0>", "k_li_direct<true, 0>", "k_li_direct<false, 64>", "k_li_direct<true, 64>"}
    assert {n for n in G.kernel_names() if n.startswith("k_li<")} == \
        {"k_li<false, 0>", "k_li<true, 0>", "k_li<false, 64>", "k_li<true, 64>"}
    assert {c.kernel for c in T.CASES.values()} == {n for n in G.kernel_names() if n.startswith("k_li_direct<")}


# ------------------------------------- the GPU cases' preconditions, on the oracle alone
def extra_closest(name, max_depth, strategy=T.ALL):
    """Closest-hit rays beyond one per path: the levels the recursion through glass pushed."""
    _, st = T.oracle_film(name, max_depth, strategy)
    return st.closest_rays - st.paths


def test_every_oracle_render_of_the_gpu_cases_is_clean_and_the_kernel_is_the_scenes():
    for name, max_depth, strategy in T.ORACLE_RUNS:
        film, st = T.oracle_film(name, max_depth, strategy)   # asserts rc == 0 and a finite film
        fd = T.scene_of(name).desc.film
        assert st.paths == len(T.samples_of(name).k) == fd.res_x * fd.res_y * (T.SPP - 1) <= 3072, name
        assert fd.res_x <= 48 and fd.res_y <= 32, name
        # (a glass stack is black until the recursion reaches the wall: its ray counts are the check
        # at max_depth 5, its film at 63 and 64, test_the_glass_stacks_reach_the_last_level)
        assert film.any() or (name.startswith("glass_stack") and max_depth == 5), name
    nodes = {name: T.scene_of(name).desc.n_nodes for name in T.CASES}
    for name, case in T.CASES.items():
        assert case.kernel.endswith(", 64>") == (nodes[name] > 64), (name, nodes[name])
        assert case.kernel.startswith("k_li_direct<false") == (name in T.MATTE_CASES), name
    assert (nodes["crowd_kx"], nodes["crowd_matte"], nodes["material_scene"]) == (121, 121, 7)
    assert (nodes["glass_stack34"], nodes["glass_stack20"]) == (69, 41)


def test_the_matte_cases_trace_one_closest_ray_per_path():
    for name in T.MATTE_CASES:
        for strategy in (T.ALL, T.ONE):
            assert extra_closest(name, 5, strategy) == 0, name
    assert extra_closest("readme40x24", 1) == 0


def test_the_kx_cases_recurse():
    assert T.samples_of("crowd_kx").k.size == 3072 and extra_closest("crowd_kx", 5) >= 200
    assert extra_closest("crowd_kx", 2) >= 150   # one level: the stride loop's case still pushes records
    assert T.samples_of("material_scene").k.size == 1536 and extra_closest("material_scene", 5) >= 150
    assert extra_closest("glass", 5) > 0
    for strategy in (T.ALL, T.ONE):   # the strategy changes no refraction
        assert extra_closest("crowd_kx", 5, strategy) == extra_closest("crowd_kx", 5)


def test_the_glass_stacks_reach_the_last_level():
    """glass_stack(34): at max_depth 64 some paths push all 32 level records (closest rays grow from
    max_depth 62 to 64); glass_stack(20): every path ends on the wall before the records run out."""
    assert T.samples_of("glass_stack34").k.size == 512
    c62 = T.oracle_film.__wrapped__("glass_stack34", 62, T.ALL)[1]
    c64, c63 = T.oracle_film("glass_stack34", 64, T.ALL)[1], T.oracle_film("glass_stack34", 63, T.ALL)[1]
    assert c64.closest_rays > c62.closest_rays and c63.closest_rays == c62.closest_rays
    assert c64.closest_rays - c64.paths > 12000
    film64 = T.oracle_film("glass_stack34", 64, T.ALL)[0]
    assert int((film64.sum(axis=2) != 0).sum()) == 239
    assert extra_closest("glass_stack20", 64) == extra_closest("glass_stack20", 63) > 9993 - 1
    film20 = T.oracle_film("glass_stack20", 64, T.ALL)[0]
    assert int((film20.sum(axis=2) != 0).sum()) == 256 and film20.max() < 1e-3

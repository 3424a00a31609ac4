"""pbrt_gpu_frame_samples_stratified_device and pbrt_gpu_li_stratified_device without a
GPU: the symbols exist and are declared, the ctypes mirrors of their structs have the
header's sizes and offsets (a compiled C snippet), a NULL context is refused before any
device call, and li_stratified_device's wrapper checks its buffers before the library.
CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pbrtgpu as G
from pbrtgpu import abi
from test_li_abi import li_bufs
from test_query_abi import FakeRenderer, fake

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = abi.PBRT_E_INVALID


def test_the_symbols_are_exported_and_declared():
    L = G.lib()
    assert abi.STRAT_SYMBOLS == ("pbrt_gpu_frame_samples_stratified_device", "pbrt_gpu_li_stratified_device")
    for name in abi.STRAT_SYMBOLS:
        assert hasattr(L, name), name
    assert len(L.pbrt_gpu_frame_samples_stratified_device.argtypes) == 5
    assert len(L.pbrt_gpu_li_stratified_device.argtypes) == 7
    hdr = open(os.path.join(REPO, "include", "pbrt_gpu.h")).read()
    for name in abi.STRAT_SYMBOLS:
        assert f"int {name}(" in hdr
    names = set(G.kernel_names())
    assert {"k_strat_pixels"} | {f"k_li_strat<{kx}, {d}>" for kx in ("false", "true") for d in (0, 64)} <= names
    for kx in (False, True):   # the selector's table is the four instantiations
        for depth in (0, 64):
            assert G.kernel_choice("k_li_strat", kx, depth) == f"k_li_strat<{str(kx).lower()}, {depth}>"
    assert G.kernel_choice("k_li_strat", False, 32) is None


def test_ctypes_mirrors_have_the_headers_layout(tmp_path):
    mirrors = {"pbrt_strat_sampler_desc": abi.StratSamplerDesc, "pbrt_strat_samples_soa": abi.StratSamplesSoA,
               "pbrt_strat_soa": abi.StratSoA}
    fields = {"pbrt_strat_sampler_desc": ("sampler_x", "sampler_y", "n_dims", "jitter", "reserved"),
              "pbrt_strat_samples_soa": ("k", "table", "s1d"),
              "pbrt_strat_soa": ("s1d", "table", "k", "n_tables", "spp", "n_dims", "first_1d", "first_2d", "reserved")}
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pbrt_gpu.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in mirrors) +
                   "".join(f'    printf("{n}.{f} %zu\\n", offsetof({n}, {f}));\n' for n, fs in fields.items() for f in fs) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o", str(exe),
                    str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    for n, m in mirrors.items():
        assert int(got[n]) == C.sizeof(m), n
        assert tuple(f for f, _ in m._fields_) == fields[n]
        for f in fields[n]:
            assert int(got[f"{n}.{f}"]) == getattr(m, f).offset, (n, f)
    assert C.sizeof(abi.StratSamplerDesc) == 20 and C.sizeof(abi.StratSamplesSoA) == 24 and C.sizeof(abi.StratSoA) == 48
    s = abi.strat_sampler_desc(8, 8, 4, True)
    assert (s.sampler_x, s.sampler_y, s.n_dims, s.jitter, s.reserved) == (8, 8, 4, 1, 0)
    assert [abi.camera_cursors(n) for n in range(4)] == [(0, 0), (1, 1), (1, 2), (1, 2)]
    assert G.STRAT_BYTES_PER_SAMPLE == G.FRAME_BYTES_PER_SAMPLE + 8 == 112


def test_null_context_is_invalid_with_no_device():
    L = G.lib()
    n = 4
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    cols = [np.zeros(n) for _ in range(7)]
    rays = abi.RaySoA(*[c.ctypes.data_as(dp) for c in cols])
    st, inc = np.zeros(n, np.uint64), np.ones(n, np.uint64)
    rng = abi.RngSoA(st.ctypes.data_as(C.POINTER(C.c_uint64)), inc.ctypes.data_as(C.POINTER(C.c_uint64)))
    rgb = [np.full(n, 7.0) for _ in range(3)]
    out = abi.RadianceSoA(*[c.ctypes.data_as(dp) for c in rgb])
    tab, kk, tb = np.full(8, 3.0), np.zeros(n, np.int32), np.zeros(n, np.int32)
    strat = abi.StratSoA(tab.ctypes.data_as(dp), tb.ctypes.data_as(ip), kk.ctypes.data_as(ip), 1, 4, 2, 1, 2, 0)
    d = abi.li_desc(max_depth=5)
    assert L.pbrt_gpu_li_stratified_device(None, C.byref(d), C.byref(rays), C.byref(rng), n, C.byref(out),
                                           C.byref(strat)) == INVALID
    assert L.pbrt_gpu_li_stratified_device(None, None, None, None, 0, None, None) == INVALID
    fd, sm = abi.frame_desc(16, 3, 0, 1), abi.strat_sampler_desc(2, 2, 4)
    fs, ss = abi.FrameSamplesSoA(), abi.StratSamplesSoA(kk.ctypes.data_as(ip), tb.ctypes.data_as(ip), tab.ctypes.data_as(dp))
    assert L.pbrt_gpu_frame_samples_stratified_device(None, C.byref(fd), C.byref(sm), C.byref(fs), C.byref(ss)) == INVALID
    assert L.pbrt_gpu_frame_samples_stratified_device(None, None, None, None, None) == INVALID
    assert all((c == 7.0).all() for c in rgb) and (tab == 3.0).all() and not kk.any()   # never dereferenced


class FakeStrat(FakeRenderer):
    """A Renderer whose li_stratified_device stops at its buffer check (no context behind it)."""
    li_stratified_device = G.Renderer.li_stratified_device
    h = None


def test_li_stratified_device_checks_its_buffers_before_the_library():
    r = FakeStrat()
    n, nt, spp, nd = 10, 3, 4, 2
    good = lambda: dict(s1d=fake(r, nt * spp * nd), table=fake(r, n, np.int32), k=fake(r, n, np.int32))   # noqa: E731
    cases = {
        "a short table array": dict(s1d=fake(r, nt * spp * nd - 1)),
        "s1d of the wrong type": dict(s1d=fake(r, nt * spp * nd, np.uint64)),
        "k of the wrong type": dict(k=fake(r, n, np.uint32)),
        "a short table index": dict(table=fake(r, n - 1, np.int32)),
        "closed": dict(k=fake(r, n, np.int32, handle=None)),
        "an unknown key": dict(alpha=fake(r, n, np.int32)),
    }
    for what, bad in cases.items():
        rays, rng, out = li_bufs(r, n)
        with pytest.raises(G.PbrtError) as e:
            r.li_stratified_device(rays, rng, n, out, dict(good(), **bad), nt, spp, nd, 1, 2)
        assert e.value.code == INVALID, what
    rays, rng, out = li_bufs(r, n, r=fake(r, n - 1))   # li_device's own check comes first
    with pytest.raises(G.PbrtError):
        r.li_stratified_device(rays, rng, n, out, good(), nt, spp, nd, 1, 2)

"""pbrt_gpu_li_device without a GPU: the symbol exists, the ctypes mirrors of its three
structs have the header's sizes and offsets, a NULL context is refused before any
device call, and the wrapper's buffer check (the only bounds protection of the device
call) refuses what it must for the new element types. CPU only; numpy and ctypes only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pbrtgpu as G
from pbrtgpu import abi
from test_query_abi import FakeRenderer, fake

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = abi.PBRT_E_INVALID


def test_the_symbol_is_exported_and_declared():
    L = G.lib()
    assert abi.LI_SYMBOLS == ("pbrt_gpu_li_device",)
    for name in abi.LI_SYMBOLS:
        assert hasattr(L, name), name
    assert L.pbrt_gpu_li_device.argtypes is not None and len(L.pbrt_gpu_li_device.argtypes) == 6


def test_ctypes_mirrors_have_the_headers_layout(tmp_path):
    mirrors = {"pbrt_li_desc": abi.LiDesc, "pbrt_rng_soa": abi.RngSoA, "pbrt_radiance_soa": abi.RadianceSoA}
    fields = {"pbrt_li_desc": ("integrator", "max_depth", "light_strategy", "reserved", "rr_threshold"),
              "pbrt_rng_soa": ("state", "inc"), "pbrt_radiance_soa": ("r", "g", "b", "state", "draws", "rays")}
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
    assert C.sizeof(abi.LiDesc) == 24 and C.sizeof(abi.RngSoA) == 16 and C.sizeof(abi.RadianceSoA) == 48
    d = abi.li_desc()
    assert (d.integrator, d.max_depth, d.light_strategy, d.reserved, d.rr_threshold) == \
        (abi.PBRT_INTEGRATOR_PATH, 10, abi.PBRT_LIGHT_STRATEGY_UNIFORM, 0, 1.0)


def test_null_context_is_invalid_with_no_device():
    L = G.lib()
    n = 4
    cols = [np.zeros(n) for _ in range(7)]
    rays = abi.RaySoA(*[c.ctypes.data_as(C.POINTER(C.c_double)) for c in cols])
    st, inc = np.zeros(n, np.uint64), np.ones(n, np.uint64)
    rng = abi.RngSoA(st.ctypes.data_as(C.POINTER(C.c_uint64)), inc.ctypes.data_as(C.POINTER(C.c_uint64)))
    rgb = [np.full(n, 7.0) for _ in range(3)]
    out = abi.RadianceSoA(*[c.ctypes.data_as(C.POINTER(C.c_double)) for c in rgb])
    d = abi.li_desc(max_depth=5)
    assert L.pbrt_gpu_li_device(None, C.byref(d), C.byref(rays), C.byref(rng), n, C.byref(out)) == INVALID
    assert L.pbrt_gpu_li_device(None, None, None, None, 0, None) == INVALID
    assert all((c == 7.0).all() for c in rgb)   # never dereferenced


def li_bufs(renderer, n, **other):
    """(rays, rng, out) of fake buffers with li_device's element types; other: name -> buffer."""
    rays = {k: fake(renderer, n) for k in G.RAY_KEYS}
    rng = {k: fake(renderer, n, np.uint64) for k in G.RNG_KEYS}
    out = {k: fake(renderer, n, dt) for k, dt in G.LI_DTYPES.items()}
    for k, b in other.items():
        (rays if k in rays else rng if k in rng else out)[k] = b
    return rays, rng, out


class FakeLi(FakeRenderer):
    """A Renderer whose li_device stops at its buffer check (no context behind it)."""
    li_device = G.Renderer.li_device
    h = None


def test_li_device_checks_its_buffers_before_the_library():
    r, other = FakeLi(), FakeLi()
    assert G.LI_DTYPES == {"r": np.float64, "g": np.float64, "b": np.float64, "state": np.uint64,
                           "draws": np.uint32, "rays": np.uint32}
    for dt in (np.uint64, np.uint32):
        assert np.dtype(dt) in G.BUFFER_DTYPES
    cases = {
        "state of the wrong type": dict(state=fake(r, 10, np.float64)),
        "inc of the wrong type": dict(inc=fake(r, 10, np.int32)),
        "r of the wrong type": dict(r=fake(r, 10, np.uint64)),
        "draws of the wrong type": dict(draws=fake(r, 10, np.uint64)),
        "rays of the wrong type": dict(rays=fake(r, 10, np.int32)),
        "a short rng buffer": dict(inc=fake(r, 9, np.uint64)),
        "a short output": dict(b=fake(r, 9)),
        "a short optional output": dict(draws=fake(r, 9, np.uint32)),
        "another renderer's": dict(g=fake(other, 10)),
        "closed": dict(state=fake(r, 10, np.uint64, handle=None)),
        "not a buffer": dict(r=np.zeros(10)),
    }
    for what, bad in cases.items():
        rays, rng, out = li_bufs(r, 10, **bad)
        with pytest.raises(G.PbrtError) as e:
            r.li_device(rays, rng, 10, out)
        assert e.value.code == INVALID, what
    rays, rng, out = li_bufs(r, 10)
    for bad_call in (lambda: r.li_device(rays, rng, 11, out),                                    # n beyond every buffer
                     lambda: r.li_device(rays, rng, 10, {k: v for k, v in out.items() if k != "g"}),   # g is required
                     lambda: r.li_device(rays, {"state": rng["state"]}, 10, out),                 # inc is required
                     lambda: r.li_device(rays, rng, 10, dict(out, alpha=out["r"])),               # an unknown output
                     lambda: r.li_device(rays, rng, 2**31, out)):
        with pytest.raises(G.PbrtError) as e:
            bad_call()
        assert e.value.code == INVALID
    r._token.alive = False   # the renderer closes: every buffer it made is closed with it
    with pytest.raises(G.PbrtError):
        r.li_device(rays, rng, 10, out)

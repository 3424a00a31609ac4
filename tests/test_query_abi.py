"""Device-resident ray queries and context-owned buffers (pbrt_gpu_buffer_*,
pbrt_gpu_*_device, pbrt_gpu_query_status) without a GPU: the symbols exist,
argument validation happens before any device call, the ctypes mirrors have the
header's sizes, the wrapper's buffer check (the only bounds protection of the
device calls) rejects what it must, and the buffer bookkeeping
(go-pbrt_amd/csrc/query_buffers.h) runs clean under ASan + UBSan as a
stand-alone host program. CPU only; numpy and ctypes only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pbrtgpu as G
from pbrtgpu import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = abi.PBRT_E_INVALID


def test_every_new_symbol_is_exported():
    L = G.lib()
    assert len(abi.QUERY_SYMBOLS) == 10
    for name in abi.QUERY_SYMBOLS:
        assert hasattr(L, name), name


def _rays(n=4):
    """A pbrt_ray_soa / pbrt_hit_soa over host arrays: never dereferenced here."""
    cols = [np.zeros(n) for _ in range(7)]
    soa = abi.RaySoA(*[c.ctypes.data_as(C.POINTER(C.c_double)) for c in cols])
    hit = np.zeros(n, np.uint8)
    hs = abi.HitSoA(hit.ctypes.data_as(C.POINTER(C.c_uint8)))
    return cols, soa, hit, hs


def test_null_context_is_invalid_for_every_call():
    L = G.lib()
    cols, soa, hit, hs = _rays()
    h = C.c_void_p(0xdead)   # must be cleared on failure
    assert L.pbrt_gpu_buffer_create(None, 64, C.byref(h)) == INVALID and not h.value
    assert L.pbrt_gpu_buffer_create(None, 64, None) == INVALID   # NULL out
    assert L.pbrt_gpu_intersect_device(None, C.byref(soa), 4, C.byref(hs)) == INVALID
    assert L.pbrt_gpu_intersect_p_device(None, C.byref(soa), 4, hit.ctypes.data) == INVALID
    d = abi.CameraRaysDesc(0, 0, 1, 1, 0.5, 0.5, 0.5, 0.5, 0.0)
    out = abi.RaySoAOut(*[c.ctypes.data_as(C.POINTER(C.c_double)) for c in cols])
    assert L.pbrt_gpu_camera_rays_device(None, C.byref(d), C.byref(out)) == INVALID
    rec = abi.QueryRecord()
    assert L.pbrt_gpu_query_status(None, C.byref(rec)) == INVALID


def test_null_buffer_calls_are_harmless():
    L = G.lib()
    x = np.zeros(4)
    assert L.pbrt_gpu_buffer_ptr(None) is None
    assert L.pbrt_gpu_buffer_size(None) == 0
    assert L.pbrt_gpu_buffer_upload(None, 0, x.ctypes.data, 8) == INVALID
    assert L.pbrt_gpu_buffer_download(None, 0, x.ctypes.data, 8) == INVALID
    L.pbrt_gpu_buffer_destroy(None)


def test_ctypes_mirrors_have_the_headers_sizes(tmp_path):
    """sizeof of the new structs, printed by a C program compiled against the header."""
    mirrors = {"pbrt_ray_soa_out": abi.RaySoAOut, "pbrt_camera_rays_desc": abi.CameraRaysDesc,
               "pbrt_query_record": abi.QueryRecord, "pbrt_ray_soa": abi.RaySoA, "pbrt_hit_soa": abi.HitSoA}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "pbrt_gpu.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in mirrors) +
                   '    printf("first_ray %zu\\n", offsetof(pbrt_query_record, first_ray));\n'
                   '    printf("film_dx %zu\\n", offsetof(pbrt_camera_rays_desc, film_dx));\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o", str(exe),
                    str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    for n, m in mirrors.items():
        assert int(got[n]) == C.sizeof(m), n
    assert int(got["first_ray"]) == abi.QueryRecord.first_ray.offset
    assert int(got["film_dx"]) == abi.CameraRaysDesc.film_dx.offset
    assert C.sizeof(abi.QueryRecord) == 24 and C.sizeof(abi.CameraRaysDesc) == 72


class FakeRenderer:
    """What check_buffers and DeviceBuffer need of a Renderer: its token."""

    def __init__(self):
        self._token = G.ContextToken()


class FakeBuffer(G.DeviceBuffer):
    """A DeviceBuffer with a made-up handle that never reaches the library."""

    def close(self):
        self._h = None


def fake(r, n, dtype=np.float64, handle=1):
    return FakeBuffer(r, handle, 0x1000, n, dtype)


def test_buffer_check_accepts_what_fits():
    r = FakeRenderer()
    b = fake(r, 10)
    G.check_buffers(r, 10, [("ox", b, np.float64)])
    G.check_buffers(r, 0, [("ox", b, np.float64)])


def test_buffer_check_rejects_bad_buffers():
    r, other = FakeRenderer(), FakeRenderer()
    good = fake(r, 10)
    cases = {
        "wrong dtype": (10, fake(r, 10, np.int32)),
        "n larger than the buffer": (11, good),
        "another renderer's": (10, fake(other, 10)),
        "closed": (10, fake(r, 10, handle=None)),
        "not a buffer": (10, np.zeros(10)),
        "n beyond int32": (2**31, fake(r, 2**31)),
    }
    for what, (n, b) in cases.items():
        with pytest.raises(G.PbrtError) as e:
            G.check_buffers(r, n, [("ox", good, np.float64), ("oy", b, np.float64)])
        assert e.value.code == INVALID, what
    # the renderer closes: every buffer it made is closed with it
    r._token.alive = False
    with pytest.raises(G.PbrtError):
        G.check_buffers(r, 1, [("ox", good, np.float64)])
    with pytest.raises(G.PbrtError):
        good.ptr
    with pytest.raises(G.PbrtError):
        good.upload(np.zeros(1))
    real = G.DeviceBuffer(r, 0xdead, 0x1000, 10, np.float64)
    real.close()   # silent, and does not reach the library: its context is gone
    assert real.closed
    del real


def test_ray_argument_forms():
    r = FakeRenderer()
    bufs = [fake(r, 4) for k in range(7)]
    from pbrtgpu import _ray_bufs
    assert [k for k, _, _ in _ray_bufs(tuple(bufs[:6]))] == list(G.RAY_KEYS)
    assert [k for k, _, _ in _ray_bufs(tuple(bufs))] == list(G.RAY_KEYS) + ["tmax"]
    assert len(_ray_bufs(dict(zip(G.RAY_KEYS, bufs)))) == 6
    for bad in (tuple(bufs[:5]), {"ox": bufs[0]}, dict(zip(G.RAY_KEYS + ("tmin",), bufs))):
        with pytest.raises(G.PbrtError):
            _ray_bufs(bad)


def test_wrapper_sources_do_not_import_torch():
    """The query path owns its device memory: neither the wrapper nor its GPU
    tests or tool import torch or name one of its stream types."""
    for rel in ("go-pbrt_amd/pbrtgpu/__init__.py", "go-pbrt_amd/pbrtgpu/abi.py", "tests/test_gpu_query.py",
                "tools/query_bench.py"):
        src = open(os.path.join(REPO, rel)).read()
        assert not re.search(r"^\s*(import|from)\s+torch\b", src, re.M), rel
        assert "record_stream" not in src and "ExternalStream" not in src, rel


def test_buffer_bookkeeping_under_sanitizers(tmp_path):
    """query_buffers.h as a stand-alone host program under ASan + UBSan."""
    exe = tmp_path / "qbc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(REPO, "tests", "query_buffer_check.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"ranges=(\d+) buffers=(\d+) freed=(\d+) bad=(\d+)", r.stdout)
    assert m and int(m.group(4)) == 0
    assert int(m.group(1)) == 13 * 15 * 15 + 10 and int(m.group(2)) == int(m.group(3)) > 500

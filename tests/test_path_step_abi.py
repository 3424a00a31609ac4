"""pbrt_gpu_path_begin_device / pbrt_gpu_path_step_device without a GPU: the symbols exist and
the header declares them, the ctypes mirrors of the three structs have the header's sizes
and offsets, a NULL context is refused before any device call, the wrappers' buffer checks
refuse what they must, and the Go shim's new C identifiers exist in the headers. CPU only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pbrtgpu as G
from pbrtgpu import abi
from test_query_abi import FakeRenderer, fake

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = abi.PBRT_E_INVALID
HEADER = open(os.path.join(REPO, "include", "pbrt_gpu.h")).read()
PATH_FIELDS = ("ox", "oy", "oz", "dx", "dy", "dz", "tmax", "lr", "lg", "lb", "br", "bg", "bb", "eta_scale", "state",
               "inc", "draws", "rays", "bounces", "status")


def test_the_symbols_are_exported_and_declared():
    L = G.lib()
    assert abi.PATH_SYMBOLS == ("pbrt_gpu_path_begin_device", "pbrt_gpu_path_step_device")
    for name in abi.PATH_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\bint %s\(pbrt_gpu_ctx\* ctx," % name, HEADER), name
    assert len(L.pbrt_gpu_path_begin_device.argtypes) == 5 and len(L.pbrt_gpu_path_step_device.argtypes) == 7
    assert (abi.PBRT_PATH_UNUSED, abi.PBRT_PATH_ALIVE, abi.PBRT_PATH_ENDED, abi.PBRT_PATH_PANICKED) == (0, 1, 2, 3)
    assert "PBRT_PATH_UNUSED = 0, PBRT_PATH_ALIVE = 1, PBRT_PATH_ENDED = 2, PBRT_PATH_PANICKED = 3" in HEADER


def test_ctypes_mirrors_have_the_headers_layout(tmp_path):
    mirrors = {"pbrt_path_soa": abi.PathSoA, "pbrt_path_queue": abi.PathQueue, "pbrt_path_step_soa": abi.PathStepSoA}
    fields = {"pbrt_path_soa": PATH_FIELDS, "pbrt_path_queue": ("index", "count"),
              "pbrt_path_step_soa": ("hit", "material", "ar", "ag", "ab")}
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pbrt_gpu.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in mirrors) +
                   "".join(f'    printf("{n}.{f} %zu\\n", offsetof({n}, {f}));\n' for n, fs in fields.items() for f in fs) +
                   '    printf("status %d %d %d %d\\n", PBRT_PATH_UNUSED, PBRT_PATH_ALIVE, PBRT_PATH_ENDED, PBRT_PATH_PANICKED);\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o", str(exe),
                    str(src)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    got = dict(line.split() for line in lines if not line.startswith("status"))
    assert "status 0 1 2 3" in lines
    for n, m in mirrors.items():
        assert int(got[n]) == C.sizeof(m), n
        assert tuple(f for f, _ in m._fields_) == fields[n]
        for f in fields[n]:
            assert int(got[f"{n}.{f}"]) == getattr(m, f).offset, (n, f)
    assert C.sizeof(abi.PathSoA) == 160 and C.sizeof(abi.PathQueue) == 16
    assert C.sizeof(abi.PathStepSoA) == C.sizeof(abi.HitSoA) + 32
    # the element types of the wrappers' buffers are the structs' pointer targets
    ctype = {np.float64: C.c_double, np.uint64: C.c_uint64, np.uint32: C.c_uint32, np.int32: C.c_int32,
             np.uint8: C.c_uint8}
    assert tuple(G.PATH_DTYPES) == PATH_FIELDS
    for f, t in abi.PathSoA._fields_:
        assert t._type_ is ctype[G.PATH_DTYPES[f]], f
    assert sum(C.sizeof(t._type_) for _, t in abi.PathSoA._fields_) == 141 == G.PATH_BYTES
    for f, t in abi.PathStepSoA._fields_[1:]:
        assert t._type_ is ctype[G.STEP_DTYPES[f]], f


def test_null_context_is_invalid_with_no_device():
    L = G.lib()
    assert L.pbrt_gpu_path_begin_device(None, None, None, 0, None) == INVALID
    assert L.pbrt_gpu_path_step_device(None, None, None, None, None, 0, None) == INVALID
    d = abi.li_desc(max_depth=5)
    ps = abi.PathSoA()
    assert L.pbrt_gpu_path_step_device(None, C.byref(d), C.byref(ps), None, None, 4, None) == INVALID


class FakePath(FakeRenderer):
    """A Renderer whose path calls stop at their buffer checks (no context behind it)."""
    path_begin = G.Renderer.path_begin
    path_step = G.Renderer.path_step
    _path_soa = G.Renderer._path_soa
    _path_queue = G.Renderer._path_queue
    h = None


def path_bufs(r, n, **other):
    pb = {k: fake(r, n, dt) for k, dt in G.PATH_DTYPES.items()}
    pb.update(other)
    return pb


def test_the_wrappers_check_their_buffers_before_the_library():
    r, other = FakePath(), FakePath()
    n = 10
    rays = {k: fake(r, n) for k in G.RAY_KEYS}
    rng = {k: fake(r, n, np.uint64) for k in G.RNG_KEYS}
    q = lambda rr=r, m=n: {"index": fake(rr, m, np.int32), "count": fake(rr, 1, np.uint32)}   # noqa: E731
    bad_paths = {
        "status of the wrong type": dict(status=fake(r, n, np.int32)),
        "bounces of the wrong type": dict(bounces=fake(r, n, np.uint32)),
        "lr of the wrong type": dict(lr=fake(r, n, np.uint64)),
        "a short state array": dict(bb=fake(r, n - 1)),
        "a short optional tmax": dict(tmax=fake(r, n - 1)),
        "another renderer's": dict(draws=fake(other, n, np.uint32)),
        "closed": dict(state=fake(r, n, np.uint64, handle=None)),
        "not a buffer": dict(eta_scale=np.zeros(n)),
        "an unknown array": dict(alpha=fake(r, n)),
        "a missing array": dict(inc=None),
    }
    for what, bad in bad_paths.items():
        for call in (lambda pb: r.path_begin(rays, rng, n, pb), lambda pb: r.path_step(pb, n)):
            with pytest.raises(G.PbrtError) as e:
                call(path_bufs(r, n, **bad))
            assert e.value.code == INVALID, what
    pb = path_bufs(r, n)
    qa = q()
    bad_calls = {
        "n beyond every buffer": lambda: r.path_step(pb, n + 1),
        "n beyond 2^31 - 1": lambda: r.path_step(pb, 2**31),
        "a short queue": lambda: r.path_step(pb, n, in_queue=q(m=n - 1)),
        "a queue index of the wrong type": lambda: r.path_step(pb, n, out_queue={"index": fake(r, n, np.uint32),
                                                                                 "count": fake(r, 1, np.uint32)}),
        "a queue count of the wrong type": lambda: r.path_step(pb, n, out_queue={"index": fake(r, n, np.int32),
                                                                                 "count": fake(r, 1, np.int32)}),
        "a queue without its count": lambda: r.path_step(pb, n, in_queue={"index": fake(r, n, np.int32)}),
        "another renderer's queue": lambda: r.path_step(pb, n, out_queue=q(other)),
        "aliased queues": lambda: r.path_step(pb, n, in_queue=qa, out_queue=qa),
        "queues sharing a count": lambda: r.path_step(pb, n, in_queue=qa, out_queue=dict(q(), count=qa["count"])),
        "a short step output": lambda: r.path_step(pb, n, step={"ar": fake(r, n - 1)}),
        "a step output of the wrong type": lambda: r.path_step(pb, n, step={"material": fake(r, n)}),
        "an unknown step output": lambda: r.path_step(pb, n, step={"beta": fake(r, n)}),
        "begin: a short ray array": lambda: r.path_begin(dict(rays, oz=fake(r, n - 1)), rng, n, pb),
        "begin: rng without inc": lambda: r.path_begin(rays, {"state": rng["state"]}, n, pb),
    }
    for what, call in bad_calls.items():
        with pytest.raises(G.PbrtError) as e:
            call()
        assert e.value.code == INVALID, what
    r._token.alive = False   # the renderer closes: every buffer it made is closed with it
    with pytest.raises(G.PbrtError):
        r.path_step(pb, n)


def test_go_shim_names_the_new_entry_points():
    """The new Go types and methods exist, and every C identifier they use is in the headers
    (tests/test_go_shim.py compiles the whole shim's identifiers; here: that the new ones are among them)."""
    src = open(os.path.join(REPO, "integration", "go", "pbrtgpu", "pbrtgpu.go")).read()
    for decl in ("func (r *Renderer) PathBeginDevice(", "func (r *Renderer) PathStepDevice(", "type DevicePaths struct",
                 "type DevicePathQueue struct", "type DevicePathStep struct"):
        assert decl in src, decl
    used = set(re.findall(r"\bC\.(pbrt_path\w*|pbrt_gpu_path\w*|PBRT_PATH_\w+)", src))
    assert used == {"pbrt_path_soa", "pbrt_path_queue", "pbrt_path_step_soa", "pbrt_gpu_path_begin_device",
                    "pbrt_gpu_path_step_device", "PBRT_PATH_UNUSED", "PBRT_PATH_ALIVE", "PBRT_PATH_ENDED",
                    "PBRT_PATH_PANICKED"}
    for name in used:
        assert re.search(r"\b%s\b" % name, HEADER), name
    body = src[src.index("func (r *Renderer) pathSoA("):src.index("func (r *Renderer) PathBeginDevice(")]
    assert set(re.findall(r"\bps\.(\w+)", body)) == set(PATH_FIELDS)   # every field of the state is set
    assert "r.devPtr(d, n, elem[k], k == 6)" in body   # each through devPtr; only tmax optional

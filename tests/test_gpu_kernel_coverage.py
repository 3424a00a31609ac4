"""Every compiled kernel runs under a bit-exact check, and the launch log proves it ran.

tests/kernel_cases.py maps each kernel of the manifest to one small case. Per
case, on one context: two frames (the second runs the learned schedule, where
the heavy/light split and the completion-driven path stage live); each frame's
film and paths_traced are the oracle's bit for bit, st.kernel is the expected
family, and the kernels the table assigns to the case are in the frames' launch
logs (Renderer.launches()); the kernels of a forced split must be in the learned
frame's. Every log read here is checked for the launch invariants of
tests/launch_checks.py (block size, positive grid, dynamic + static LDS within
the device's limit per workgroup).

The ray-query kernels and the mesh LBVH build run outside a frame; their
records are in the context's second log (launches(outside=True)), and the
queries' results are compared with the oracle's intersections.
"""
import functools
import os

import numpy as np
import pytest

import kernel_cases as K
import oracle_lib as O
import pbrtgpu as G
from launch_checks import assert_launched, check_invariants, names
from pbrtgpu import abi

pytestmark = pytest.mark.gpu

THREADS = max(1, min(int(os.environ.get("OMP_NUM_THREADS", "16") or 16), os.cpu_count() or 1))
KNOB_PREFIXES = ("PBRT_CI_", "PBRT_PATHS_", "PBRT_PW_", "PBRT_SP_", "PBRT_CULL_", "PBRT_GATE_", "PBRT_WAVE_BUFFER_")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def oracle_film(scene_key, rd_items):
    """The oracle's film of a (scene, render) pair: computed once, shared by the cases, never written to."""
    scene = K.SCENES[scene_key]()   # (owns the descriptor's arrays: alive until the oracle returns)
    rc, film, st = O.render(scene.desc, abi.render_desc(**dict(rd_items)), threads=THREADS)
    assert rc == 0
    film.setflags(write=False)
    return film, st.paths


def only_these_knobs(monkeypatch, env):
    """The case's knobs and no other (conftest's PBRT_CI_ORDER_CACHE=0 stays)."""
    for k in list(os.environ):
        if k.startswith(KNOB_PREFIXES) and k != "PBRT_CI_ORDER_CACHE":
            monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("name", list(K.CASES))
def test_case_launches_its_kernels(name, monkeypatch):
    case = K.CASES[name]
    only_these_knobs(monkeypatch, case.env)
    ofilm, opaths = oracle_film(case.scene, tuple(sorted(case.rd.items())))
    assert ofilm.max() > 0
    rd = K.make_rd(case)
    logs = []
    with G.Renderer(K.SCENES[case.scene](), **case.opts) as r:
        lds_max = r.lds_per_block()
        outside = r.launches(outside=True)
        check_invariants(outside, lds_max, r.launch_overflow)
        for frame in range(2):
            film, st = r.render(rd)
            assert st.kernel == case.family, (frame, st.kernel)
            assert st.paths_traced == opaths, (frame, st.paths_traced, opaths)
            assert np.array_equal(bits(film), bits(ofilm)), (frame, int((film != ofilm).sum()))
            log = r.launches()
            assert log and log[-1].name == "k_merge_film", (frame, sorted(names(log)))
            check_invariants(log, lds_max, r.launch_overflow)
            logs.append(log)
    assert_launched(logs[0] + logs[1], case.covers, name)
    assert_launched(logs[1], case.learned, name + " (learned frame)")
    assert_launched(outside, case.outside, name + " (outside a frame)")
    for k in case.learned:   # the split's light launch and the path chunks leave the main stream
        if k == "k_gate":
            assert {rec.stream for rec in logs[1] if rec.name == k} <= {2, 3}


def download(bufs, keys):
    return {k: bufs[k].download() for k in keys}


@pytest.mark.parametrize("name", list(K.QUERY_CASES))
def test_query_kernels(name, monkeypatch):
    """Camera rays, closest and any hits over device arrays (k_query_*), and the host-array
    batch (k_intersect): every result is the oracle's, and the log names the kMeshOnly choice."""
    scene_key, kernels = K.QUERY_CASES[name]
    only_these_knobs(monkeypatch, {})
    scene = K.SCENES[scene_key]()
    with G.Renderer(scene) as r:
        before = len(r.launches(outside=True))
        ph = r.primary_hits()
        n = ph["n"]
        occ = r.buffer(n, np.uint8)
        assert r.intersect_p_device(ph["rays"], n, occ) == 0
        rc, _ = r.query_status()
        assert rc == 0
        rays = download(ph["rays"], G.RAY_KEYS + ("tmax",))
        got = np.stack([ph["hits"][k].download().astype(np.float64) for k in G.HIT_DTYPES], axis=1)
        occluded = occ.download()
        packed = np.stack([rays[k] for k in G.RAY_KEYS + ("tmax",)], axis=1)
        rc, batch = r.intersect(packed)
        assert rc == 0
        staged = any(k.startswith("k_query_hit_staged") for k in kernels)
        if staged:   # the same queries on the LDS-staged walk (include/pbrt_diag.h)
            shits = {k: r.buffer(n, dt) for k, dt in G.HIT_DTYPES.items()}
            socc = r.buffer(n, np.uint8)
            assert r.intersect_device(ph["rays"], n, shits, staged=True) == 0
            assert r.intersect_p_device(ph["rays"], n, socc, staged=True) == 0
            assert r.query_status()[0] == 0
            sgot = np.stack([shits[k].download().astype(np.float64) for k in G.HIT_DTYPES], axis=1)
            soccluded = socc.download()
        else:   # a mesh: the staged entry refuses
            assert r.intersect_p_device(ph["rays"], n, occ, staged=True) == abi.PBRT_E_INVALID
        log = r.launches(outside=True)[before:]
        check_invariants(log, r.lds_per_block(), r.launch_overflow)
    want = O.intersect(scene.desc, packed, closest=True)   # rows of hit, t_max, prim, p, n
    want_any = O.intersect(scene.desc, packed, closest=False)
    assert 0 < want[:, 0].sum() and want.shape == (n, 9)
    assert np.array_equal(bits(got), bits(want)), int((got != want).sum())
    assert np.array_equal(bits(batch), bits(want)), int((batch != want).sum())
    assert np.array_equal(occluded.astype(np.float64), want_any)
    if staged:
        assert np.array_equal(bits(sgot), bits(want)), int((sgot != want).sum())
        assert np.array_equal(soccluded.astype(np.float64), want_any)
    assert_launched(log, set(kernels) | {"k_query_camera", "k_intersect"}, name)
    mesh_only = scene.desc.n_prims == 0
    other = "false" if mesh_only else "true"
    assert not {k for k in names(log) if k.startswith("k_query_hit") and k.endswith(f", {other}>")}, sorted(names(log))

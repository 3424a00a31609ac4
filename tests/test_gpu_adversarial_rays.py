"""Every BVH walk on rays aimed at its decision boundaries, against the oracle bit for bit.

The scenes and ray families are tests/adversarial_rays.py's (checked on the oracle
alone by tests/test_adversarial_rays_host.py). Per scene and family:

- the [64]-stack walk: intersect_device (all nine outputs) and intersect_p_device
  (k_query_hit), on edge_large also the host-array pbrt_gpu_intersect (k_intersect);
- the LDS-staged walks on edge_small(1) and edge_small(4) (several primitives in a
  leaf), through the diagnostic entry of include/pbrt_diag.h (k_query_hit_staged):
  with the default knobs (culling groups), with PBRT_CULL_GROUPS=0 (the plain
  leaf-preorder scan) and with PBRT_CULL_GROUP=2. Each equals the oracle, and the
  stack walk's result bit for bit in every element that is not NaN on both sides:
  "interior nodes decide nothing" (csrc/pbrt_path.h) on rays with zero direction
  components and origins on box planes.

Comparison rule. Rows on which the reference does not panic match on the uint64
view, except that where the oracle's element is NaN the device's must be NaN
(payload and sign are not compared: the default NaN of 0/0 differs between host and
device and Go does not specify it). A panicking row reads as a miss with the ray's own
TMax, and status() is (PBRT_E_REF_PANIC, count, first, kind) of the oracle's panics.
"""
import os

import numpy as np
import pytest

import adversarial_rays as A
import pbrtgpu as G
from pbrtgpu import abi
from test_gpu_query import CLEAN, SENTINEL, any_hit, bits, closest, head, hit_buffers, padded, rows, status, upload_rays

pytestmark = pytest.mark.gpu

KNOB_PREFIXES = ("PBRT_CI_", "PBRT_PATHS_", "PBRT_PW_", "PBRT_SP_", "PBRT_CULL_", "PBRT_GATE_", "PBRT_WAVE_BUFFER_")
FAMILIES = list(A.FAMILIES)
# the staged walks: environment, and whether the context must have culling groups
STAGED = {"groups": ({}, True), "no_groups": ({"PBRT_CULL_GROUPS": "0"}, False), "group2": ({"PBRT_CULL_GROUP": "2"}, True)}
SIZES = (1, 63, 65, 257)   # ragged waves and blocks, on the head of a family


def knobs(monkeypatch, **env):
    """These knobs and no other (conftest's PBRT_CI_ORDER_CACHE=0 stays), set before the context is created."""
    for k in list(os.environ):
        if k.startswith(KNOB_PREFIXES) and k != "PBRT_CI_ORDER_CACHE":
            monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def staged_closest(r, rays):
    n = rays.shape[0]
    rb, hb = upload_rays(r, rays), hit_buffers(r, n)
    assert r.intersect_device(rb, n, hb, staged=True) == 0
    return rows(hb, n)


def staged_any(r, rays):
    n = rays.shape[0]
    rb, occ = upload_rays(r, rays), padded(r, n, np.uint8)
    assert r.intersect_p_device(rb, n, occ, staged=True) == 0
    return head(occ, n)


def expected_status(want):
    pan = A.panicked(want)
    if not pan.any():
        return CLEAN
    return (abi.PBRT_E_REF_PANIC, int(pan.sum()), int(np.argmax(pan)), abi.PBRT_PANIC_EFLOAT)


def same_as_oracle(got, occ, want, wocc, rays, what):
    """The comparison rule of the module docstring; returns (rays, panics, NaN-class elements)."""
    n = rays.shape[0]
    assert got.shape == (n, 9) and occ.shape == (n,)
    pan = A.panicked(want)
    miss = np.concatenate([np.zeros((n, 1)), rays[:, 6:7], np.full((n, 1), -1.0), np.zeros((n, 6))], axis=1)
    exp = np.where(pan[:, None], miss, want)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), (what, int((np.isnan(got) != nan).sum()))
    differ = (bits(got) != bits(exp)) & ~nan
    assert not differ.any(), (what, int(differ.any(axis=1).sum()), np.flatnonzero(differ.any(axis=1))[:5],
                              rays[differ.any(axis=1)][:2], got[differ.any(axis=1)][:2], exp[differ.any(axis=1)][:2])
    assert set(np.unique(occ)) <= {0, 1}
    assert (occ[pan] == 0).all() and np.array_equal(occ[~pan] == 1, wocc[~pan] == 1), what
    return n, int(pan.sum()), int(nan.sum())


def same_where_not_nan(a, b, what):
    """Two walks' rows: bit for bit in every element that is not NaN on both sides."""
    both_nan = np.isnan(a) & np.isnan(b)
    differ = (bits(a) != bits(b)) & ~both_nan
    assert not differ.any(), (what, int(differ.any(axis=1).sum()))


def check_family(r, key, family, staged, n=None):
    """One family (its first n rays) on one context: the stack walk, and with `staged` the
    staged walk too, each against the oracle and its status against the oracle's panics."""
    rays, (want, wocc) = A.rays(key, family), A.oracle(key, family)
    if n is not None:
        rays, want, wocc = rays[:n], want[:n], wocc[:n]
    what = f"{key} {family}"
    got = closest(r, rays)
    assert status(r) == expected_status(want), what
    occ = any_hit(r, rays)
    assert status(r) == expected_status(want), what
    figures = same_as_oracle(got, occ, want, wocc, rays, what + " stack")
    if staged:
        sgot = staged_closest(r, rays)
        assert status(r) == expected_status(want), what
        socc = staged_any(r, rays)
        assert status(r) == expected_status(want), what
        assert same_as_oracle(sgot, socc, want, wocc, rays, what + " staged") == figures
        same_where_not_nan(sgot, got, what + " staged against stack")
        assert np.array_equal(socc, occ), what
    print(f"{what}: {figures[0]} rays, {figures[1]} panics, {figures[2]} NaN-class elements"
          f"{' (stack and staged)' if staged else ' (stack)'}")
    return got


def query_kernels(r, before):
    return {rec.name for rec in r.launches(outside=True)[before:] if rec.name.startswith(("k_query_hit", "k_intersect"))}


# ------------------------------------------------------------- the stack walk
@pytest.mark.parametrize("key", list(A.SCENES))
def test_stack_walk(key, monkeypatch):
    """k_query_hit reads the nodes from memory: the [64]-stack branch on all three trees."""
    knobs(monkeypatch)
    scene = A.SCENES[key]()
    with G.Renderer(scene) as r:
        assert status(r) == CLEAN
        before = len(r.launches(outside=True))
        for family in FAMILIES:
            got = check_family(r, key, family, staged=False)
            if key == "large":   # the host-array batch: k_intersect
                rays, (want, _) = A.rays(key, family), A.oracle(key, family)
                rc, host = r.intersect(rays)
                assert rc == (abi.PBRT_E_REF_PANIC if A.panicked(want).any() else 0), family
                pan = A.panicked(want)   # (a panicking row: hit 0, its other outputs are not written)
                same_where_not_nan(host[~pan], got[~pan], f"{key} {family} host-array batch")
                assert np.array_equal(np.isnan(host[~pan]), np.isnan(got[~pan])) and (host[pan, 0] == 0).all(), family
        kernels = query_kernels(r, before)
    assert kernels == {"k_query_hit<false, false>", "k_query_hit<true, false>"} | ({"k_intersect"} if key == "large" else set())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("key", list(A.SCENES))
def test_ragged_sizes(key, n, monkeypatch):
    """The head of every family at sizes that end inside a wave and inside a block."""
    knobs(monkeypatch)
    with G.Renderer(A.SCENES[key]()) as r:
        for family in FAMILIES:
            check_family(r, key, family, staged=(key != "large"), n=n)


# ---------------------------------------------------------- the staged walks
@pytest.mark.parametrize("walk", list(STAGED))
@pytest.mark.parametrize("key", ["small1", "small4"])
def test_staged_walks(key, walk, monkeypatch):
    env, grouped = STAGED[walk]
    knobs(monkeypatch, **env)
    with G.Renderer(A.SCENES[key]()) as r:
        groups = r.cull_groups()
        print(f"{key} {walk}: {groups} culling groups")
        assert (groups > 0) == grouped and groups <= 16
        before = len(r.launches(outside=True))
        for family in FAMILIES:
            check_family(r, key, family, staged=True)
        assert {"k_query_hit_staged<false>", "k_query_hit_staged<true>"} <= query_kernels(r, before)
        for rec in r.launches(outside=True)[before:]:
            if rec.name.startswith("k_query_hit"):
                assert rec.block == (256, 1, 1) and rec.lds + rec.lds_static <= r.lds_per_block()


def test_group_size_changes_the_groups(monkeypatch):
    """PBRT_CULL_GROUP=2 reaches the context: more, smaller groups than the default 4 leaves."""
    counts = {}
    for walk in ("groups", "group2"):
        knobs(monkeypatch, **STAGED[walk][0])
        with G.Renderer(A.SCENES["small1"]()) as r:
            counts[walk] = r.cull_groups()
    assert 0 < counts["groups"] < counts["group2"], counts


def test_staged_entry_refuses_what_is_not_staged(monkeypatch):
    knobs(monkeypatch)
    rays = A.rays("large", "random")[:65]
    for scene in (A.SCENES["large"](), G.Scene.heightfield(48, 32, quads=8, seed=1, spheres=True)):
        with G.Renderer(scene) as r:
            rb, hb = upload_rays(r, rays), hit_buffers(r, 65)
            assert r.intersect_device(rb, 65, hb, staged=True) == abi.PBRT_E_INVALID
            assert r.intersect_p_device(rb, 65, hb["hit"], staged=True) == abi.PBRT_E_INVALID
            assert status(r) == CLEAN
            for k, b in hb.items():   # nothing was enqueued
                assert (b.download() == SENTINEL[b.dtype]).all(), k

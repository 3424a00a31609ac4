"""Trees beyond 64 BVH nodes on the routes that took only LDS-staged trees, against
the oracle on the uint64 view of the fp64 film.

- Mirror / Glass / OrenNayar in EXACT mode (AUTO): k_chain_ci<kW, 64, true, ...>, the
  kX chain with the reference's [64] traversal stack, then the kX path wavefront,
  where the serial kernel ran before;
- the camera-start route (kernel="wave_cam"): k_chain_cam_stack (THROUGHPUT:
  k_cam_setup) and k_paths_cam_stack<P, kMB>, where the route refused the render.

The renders are tests/large_trees.py's RENDERS (crowd(): 121 nodes), each checked
on the host by tests/test_large_trees_host.py; the oracle's film of a render is
computed once. Every context is created with the knobs cleared and renders the
cold frame and the learned one; every comparison covers the film's bits,
paths_traced, rays_closest and rays_shadow (camera_samples too on the camera-start
route); every log read goes through launch_checks.check_invariants.
"""
import os

import numpy as np
import pytest

import large_trees as T
import pbrtgpu as G
from launch_checks import assert_launched, chain, check_invariants, names
from pbrtgpu import abi

pytestmark = pytest.mark.gpu

CI, CAM, SERIAL = abi.PBRT_KERNEL_WAVE_CI, abi.PBRT_KERNEL_WAVE_CAM, abi.PBRT_KERNEL_SERIAL
KNOB_PREFIXES = ("PBRT_CI_", "PBRT_PATHS_", "PBRT_PW_", "PBRT_SP_", "PBRT_CULL_", "PBRT_GATE_", "PBRT_WAVE_BUFFER_")
PW_KX = ("k_pw_cache<true>", "k_pw_start<false, true>", "k_pw_trace<false>", "k_pw_shade<true>", "k_pw_shadow<false>")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def knobs(monkeypatch, **env):
    """These knobs and no other (conftest's PBRT_CI_ORDER_CACHE=0 stays)."""
    for k in list(os.environ):
        if k.startswith(KNOB_PREFIXES) and k != "PBRT_CI_ORDER_CACHE":
            monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def chains(log):
    return {k for k in names(log) if k.startswith("k_chain_ci<")}


def panic_site(st):
    return (st.panic_kind, st.panic_tile, st.panic_pixel_x, st.panic_pixel_y, st.panic_sample, st.panic_bounce)


def same_as_oracle(name, film, st, cam=False):
    rc, ofilm, ost = T.oracle(name)
    assert rc == 0
    assert np.array_equal(bits(film), bits(ofilm)), (name, int((film != ofilm).sum()))
    assert (st.paths_traced, st.rays_closest, st.rays_shadow) == (ost.paths, ost.closest_rays, ost.shadow_rays), name
    if cam:
        assert st.camera_samples == ost.camera_samples, name


def oracle_site(name):
    rc, _, ost = T.oracle(name)
    assert rc == abi.PBRT_E_REF_PANIC
    return (ost.panic_kind, ost.panic_tile, ost.panic_px, ost.panic_py, ost.panic_sample, ost.panic_bounce)


def checked_log(r):
    log = r.launches()
    check_invariants(log, r.lds_per_block(), r.launch_overflow)
    for rec in log:   # (launch_checks.ONE_WAVE does not know the stack kernels' names)
        if rec.name.startswith(("k_chain_cam_stack", "k_paths_cam_stack")):
            assert rec.block == (64, 1, 1), rec
    return log


def frames(name, family, n=2, cam=False, **opts):
    """n frames of RENDERS[name] on one context (the cold frame, then the learned one), each the
    oracle's; returns the frames' checked launch logs."""
    logs = []
    rd = T.make_rd(name)
    with G.Renderer(T.RENDERS[name].scene(), **opts) as r:
        for frame in range(n):
            film, st = r.render(rd)
            assert st.kernel == family, (name, frame, st.kernel)
            same_as_oracle(name, film, st, cam)
            logs.append(checked_log(r))
    return logs


def panics_at_the_oracles_site(name, family, **opts):
    with G.Renderer(T.RENDERS[name].scene(), **opts) as r:
        for frame in range(2):
            with pytest.raises(G.PbrtError) as ei:
                r.render(T.make_rd(name))
            assert ei.value.code == abi.PBRT_E_REF_PANIC and ei.value.stats.kernel == family
            assert panic_site(ei.value.stats) == oracle_site(name), frame
            yield checked_log(r)


# ------------------------------------------------------------ A. the kX chain
# all three wave counts on kx_exact, kx_exact_glass and kx_exact_mesh, one (in turn) on the rest
A_ALL_WAVES = ("kx_exact", "kx_exact_glass", "kx_exact_mesh")
A_CASES = [(n, w) for n in A_ALL_WAVES for w in (1, 2, 4)] + \
          [(n, (1, 2, 4)[i % 3]) for i, n in enumerate(x for x in T.A_RENDERS if x not in A_ALL_WAVES)]


@pytest.mark.parametrize("name,w", A_CASES)
def test_kx_exact_beyond_64_nodes(name, w, monkeypatch):
    knobs(monkeypatch, PBRT_CI_WAVES=str(w))
    logs = frames(name, CI)
    for frame, log in enumerate(logs):
        assert chain(w, 64, kx=True, multi=(w == 1)) in chains(log), (name, frame, chains(log))
        assert all(", 64, true, " in k for k in chains(log)), chains(log)   # no LDS-staged or Matte chain
        assert_launched(log, PW_KX + ("k_wf_primary<true>",), name)
        assert not [k for k in names(log) if k.startswith("k_paths_ci")]
    assert "k_tile_cost<true>" in names(logs[0])   # the cold frame probes


def test_every_a_render_is_run():
    assert {n for n, _ in A_CASES} == set(T.A_RENDERS)
    assert {w for n, w in A_CASES if n not in A_ALL_WAVES} == {1, 2, 4}


def test_kx_exact_two_tiles_per_wave(monkeypatch):
    knobs(monkeypatch)
    for log in frames("kx_exact", CI, lanes_per_wave=2):
        assert chains(log) == {chain(1, 64, kx=True, multi=True)}


def test_kx_exact_serial_gives_the_same_bits(monkeypatch):
    knobs(monkeypatch)
    for log in frames("kx_exact", SERIAL, kernel="serial"):
        assert_launched(log, ("k_render_exact<1>",))
        assert not chains(log)


@pytest.mark.parametrize("w", [1, 4])
def test_kx_exact_panic_site(w, monkeypatch):
    knobs(monkeypatch, PBRT_CI_WAVES=str(w))
    for log in panics_at_the_oracles_site("kx_exact_bright", CI, kernel="wave_ci"):
        assert chain(w, 64, kx=True, multi=(w == 1)) in chains(log)
        assert_launched(log, PW_KX)


# ----------------------------------------------------- B. the camera-start route
CAM_PATHS = {"cam_nodes": "k_paths_cam_stack<64, false>", "cam_nodes_s33": "k_paths_cam_stack<16, false>",
             "cam_nodes_random5": "k_paths_cam_stack<64, false>", "cam_nodes_lens": "k_paths_cam_stack<64, false>",
             "cam_nodes_tp": "k_paths_cam_stack<64, true>", "cam_nodes_l20": "k_paths_cam_stack<64, false>",
             "cam_nodes_s66": "k_paths_cam_stack<4, false>"}


def cam_kernels(log):
    return {k for k in names(log) if k.startswith(("k_chain_cam", "k_paths_cam", "k_cam_setup"))}


@pytest.mark.parametrize("name", T.B_RENDERS)
def test_cam_beyond_64_nodes(name, monkeypatch):
    knobs(monkeypatch)
    for log in frames(name, CAM, cam=True, kernel="wave_cam"):
        # the stack kernels, and none of the small-tree k_chain_cam / k_paths_cam<...>
        assert cam_kernels(log) == {"k_cam_setup" if name.endswith("_tp") else "k_chain_cam_stack", CAM_PATHS[name]}, name


def test_every_b_render_is_run():
    assert set(CAM_PATHS) == set(T.B_RENDERS)


def test_cam_panic_site(monkeypatch):
    knobs(monkeypatch)
    for log in panics_at_the_oracles_site("cam_nodes_bright", CAM, kernel="wave_cam"):
        assert cam_kernels(log) == {"k_chain_cam_stack", "k_paths_cam_stack<64, false>"}


# ------------------------------------------------- small scenes, unchanged
def test_small_scenes_keep_their_kernels(monkeypatch):
    knobs(monkeypatch)
    with G.Renderer(G.Scene.readme(45, 30), kernel="wave_cam") as r:
        r.render(T.make_rd("cam_nodes"))
        assert cam_kernels(checked_log(r)) == {"k_chain_cam", "k_paths_cam<64, false>"}
    with G.Renderer(G.Scene.readme_glass(48, 32)) as r:
        _, st = r.render(T.make_rd("kx_exact"))
        log = checked_log(r)
        assert st.kernel == CI and chains(log) and all(", 0, true, " in k for k in chains(log)), chains(log)

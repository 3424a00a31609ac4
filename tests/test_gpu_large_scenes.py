"""Scenes beyond 16 lights, and Mirror / Glass / OrenNayar beyond 64 BVH nodes in
THROUGHPUT mode, on the wave routes, against the oracle on the uint64 view of the
fp64 film.

- 17 to 64 lights: the wave pipeline with the path wavefront, whose bounce-1
  estimates live in global arrays of n_lights per pixel (k_paths_ci's LDS
  cache holds 16), where the serial kernel ran before; Matte and kX, EXACT and
  THROUGHPUT, LDS-staged and larger trees;
- the camera-start route (kernel="wave_cam") with 20 and 64 lights, which it refused;
- Mirror / Glass / OrenNayar on a 121-node tree in THROUGHPUT mode: k_mb_setup<true>
  and the kX path wavefront (no chain), where the serial kernel ran before.

The scenes and renders are tests/large_scenes.py's RENDERS, each checked on the
host by tests/test_large_scenes_host.py; the oracle's film of a render is
computed once. Every comparison covers the film's bits, paths_traced,
rays_closest and rays_shadow (camera_samples too on the camera-start route);
every log read goes through launch_checks.check_invariants.
"""
import os
import re

import numpy as np
import pytest

import large_scenes as L
import pbrtgpu as G
from launch_checks import assert_launched, chain, check_invariants, names
from pbrtgpu import abi

pytestmark = pytest.mark.gpu

CI, WAVE, CAM, SERIAL = (abi.PBRT_KERNEL_WAVE_CI, abi.PBRT_KERNEL_WAVE, abi.PBRT_KERNEL_WAVE_CAM,
                         abi.PBRT_KERNEL_SERIAL)
KNOB_PREFIXES = ("PBRT_CI_", "PBRT_PATHS_", "PBRT_PW_", "PBRT_SP_", "PBRT_CULL_", "PBRT_GATE_", "PBRT_WAVE_BUFFER_")
PW_KX = ("k_pw_cache<true>", "k_pw_start<false, true>", "k_pw_trace<false>", "k_pw_shade<true>", "k_pw_shadow<false>")
PW_MATTE = ("k_pw_cache<false>", "k_pw_start<false, false>", "k_pw_trace<false>", "k_pw_shade<false>",
            "k_pw_shadow<false>")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def knobs(monkeypatch, **env):
    """These knobs and no other (conftest's PBRT_CI_ORDER_CACHE=0 stays)."""
    for k in list(os.environ):
        if k.startswith(KNOB_PREFIXES) and k != "PBRT_CI_ORDER_CACHE":
            monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def same_as_oracle(name, film, st, cam=False):
    rc, ofilm, ost = L.oracle(name)
    assert rc == 0
    assert np.array_equal(bits(film), bits(ofilm)), (name, int((film != ofilm).sum()))
    assert (st.paths_traced, st.rays_closest, st.rays_shadow) == (ost.paths, ost.closest_rays, ost.shadow_rays), name
    if cam:
        assert st.camera_samples == ost.camera_samples, name


def frames(name, family, n=2, cam=False, **opts):
    """n frames of RENDERS[name] on one context (the cold frame, then the learned one), each the
    oracle's; returns the frames' checked launch logs."""
    logs = []
    rd = L.make_rd(name)
    with G.Renderer(L.RENDERS[name].scene(), **opts) as r:
        lds_max = r.lds_per_block()
        for frame in range(n):
            film, st = r.render(rd)
            assert family is None or st.kernel == family, (name, frame, st.kernel)
            same_as_oracle(name, film, st, cam)
            log = r.launches()
            check_invariants(log, lds_max, r.launch_overflow)
            logs.append(log)
    return logs


def chains(log):
    return {k for k in names(log) if k.startswith("k_chain_ci<")}


# ---------------------------------------------------------- 1. kX, THROUGHPUT
@pytest.mark.parametrize("name", ["kx_tp", "kx_tp_s33_d12", "kx_l20_tp"])
def test_kx_throughput_beyond_64_nodes(name, monkeypatch):
    knobs(monkeypatch)
    for log in frames(name, WAVE):
        assert_launched(log, ("k_mb_setup<true>", "k_pw_cache<true>", "k_pw_start<true, true>", "k_pw_trace<false>",
                              "k_pw_shade<true>", "k_pw_shadow<false>"), name)
        assert not chains(log) and not [k for k in names(log) if k.startswith("k_paths_ci")]


def test_kx_throughput_serial_gives_the_same_bits(monkeypatch):
    knobs(monkeypatch)
    (log,) = frames("kx_tp", SERIAL, n=1, kernel="serial")
    assert_launched(log, ("k_render_exact<1>",))


# ------------------------------------------------------------------ 2. lights
@pytest.mark.parametrize("name", ["matte_l17", "matte_l20", "matte_l64", "readme_l20", "kx_small_l20"])
def test_more_than_16_lights(name, monkeypatch):
    knobs(monkeypatch)
    for log in frames(name, CI):
        assert chains(log)
        assert_launched(log, PW_KX if name == "kx_small_l20" else PW_MATTE, name)
        assert not [k for k in names(log) if k.startswith("k_paths_ci")]


def test_more_than_16_lights_throughput(monkeypatch):
    knobs(monkeypatch)
    for log in frames("matte_l20_tp", WAVE):
        assert_launched(log, ("k_mb_setup<false>", "k_pw_cache<false>", "k_pw_start<true, false>"))
        assert not chains(log) and not [k for k in names(log) if k.startswith("k_paths_ci")]


def test_forced_paths_ci_with_more_than_16_lights(monkeypatch):
    """PBRT_PATHS_CI=2 would fit 2 * 20 light lanes in a wave, but PixelCache::ld[] holds 16:
    the wavefront still runs the paths"""
    knobs(monkeypatch, PBRT_PATHS_CI="2")
    for log in frames("readme_l20", CI):
        assert_launched(log, PW_MATTE)
        assert not [k for k in names(log) if k.startswith("k_paths_ci")]


def test_16_lights_as_before(monkeypatch):
    """(whatever kernels it took before: only the bits are pinned)"""
    knobs(monkeypatch)
    frames("matte_l16", None)


# ------------------------------------------------------------------- 3. panic
def panic_site(st):
    return (st.panic_kind, st.panic_tile, st.panic_pixel_x, st.panic_pixel_y, st.panic_sample, st.panic_bounce)


def oracle_site(name):
    rc, _, ost = L.oracle(name)
    assert rc == abi.PBRT_E_REF_PANIC
    return (ost.panic_kind, ost.panic_tile, ost.panic_px, ost.panic_py, ost.panic_sample, ost.panic_bounce)


@pytest.mark.parametrize("waves", ["1", "4"])
def test_panic_site_with_20_lights(waves, monkeypatch):
    knobs(monkeypatch, PBRT_CI_WAVES=waves)
    with G.Renderer(L.RENDERS["bright_l20"].scene(), kernel="wave_ci") as r:
        for frame in range(2):
            with pytest.raises(G.PbrtError) as ei:
                r.render(L.make_rd("bright_l20"))
            assert ei.value.code == abi.PBRT_E_REF_PANIC and ei.value.stats.kernel == CI
            assert panic_site(ei.value.stats) == oracle_site("bright_l20"), frame
            check_invariants(r.launches(), r.lds_per_block(), r.launch_overflow)
            assert_launched(r.launches(), PW_MATTE)


# ------------------------------------------------------------ 4. camera-start
CAM_PATHS = {"cam_l20": "k_paths_cam<64, false>", "cam_l20_s33": "k_paths_cam<16, false>",
             "cam_l20_random5": "k_paths_cam<64, false>", "cam_l20_tp": "k_paths_cam<64, true>",
             "cam_l64": "k_paths_cam<64, false>"}


@pytest.mark.parametrize("name", sorted(CAM_PATHS))
def test_cam_with_more_than_16_lights(name, monkeypatch):
    knobs(monkeypatch)
    for log in frames(name, CAM, cam=True, kernel="wave_cam"):
        assert_launched(log, ("k_cam_setup" if name.endswith("_tp") else "k_chain_cam", CAM_PATHS[name]), name)


# ------------------------------------------------- 5. small scenes, unchanged
def test_small_scenes_keep_their_kernels(monkeypatch):
    knobs(monkeypatch, PBRT_CI_WAVES="1")
    for log in frames("small_kx", CI):
        assert chains(log) == {chain(1, kx=True, multi=True)}
        assert_launched(log, ("k_paths_ci<8, false, true>",))
        assert not [k for k in names(log) if k.startswith("k_pw_")]
    for log in frames("small_readme", CI):
        # (the learned frame may add the heavy tiles' 4-wave launch: still kDepth 0, Matte)
        assert chains(log) and all(re.fullmatch(chain("[14]", eu=None), k) for k in chains(log)), chains(log)
        assert_launched(log, ("k_paths_ci<8, false, false>",))
        assert not [k for k in names(log) if k.startswith("k_pw_")]
    knobs(monkeypatch)
    with G.Renderer(G.Scene.readme(45, 30), kernel="wave_cam") as r:
        r.render(L.make_rd("cam_l20"))
        cam = {k for k in names(r.launches()) if k.startswith(("k_chain_cam", "k_paths_cam"))}
        assert cam == {"k_chain_cam", "k_paths_cam<64, false>"}

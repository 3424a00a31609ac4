"""k_chain_ci keeps the state every lane of a workgroup shares in scalar registers.

The one-tile-per-workgroup instantiations read the tile's CiGroup, slot, PCG32
stream and pixel record as wave-uniform values (readfirstlane); the
several-tiles-per-wave ones (kMulti, opts.lanes_per_wave = 2 or 4) keep them per
lane, because there the lanes of a wave hold different groups. A uniform read
that leaked into the wrong variant, or sat where the lanes disagree, would
broadcast one group's state to the others: the shapes below are the smallest at
which the groups of a wave differ (tiles of different pixel counts, empty groups
in the last wave, groups in different phases).

Every film is the oracle's, bit for bit, on two consecutive frames of one
context: the first launches in probe order, the second in the learned order
(order[] non-null). No tolerance anywhere: the films are deterministic.
"""
import functools
import os

import numpy as np
import pytest

import oracle_lib as O
import pbrtgpu as G
from launch_checks import assert_chain, chain, check_invariants
from pbrtgpu import abi

pytestmark = pytest.mark.gpu

THREADS = max(1, min(int(os.environ.get("OMP_NUM_THREADS", "16") or 16), os.cpu_count() or 1))

SCENES = {
    "readme45x30": lambda: G.Scene.readme(45, 30),   # 6 tiles of 16 px, ragged: 256, 208, 224 and 182 pixels
    "readme80x48": lambda: G.Scene.readme(80, 48),   # 15 tiles: a multiple of neither 2 nor 4
    "readme16x16": lambda: G.Scene.readme(16, 16),   # one tile
    "glass48x32": lambda: G.Scene.readme_glass(48, 32),
    "mesh48x32": lambda: G.Scene.heightfield(48, 32, quads=8, seed=1),
}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def oracle_film(scene_key, rd_items):
    """The oracle's film of a (scene, render) pair: computed once, shared by the cases, never written to."""
    scene = SCENES[scene_key]()
    rc, film, st = O.render(scene.desc, abi.render_desc(**dict(rd_items)), threads=THREADS)
    assert rc == 0
    film.setflags(write=False)
    return film, st.paths


def check_two_frames(scene_key, lanes_per_wave=0, expect=None, **rd_kw):
    """expect: the k_chain_ci instantiation the case names (launch_checks.chain), asserted
    against the two frames' launch logs."""
    ofilm, opaths = oracle_film(scene_key, tuple(sorted(rd_kw.items())))
    assert ofilm.max() > 0
    rd = abi.render_desc(**rd_kw)
    log = []
    with G.Renderer(SCENES[scene_key](), lanes_per_wave=lanes_per_wave) as r:
        for frame in range(2):
            film, st = r.render(rd)
            assert st.kernel == abi.PBRT_KERNEL_WAVE_CI, (frame, st.kernel)
            assert st.paths_traced == opaths, (frame, st.paths_traced, opaths)
            assert np.array_equal(bits(film), bits(ofilm)), (frame, int((film != ofilm).sum()))
            log += r.launches()
            check_invariants(log, r.lds_per_block(), r.launch_overflow)
    if expect is not None:
        assert_chain(log, expect, scene_key)


@pytest.mark.parametrize("spp", [2, 4])
@pytest.mark.parametrize("eu", ["3", "2"])
def test_one_tile_per_wave(eu, spp, monkeypatch):
    """The one-wave instantiations, at the 3- and the 2-waves/SIMD build."""
    monkeypatch.setenv("PBRT_CI_WAVES", "1")
    monkeypatch.setenv("PBRT_CI_EU", eu)
    check_two_frames("readme45x30", expect=chain(1, eu=0 if eu == "3" else 2), spp_x=spp, spp_y=spp)


@pytest.mark.parametrize("scene_key", ["readme80x48", "readme45x30"])
@pytest.mark.parametrize("lpw", [2, 4])
def test_several_tiles_per_wave(lpw, scene_key):
    """kMulti: groups of one wave in different pixels and phases, of different
    pixel counts, and (80x48: 15 tiles) empty groups in the last wave."""
    check_two_frames(scene_key, lanes_per_wave=lpw, expect=chain(1, eu=None, multi=True), spp_x=2, spp_y=2)


@pytest.mark.parametrize("nps", ["default", "0"])
@pytest.mark.parametrize("waves", ["2", "4", "8"])
def test_multi_wave_tiles(waves, nps, monkeypatch):
    """One tile per workgroup of 2, 4, 8 waves, with and without next-pixel speculation."""
    monkeypatch.setenv("PBRT_CI_WAVES", waves)
    if nps != "default":
        monkeypatch.setenv("PBRT_CI_NPS", nps)
    check_two_frames("readme45x30", expect=chain(int(waves)), spp_x=4, spp_y=4)


def test_windowed_start_pixel():
    """The kSpWin instantiation: 121 spp without jitter on a one-tile image."""
    check_two_frames("readme16x16", expect=chain(4, spwin=True), spp_x=11, spp_y=11, jitter=False)   # 1 tile: 4 waves


@pytest.mark.parametrize("waves", ["1", "2", "4"])
def test_kx(waves, monkeypatch):
    """kX: per-lane state in the one-wave kernel, scalar in the multi-wave ones
    (6 tiles run 4 waves each by default)."""
    monkeypatch.setenv("PBRT_CI_WAVES", waves)
    check_two_frames("glass48x32", expect=chain(int(waves), kx=True, multi=waves == "1"), spp_x=2, spp_y=2)


@pytest.mark.parametrize("waves", ["1", "4"])
def test_mesh(waves, monkeypatch):
    monkeypatch.setenv("PBRT_CI_WAVES", waves)
    check_two_frames("mesh48x32", expect=chain(int(waves), -1), spp_x=2, spp_y=2)


def panic_scene():
    """The existing panic tests' scene (test_gpu_parity.py): a point light so
    bright that UniformSampleOneLight panics on the first lit hit."""
    s = G.Scene()
    chk = s.add_matte((0.8, 0.8, 0.8))
    d = s.add_disk(G.mul(G.translate(0, 0, 0), G.rotate(0, 90)), 0.0, 100.0)
    s.add_primitive(d, chk)
    s.add_point_light(G.translate(0, 5, 0), (1e5, 1e5, 1e5))
    s.set_film(32, 32)
    s.set_camera(G.look_at((0, 20, 20), (0, 0, 0), (0, 1, 0)), fov=60)
    return s.build()


@pytest.mark.parametrize("waves", ["1", "4"])
def test_panic_report_unchanged(waves, monkeypatch):
    monkeypatch.setenv("PBRT_CI_WAVES", waves)
    scene = panic_scene()
    rd = abi.render_desc(2, 2)
    rc, _, ost = O.render(scene.desc, rd, threads=1)
    assert rc == abi.PBRT_E_REF_PANIC
    with G.Renderer(scene, kernel="wave_ci") as r:
        for frame in range(2):
            with pytest.raises(G.PbrtError) as ei:
                r.render(rd)
            st = ei.value.stats
            assert ei.value.code == abi.PBRT_E_REF_PANIC and st.kernel == abi.PBRT_KERNEL_WAVE_CI
            assert (st.panic_kind, st.panic_tile, st.panic_pixel_x, st.panic_pixel_y, st.panic_sample,
                    st.panic_bounce) == (ost.panic_kind, ost.panic_tile, ost.panic_px, ost.panic_py,
                                         ost.panic_sample, ost.panic_bounce), frame

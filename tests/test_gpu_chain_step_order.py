"""k_chain_ci runs one scatter per step, for new and for continuing lanes alike.

A step of the chain kernel is: traversal of the live trajectories, the leader's
walk through the ring, the drop of candidates the chain has passed, StartPixel,
the issue of offsets to idle lanes, and then ONE scatter block that serves both
the lanes just issued (interaction and BSDF of the pixel's bounce 1) and the
lanes whose traversal found a hit (prim_si + compute_bsdf first). A trajectory
that ends inside the scatter is therefore seen by the next step's walk, and a
candidate the walk has passed is dropped with its hit still unprocessed. The
cases below are the smallest renders in which a step has only one of the two
lane sets, every walk ends a pixel, in-flight hits are dropped at every pixel,
and trajectories end inside the scatter by depth, by a black sample or by
Russian roulette, in every instantiation of the kernel. (The mesh-only and the
windowed-StartPixel instantiations keep the earlier order, issue + scatter of
the new lanes, traversal + hit processing + scatter, walk, drop: the same cases
pin both orders, since a film does not depend on the schedule.)

Every film is the oracle's, bit for bit, on two consecutive frames of one
context: the first launches in probe order, the second in the learned order.
No tolerance anywhere: the films are deterministic.
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


def many_spheres_scene(n, seed):
    """test_gpu_parity.py's scene of n Matte spheres: a BVH beyond the 64
    LDS-staged nodes, so k_chain_ci walks with the [64] stack."""
    rng = np.random.default_rng(seed)
    s = G.Scene()
    mats = [s.add_matte(tuple(rng.uniform(0.2, 0.9, 3))) for _ in range(3)]
    floor = s.add_disk(G.mul(G.translate(0, -1, 0), G.rotate(0, 90)), 0.0, 50.0)
    s.add_primitive(floor, mats[0])
    for i in range(n):
        c = (rng.uniform(-6, 6), rng.uniform(-0.5, 4), rng.uniform(-6, 6))
        sph = s.add_sphere(G.translate(*c), rng.uniform(0.2, 0.8), reverse=bool(i % 7 == 3))
        s.add_primitive(sph, mats[i % 3])
    s.add_point_light(G.translate(0, 8, 0), (40, 40, 40))
    s.add_distant_light(G.translate(0, 0, 0), (0.6, 0.6, 0.6), (1, 2, 1))
    s.set_film(64, 48)
    s.set_camera(G.look_at((0, 5, 14), (0, 0, 0), (0, 1, 0)), fov=50)
    return s.build()


SCENES = {
    "readme45x30": lambda: G.Scene.readme(45, 30),   # 6 tiles of 16 px, ragged
    "readme80x48": lambda: G.Scene.readme(80, 48),   # 15 tiles: a multiple of neither 2 nor 4
    "readme16x16": lambda: G.Scene.readme(16, 16),   # one tile
    "cornell32x32": lambda: G.Scene.cornell(32, 32),
    "glass48x32": lambda: G.Scene.readme_glass(48, 32),
    "mesh48x32": lambda: G.Scene.heightfield(48, 32, quads=8, seed=1),
    "spheres90": lambda: many_spheres_scene(90, 5),
}

# (scene, RenderDesc arguments) of the step-order cases
CASES = {
    # every trajectory ends at its first scatter's depth test: a step has only fresh lanes, nothing is traversed
    "fresh_only": ("readme45x30", dict(spp_x=2, spp_y=2, max_depth=2)),
    # trajectories end in the second scatter or by a miss
    "second_scatter": ("readme45x30", dict(spp_x=2, spp_y=2, max_depth=3)),
    # one traced sample per pixel: drop, StartPixel and issue all fall in one step
    "walk_ends_pixel": ("readme45x30", dict(spp_x=2, spp_y=1)),
    # the draw parity flips, so in-flight hits are dropped
    "parity_nd1": ("readme45x30", dict(spp_x=3, spp_y=3, n_dims=1)),
    "parity_nd2": ("readme45x30", dict(spp_x=3, spp_y=3, n_dims=2)),
    # endings inside the scatter by Russian roulette
    "cornell_rr1": ("cornell32x32", dict(spp_x=2, spp_y=2, max_depth=8, rr_threshold=1.0)),
    "cornell_rr025": ("cornell32x32", dict(spp_x=2, spp_y=2, max_depth=8, rr_threshold=0.25)),
    "second_scatter80": ("readme80x48", dict(spp_x=2, spp_y=2, max_depth=3)),
}
VARIANT_CASES = ["second_scatter", "cornell_rr1", "cornell_rr025"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def oracle_film(scene_key, rd_items):
    """The oracle's film of a (scene, render) pair: computed once, shared by the cases, never written to."""
    scene = SCENES[scene_key]()   # (owns the descriptor's arrays: alive until the oracle returns)
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


def chain_of(scene_key, waves, **kw):
    """The instantiation a scene's class and PBRT_CI_WAVES select (frame_route.h chain_launch): the
    mesh-only walk, the [64]-stack walk beyond 64 nodes, kX; at one wave the register build
    is ci_eu3_fits' choice unless PBRT_CI_EU sets it."""
    w = int(waves)
    depth = {"mesh48x32": -1, "spheres90": 64}.get(scene_key, 0)
    kx = scene_key == "glass48x32"
    eu = 0 if (w > 1 or kx or depth < 0) else None
    return chain(w, depth, kx=kx, eu=kw.pop("eu", eu), multi=kx and w == 1, **kw)


def check_case(name, lanes_per_wave=0, expect=None):
    scene_key, rd_kw = CASES[name]
    check_two_frames(scene_key, lanes_per_wave=lanes_per_wave, expect=expect, **rd_kw)


def test_russian_roulette_is_reached():
    """The two Cornell cases differ only in rr_threshold: their films differ, so paths end by RR."""
    a, _ = oracle_film("cornell32x32", tuple(sorted(CASES["cornell_rr1"][1].items())))
    b, _ = oracle_film("cornell32x32", tuple(sorted(CASES["cornell_rr025"][1].items())))
    assert not np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name", ["fresh_only", "second_scatter", "walk_ends_pixel", "parity_nd1", "parity_nd2",
                                  "cornell_rr1", "cornell_rr025"])
@pytest.mark.parametrize("eu", ["3", "2"])
def test_one_wave(eu, name, monkeypatch):
    """The one-wave Matte instantiations, at the 3- and the 2-waves/SIMD build."""
    monkeypatch.setenv("PBRT_CI_WAVES", "1")
    monkeypatch.setenv("PBRT_CI_EU", eu)
    check_case(name, expect=chain(1, eu=0 if eu == "3" else 2))


@pytest.mark.parametrize("name", VARIANT_CASES)
@pytest.mark.parametrize("nps", ["default", "0"])
@pytest.mark.parametrize("waves", ["2", "4", "8"])
def test_multi_wave(waves, nps, name, monkeypatch):
    """One tile per workgroup of 2, 4, 8 waves, with and without next-pixel speculation."""
    monkeypatch.setenv("PBRT_CI_WAVES", waves)
    if nps != "default":
        monkeypatch.setenv("PBRT_CI_NPS", nps)
    check_case(name, expect=chain(int(waves)))


@pytest.mark.parametrize("name", ["second_scatter80", "cornell_rr1", "cornell_rr025"])
@pytest.mark.parametrize("lpw", [2, 4])
def test_several_tiles_per_wave(lpw, name):
    """kMulti: the group's state, and with it the ring of a pending hit, is per lane."""
    check_case(name, lanes_per_wave=lpw, expect=chain(1, eu=None, multi=True))


@pytest.mark.parametrize("max_depth", [10, 3])
@pytest.mark.parametrize("waves", ["1", "2", "4"])
def test_kx(waves, max_depth, monkeypatch):
    """kX: a trajectory's RR-branch records are held across the walk."""
    monkeypatch.setenv("PBRT_CI_WAVES", waves)
    check_two_frames("glass48x32", expect=chain_of("glass48x32", waves), spp_x=2, spp_y=2, max_depth=max_depth)


@pytest.mark.parametrize("max_depth", [10, 3])
@pytest.mark.parametrize("waves", ["1", "4"])
def test_mesh(waves, max_depth, monkeypatch):
    monkeypatch.setenv("PBRT_CI_WAVES", waves)
    check_two_frames("mesh48x32", expect=chain_of("mesh48x32", waves), spp_x=2, spp_y=2, max_depth=max_depth)


@pytest.mark.parametrize("max_depth", [6, 2])
@pytest.mark.parametrize("waves", ["1", "4"])
def test_stack_walk(waves, max_depth, monkeypatch):
    monkeypatch.setenv("PBRT_CI_WAVES", waves)
    check_two_frames("spheres90", expect=chain_of("spheres90", waves), spp_x=3, spp_y=3, max_depth=max_depth)


def test_windowed_start_pixel():
    """The kSpWin instantiation: 121 spp without jitter on a one-tile image."""
    check_two_frames("readme16x16", expect=chain(4, spwin=True), spp_x=11, spp_y=11, jitter=False, max_depth=3)   # 1 tile: 4 waves

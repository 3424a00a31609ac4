"""k_chain_ci issues PCG32 states by one table step from a carried state.

With one tile per workgroup the group carries the PCG32 state at `nxt` (and, with
next-pixel speculation, at `nnx`). The issue gives an idle lane the state
`pcg_step(J, base, inc, cs * r)`, r its rank among its wave's idle lanes of its
class and `base` the carried state moved to the wave's first rank; the carried
states move with nxt and nnx: by `cs * nspec` in the issue, to the state at the
head (the last walked ring entry's, its draw count on) when the walk resets nxt,
to StartPixel's end state or the speculation's at a pixel's start. The
re-issued exact head reads the state its ring entry already holds. All of it is
integer arithmetic mod 2^64, so every state is the one the generic jump from the
pixel's first sample gave, and every film is the oracle's, bit for bit, on two
consecutive frames of one context (probe order, then the learned order). No
tolerance anywhere.

The shapes are the smallest at which the new code can go wrong:
- one wave, both register builds and both candidate strides: rank 63 at stride 2
  is table index 126 (8x8 spp reaches it, and offsets beyond 2^9); 2x1 spp makes
  reset, StartPixel and issue fall in one step;
- n_dims 1..5: odd draw counts flip the parity, which resets nxt to the head;
- Cornell at max_depth 20 without roulette: the longest draw counts (the upper
  bound is 8 per bounce: 176 draws). The oracle counts draws per pixel, not per
  path: the largest pixel has 263, about 38 of them StartPixel's, so its three
  traced samples share 225 and a single path of more than 127 draws is not
  established. The paths of pcg_advance_near beyond the 128-entry table are
  therefore pinned by tests/test_pcg_steps_host.py, not by this case;
- 2, 4, 8 waves with and without next-pixel speculation: per-wave bases, nnx;
- the mesh-only, stack-walk and windowed-StartPixel instantiations;
- several tiles per wave and the kX kernels, whose issue is unchanged by design;
- the camera-start route (k_chain_cam), which carries the state at nxt the same way.
"""
import functools
import os

import numpy as np
import pytest

import oracle_lib as O
import pbrtgpu as G
from launch_checks import assert_chain, assert_launched, chain, check_invariants
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
LONG_REACH = dict(spp_x=2, spp_y=2, max_depth=20, rr_threshold=0.0)


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


@pytest.mark.parametrize("max_depth", [2, 5, 10])
@pytest.mark.parametrize("spp", [(2, 1), (2, 2), (3, 3), (8, 8)])
@pytest.mark.parametrize("stride", ["1", "2"])
@pytest.mark.parametrize("eu", ["3", "2"])
def test_one_wave(eu, stride, spp, max_depth, monkeypatch):
    """The one-wave Matte instantiations: both builds, both candidate strides."""
    monkeypatch.setenv("PBRT_CI_WAVES", "1")
    monkeypatch.setenv("PBRT_CI_EU", eu)
    monkeypatch.setenv("PBRT_CI_STRIDE", stride)
    check_two_frames("readme45x30", expect=chain(1, eu=0 if eu == "3" else 2), spp_x=spp[0], spp_y=spp[1],
                     max_depth=max_depth)


@pytest.mark.parametrize("n_dims", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("waves", ["1", "4"])
def test_parity_flips(waves, n_dims, monkeypatch):
    """Odd draw counts reset nxt to the head; n_dims also moves the scatter's
    light draws across the stratified / PCG32 boundary."""
    monkeypatch.setenv("PBRT_CI_WAVES", waves)
    check_two_frames("readme45x30", expect=chain_of("readme45x30", waves), spp_x=3, spp_y=3, max_depth=5, n_dims=n_dims)


@pytest.mark.parametrize("waves", ["1", "4"])
def test_long_reach(waves, monkeypatch):
    """Cornell, 20 bounces, no roulette: the longest draw counts of any case here
    (up to 263 draws per pixel; see the module docstring on what that pins)."""
    monkeypatch.setenv("PBRT_CI_WAVES", waves)
    check_two_frames("cornell32x32", expect=chain_of("cornell32x32", waves), **LONG_REACH)


@pytest.mark.parametrize("case", [("readme45x30", dict(spp_x=3, spp_y=3)), ("cornell32x32", dict(spp_x=2, spp_y=2))],
                         ids=["readme45x30", "cornell32x32"])
@pytest.mark.parametrize("nps", ["default", "0"])
@pytest.mark.parametrize("waves", ["2", "4", "8"])
def test_multi_wave(waves, nps, case, monkeypatch):
    """One tile per workgroup of 2, 4, 8 waves: each wave moves the bases to its
    first rank; with next-pixel speculation the state at nnx is carried too."""
    monkeypatch.setenv("PBRT_CI_WAVES", waves)
    if nps != "default":
        monkeypatch.setenv("PBRT_CI_NPS", nps)
    check_two_frames(case[0], expect=chain(int(waves)), **case[1])


@pytest.mark.parametrize("scene_key", ["mesh48x32", "spheres90"])
@pytest.mark.parametrize("waves", ["1", "4"])
def test_mesh_and_stack_walk(waves, scene_key, monkeypatch):
    monkeypatch.setenv("PBRT_CI_WAVES", waves)
    check_two_frames(scene_key, expect=chain_of(scene_key, waves), spp_x=2, spp_y=2)


def test_windowed_start_pixel():
    """The kSpWin instantiation: 121 spp without jitter on a one-tile image."""
    check_two_frames("readme16x16", expect=chain(4, spwin=True), spp_x=11, spp_y=11, jitter=False, max_depth=3)   # 1 tile: 4 waves


@pytest.mark.parametrize("lpw", [2, 4])
def test_several_tiles_per_wave(lpw):
    """kMulti keeps the jump from the pixel's first sample (per-lane group state)."""
    check_two_frames("readme80x48", lanes_per_wave=lpw, expect=chain(1, eu=None, multi=True), spp_x=2, spp_y=2)


@pytest.mark.parametrize("waves", ["1", "2", "4"])
def test_kx(waves, monkeypatch):
    """kX: one wave runs the per-lane code (unchanged); 2 and 4 waves carry the state."""
    monkeypatch.setenv("PBRT_CI_WAVES", waves)
    check_two_frames("glass48x32", expect=chain_of("glass48x32", waves), spp_x=2, spp_y=2)


def test_wave_cam():
    """k_chain_cam (kernel="wave_cam", RandomSampler: no sampled dimensions): five camera draws
    per sample, so the draw counts are mostly odd and the chain often overtakes the issue."""
    scene = G.Scene.readme(45, 30)
    rd = abi.render_desc()
    G.lib().pbrt_random_sampler(4, G.C.byref(rd))
    rc, ofilm, ost = O.render(scene.desc, rd, threads=THREADS)
    assert rc == 0 and ofilm.max() > 0
    with G.Renderer(scene, kernel="wave_cam") as r:
        for frame in range(2):
            film, st = r.render(rd)
            assert st.kernel == abi.PBRT_KERNEL_WAVE_CAM, (frame, st.kernel)
            assert st.paths_traced == ost.paths, (frame, st.paths_traced, ost.paths)
            assert np.array_equal(bits(film), bits(ofilm)), (frame, int((film != ofilm).sum()))
            assert_launched(r.launches(), ["k_chain_cam", "k_paths_cam<64, false>", "k_film_cam<false>"], f"frame {frame}")

"""oracle_path_li and oracle_direct_li (the oracle's integrators on caller rays, tests/oracle_lib.py
path_li / direct_li) tied to the oracle's own render path. No GPU.

The render can run Li only behind its camera; the per-ray entries take any ray. Here they get
the render's own rays and streams: li_reference.samples() gives every traced sample of a
THROUGHPUT render with n_dims = 0 and its PCG32 state after the five camera draws,
test_gpu_query.oracle_camera_rays the sample's camera ray from the oracle's own exports (pinhole
cameras), and li_reference.film() the film of the radiances. That film is oracle_render's bit for
bit and the summed ray counts are its statistics, for Path and for DirectLighting with both
strategies. Then the step limit: k iterations and max_depth - k more from the returned state are
one run to the end, and the state after k iterations is the run at max_depth = k + 1 (the rule
tests/test_gpu_path_step.py states for the device).
"""
import functools
import os

import numpy as np
import pytest

import li_reference as R
import oracle_lib as O
import pbrtgpu as G
from pbrtgpu import abi
from test_gpu_query import oracle_camera_rays

THREADS = min(16, os.cpu_count() or 1)
SPP = 3   # Stratified(3, 1): samples 1 and 2 of a pixel are traced
MAX_DEPTH = 5
SCENES = {"readme40x24": lambda: G.Scene.readme(40, 24), "cornell32": lambda: G.Scene.cornell(32, 32),
          "glass48x32": lambda: G.Scene.readme_glass(48, 32)}
DL = {"all": abi.PBRT_DL_UNIFORM_SAMPLE_ALL, "one": abi.PBRT_DL_UNIFORM_SAMPLE_ONE}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def batch(name):
    """(scene, samples, their camera rays): every traced sample of the scene's film."""
    scene = SCENES[name]()
    assert scene.desc.camera.lens_radius == 0
    s = R.samples(scene.desc.film, SPP)
    rays = np.concatenate([oracle_camera_rays(scene.desc, (int(x), int(y), int(x) + 1, int(y) + 1), (fx, fy))
                           for x, y, fx, fy in zip(s.px, s.py, s.film_x, s.film_y)])
    rays.setflags(write=False)
    return scene, s, rays


@functools.lru_cache(maxsize=None)
def whole(name):
    scene, s, rays = batch(name)
    return O.path_li(scene.desc, rays, s.state, s.inc, max_depth=MAX_DEPTH)


def render(scene, **kw):
    rd = abi.render_desc(SPP, 1, n_dims=0, max_depth=MAX_DEPTH, mode=abi.PBRT_MODE_THROUGHPUT, **kw)
    rc, film, st = O.render(scene.desc, rd, threads=THREADS)
    assert rc == 0 and film.max() > 0
    return film, st


@pytest.mark.parametrize("name", sorted(SCENES))
def test_path_li_is_the_renders(name):
    scene, s, rays = batch(name)
    ofilm, ost = render(scene)
    got = whole(name)
    assert len(s.k) == ost.paths
    film = R.film(scene.desc.film, s, got.L)
    assert np.array_equal(bits(film), bits(ofilm)), int((bits(film) != bits(ofilm)).sum())
    assert (int(got.closest.sum()), int(got.shadow.sum())) == (ost.closest_rays, ost.shadow_rays)
    assert (got.status == O.ENDED).all() and not got.panic.any()
    assert same(got.state, R.pcg_advance(s.state, s.inc, got.draws))
    assert (got.bounces >= 1).all() and got.bounces.max() == MAX_DEPTH and same(got.bounces.astype(np.uint32), got.closest)
    assert len(set(got.draws.tolist())) > 3


@pytest.mark.parametrize("strategy", sorted(DL))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_direct_li_is_the_renders(name, strategy):
    scene, s, rays = batch(name)
    ofilm, ost = render(scene, integrator=abi.PBRT_INTEGRATOR_DIRECT_LIGHTING, dl_strategy=DL[strategy])
    got = O.direct_li(scene.desc, rays, s.state, s.inc, max_depth=MAX_DEPTH, dl_strategy=DL[strategy])
    film = R.film(scene.desc.film, s, got.L)
    assert np.array_equal(bits(film), bits(ofilm)), int((bits(film) != bits(ofilm)).sum())
    assert (int(got.closest.sum()), int(got.shadow.sum())) == (ost.closest_rays, ost.shadow_rays)
    assert not got.panic.any()
    assert same(got.state, R.pcg_advance(s.state, s.inc, got.draws))
    if name == "glass48x32":   # SpecularTransmit recursed through the glass
        assert got.closest.max() > 1


@pytest.mark.parametrize("name", sorted(SCENES))
def test_step_limit_and_prefix_rule(name):
    scene, s, rays = batch(name)
    end = whole(name)
    fresh = O.PathStart(np.zeros((len(s.k), 3)), np.ones((len(s.k), 3)), np.ones(len(s.k)), *[np.zeros(len(s.k), dtype=np.int32)] * 4)
    explicit = O.path_li(scene.desc, rays, s.state, s.inc, max_depth=MAX_DEPTH, start=fresh)
    for a, b in zip(explicit, end):   # an absent start state is the fresh one
        assert same(a, b)
    for k in range(1, MAX_DEPTH):
        head = O.path_li(scene.desc, rays, s.state, s.inc, max_depth=MAX_DEPTH, k=k)
        alive = head.status == O.ALIVE
        assert alive.any() and (head.status[~alive] == O.ENDED).all()
        assert (head.bounces[alive] == k).all() and (head.bounces <= k).all()
        assert np.isinf(head.ray[alive, 6]).all()   # a scatter's ray
        # continued from the returned state: only the live paths move
        rest = O.path_li(scene.desc, head.ray[alive], head.state[alive], s.inc[alive], max_depth=MAX_DEPTH, k=MAX_DEPTH - k,
                         start=O.PathStart(*[getattr(head, f)[alive] for f in O.PathStart._fields]))
        assert (rest.status == O.ENDED).all()
        for f in ("L", "bounces", "state", "draws", "closest", "shadow"):
            joined = np.array(getattr(head, f))
            joined[alive] = getattr(rest, f)
            assert same(joined, getattr(end, f)), (k, f)
        # the prefix rule: Russian roulette depends on bounces, not on max_depth
        short = O.path_li(scene.desc, rays, s.state, s.inc, max_depth=k + 1)
        assert same(head.L, short.L), k
        assert (short.status == O.ENDED).all()
        # the path that ran k iterations and is alive asked one closest hit fewer than the one cut at k + 1
        assert same(head.closest + alive.astype(np.uint32), short.closest) and same(head.shadow, short.shadow)
        assert same(head.draws, short.draws) and same(head.state, short.state)

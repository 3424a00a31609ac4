"""pbrt_gpu_direct_li_device (Renderer.direct_li_device, k_li_direct) on the GPU: batched
DirectLighting.Li over ray and PCG32-stream arrays that live on the device.

1. Against the oracle, bit for bit. A THROUGHPUT DirectLighting render with n_dims = 0
   starts sample (tile, pi, k) at mb_state(tile, pi, k), draws five camera values and
   calls Li. The samples come from frame_samples (one launch; its order, rays and states
   are pinned to li_reference.samples() by tests/test_gpu_open_frame.py), the radiances
   from direct_li_device, the film from li_reference.film() in numpy; its uint64 view is
   the oracle's, and the summed ray counts are the oracle's. Stratified(3, 1): two traced
   samples per pixel. tests/test_direct_li_host.py asserts on the oracle alone that the
   cases recurse as deep as they are meant to.
2. out.state is the input advanced by out.draws steps; the draw counts of a Matte level.
3. Batch shape: n around the wave and work-list sizes, forwards and reversed, sentinel-
   padded buffers, every combination of the optional outputs, the grid cap at 1 and 2.
4. The composed DirectLighting frame of render_samples against the oracle and against
   pbrt_gpu_render of the same render desc.
5. The contract: panics as data, refusals, PBRT_E_INVALID, frames around a query, the
   level-record buffer's size, and a Path query between two direct ones.

Every buffer handed to a query is 64 elements longer than the query and pre-filled with
a sentinel (tests/test_gpu_li.py's); the tail must come back unchanged.
"""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np
import pytest

import li_reference as R
import oracle_lib as O
import pbrtgpu as G
import test_gpu_li as T
import test_gpu_query as Q
from large_scenes import MATTE, crowd
from pbrtgpu import abi
from scenes import material_scene
from test_gpu_wave_cam import efloat_scene

pytestmark = pytest.mark.gpu

THREADS = T.THREADS
PAD, SENTINEL = T.PAD, T.SENTINEL
padded, head, bits, same = T.padded, T.head, T.bits, T.same
SPP = T.SPP   # Stratified(3, 1): samples 1 and 2 are traced
RAY_KEYS = T.RAY_KEYS
OUT_KEYS = T.OUT_KEYS
ALL, ONE = abi.PBRT_DL_UNIFORM_SAMPLE_ALL, abi.PBRT_DL_UNIFORM_SAMPLE_ONE
DIRECT = abi.PBRT_INTEGRATOR_DIRECT_LIGHTING
INV, UNS = abi.PBRT_E_INVALID, abi.PBRT_E_UNSUPPORTED
GRID_CAP = 8192          # knobs.h: direct_li_grid
RECORD_BYTES = 64 * 56   # a level of a workgroup: 64 lanes of 7 doubles


def glass_stack(k, w=16, h=16, fov=40.0, shrink=0.1):
    """k smooth-glass disks one unit apart along -z, normals towards the camera, before a Matte
    wall and two point lights: a camera ray refracts through disk after disk (the local-frame wi
    of a disk with normal +z continues along -z, SURVEY #7), one level of DirectLighting.Li's
    recursion each."""
    s = G.Scene()
    glass = s.add_glass(kr=(.5, .5, .5), kt=(.9, .8, .7), u_roughness=0.0, v_roughness=0.0)
    wall_m = s.add_matte((.7, .6, .5))
    for i in range(k):   # world z = -i, normal +z: the local-frame wi then continues along -z
        s.add_primitive(s.add_disk(G.rotate(0, 180), 1.0 * i, 4.0 - shrink * i), glass)
    s.add_primitive(s.add_disk(G.translate(0, 0, -1.0 * k - 5.0), 0.0, 50.0), wall_m)
    s.add_point_light(G.translate(3, 3, -1.0 * k - 2.0), (400, 300, 200))
    s.add_point_light(G.translate(-6, 2, 3), (100, 120, 140))
    s.set_film(w, h)
    s.set_camera(G.look_at((0, 0, 6), (0, 0, 0), (0, 1, 0)), fov=fov)
    return s.build(max_prims_in_node=1)


Case = namedtuple("Case", "scene kernel")
CASES = {
    "readme40x24": Case(T.CASES["readme40x24"].scene, "k_li_direct<false, 0>"),   # ragged last tile column
    "cornell32": Case(T.CASES["cornell32"].scene, "k_li_direct<false, 0>"),
    "lights20": Case(T.CASES["lights20"].scene, "k_li_direct<false, 0>"),
    "mesh_spheres": Case(T.CASES["mesh_spheres"].scene, "k_li_direct<false, 0>"),
    "mesh_only": Case(T.CASES["mesh_only"].scene, "k_li_direct<false, 0>"),
    "edges": Case(T.CASES["edges"].scene, "k_li_direct<false, 0>"),
    "crowd_matte": Case(lambda: crowd(kinds=MATTE), "k_li_direct<false, 64>"),   # 121 BVH nodes
    "glass": Case(T.CASES["glass"].scene, "k_li_direct<true, 0>"),
    "material_scene": Case(lambda: material_scene(), "k_li_direct<true, 0>"),
    "glass_stack20": Case(lambda: glass_stack(20), "k_li_direct<true, 0>"),      # 41 nodes
    "crowd_kx": Case(lambda: crowd(), "k_li_direct<true, 64>"),
    "glass_stack34": Case(lambda: glass_stack(34), "k_li_direct<true, 64>"),     # 69 nodes
}
MATTE_CASES = ("readme40x24", "cornell32", "lights20", "mesh_spheres", "mesh_only", "edges", "crowd_matte")
# beyond (every case, both strategies, max_depth 5): the deepest recursions, the shallowest, no recursion at all
EXTRA = [("glass_stack34", 64, ALL), ("glass_stack34", 63, ALL), ("glass_stack20", 64, ALL), ("glass_stack20", 63, ALL),
         ("crowd_kx", 2, ALL), ("readme40x24", 1, ALL)]
ORACLE_RUNS = [(name, 5, st) for name in sorted(CASES) for st in (ALL, ONE)] + EXTRA


def render_desc(max_depth, strategy):
    return abi.render_desc(SPP, 1, n_dims=0, integrator=DIRECT, max_depth=max_depth, dl_strategy=strategy,
                           mode=abi.PBRT_MODE_THROUGHPUT)


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return CASES[name].scene()


@functools.lru_cache(maxsize=None)
def oracle_film(name, max_depth, strategy):
    """(film, stats) of the oracle's THROUGHPUT n_dims = 0 DirectLighting render, computed once."""
    rc, film, st = O.render(scene_of(name).desc, render_desc(max_depth, strategy), threads=THREADS)
    assert rc == 0 and np.isfinite(film).all(), (name, max_depth, strategy, rc)
    film.setflags(write=False)
    return film, st


@functools.lru_cache(maxsize=None)
def samples_of(name):
    return R.samples(scene_of(name).desc.film, SPP)


def dli(r, rb, gb, n, keys=OUT_KEYS, **desc):
    """direct_li_device into fresh padded outputs of n elements; returns {key: the first n}."""
    ob = {k: padded(r, n, G.LI_DTYPES[k]) for k in keys}
    rc = r.direct_li_device(rb, gb, n, ob, **desc)
    assert rc == 0, (rc, r.last_error())
    return {k: head(b, n) for k, b in ob.items()}


def frame_sample_buffers(r, n):
    sb = {k: padded(r, n, G.SAMPLE_DTYPES[k]) for k in G.SAMPLE_REQUIRED}
    before = len(r.launches(outside=True))
    assert r.frame_samples(sb, SPP - 1) == 0, r.last_error()
    assert [rec.name for rec in r.launches(outside=True)[before:]] == ["k_frame_samples"]
    return sb


@functools.lru_cache(maxsize=None)
def device_batch(name, max_depth, strategy):
    """The case's samples through frame_samples and direct_li_device on one context: the
    outputs (read-only) and the rays frame_samples wrote, as an (n, 6) array."""
    scene = scene_of(name)
    fd = scene.desc.film
    assert fd.res_x <= 48 and fd.res_y <= 32 and not 0.0 > fd.max_sample_luminance
    s = samples_of(name)
    n = len(s.k)
    assert n <= 3072
    with G.Renderer(scene) as r:
        assert r.frame_count(SPP - 1) == n
        sb = frame_sample_buffers(r, n)
        rb, gb = {k: sb[k] for k in G.RAY_KEYS}, {k: sb[k] for k in G.RNG_KEYS}
        rays = np.stack([head(sb[k], n) for k in G.RAY_KEYS], axis=1)
        assert np.array_equal(head(sb["state"], n), s.state) and np.array_equal(head(sb["inc"], n), s.inc)
        before = len(r.launches(outside=True))
        got = dli(r, rb, gb, n, max_depth=max_depth, dl_strategy=strategy)
        assert Q.status(r) == Q.CLEAN
        names = [rec.name for rec in r.launches(outside=True)[before:]]
        assert names == [CASES[name].kernel], names   # one launch, of the instantiation the scene selects
        rec = r.launches(outside=True)[-1]
        assert rec.block == (64, 1, 1) and rec.grid == (min((n + 255) // 256, GRID_CAP), 1, 1) and rec.lds == 0
        for k in G.RAY_KEYS:   # the inputs are untouched
            assert same(head(sb[k], n), rays[:, G.RAY_KEYS.index(k)])
        assert np.array_equal(head(sb["state"], n), s.state) and np.array_equal(head(sb["inc"], n), s.inc)
    for a in list(got.values()) + [rays]:
        a.setflags(write=False)
    return got, rays


# ------------------------------------------------- 1. against the oracle's film
@pytest.mark.parametrize("name,max_depth,strategy", ORACLE_RUNS)
def test_film_of_direct_li_is_the_oracles(name, max_depth, strategy):
    ofilm, ost = oracle_film(name, max_depth, strategy)
    s = samples_of(name)
    got, _ = device_batch(name, max_depth, strategy)
    assert len(s.k) == ost.paths
    L = np.stack([got["r"], got["g"], got["b"]], axis=1)
    film = R.film(scene_of(name).desc.film, s, L)
    print(name, max_depth, strategy, "differing film values:", int((bits(film) != bits(ofilm)).sum()),
          "closest", int((got["rays"] & 0xFFFF).sum()), ost.closest_rays, "shadow", int((got["rays"] >> 16).sum()),
          ost.shadow_rays)
    assert np.array_equal(bits(film), bits(ofilm)), int((bits(film) != bits(ofilm)).sum())
    # the reference's ray counts of the frame are the rays' own
    assert int((got["rays"] & 0xFFFF).sum()) == ost.closest_rays and int((got["rays"] >> 16).sum()) == ost.shadow_rays


# --------------------------------------------------------------- 2. state and draws
@pytest.mark.parametrize("name,max_depth,strategy", ORACLE_RUNS)
def test_state_is_the_input_advanced_by_draws(name, max_depth, strategy):
    s = samples_of(name)
    got, _ = device_batch(name, max_depth, strategy)
    assert np.array_equal(got["state"], R.pcg_advance(s.state, s.inc, got["draws"]))


@pytest.mark.parametrize("name,max_depth,strategy", [r for r in ORACLE_RUNS if r[0] in MATTE_CASES])
def test_draws_of_a_matte_level(name, max_depth, strategy):
    """A Matte ray is one level: one closest-hit query; a miss draws nothing; a hit draws uLight and
    uScattering per light (ALL: 4 * n_lights) or the light index, uLight and uScattering (ONE: 5),
    then the Get2D of SpecularReflect and of SpecularTransmit where depth + 1 < max_depth (4)."""
    scene = scene_of(name)
    got, rays = device_batch(name, max_depth, strategy)
    nl = scene.desc.n_lights
    assert nl > 0
    hit = O.intersect(scene.desc, np.concatenate([rays, np.full((len(rays), 1), np.inf)], axis=1), closest=True)[:, 0]
    assert not np.isnan(hit).any() and (hit == 1).any()
    want = (4 * nl if strategy == ALL else 5) + (4 if max_depth > 1 else 0)
    assert ((got["rays"] & 0xFFFF) == 1).all()
    assert (got["draws"][hit == 1] == want).all() and (got["draws"][hit != 1] == 0).all()
    assert ((got["rays"] >> 16)[hit != 1] == 0).all() and ((got["rays"] >> 16) <= (nl if strategy == ALL else 1)).all()


# ------------------------------------------------------------------ 3. batch shape
N = 1000


def test_batch_shape_and_optional_outputs():
    """On crowd(): its rays end after one to three levels, so lanes finish at different levels and
    a refilled lane runs beside lanes deep in a recursion."""
    full, rays6 = device_batch("crowd_kx", 5, ALL)
    s = samples_of("crowd_kx")
    assert len(set((full["rays"][:N] & 0xFFFF).tolist())) >= 3
    rays = np.concatenate([rays6[:N], np.full((N, 1), np.inf)], axis=1)
    with G.Renderer(scene_of("crowd_kx")) as r:
        for order in (slice(None), slice(None, None, -1)):
            rb, gb = T.upload_batch(r, rays[order], s.state[:N][order], s.inc[:N][order])
            ref = dli(r, rb, gb, N, max_depth=5)
            for k in OUT_KEYS:   # a ray's result depends on its ray and stream only
                assert same(ref[k], full[k][:N][order]), k
            for n in (1, 63, 64, 65, 255, 256, 257, 513):
                got = dli(r, rb, gb, n, max_depth=5)
                for k in OUT_KEYS:
                    assert same(got[k], ref[k][:n]), (n, k)
        optional = ("state", "draws", "rays")
        for mask in range(8):   # every combination of the optional outputs
            extra = tuple(k for i, k in enumerate(optional) if mask >> i & 1)
            got = dli(r, rb, gb, 257, keys=("r", "g", "b") + extra, max_depth=5)
            assert set(got) == {"r", "g", "b"} | set(extra)
            for k in got:
                assert same(got[k], ref[k][:257]), (extra, k)
        assert Q.status(r) == Q.CLEAN


@pytest.mark.parametrize("cap", [1, 2])
def test_grid_cap_strides_over_the_work_lists(cap, monkeypatch):
    """PBRT_DIRECT_LI_GRID at 1 and 2: the four work lists of 1000 rays run on one or two
    workgroups, which reuse their level records list after list."""
    monkeypatch.setenv("PBRT_DIRECT_LI_GRID", str(cap))
    full, rays6 = device_batch("crowd_kx", 5, ALL)
    s = samples_of("crowd_kx")
    rays = np.concatenate([rays6[:N], np.full((N, 1), np.inf)], axis=1)
    with G.Renderer(scene_of("crowd_kx")) as r:
        rb, gb = T.upload_batch(r, rays, s.state[:N], s.inc[:N])
        got = dli(r, rb, gb, N, max_depth=5)
        rec = r.launches(outside=True)[-1]
        assert rec.name == "k_li_direct<true, 64>" and rec.grid == (cap, 1, 1)
        assert r.direct_li_scratch_bytes() == cap * 2 * RECORD_BYTES
        for k in OUT_KEYS:
            assert same(got[k], full[k][:N]), k
        assert Q.status(r) == Q.CLEAN


# ------------------------------------------------------------- 4. the composed frame
@pytest.mark.parametrize("strategy", [ALL, ONE])
@pytest.mark.parametrize("name", ["readme40x24", "material_scene"])
def test_composed_frame_is_the_oracles_and_the_renders(name, strategy):
    ofilm, ost = oracle_film(name, 5, strategy)
    budget = G.FRAME_BYTES_PER_SAMPLE * (SPP - 1) * 16 * 16   # one tile of 16 x 16 a range: 6 and 4 ranges
    with G.Renderer(scene_of(name)) as r:
        before = len(r.launches(outside=True))
        film, info = r.render_samples(SPP, max_depth=5, budget_bytes=budget, count_rays=True, integrator=DIRECT,
                                      dl_strategy=strategy)
        assert info["ranges"] >= 3 and info["samples"] == ost.paths
        names = [rec.name for rec in r.launches(outside=True)[before:]]
        assert names.count(CASES[name].kernel) == info["ranges"] and not any(x.startswith("k_li<") for x in names)
        assert np.array_equal(bits(film), bits(ofilm)), int((bits(film) != bits(ofilm)).sum())
        assert (info["closest_rays"], info["shadow_rays"]) == (ost.closest_rays, ost.shadow_rays)
        rfilm, _ = r.render(render_desc(5, strategy))   # pbrt_gpu_render of the same render desc
        assert np.array_equal(bits(film), bits(rfilm))


def test_render_samples_keeps_its_positional_arguments():
    """The new keywords trail: the positional call of tests/test_gpu_open_frame.py is Path's."""
    case = T.CASES["readme40x24"]
    _, ofilm, _ = T.oracle_film(case)
    with G.Renderer(scene_of("readme40x24")) as r:
        film, _ = r.render_samples(SPP, case.max_depth, case.strategy)
        assert np.array_equal(bits(film), bits(ofilm))
        with pytest.raises(G.PbrtError):
            r.render_samples(SPP, integrator=0)


# ------------------------------------------------------------------------ 5. contract
def test_panics_are_reported_as_data():
    """tests/test_gpu_li.py's EFloat-overflow sphere: max_depth 2 on a Matte scene is one level, so
    the camera ray is the only closest-hit query and the panicking rays are those the oracle's
    intersection reports; they have L = 0, the outputs at the panic, and are counted."""
    sc = efloat_scene((20, 40, 0))
    with G.Renderer(sc) as r:
        cam = r.camera_rays()
        rays = np.stack([cam[k].download() for k in RAY_KEYS], axis=1)
        gx, gz = np.meshgrid(np.linspace(-3.0, 3.0, 8), np.linspace(-3.0, 3.0, 8))
        down = np.zeros((64, 7))
        down[:, 0], down[:, 1], down[:, 2], down[:, 4], down[:, 6] = gx.ravel(), 2.0, gz.ravel(), -1.0, np.inf
        rays = np.concatenate([down, rays])
        n = rays.shape[0]
        pan = np.isnan(O.intersect(sc.desc, rays, closest=True)[:, 0])
        assert 0 < pan.sum() < n and not pan[0]
        first = int(np.argmax(pan))
        rng = np.random.default_rng(5)
        state = rng.integers(0, 2**64, size=n, dtype=np.uint64)
        inc = rng.integers(0, 2**63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        clean = ~pan
        rb, gb = T.upload_batch(r, rays[clean], state[clean], inc[clean])
        alone = dli(r, rb, gb, int(clean.sum()), max_depth=2)
        assert Q.status(r) == Q.CLEAN
        assert max(alone["r"].max(), alone["g"].max(), alone["b"].max()) > 0
        rb, gb = T.upload_batch(r, rays, state, inc)
        mixed = dli(r, rb, gb, n, max_depth=2)
        assert Q.status(r) == (abi.PBRT_E_REF_PANIC, int(pan.sum()), first, abi.PBRT_PANIC_EFLOAT)
        for k in ("r", "g", "b"):
            assert (mixed[k][pan] == 0).all()
            assert np.array_equal(bits(mixed[k][clean]), bits(alone[k]))   # the neighbours of a panic are untouched
        assert (mixed["draws"][pan] == 0).all() and (mixed["rays"][pan] == 1).all()   # the values at the panic
        assert np.array_equal(mixed["state"][pan], state[pan])
        assert Q.status(r) == Q.CLEAN   # the record was cleared


def test_ld_above_10_is_a_panic_of_sample_one_only():
    """UniformSampleOneLight panics where a light estimate exceeds 10 (integrator.go:71-73);
    UniformSampleAllLights has no such check. crowd(bright=True): the oracle of each strategy says
    which, and the query record counts the rays the oracle's render would have stopped at."""
    scene = crowd(bright=True)
    rc_one, _, _ = O.render(scene.desc, render_desc(5, ONE), threads=THREADS)
    rc_all, film_all, _ = O.render(scene.desc, render_desc(5, ALL), threads=THREADS)
    assert rc_one == abi.PBRT_E_REF_PANIC and rc_all == 0
    s = R.samples(scene.desc.film, SPP)
    n = len(s.k)
    with G.Renderer(scene) as r:
        sb = frame_sample_buffers(r, n)
        rb, gb = {k: sb[k] for k in G.RAY_KEYS}, {k: sb[k] for k in G.RNG_KEYS}
        one = dli(r, rb, gb, n, max_depth=5, dl_strategy=ONE)
        rc, panics, first, kind = Q.status(r)
        assert rc == abi.PBRT_E_REF_PANIC and panics >= 1 and kind == abi.PBRT_PANIC_LD_GT_10
        zero = (one["r"] == 0) & (one["g"] == 0) & (one["b"] == 0)
        assert zero[first] and zero.sum() >= panics
        every = dli(r, rb, gb, n, max_depth=5, dl_strategy=ALL)
        assert Q.status(r) == Q.CLEAN
        L = np.stack([every["r"], every["g"], every["b"]], axis=1)
        assert np.array_equal(bits(R.film(scene.desc.film, s, L)), bits(film_all))


REFUSALS = {
    "strategy_0": (lambda: G.Scene.readme(32, 32), dict(dl_strategy=0), "strategy"),
    "strategy_3": (lambda: G.Scene.readme(32, 32), dict(dl_strategy=3), "strategy"),
    "rough_glass": (lambda: material_scene(rough=0.2), {}, "rough glass"),
    "max_depth_65_glass": (lambda: G.Scene.readme_glass(48, 32), dict(max_depth=65), "maxDepth > 64"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(name):
    make, desc, word = REFUSALS[name]
    n = 16
    with G.Renderer(make()) as r:
        rays = np.zeros((n, 7))
        rays[:, 5] = 1.0
        rb, gb = T.upload_batch(r, rays, np.arange(n, dtype=np.uint64), np.ones(n, dtype=np.uint64))
        ob = {k: padded(r, n, dt) for k, dt in G.LI_DTYPES.items()}
        before = len(r.launches(outside=True))
        assert r.direct_li_device(rb, gb, n, ob, **desc) == UNS
        assert word in r.last_error(), r.last_error()   # the reason is named
        assert Q.status(r) == Q.CLEAN
        for b in ob.values():   # nothing was enqueued
            assert (b.download() == SENTINEL[b.dtype]).all()
        assert r.direct_li_device(rb, gb, 0, ob, **desc) == UNS   # n = 0 is refused alike
        assert len(r.launches(outside=True)) == before and r.direct_li_scratch_bytes() == 0


def test_any_max_depth_on_a_matte_scene():
    """The recursion cannot start without a SPEC_PAIR BSDF: max_depth 65 (and far beyond) is
    max_depth 5's value and draws, with no level records."""
    at5, rays6 = device_batch("readme40x24", 5, ALL)
    s = samples_of("readme40x24")
    n = 300
    rays = np.concatenate([rays6[:n], np.full((n, 1), np.inf)], axis=1)
    with G.Renderer(scene_of("readme40x24")) as r:
        rb, gb = T.upload_batch(r, rays, s.state[:n], s.inc[:n])
        for md in (65, 2**31 - 1):
            got = dli(r, rb, gb, n, max_depth=md)
            for k in OUT_KEYS:
                assert same(got[k], at5[k][:n]), (md, k)
        assert r.direct_li_scratch_bytes() == 0 and Q.status(r) == Q.CLEAN


def test_invalid_arguments_and_n_zero():
    full, rays6 = device_batch("readme40x24", 5, ALL)
    s = samples_of("readme40x24")
    scene = scene_of("readme40x24")
    n = 65
    L = G.lib()
    with G.Renderer(scene) as r:
        rays = np.concatenate([rays6[:n], np.full((n, 1), np.inf)], axis=1)
        rb, gb = T.upload_batch(r, rays, s.state[:n], s.inc[:n])
        ob = {k: padded(r, n, dt) for k, dt in G.LI_DTYPES.items()}
        rs = G._soa(abi.RaySoA, [(k, b, np.float64) for k, b in rb.items()])
        gs = G._soa(abi.RngSoA, [(k, b, np.uint64) for k, b in gb.items()])
        os_ = G._soa(abi.RadianceSoA, [(k, b, G.LI_DTYPES[k]) for k, b in ob.items()])
        d = abi.direct_li_desc(max_depth=5)
        call = lambda dd=d, rr=rs, gg=gs, nn=n, oo=os_: L.pbrt_gpu_direct_li_device(   # noqa: E731
            r.h, C.byref(dd) if dd is not None else None, C.byref(rr) if rr is not None else None,
            C.byref(gg) if gg is not None else None, nn, C.byref(oo) if oo is not None else None)
        assert L.pbrt_gpu_direct_li_device(None, C.byref(d), C.byref(rs), C.byref(gs), n, C.byref(os_)) == INV
        assert call(dd=None) == INV and call(rr=None) == INV and call(gg=None) == INV and call(oo=None) == INV
        for k in G.RAY_KEYS:   # every ray pointer but tmax is required
            bad = G._soa(abi.RaySoA, [(q, b, np.float64) for q, b in rb.items() if q != k])
            assert call(rr=bad) == INV, k
        no_tmax = G._soa(abi.RaySoA, [(q, b, np.float64) for q, b in rb.items() if q != "tmax"])
        for k in G.RNG_KEYS:
            assert call(gg=G._soa(abi.RngSoA, [(q, b, np.uint64) for q, b in gb.items() if q != k])) == INV, k
        for k in ("r", "g", "b"):
            bad = G._soa(abi.RadianceSoA, [(q, b, G.LI_DTYPES[q]) for q, b in ob.items() if q != k])
            assert call(oo=bad) == INV, k
        assert call(nn=2**31) == INV
        assert call(dd=abi.direct_li_desc(max_depth=0)) == INV
        assert call(dd=abi.direct_li_desc(reserved=(0, 1))) == INV and "reserved" in r.last_error()
        assert call(dd=abi.direct_li_desc(reserved=(1, 0))) == INV
        assert call(nn=0) == 0
        assert Q.status(r) == Q.CLEAN
        for b in ob.values():   # none of the above wrote anything
            assert (b.download() == SENTINEL[b.dtype]).all()
        # a query while a frame is in flight is refused and leaves the frame alone
        rd = abi.render_desc(2, 2)
        rc, ofilm, _ = O.render(scene.desc, rd, threads=THREADS)
        assert rc == 0
        r.render_async(rd)
        rc_q = call()
        r.synchronize()
        assert rc_q == INV and np.array_equal(bits(r.film()), bits(ofilm))
        assert (ob["r"].download() == SENTINEL[np.dtype(np.float64)]).all()
        assert call(rr=no_tmax) == 0   # tmax NULL: +Inf
        assert Q.status(r) == Q.CLEAN
        for k in OUT_KEYS:
            assert same(head(ob[k], n), full[k][:n]), k
        with pytest.raises(G.PbrtError):   # the wrapper's own check: a buffer shorter than n
            r.direct_li_device(rb, gb, n + PAD + 1, ob)
        with pytest.raises(G.PbrtError):
            r.direct_li_device(rb, gb, n, {k: v for k, v in ob.items() if k != "g"})


def test_frames_around_a_query():
    """A frame, a query, a frame on one context: both films are the oracle's and the query is the
    batch's; the frames are a Path render and the DirectLighting render of the query's desc."""
    name = "material_scene"
    full, rays6 = device_batch(name, 5, ALL)
    s = samples_of(name)
    scene = scene_of(name)
    n = 257
    rays = np.concatenate([rays6[:n], np.full((n, 1), np.inf)], axis=1)
    prd = abi.render_desc(2, 2)
    rc, pfilm, _ = O.render(scene.desc, prd, threads=THREADS)
    assert rc == 0
    dfilm, _ = oracle_film(name, 5, ALL)
    with G.Renderer(scene) as r:
        rb, gb = T.upload_batch(r, rays, s.state[:n], s.inc[:n])
        film1, _ = r.render(prd)
        got = dli(r, rb, gb, n, max_depth=5)
        film2, _ = r.render(render_desc(5, ALL))
        again = dli(r, rb, gb, n, max_depth=5)
        assert np.array_equal(bits(film1), bits(pfilm)) and np.array_equal(bits(film2), bits(dfilm))
        for k in OUT_KEYS:
            assert same(got[k], full[k][:n]) and same(again[k], full[k][:n]), k
        assert Q.status(r) == Q.CLEAN


def test_level_records_are_allocated_once_and_a_path_query_between_two_direct_ones():
    full, rays6 = device_batch("crowd_kx", 5, ALL)
    s = samples_of("crowd_kx")
    n = len(s.k)
    lists = (n + 255) // 256
    rays = np.concatenate([rays6, np.full((n, 1), np.inf)], axis=1)
    with G.Renderer(scene_of("readme40x24")) as r:   # a Matte scene: no level records, ever
        m = 300
        rb, gb = T.upload_batch(r, rays[:m], s.state[:m], s.inc[:m])
        dli(r, rb, gb, m, max_depth=64)
        assert r.direct_li_scratch_bytes() == 0
    with G.Renderer(scene_of("crowd_kx")) as r:
        assert r.direct_li_scratch_bytes() == 0
        rb, gb = T.upload_batch(r, rays, s.state, s.inc)
        d1 = dli(r, rb, gb, n, max_depth=5)
        size = r.direct_li_scratch_bytes()
        assert size == lists * 2 * RECORD_BYTES   # grid * levels(5) * 64 lanes * 56 B
        path = T.li(r, rb, gb, n, max_depth=5)
        d2 = dli(r, rb, gb, n, max_depth=5)
        assert r.direct_li_scratch_bytes() == size
        small = dli(r, rb, gb, 300, max_depth=3)
        assert r.direct_li_scratch_bytes() == size
        path2 = T.li(r, rb, gb, n, max_depth=5)
        for k in OUT_KEYS:
            assert same(d1[k], full[k]) and same(d2[k], full[k]), k
            assert same(path[k], path2[k]), k
        assert not same(path["draws"], d1["draws"])   # (they are different integrators)
        shallow, _ = device_batch("crowd_kx", 2, ALL)   # max_depth 3 is one level, as 2 is
        assert same(small["r"], shallow["r"][:300]) and same(small["rays"], shallow["rays"][:300])
        deep = dli(r, rb, gb, n, max_depth=64)   # more levels: the buffer grows, once
        assert r.direct_li_scratch_bytes() == lists * 32 * RECORD_BYTES
        dli(r, rb, gb, n, max_depth=5)
        assert r.direct_li_scratch_bytes() == lists * 32 * RECORD_BYTES
        assert (deep["rays"] & 0xFFFF).sum() >= (d1["rays"] & 0xFFFF).sum()
        assert Q.status(r) == Q.CLEAN


def test_direct_radiance_convenience():
    full, rays6 = device_batch("glass", 5, ONE)
    s = samples_of("glass")
    n = 300
    with G.Renderer(scene_of("glass")) as r:
        L, state, draws, nrays = r.direct_radiance(rays6[:n], s.state[:n], s.inc[:n], max_depth=5, dl_strategy=ONE)
    want = np.stack([full["r"][:n], full["g"][:n], full["b"][:n]], axis=1)
    assert np.array_equal(bits(L), bits(want))
    assert np.array_equal(state, full["state"][:n]) and np.array_equal(draws, full["draws"][:n])
    assert np.array_equal(nrays, full["rays"][:n])

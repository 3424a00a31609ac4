"""pbrt_gpu_li_device (Renderer.li_device, k_li) on the GPU: batched Path.Li over
ray and PCG32-stream arrays that live on the device.

1. Against the oracle, bit for bit. A THROUGHPUT render with n_dims = 0 starts
   sample (tile, pi, k) at mb_state(tile, pi, k), draws five camera values and
   calls Li. tests/li_reference.py restates those states and draws; each
   sample's camera ray comes from pbrt_gpu_camera_rays_device on a 1 x 1 window
   with the sample's own offsets (pinned to the oracle by tests/test_gpu_query.py);
   li_device runs from the states after the camera draws; li_reference.film()
   builds the film in numpy as k_film_cam documents it; its uint64 view is the
   oracle's. Stratified(3, 1): two traced samples per pixel.
2. Independently of the oracle: tests/onebounce_reference.py's closed form.
3. out.state is the input state advanced by out.draws PCG32 steps.
4. Batch shape: n around the wave and work-list sizes, forwards and reversed,
   sentinel-padded buffers, every combination of the optional outputs.
5. Panics: the EFloat-overflow sphere, reported as data in the query record.
6. Refusals, n = 0, frames around a query, the two light strategies in turn.

Every buffer handed to a query is 64 elements longer than the query and
pre-filled with a sentinel (tests/test_gpu_query.py's, and two more for the
uint64 and uint32 outputs); the tail must come back unchanged.
"""
import ctypes as C
import functools
import os
from collections import namedtuple

import numpy as np
import pytest

import li_reference as R
import onebounce_reference as B
import oracle_lib as O
import pbrtgpu as G
import test_gpu_query as Q
from large_scenes import MATTE, crowd
from pbrtgpu import abi
from scenes import material_scene, readme_lights_scene
from test_gpu_edges import edge_scene
from test_gpu_wave_cam import efloat_scene
from test_onebounce_host import TOL

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
PAD = Q.PAD
SENTINEL = dict(Q.SENTINEL)
SENTINEL[np.dtype(np.uint64)] = 0xA5A5A5A5DEADBEEF
SENTINEL[np.dtype(np.uint32)] = 0xDEADBEEF
UNIFORM, POWER = abi.PBRT_LIGHT_STRATEGY_UNIFORM, abi.PBRT_LIGHT_STRATEGY_POWER
SPP = 3   # Stratified(3, 1): samples 1 and 2 are traced
RAY_KEYS = G.RAY_KEYS + ("tmax",)
OUT_KEYS = tuple(G.LI_DTYPES)

Case = namedtuple("Case", "scene max_depth strategy kernel")
CASES = {
    "readme40x24": Case(lambda: G.Scene.readme(40, 24), 5, UNIFORM, "k_li<false, 0>"),   # ragged last tile column
    # the reference's Power distribution: 2n entries of Y() == 0 (SURVEY #28), every pick has pdf 0
    "readme_d10_power": Case(lambda: G.Scene.readme(40, 24), 10, POWER, "k_li<false, 0>"),
    "cornell32": Case(lambda: G.Scene.cornell(32, 32), 5, UNIFORM, "k_li<false, 0>"),
    "glass": Case(lambda: G.Scene.readme_glass(48, 32), 5, UNIFORM, "k_li<true, 0>"),
    "crowd_matte": Case(lambda: crowd(kinds=MATTE), 5, UNIFORM, "k_li<false, 64>"),   # 121 BVH nodes
    "crowd_kx": Case(lambda: crowd(), 5, UNIFORM, "k_li<true, 64>"),
    "lights20": Case(lambda: readme_lights_scene(32, 32, extra=16), 5, UNIFORM, "k_li<false, 0>"),
    "mesh_spheres": Case(lambda: G.Scene.heightfield(48, 32, quads=24, seed=1, spheres=True), 5, UNIFORM,
                         "k_li<false, 0>"),
    "mesh_only": Case(lambda: G.Scene.heightfield(48, 32, quads=24, seed=1), 5, UNIFORM, "k_li<false, 0>"),
    "edges": Case(lambda: edge_scene(partial=True, disk_edges=True), 5, UNIFORM, "k_li<false, 0>"),
}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    """Equal element type, shape and bits (a float compares by its bits, an integer exactly)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ buffers
def padded(r, n, dtype, data=None):
    dtype = np.dtype(dtype)
    host = np.full(n + PAD, SENTINEL[dtype], dtype=dtype)
    if data is not None:
        host[:n] = data
    return r.upload(host)


def head(buf, n):
    host = buf.download()
    assert host.size == n + PAD
    assert (host[n:] == SENTINEL[buf.dtype]).all(), "a query wrote past its n elements"
    return host[:n]


def upload_batch(r, rays, state, inc):
    """(ray buffers, rng buffers) of an (n, 7) ray array and its streams, padded."""
    n = rays.shape[0]
    rb = {k: padded(r, n, np.float64, rays[:, i]) for i, k in enumerate(RAY_KEYS)}
    return rb, {"state": padded(r, n, np.uint64, state), "inc": padded(r, n, np.uint64, inc)}


def li(r, rb, gb, n, keys=OUT_KEYS, **desc):
    """li_device into fresh padded outputs of n elements; returns {key: the first n}."""
    ob = {k: padded(r, n, G.LI_DTYPES[k]) for k in keys}
    rc = r.li_device(rb, gb, n, ob, **desc)
    assert rc == 0, (rc, r.last_error())
    return {k: head(b, n) for k, b in ob.items()}


def sample_rays(r, s):
    """Each sample's camera ray from pbrt_gpu_camera_rays_device on the 1 x 1 window of its
    pixel, with its own pFilm offset, lens point and time value, written to element i of
    padded ray buffers (enqueue only: one launch per sample)."""
    n = len(s.k)
    bufs = {k: padded(r, n, np.float64) for k in RAY_KEYS}
    L, dp = G.lib(), C.POINTER(C.c_double)
    for i in range(n):
        x, y = int(s.px[i]), int(s.py[i])
        d = abi.CameraRaysDesc(x, y, x + 1, y + 1, s.film_x[i], s.film_y[i], s.lens_u[i], s.lens_v[i], s.time_u[i])
        out = abi.RaySoAOut(*[C.cast(C.c_void_p(bufs[k].ptr + 8 * i), dp) for k in RAY_KEYS])
        assert L.pbrt_gpu_camera_rays_device(r.h, C.byref(d), C.byref(out)) == 0
    return bufs


# ------------------------------------------------- 1. against the oracle's film
def oracle_film(case):
    scene = case.scene()
    rd = abi.render_desc(SPP, 1, n_dims=0, max_depth=case.max_depth, light_strategy=case.strategy,
                         mode=abi.PBRT_MODE_THROUGHPUT)
    rc, film, st = O.render(scene.desc, rd, threads=THREADS)
    assert rc == 0 and np.isfinite(film).all()
    return scene, film, st


def device_batch(case):
    """The case's samples through camera_rays_device and li_device on one context."""
    scene, ofilm, ost = oracle_film(case)
    fd = scene.desc.film
    assert fd.res_x <= 48 and fd.res_y <= 32 and not 0.0 > fd.max_sample_luminance
    s = R.samples(fd, SPP)
    n = len(s.k)
    assert n == ost.paths == (fd.crop_max_x - fd.crop_min_x) * (fd.crop_max_y - fd.crop_min_y) * (SPP - 1)
    with G.Renderer(scene) as r:
        rb = sample_rays(r, s)
        gb = {"state": padded(r, n, np.uint64, s.state), "inc": padded(r, n, np.uint64, s.inc)}
        before = len(r.launches(outside=True))
        got = li(r, rb, gb, n, max_depth=case.max_depth, light_strategy=case.strategy)
        assert Q.status(r) == Q.CLEAN
        names = [rec.name for rec in r.launches(outside=True)[before:]]
        assert names == [case.kernel], names   # one launch, of the instantiation the scene selects
        rec = r.launches(outside=True)[-1]
        assert rec.block == (64, 1, 1) and rec.grid == ((n + 255) // 256, 1, 1) and rec.lds == 0
        for k in RAY_KEYS:   # the inputs are untouched
            head(rb[k], n)
        assert np.array_equal(head(gb["state"], n), s.state) and np.array_equal(head(gb["inc"], n), s.inc)
    return scene, s, got, ofilm, ost


@functools.lru_cache(maxsize=None)
def readme_batch():
    out = device_batch(CASES["readme40x24"])
    for a in out[2].values():
        a.setflags(write=False)
    return out


def film_is_the_oracles(scene, s, got, ofilm, ost):
    L = np.stack([got["r"], got["g"], got["b"]], axis=1)
    film = R.film(scene.desc.film, s, L)
    assert np.array_equal(bits(film), bits(ofilm)), int((bits(film) != bits(ofilm)).sum())
    # the reference's ray counts of the frame are the paths' own
    assert int((got["rays"] & 0xFFFF).sum()) == ost.closest_rays and int((got["rays"] >> 16).sum()) == ost.shadow_rays


@pytest.mark.parametrize("name", sorted(CASES))
def test_film_of_li_is_the_oracles(name):
    film_is_the_oracles(*(readme_batch() if name == "readme40x24" else device_batch(CASES[name])))


def test_power_strategy_draws_one_value_per_light_sample():
    """Under Power every picked light has pdf 0: UniformSampleOneLight returns black after its one
    draw (integrator.go:56-58), so a bounce consumes 3 draws (the pick and the BSDF sample) where
    Uniform consumes 7, no shadow ray is traced and no light reaches L. The oracle's film of the
    case (test_film_of_li_is_the_oracles[readme_d10_power]) is black for the same reason; what
    pins the kernel there is the draw order, through the ray counts and every later bounce."""
    _, su, uni, ufilm, _ = readme_batch()
    _, sp, pw, pfilm, post = device_batch(CASES["readme_d10_power"])
    assert ufilm.max() > 0 and not pfilm.any() and post.shadow_rays == 0
    assert not (pw["rays"] >> 16).any() and (uni["rays"] >> 16).any()
    assert not pw["r"].any() and not pw["g"].any() and not pw["b"].any()
    # Russian roulette draws only beyond the third bounce (path.go:139): a path of at most three
    # closest-hit queries consumed whole bounces, 3 draws each under Power, 7 under Uniform
    short_p, short_u = (pw["rays"] & 0xFFFF) <= 3, (uni["rays"] & 0xFFFF) <= 3
    assert short_p.any() and (pw["draws"][short_p] % 3 == 0).all() and (pw["draws"][short_p] > 0).any()
    assert short_u.any() and (uni["draws"][short_u] % 7 == 0).all()
    assert np.array_equal(pw["state"], R.pcg_advance(sp.state, sp.inc, pw["draws"]))


# ---------------------------------------- 2. independently of the oracle: one bounce
def onebounce(r, seed):
    rays = B.camera_rays()
    n = rays.shape[0]
    rng = np.random.default_rng(seed)
    state = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    inc = rng.integers(0, 2**63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    rb, gb = upload_batch(r, rays, state, inc)
    return li(r, rb, gb, n, max_depth=B.MAX_DEPTH), state, inc


def test_one_bounce_closed_form():
    """max_depth 2, one point light: L is Kd / pi * |wi . n| * I / d^2 where lit, else 0, and
    nothing in it is random: two seed arrays give the same bits. A hit draws 7 values (the
    light index, uLight, uScattering, the BSDF sample) and asks two closest hits (the second
    ends on bounces >= maxDepth) and a shadow ray where f is not black; a miss draws nothing."""
    f = B.film()
    H, W = f.compared.shape
    want = f.L.reshape(-1, 3)
    # a corner ray is decided if a pixel it contributes to is compared (film(): a compared
    # pixel has only decided corners)
    decided = np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            decided[y, x] = any(f.compared[py, px] for py in (y - 1, y) for px in (x - 1, x) if px >= 0 and py >= 0)
    decided = decided.ravel()
    assert decided.sum() > 0.7 * decided.size
    with G.Renderer(B.scene()) as r:
        (a, sa, ia), (b, sb, ib) = onebounce(r, 1), onebounce(r, 2)
        assert Q.status(r) == Q.CLEAN
    assert not np.array_equal(sa, sb)
    for k in ("r", "g", "b", "draws"):
        assert same(a[k], b[k]), k
    assert same(a["rays"] >> 16, b["rays"] >> 16)   # (the closest-hit count may depend on the BSDF draws: below)
    got = np.stack([a["r"], a["g"], a["b"]], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):   # as onebounce_reference.gap
        rel = np.where(want != 0, np.abs(got - want) / np.abs(want), np.where(got == want, 0.0, np.inf))
    gap = float(rel[decided].max())
    print(f"one-bounce gap {gap:.3e} (bound {TOL:.3e}) over {int(decided.sum())} of {decided.size} corner rays")
    assert gap <= TOL
    labels = f.corner_labels.ravel()
    miss = labels == "background"
    assert miss[decided].any() and (~miss)[decided].any()
    floor = np.isin(labels, ("lit floor", "shadowed floor")) | (want.max(axis=1) > 0)   # f is not black there
    ends = 0
    for s0, i0, o in ((sa, ia, a), (sb, ib, b)):
        d, ry = o["draws"][decided], o["rays"][decided]
        assert (d[miss[decided]] == 0).all() and (d[~miss[decided]] == 7).all()
        assert (ry[miss[decided]] == 1).all()
        assert ((ry[~miss[decided]] >> 16) <= 1).all() and ((ry[floor[decided]] >> 16) == 1).all()
        assert (got[decided][(ry >> 16) == 0] == 0).all()
        # The second closest-hit query (counted, then ended by bounces >= maxDepth) is asked unless
        # the BSDF sample ends the path (path.go:99: f black or pdf 0). CosineSampleHemisphere gives
        # pdf 0 only on the rim of the disk, which ConcentricSampleDisk reaches only from a draw
        # that is exactly 0 (the reference's PCG32 returns 0 once in about 150 draws); the BSDF
        # sample is draws 5 and 6 of the stream.
        st5 = R.pcg_advance(s0, i0, 5)
        st6, ux = R.pcg_float(st5, i0)
        _, uy = R.pcg_float(st6, i0)
        inside = ((ux != 0) & (uy != 0))[decided]
        closest = ry & 0xFFFF
        assert (closest[~miss[decided] & inside] == 2).all()
        assert np.isin(closest[~miss[decided] & ~inside], (1, 2)).all()
        ends += int((closest[~miss[decided]] == 1).sum())
        assert np.array_equal(o["state"], R.pcg_advance(s0, i0, o["draws"]))
    print(f"paths ended by a BSDF sample on the rim: {ends}")


# --------------------------------------------------------------- 3. state and draws
def test_state_is_the_input_advanced_by_draws():
    _, s, got, _, _ = readme_batch()
    assert got["draws"].max() > 7 and len(set(got["draws"].tolist())) > 3   # paths of one and of several bounces
    assert np.array_equal(got["state"], R.pcg_advance(s.state, s.inc, got["draws"]))


# ------------------------------------------------------------------ 4. batch shape
def test_batch_shape_and_optional_outputs():
    scene, s, full, _, _ = readme_batch()
    N = 1000
    with G.Renderer(scene) as r:
        rb0 = sample_rays(r, R.Samples(*[v[:N] for v in s]))
        rays = np.stack([head(rb0[k], N) for k in RAY_KEYS], axis=1)
        for order in (slice(None), slice(None, None, -1)):
            rb, gb = upload_batch(r, rays[order], s.state[:N][order], s.inc[:N][order])
            ref = li(r, rb, gb, N, max_depth=5)
            for k in OUT_KEYS:   # a path's result depends on its ray and stream only
                assert same(ref[k], full[k][:N][order]), k
            for n in (1, 63, 64, 65, 255, 256, 257):
                got = li(r, rb, gb, n, max_depth=5)
                for k in OUT_KEYS:
                    assert same(got[k], ref[k][:n]), (n, k)
        for extra in ((), ("state",), ("draws",), ("rays",)):   # each optional output alone, and none
            got = li(r, rb, gb, 257, keys=("r", "g", "b") + extra, max_depth=5)
            for k in got:
                assert same(got[k], ref[k][:257]), (extra, k)
        assert Q.status(r) == Q.CLEAN


# ------------------------------------------------------------------------ 5. panics
def test_panics_are_reported_as_data():
    """The camera turned towards the sphere of radius 5e159: a camera ray that reaches its leaf
    box overflows EFloat (efloat.go:102-111). max_depth 2: the camera ray is the only ray of a
    path that can reach it (the shadow rays end at the lights, the BSDF-sampled ray is not
    traced), so the panicking paths are the rays the oracle's orc_intersect reports."""
    sc = efloat_scene((20, 40, 0))
    with G.Renderer(sc) as r:
        cam = r.camera_rays()
        rays = np.stack([cam[k].download() for k in RAY_KEYS], axis=1)
        # (the camera sees sky and the sphere only: 64 rays straight down onto the lit floor come first)
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
        rb, gb = upload_batch(r, rays[clean], state[clean], inc[clean])
        alone = li(r, rb, gb, int(clean.sum()), max_depth=2)
        assert Q.status(r) == Q.CLEAN
        assert max(alone["r"].max(), alone["g"].max(), alone["b"].max()) > 0
        rb, gb = upload_batch(r, rays, state, inc)
        mixed = li(r, rb, gb, n, max_depth=2)
        rc, panics, first_ray, kind = Q.status(r)
        assert (rc, panics, first_ray, kind) == (abi.PBRT_E_REF_PANIC, int(pan.sum()), first, abi.PBRT_PANIC_EFLOAT)
        assert panics >= 1
        for k in ("r", "g", "b"):
            assert (mixed[k][pan] == 0).all()
            assert np.array_equal(bits(mixed[k][clean]), bits(alone[k]))   # the neighbours of a panic are untouched
        assert (mixed["draws"][pan] == 0).all() and (mixed["rays"][pan] == 1).all()   # the values at the panic
        assert np.array_equal(mixed["state"][pan], state[pan])
        assert Q.status(r) == Q.CLEAN   # the record was cleared
        li(r, rb, gb, n, max_depth=2)
        li(r, rb, gb, n, max_depth=2)
        assert Q.status(r) == (abi.PBRT_E_REF_PANIC, 2 * int(pan.sum()), first, abi.PBRT_PANIC_EFLOAT)


# ------------------------------------------------------------- 6. refusals, ordering
def test_invalid_arguments_and_n_zero():
    scene, s, full, _, _ = readme_batch()
    n = 65
    L = G.lib()
    with G.Renderer(scene) as r:
        rays = np.zeros((n, 7))
        rays[:, 5] = 1.0
        rb, gb = upload_batch(r, rays, s.state[:n], s.inc[:n])
        ob = {k: padded(r, n, dt) for k, dt in G.LI_DTYPES.items()}
        rs = G._soa(abi.RaySoA, [(k, b, np.float64) for k, b in rb.items()])
        gs = G._soa(abi.RngSoA, [(k, b, np.uint64) for k, b in gb.items()])
        os_ = G._soa(abi.RadianceSoA, [(k, b, G.LI_DTYPES[k]) for k, b in ob.items()])
        d = abi.li_desc(max_depth=5)
        call = lambda dd=d, rr=rs, gg=gs, nn=n, oo=os_: L.pbrt_gpu_li_device(   # noqa: E731
            r.h, C.byref(dd) if dd is not None else None, C.byref(rr) if rr is not None else None,
            C.byref(gg) if gg is not None else None, nn, C.byref(oo) if oo is not None else None)
        INV = abi.PBRT_E_INVALID
        assert L.pbrt_gpu_li_device(None, C.byref(d), C.byref(rs), C.byref(gs), n, C.byref(os_)) == INV
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
        assert call(dd=abi.li_desc(max_depth=0)) == INV and call(dd=abi.li_desc(max_depth=5, reserved=1)) == INV
        assert "reserved" in r.last_error()
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
        assert call(rr=no_tmax) == 0   # tmax NULL: +Inf; rays from the origin along +z
        assert Q.status(r) == Q.CLEAN and np.isfinite(head(ob["r"], n)).all()
        with pytest.raises(G.PbrtError):   # the wrapper's own check: a buffer shorter than n
            r.li_device(rb, gb, n + PAD + 1, ob)
        with pytest.raises(G.PbrtError):
            r.li_device(rb, gb, n, {k: v for k, v in ob.items() if k != "g"})


REFUSALS = {
    "direct_lighting": (lambda: G.Scene.readme(32, 32), dict(integrator=abi.PBRT_INTEGRATOR_DIRECT_LIGHTING), "Path"),
    "rough_glass": (lambda: material_scene(rough=0.2), {}, "rough glass"),
    "strategy_3": (lambda: G.Scene.readme(32, 32), dict(light_strategy=3), "strategy"),
    "max_depth_2049": (lambda: G.Scene.readme(32, 32), dict(max_depth=2049), "2048"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(name):
    make, desc, word = REFUSALS[name]
    n = 16
    with G.Renderer(make()) as r:
        rays = np.zeros((n, 7))
        rays[:, 5] = 1.0
        rb, gb = upload_batch(r, rays, np.arange(n, dtype=np.uint64), np.ones(n, dtype=np.uint64))
        ob = {k: padded(r, n, dt) for k, dt in G.LI_DTYPES.items()}
        assert r.li_device(rb, gb, n, ob, **desc) == abi.PBRT_E_UNSUPPORTED
        assert word in r.last_error(), r.last_error()   # the reason is named
        assert Q.status(r) == Q.CLEAN
        for b in ob.values():   # nothing was enqueued
            assert (b.download() == SENTINEL[b.dtype]).all()
        assert r.li_device(rb, gb, 0, ob, **desc) == abi.PBRT_E_UNSUPPORTED   # n = 0 is refused alike


def test_frames_around_a_query_and_strategies_in_turn():
    """Frame, query, frame on one context: both films are the oracle's and the query is the
    batch's. Then the two strategies in turn, which uploads the query's own distribution each
    time the strategy changes: Uniform gives the batch's bits, Power its own (black, three draws
    a bounce), every time; a frame rendered under Power uses the frame's own buffer and leaves
    the query's alone."""
    scene, s, full, _, _ = readme_batch()
    n = 257
    rd = abi.render_desc(2, 2)
    rc, ofilm, _ = O.render(scene.desc, rd, threads=THREADS)
    assert rc == 0
    with G.Renderer(scene) as r:
        rb0 = sample_rays(r, R.Samples(*[v[:n] for v in s]))
        gb = {"state": padded(r, n, np.uint64, s.state[:n]), "inc": padded(r, n, np.uint64, s.inc[:n])}
        film1, _ = r.render(rd)
        got = li(r, rb0, gb, n, max_depth=5)
        film2, _ = r.render(rd)
        assert np.array_equal(bits(film1), bits(ofilm)) and np.array_equal(bits(film2), bits(ofilm))
        same_batch = lambda g: all(same(g[k], full[k][:n]) for k in OUT_KEYS)   # noqa: E731
        assert same_batch(got)
        power = li(r, rb0, gb, n, max_depth=5, light_strategy=POWER)
        assert not power["g"].any() and not (power["rays"] >> 16).any() and (power["draws"] < got["draws"]).any()
        for _ in range(2):
            assert same_batch(li(r, rb0, gb, n, max_depth=5, light_strategy=UNIFORM))
            again = li(r, rb0, gb, n, max_depth=5, light_strategy=POWER)
            assert all(same(again[k], power[k]) for k in OUT_KEYS)
        assert all(same(li(r, rb0, gb, n, max_depth=5, light_strategy=POWER)[k], power[k]) for k in OUT_KEYS)   # no change
        prd = abi.render_desc(2, 2, light_strategy=POWER)
        rc, pfilm, _ = O.render(scene.desc, prd, threads=THREADS)
        film3, _ = r.render(prd)
        assert rc == 0 and np.array_equal(bits(film3), bits(pfilm))
        assert all(same(li(r, rb0, gb, n, max_depth=5, light_strategy=POWER)[k], power[k]) for k in OUT_KEYS)
        assert same_batch(li(r, rb0, gb, n, max_depth=5, light_strategy=UNIFORM))
        assert Q.status(r) == Q.CLEAN


def test_radiance_convenience():
    scene, s, full, _, _ = readme_batch()
    n = 300
    with G.Renderer(scene) as r:
        rb0 = sample_rays(r, R.Samples(*[v[:n] for v in s]))
        rays = np.stack([head(rb0[k], n) for k in RAY_KEYS], axis=1)
        L, state, draws, nrays = r.radiance(rays, s.state[:n], s.inc[:n], max_depth=5)
        L6, _, _, _ = r.radiance(rays[:, :6], s.state[:n], s.inc[:n], max_depth=5)   # no tmax: +Inf
    want = np.stack([full["r"][:n], full["g"][:n], full["b"][:n]], axis=1)
    assert np.array_equal(bits(L), bits(want)) and np.array_equal(bits(L6), bits(want))
    assert np.array_equal(state, full["state"][:n]) and np.array_equal(draws, full["draws"][:n])
    assert np.array_equal(nrays, full["rays"][:n])

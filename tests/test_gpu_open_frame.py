"""A frame from public pieces on the GPU: pbrt_gpu_frame_samples_device,
pbrt_gpu_li_device, pbrt_gpu_film_add_device, pbrt_gpu_film_rgba8_device
(Renderer.frame_samples / li_device / film_add / film_rgba8 / render_samples;
go-pbrt_amd/csrc/k_film_q.hip).

1. frame_samples against tests/li_reference.py's samples() bit for bit, its rays
   against pbrt_gpu_camera_rays_device on each sample's 1 x 1 window
   (tests/test_gpu_li.py's sample_rays), a tile sub-range against its slice.
2. film_add against li_reference.film() in numpy, on random radiances with NaN,
   negative and zero entries: three films, four filter radii, three tile sizes,
   1, 2 and 5 samples a pixel, both gather kernels, one call and three ascending
   ranges.
3. The composed frame against the oracle's THROUGHPUT n_dims = 0 film, and
   against the library's own wave_cam frame; render_samples over several ranges.
4. film_rgba8 against the host's pbrt_film_to_rgba8 on special values and on a
   rendered device film.
5. The launch log of each call, and that a second call allocates nothing.
6. Renders around a composed frame, calls during a render, empty ranges, refusals.

Every buffer handed to a call is 64 elements longer than the call needs and
pre-filled with a sentinel (tests/test_gpu_li.py's); tails must come back
intact and inputs untouched.
"""
import functools

import numpy as np
import pytest

import li_reference as R
import oracle_lib as O
import pbrtgpu as G
import test_gpu_li as T
import test_gpu_query as Q
from pbrtgpu import abi
from test_gpu_wave_cam import lens_scene

pytestmark = pytest.mark.gpu

PAD, SENTINEL = T.PAD, T.SENTINEL
padded, head, bits, same = T.padded, T.head, T.bits, T.same
SPP = T.SPP
CROP = (0.25, 0.1, 0.8, 0.9)
SAMPLE_KEYS = tuple(G.SAMPLE_DTYPES)
INV, UNS = abi.PBRT_E_INVALID, abi.PBRT_E_UNSUPPORTED


def names_since(r, before):
    return [rec.name for rec in r.launches(outside=True)[before:]]


def sample_buffers(r, n, keys=SAMPLE_KEYS):
    return {k: padded(r, n, G.SAMPLE_DTYPES[k]) for k in keys}


# ------------------------------------------------------------------- 1. samples
SAMPLE_FILMS = {
    "readme40x24": (lambda: G.Scene.readme(40, 24), 16),
    "readme45x30_tile13": (lambda: G.Scene.readme(45, 30), 13),
    # the cropped film, behind a thin lens: the two lens draws reach the ray
    "crop64x40_lens": (lambda: lens_scene(w=64, h=40, lens=0.3, crop=CROP), 16),
    "crop64x40_tile8": (lambda: lens_scene(w=64, h=40, lens=0.0, crop=CROP), 8),
}


@pytest.mark.parametrize("name", sorted(SAMPLE_FILMS))
def test_samples_are_the_references(name):
    make, ts = SAMPLE_FILMS[name]
    scene = make()
    fd = scene.desc.film
    ns = SPP - 1
    s = R.samples(fd, SPP, tile_size=ts)
    n = len(s.k)
    nt = R.num_tiles(fd, ts)
    with G.Renderer(scene) as r:
        assert r.num_tiles(ts) == nt and r.frame_count(ns, tile_size=ts) == n
        ob = sample_buffers(r, n)
        before = len(r.launches(outside=True))
        assert r.frame_samples(ob, ns, tile_size=ts) == 0, r.last_error()
        assert names_since(r, before) == ["k_frame_samples"]
        rec = r.launches(outside=True)[-1]
        assert rec.block == (256, 1, 1) and rec.grid == ((n + 255) // 256, 1, 1) and rec.lds == 0
        got = {k: head(b, n) for k, b in ob.items()}
        assert np.array_equal(got["state"], s.state) and np.array_equal(got["inc"], s.inc)
        assert np.array_equal(got["px"], s.px.astype(np.int32)) and np.array_equal(got["py"], s.py.astype(np.int32))
        assert same(got["pfilm_x"], s.px.astype(np.float64) + s.film_x)
        assert same(got["pfilm_y"], s.py.astype(np.float64) + s.film_y)
        assert ((got["pfilm_x"] >= s.px) & (got["pfilm_x"] < s.px + 1)).all()   # film_add's contract holds
        rb = T.sample_rays(r, s)   # camera_rays_device on each sample's own 1 x 1 window
        for k in T.RAY_KEYS:
            assert same(got[k], head(rb[k], n)), k
        assert np.isinf(got["tmax"]).all()
        # a tile sub-range is the matching slice; without the optional outputs
        for b, e in ((1, nt - 1), (nt - 1, nt), (0, 1)):
            lo, hi = r.frame_count(ns, 0, b, ts), r.frame_count(ns, 0, e, ts)
            assert (lo, hi) == (int((s.tile < b).sum()), int((s.tile < e).sum())) and r.frame_count(ns, b, e, ts) == hi - lo
            sub = sample_buffers(r, hi - lo, G.SAMPLE_REQUIRED)
            assert r.frame_samples(sub, ns, b, e, ts) == 0
            for k in G.SAMPLE_REQUIRED:
                assert same(head(sub[k], hi - lo), got[k][lo:hi]), (b, e, k)
        assert Q.status(r) == Q.CLEAN


# --------------------------------------------------- 2. film_add against numpy
ADD_FILMS = {"40x24": (40, 24, (0, 0, 1, 1)), "45x30": (45, 30, (0, 0, 1, 1)), "crop64x40": (64, 40, CROP)}
RADII = (0.5, 1.0, 1.5, 2.7)
TILES = (8, 13, 16)
ADD_CASES = [(f, rad, ts, (1, 2, 5)[(i + j + k) % 3])
             for i, f in enumerate(sorted(ADD_FILMS)) for j, rad in enumerate(RADII) for k, ts in enumerate(TILES)]
ADD_CASES.append(("40x24", 1.0, 32, 2))   # a tile film of 34 x 34 pixels: beyond the LDS gather's 512


def random_radiance(n, seed):
    rng = np.random.default_rng(seed)
    L = rng.uniform(-0.5, 4.0, size=(n, 3))
    L[rng.random(n) < 0.05] = 0.0
    L[rng.random(n) < 0.03, rng.integers(0, 3)] = np.nan   # one component NaN: the whole sample becomes 0.1
    L[rng.random(n) < 0.01] = np.nan
    L[0] = (np.nan, 1.0, -2.0)
    return L


@functools.lru_cache(maxsize=None)
def add_reference(film_key, radius, ts, ns):
    """(scene, samples, L, numpy film): computed once per case and shared read-only."""
    w, h, crop = ADD_FILMS[film_key]
    scene = lens_scene(w=w, h=h, lens=0.0, crop=crop, filter_radius=radius)
    fd = scene.desc.film
    assert (fd.filter_radius_x, fd.filter_radius_y) == (radius, radius) and not 0.0 > fd.max_sample_luminance
    s = R.samples(fd, ns + 1, tile_size=ts)
    L = random_radiance(len(s.k), seed=int(radius * 10) + ts + ns)
    want = R.film(fd, s, L, tile_size=ts)
    for a in (L, want):
        a.setflags(write=False)
    return scene, s, L, want


def upload_film_samples(r, s, L):
    n = len(s.k)
    host = {"pfilm_x": s.px.astype(np.float64) + s.film_x, "pfilm_y": s.py.astype(np.float64) + s.film_y,
            "r": L[:, 0], "g": L[:, 1], "b": L[:, 2]}
    return {k: padded(r, n, np.float64, v) for k, v in host.items()}, host


def film_buffer(r, fill=None):
    n = r.hgt * r.w * 3
    return padded(r, n, np.float64, fill), n


@pytest.mark.parametrize("film_key,radius,ts,ns", ADD_CASES)
def test_film_add_is_the_numpy_film(film_key, radius, ts, ns, monkeypatch):
    scene, s, L, want = add_reference(film_key, radius, ts, ns)
    n, nt = len(s.k), R.num_tiles(scene.desc.film, ts)
    lds_fits = (ts + 2 * (int(radius) + 1)) ** 2 <= 512
    for variant in ("lds", "direct"):
        monkeypatch.setenv("PBRT_FILM_ADD", variant)   # read when the context is created
        with G.Renderer(scene) as r:
            sb, host = upload_film_samples(r, s, L)
            fb, fn = film_buffer(r)   # sentinel-filled: the clear flag must zero what no tile reaches
            before = len(r.launches(outside=True))
            assert r.film_add(sb, ns, fb, tile_size=ts, clear=True) == 0, r.last_error()
            tiles = "k_film_add_tiles<true>" if variant == "lds" and lds_fits else "k_film_add_tiles<false>"
            assert names_since(r, before) == [tiles, "k_film_add_merge"]
            rec = r.launches(outside=True)[-2]
            assert rec.grid == (nt, 1, 1) and rec.block == (256, 1, 1)
            one = head(fb, fn).reshape(want.shape)
            assert np.array_equal(bits(one), bits(want)), (variant, int((bits(one) != bits(want)).sum()))
            for k in host:   # the inputs came back untouched
                assert same(head(sb[k], n), host[k]), k
            # three ascending ranges, the clear flag on the first only, into a film that held something else;
            # a range's samples start at element 0 of its arrays (a film of two tiles: the third range is empty)
            fb3, _ = film_buffer(r, np.full(fn, 7.25))
            cuts = [0, max(1, nt // 3), max(2, nt - 1), nt] if nt >= 3 else [0, 1, nt, nt]
            for i in range(3):
                b, e = cuts[i], cuts[i + 1]
                lo, hi = r.frame_count(ns, 0, b, ts), r.frame_count(ns, 0, e, ts)
                part = {k: padded(r, hi - lo, np.float64, host[k][lo:hi]) for k in host}
                assert r.film_add(part, ns, fb3, b, e, ts, clear=i == 0) == 0, r.last_error()
            assert np.array_equal(bits(head(fb3, fn).reshape(want.shape)), bits(want)), variant
            assert Q.status(r) == Q.CLEAN
    assert np.isfinite(want).all() and (want != 0).any()


def test_film_add_leaves_its_inputs_and_other_rows_alone():
    """The inputs are untouched; without the clear flag a range adds to what the film holds and
    leaves the rows its tile films do not reach as they are. (That the additions continue in the
    single call's order, bit for bit, is the three ranges of test_film_add_is_the_numpy_film;
    here the sum is base + (the range's film), a different association where two tile films
    overlap, so those pixels are compared to a few roundings: 4 additions of 2^-53 each.)"""
    scene, s, L, want = add_reference("45x30", 1.0, 13, 2)
    fd = scene.desc.film
    ts, ns, nt = 13, 2, R.num_tiles(fd, 13)
    with G.Renderer(scene) as r:
        sb, host = upload_film_samples(r, s, L)
        base = np.random.default_rng(3).uniform(0, 1, size=want.size)
        fb, fn = film_buffer(r, base)
        last = (nt - 4, nt)   # the last tile row: 4 tiles of 13 over 45 pixels
        assert R.tile_bounds(fd, ts, last[0])[1] == 26
        lo = r.frame_count(ns, 0, last[0], ts)
        sub = {k: padded(r, len(s.k) - lo, np.float64, host[k][lo:]) for k in host}
        assert r.film_add(sub, ns, fb, last[0], last[1], ts) == 0
        got = head(fb, fn).reshape(want.shape)
        for k in host:
            assert same(head(sb[k], len(s.k)), host[k]) and same(head(sub[k], len(s.k) - lo), host[k][lo:]), k
        # (film() walks every tile; the samples of the other tiles are absent, so it is the range's film)
        part = R.film(fd, R.Samples(*[v[lo:] for v in s]), L[lo:], tile_size=ts)
        assert not part[:25].any() and part[25:].any()   # radius 1: the row's tile films begin one row above it
        assert np.array_equal(bits(got[:25]), bits(base.reshape(want.shape)[:25]))
        total = base.reshape(want.shape) + part
        assert np.allclose(got, total, rtol=0, atol=4 * 2.0 ** -53 * np.abs(total).max())
        assert (got[25:] != base.reshape(want.shape)[25:]).any()


# ------------------------------------------------------- 3. the composed frame
COMPOSED = ("readme40x24", "glass", "mesh_spheres", "crowd_matte")


def compose(r, case, ts=16, ranges=None):
    """frame_samples, li_device, film_add over tile ranges on padded buffers; (film, closest, shadow)."""
    ns = SPP - 1
    nt = r.num_tiles(ts)
    fb, fn = film_buffer(r)
    closest = shadow = 0
    for i, (b, e) in enumerate(ranges or [(0, nt)]):
        n = r.frame_count(ns, b, e, ts)
        sb = sample_buffers(r, n, G.SAMPLE_REQUIRED)
        ob = {k: padded(r, n, G.LI_DTYPES[k]) for k in ("r", "g", "b", "rays")}
        assert r.frame_samples(sb, ns, b, e, ts) == 0, r.last_error()
        rc = r.li_device({k: sb[k] for k in G.RAY_KEYS}, {k: sb[k] for k in G.RNG_KEYS}, n, ob,
                         max_depth=case.max_depth, light_strategy=case.strategy)
        assert rc == 0, r.last_error()
        fs = dict(pfilm_x=sb["pfilm_x"], pfilm_y=sb["pfilm_y"], r=ob["r"], g=ob["g"], b=ob["b"])
        assert r.film_add(fs, ns, fb, b, e, ts, clear=i == 0) == 0, r.last_error()
        rays = head(ob["rays"], n)
        closest += int((rays & 0xFFFF).sum())
        shadow += int((rays >> 16).sum())
        for b_ in list(sb.values()) + list(ob.values()):
            head(b_, n)   # no stage wrote past n
    film = head(fb, fn).reshape(r.hgt, r.w, 3)
    assert Q.status(r) == Q.CLEAN
    return film, closest, shadow


@pytest.mark.parametrize("name", COMPOSED)
def test_composed_frame_is_the_oracles(name):
    case = T.CASES[name]
    scene, ofilm, ost = T.oracle_film(case)
    with G.Renderer(scene) as r:
        film, closest, shadow = compose(r, case)
        assert np.array_equal(bits(film), bits(ofilm)), int((bits(film) != bits(ofilm)).sum())
        assert (closest, shadow) == (ost.closest_rays, ost.shadow_rays)
        # render_samples: the same frame in at least three tile ranges
        ns = SPP - 1
        budget = G.FRAME_BYTES_PER_SAMPLE * ns * 16 * 16 * 2   # two tiles of 16 x 16 a range
        rfilm, info = r.render_samples(SPP, case.max_depth, case.strategy, budget_bytes=budget, count_rays=True)
        assert info["ranges"] >= 3 and info["samples"] == ost.paths
        assert np.array_equal(bits(rfilm), bits(ofilm))
        assert (info["closest_rays"], info["shadow_rays"]) == (ost.closest_rays, ost.shadow_rays)
    if name == "readme40x24":   # Matte: the library's own camera-start frame is the same film
        rd = abi.render_desc(SPP, 1, n_dims=0, max_depth=case.max_depth, light_strategy=case.strategy,
                             mode=abi.PBRT_MODE_THROUGHPUT)
        with G.Renderer(scene, kernel="wave_cam") as r:
            wfilm, _ = r.render(rd)
        assert np.array_equal(bits(film), bits(wfilm))


# --------------------------------------------------------------------- 4. RGBA8
def special_film(w, h):
    one_up = np.nextafter(1.0, 2.0)
    special = [np.nan, -np.nan, 0.0, -0.0, 5e-324, -5e-324, 2.2e-308, 0.999999, 1.0, one_up, np.nextafter(1.0, 0.0),
               255.5, 256.0, 1e300, np.inf, -np.inf, -1.0, 0.5, 1.0 / 255, np.nextafter(1.0 / 255, 0.0), 254.0 / 255,
               0.003921568627450981, 0.00392156862745098]
    rng = np.random.default_rng(11)
    film = rng.uniform(-0.25, 1.25, size=(h, w, 3))
    film.reshape(-1)[:len(special)] = special
    film.reshape(-1)[-len(special):] = special[::-1]
    return film


@pytest.mark.parametrize("w,h", [(40, 24), (45, 31), (1, 1), (257, 3)])
def test_rgba8_is_the_hosts(w, h):
    film = special_film(w, h) if w * h * 3 >= 46 else np.array([[[np.nan, 1.0, 0.5]]])
    want = G.film_to_rgba8(film)
    with G.Renderer(G.Scene.readme(32, 32)) as r:
        fb = padded(r, w * h * 3, np.float64, film.ravel())
        ob = padded(r, w * h * 4, np.uint8)
        before = len(r.launches(outside=True))
        assert r.film_rgba8(fb, ob, w, h) is ob
        assert names_since(r, before) == ["k_film_rgba8"]
        assert r.launches(outside=True)[-1].grid == ((w * h + 255) // 256, 1, 1)
        got = head(ob, w * h * 4).reshape(h, w, 4)
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
        assert same(head(fb, w * h * 3), film.ravel())   # the film is untouched
        assert (got[..., 3] == 255).all() and got[..., :3].min() == 0 and got[..., :3].max() == 255


def test_rgba8_of_a_rendered_device_film():
    """The device film of a render_async into a caller buffer, README 64x48."""
    scene = G.Scene.readme(64, 48)
    rd = abi.render_desc(2, 2)
    with G.Renderer(scene) as r:
        fb, fn = film_buffer(r)
        r.render_async(rd, fb.ptr)
        r.synchronize()
        film = head(fb, fn).reshape(48, 64, 3)
        rc, ofilm, _ = O.render(scene.desc, rd, threads=T.THREADS)
        assert rc == 0 and np.array_equal(bits(film), bits(ofilm))
        want = G.film_to_rgba8(film)
        got = r.film_rgba8(fb).download().reshape(48, 64, 4)   # into a buffer of the call's own
        assert np.array_equal(got, want) and len(np.unique(got[..., :3])) > 50
        # the context's own film by its address
        r.render(rd)
        got2 = r.film_rgba8(r.film_device_ptr()).download().reshape(48, 64, 4)
        assert np.array_equal(got2, want)


# -------------------------------------------------- 5. launches and allocations
def test_launch_log_and_no_allocation_on_the_second_call():
    scene, s, L, want = add_reference("45x30", 1.5, 16, 2)
    ts, ns, n = 16, 2, len(s.k)
    with G.Renderer(scene) as r:
        sb, _ = upload_film_samples(r, s, L)
        ob = sample_buffers(r, n)
        fb, _ = film_buffer(r)
        rgba = padded(r, r.w * r.hgt * 4, np.uint8)
        assert r.film_scratch_bytes() == 0
        sizes = []
        for _ in range(2):
            before = len(r.launches(outside=True))
            assert r.frame_samples(ob, ns, tile_size=ts) == 0
            assert names_since(r, before) == ["k_frame_samples"]
            before = len(r.launches(outside=True))
            assert r.film_add(sb, ns, fb, tile_size=ts, clear=True) == 0
            assert names_since(r, before) == ["k_film_add_tiles<true>", "k_film_add_merge"]
            before = len(r.launches(outside=True))
            r.film_rgba8(fb, rgba)
            assert names_since(r, before) == ["k_film_rgba8"]
            sizes.append(r.film_scratch_bytes())
        nt = R.num_tiles(scene.desc.film, ts)
        assert sizes == [nt * 20 * 20 * 3 * 8] * 2   # the tile films of the range, (16 + 2 * 2)^2 pixels each
        assert r.film_add(sb, ns, fb, 0, 2, ts) == 0   # a smaller range fits what there is
        assert r.film_scratch_bytes() == sizes[0]
        assert np.array_equal(head(rgba, r.w * r.hgt * 4).reshape(r.hgt, r.w, 4), G.film_to_rgba8(want))
        assert Q.status(r) == Q.CLEAN


# ---------------------------------------------------------- 6. around renders
def test_renders_around_a_composed_frame_and_calls_during_one():
    case = T.CASES["readme40x24"]
    scene, ofilm, ost = T.oracle_film(case)
    rd = abi.render_desc(2, 2)
    rc, efilm, _ = O.render(scene.desc, rd, threads=T.THREADS)
    assert rc == 0
    ns, ts = SPP - 1, 16
    with G.Renderer(scene) as r:
        film1, _ = r.render(rd)
        film, closest, shadow = compose(r, case, ranges=[(0, 2), (2, 3), (3, 6)])
        film2, _ = r.render(rd)
        assert np.array_equal(bits(film1), bits(efilm)) and np.array_equal(bits(film2), bits(efilm))
        assert np.array_equal(bits(film), bits(ofilm)) and (closest, shadow) == (ost.closest_rays, ost.shadow_rays)
        # during a render every call is refused and the render is left alone
        n = r.frame_count(ns, tile_size=ts)
        ob = sample_buffers(r, n)
        fs = {k: padded(r, n, np.float64, np.ones(n)) for k in G.FILM_KEYS}
        fb, _ = film_buffer(r)
        rgba = padded(r, r.w * r.hgt * 4, np.uint8)
        before = len(r.launches(outside=True))
        r.render_async(rd)
        rcs = [r.frame_samples(ob, ns, tile_size=ts), r.film_add(fs, ns, fb, tile_size=ts, clear=True)]
        with pytest.raises(G.PbrtError) as err:
            r.film_rgba8(fb, rgba)
        r.synchronize()
        assert rcs == [INV, INV] and err.value.code == INV and "in flight" in r.last_error()
        assert np.array_equal(bits(r.film()), bits(efilm))
        assert names_since(r, before) == []
        for b in list(ob.values()) + [fb, rgba]:   # nothing was written
            assert (b.download() == SENTINEL[b.dtype]).all()
        # an empty range is PBRT_OK and launches nothing
        for b, e in ((0, 0), (3, 3), (6, 6)):
            assert r.frame_samples(ob, ns, b, e, ts) == 0 and r.film_add(fs, ns, fb, b, e, ts) == 0
        assert names_since(r, before) == [] and (fb.download() == SENTINEL[fb.dtype]).all()
        assert Q.status(r) == Q.CLEAN


REFUSALS = {
    "tile_257": (dict(tile_size=257, tile_end=1), UNS, "256", True),
    "radius_not_below_the_tile": (dict(tile_size=2, tile_end=4), UNS, "filter radius", False),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_their_reason_and_write_nothing(name):
    kw, code, word, samples_too = REFUSALS[name]
    scene = lens_scene(w=40, h=24, lens=0.0, filter_radius=2.7)
    with G.Renderer(scene) as r:
        n = 4096
        ob = sample_buffers(r, n)
        fs = {k: padded(r, n, np.float64, np.ones(n)) for k in G.FILM_KEYS}
        fb, _ = film_buffer(r)
        before = len(r.launches(outside=True))
        assert r.film_add(fs, 1, fb, clear=True, **kw) == code and word in r.last_error(), r.last_error()
        if samples_too:
            assert r.frame_samples(ob, 1, **kw) == code and word in r.last_error()
        else:   # the samples do not depend on the filter
            assert r.frame_samples(ob, 1, **kw) == 0
            want_px = np.array([2 * t + dx for t in range(4) for _ in range(2) for dx in range(2)], dtype=np.int32)
            assert same(head(ob["px"], n)[:16], want_px) and (head(ob["px"], n)[16:] == SENTINEL[np.dtype(np.int32)]).all()
        assert [k for k in names_since(r, before) if k != "k_frame_samples"] == []
        assert (fb.download() == SENTINEL[fb.dtype]).all()
        with pytest.raises(G.PbrtError):   # the wrapper's own checks: a tile range outside the film, short buffers
            r.frame_samples(ob, 1, 0, 99)
        with pytest.raises(G.PbrtError):
            r.film_add(fs, 5, fb)
        with pytest.raises(G.PbrtError):
            r.film_add({k: v for k, v in fs.items() if k != "g"}, 1, fb)
        assert Q.status(r) == Q.CLEAN

"""The public pieces under sampler.Stratified on the GPU:
pbrt_gpu_frame_samples_stratified_device (k_strat_pixels) and
pbrt_gpu_li_stratified_device (k_li_strat<kX, kDepth>), go-pbrt_amd/csrc/k_strat.hip.
Every comparison is bit for bit; there is no tolerance in this module.

1. frame_samples_stratified against tests/strat_reference.py: the tables, k, table, state
   (mb_state advanced by camera_draws), inc, pFilm = the pixel, and the rays against
   pbrt_gpu_camera_rays_device for the same camera sample; every StartPixel form
   (buffered, windowed, serial); two tile ranges equal one call.
2. The composed frame (samples, li_stratified_device at the cursors after the camera
   sample, film_add) against the oracle's THROUGHPUT film and against pbrt_gpu_render
   in THROUGHPUT mode, film and ray counts; render_samples_stratified over >= 3 ranges.
3. With first_1d = first_2d = n_dims, li_stratified_device is li_device in every output
   and in the panic record, on tests/li_rays.py's rays (which test_gpu_li_rays' check_li
   holds equal to the oracle's per-ray Path.Li), for the four instantiations.
4. Cursor shift: tables of N + 1 rows with row d + 1 = the frame's row d, queried with
   cursors (2, 3), give the frame's own radiances, draws and states at (1, 2).
5. Out-of-range table / k values on exactly sized arrays leave every other ray's bits.
6. Refusals launch nothing; a render in flight; n == 0 and empty ranges; a steady-state
   call is one launch and allocates nothing.
"""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np
import pytest

import li_rays as LR
import li_reference as R
import oracle_lib as O
import pbrtgpu as G
import strat_reference as S
import test_gpu_li as T
import test_gpu_li_rays as TR
import test_gpu_query as Q
from large_scenes import MATTE, crowd
from pbrtgpu import abi
from scenes import material_scene
from test_gpu_wave_cam import lens_scene

pytestmark = pytest.mark.gpu

padded, head, bits, same = T.padded, T.head, T.bits, T.same
UNIFORM, POWER = T.UNIFORM, T.POWER
INV, UNS = abi.PBRT_E_INVALID, abi.PBRT_E_UNSUPPORTED
STRAT_DTYPES = {"k": np.int32, "table": np.int32, "s1d": np.float64}
CamSamples = namedtuple("CamSamples", "k px py film_x film_y lens_u lens_v time_u")


def names_since(r, before):
    return [rec.name for rec in r.launches(outside=True)[before:]]


def hip_free_bytes():
    hip = C.CDLL(G.hip_runtimes()[0])
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def strat_samples(r, sx, sy, nd, jitter, ts=16, b=0, e=None, keys=tuple(G.SAMPLE_DTYPES)):
    """frame_samples_stratified of a tile range into fresh padded buffers: (n, pixels, sample buffers, strat buffers)."""
    spp = sx * sy
    n = r.frame_count(spp - 1, b, e, ts)
    npx = n // (spp - 1)
    sb = {k: padded(r, n, G.SAMPLE_DTYPES[k]) for k in keys}
    kb = {"k": padded(r, n, np.int32), "table": padded(r, n, np.int32), "s1d": padded(r, npx * nd * spp, np.float64)}
    rc = r.frame_samples_stratified(sb, kb, sx, sy, nd, jitter, b, e, ts)
    assert rc == 0, (rc, r.last_error())
    return n, npx, sb, kb


# ---------------------------------------------------------- 1. tables and samples
Shape = namedtuple("Shape", "scene ts sx sy nd jitter form every")
SHAPES = {
    "s2x2_nd4": Shape(lambda: G.Scene.readme(45, 30), 16, 2, 2, 4, False, 0, 1),
    "s3x3_nd1_jitter_pinhole": Shape(lambda: G.Scene.readme(45, 30), 16, 3, 3, 1, True, 0, 3),
    "s3x3_nd1_jitter_lens": Shape(lambda: lens_scene(w=45, h=30, lens=0.3), 16, 3, 3, 1, True, 0, 3),
    "s1x2_nd2": Shape(lambda: G.Scene.readme(45, 30), 16, 1, 2, 2, False, 0, 1),   # one traced sample
    "s11x11_nd4_windowed": Shape(lambda: G.Scene.readme(16, 16), 16, 11, 11, 4, False, 2, 37),
    # 4 * (2 + 3) * 49 events and their rejection margin: 4664 bytes of raw draws, beyond sp_serial's 4 KB
    "s7x7_nd4_jitter_serial": Shape(lambda: G.Scene.readme(16, 16), 16, 7, 7, 4, True, 1, 11),
    "s2x2_nd3_tile13": Shape(lambda: G.Scene.readme(45, 30), 13, 2, 2, 3, False, 0, 5),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_tables_and_samples_are_the_references(name):
    sh = SHAPES[name]
    scene = sh.scene()
    fd = scene.desc.film
    spp, ns = sh.sx * sh.sy, sh.sx * sh.sy - 1
    fr = S.frame(fd, sh.sx, sh.sy, sh.nd, sh.jitter, tile_size=sh.ts)
    nt = R.num_tiles(fd, sh.ts)
    with G.Renderer(scene) as r:
        before = len(r.launches(outside=True))
        n, npx, sb, kb = strat_samples(r, sh.sx, sh.sy, sh.nd, sh.jitter, sh.ts)
        assert names_since(r, before) == ["k_strat_pixels"]
        rec = r.launches(outside=True)[-1]
        assert rec.block == (64, 1, 1) and rec.grid == (npx, 1, 1) and 0 < rec.lds <= 48 * 1024   # one wave per pixel
        assert (n, npx) == (len(fr.k), fr.tables.shape[0]) and npx == r.frame_count(1, tile_size=sh.ts)
        got = {k: head(b, n) for k, b in sb.items()}
        tables = head(kb["s1d"], npx * sh.nd * spp).reshape(npx, sh.nd, spp)
        assert np.array_equal(bits(tables), bits(fr.tables)), int((bits(tables) != bits(fr.tables)).sum())
        assert same(head(kb["k"], n), fr.k) and same(head(kb["table"], n), fr.table)
        assert np.array_equal(got["state"], fr.state) and np.array_equal(got["inc"], fr.inc)
        assert np.array_equal(got["state"], R.pcg_advance(fr.start, fr.inc, S.camera_draws(sh.nd)))
        assert np.array_equal(got["px"], fr.px.astype(np.int32)) and np.array_equal(got["py"], fr.py.astype(np.int32))
        assert same(got["pfilm_x"], fr.px.astype(np.float64)) and same(got["pfilm_y"], fr.py.astype(np.float64))
        assert np.isinf(got["tmax"]).all()
        # the rays: camera_rays_device on each (every `every`-th) sample's own 1 x 1 window, pFilm offset (0, 0),
        # the lens values drawn (n_dims 1) or (0, 0), the time the pixel's s1d[0][k]
        pick = np.arange(0, n, sh.every)
        cs = CamSamples(fr.k[pick], fr.px[pick], fr.py[pick], np.zeros(len(pick)), np.zeros(len(pick)), fr.lens_u[pick],
                        fr.lens_v[pick], fr.tables[fr.table[pick], 0, fr.k[pick]])
        rb = T.sample_rays(r, cs)
        for k in T.RAY_KEYS:
            assert same(got[k][pick], head(rb[k], len(pick))), k
        if "lens" in name:   # the two lens draws reach the ray: a pixel's samples differ
            assert len({got["ox"][i].tobytes() for i in range(ns)}) == ns and fr.lens_u.any()
        else:
            assert all(same(got[k][:ns], np.repeat(got[k][:1], ns)) for k in T.RAY_KEYS)
        # two tile ranges are one call; without the optional outputs
        cut = max(1, nt // 2)
        parts = [strat_samples(r, sh.sx, sh.sy, sh.nd, sh.jitter, sh.ts, b, e, G.SAMPLE_REQUIRED) for b, e in ((0, cut), (cut, nt))]
        lo = 0
        for pn, ppx, psb, pkb in parts:
            for k in G.SAMPLE_REQUIRED:
                assert same(head(psb[k], pn), got[k][lo:lo + pn]), k
            assert same(head(pkb["k"], pn), fr.k[lo:lo + pn])
            assert same(head(pkb["table"], pn), fr.table[lo:lo + pn] - lo // ns)   # the index within the range
            assert same(head(pkb["s1d"], ppx * sh.nd * spp), fr.tables[lo // ns:lo // ns + ppx].ravel())
            lo += pn
        assert lo == n or nt == 1
        assert Q.status(r) == Q.CLEAN


def test_shapes_take_every_start_pixel_form():
    """The shapes above are on the sides of render_params' thresholds the host check computes
    (tests/strat_query_check.cpp prints the same plans): buffered, windowed and serial."""
    for name, sh in SHAPES.items():
        n = sh.sx * sh.sy
        events = sh.nd * ((2 * n if sh.jitter else n) + (3 * n if sh.jitter else n))
        serial = (events + 64 + events // 8) * 4 > 4 * 1024
        window = serial and not sh.jitter and sh.nd * n * 4 + 256 * 4 <= 6 * 1024
        assert sh.form == (2 if window else 1 if serial else 0), name
    assert {sh.form for sh in SHAPES.values()} == {0, 1, 2}


# ------------------------------------------------------------ 2. the composed frame
Case = namedtuple("Case", "scene nd max_depth strategy kernel sx sy jitter", defaults=(2, 2, False))
README = lambda: G.Scene.readme(45, 30)   # noqa: E731
COMPOSED = {
    **{f"readme_nd{nd}": Case(README, nd, 5, UNIFORM, "k_li_strat<false, 0>") for nd in (1, 2, 3, 4, 6)},
    "readme_nd4_power_d10": Case(README, 4, 10, POWER, "k_li_strat<false, 0>"),
    "readme_nd2_d1": Case(README, 2, 1, UNIFORM, "k_li_strat<false, 0>"),
    "readme_nd3_d10_jitter": Case(README, 3, 10, UNIFORM, "k_li_strat<false, 0>", 3, 2, True),
    # specular bounces take no light sample: Russian roulette lands on stratified dimensions
    "glass_nd4": Case(lambda: G.Scene.readme_glass(45, 30), 4, 10, UNIFORM, "k_li_strat<true, 0>"),
    # (the red sphere's Matte with sigma 30 is OrenNayar; the other spheres are Lambertian)
    "glass_nd6": Case(lambda: G.Scene.readme_glass(45, 30), 6, 10, UNIFORM, "k_li_strat<true, 0>"),
    "oren_nd4": Case(lambda: material_scene("matte", w=45, h=30, sigma=30.0), 4, 10, UNIFORM, "k_li_strat<true, 0>"),
    "oren_nd6": Case(lambda: material_scene("matte", w=45, h=30, sigma=30.0), 6, 10, UNIFORM, "k_li_strat<true, 0>"),
    "crowd_matte_nd4": Case(lambda: crowd(kinds=MATTE), 4, 5, UNIFORM, "k_li_strat<false, 64>"),   # 121 BVH nodes
    "crowd_kx_nd4": Case(crowd, 4, 8, UNIFORM, "k_li_strat<true, 64>"),
    "mesh_spheres_nd4": Case(lambda: G.Scene.heightfield(45, 30, quads=24, seed=1, spheres=True), 4, 5, UNIFORM,
                             "k_li_strat<false, 0>"),
    "lens_nd1": Case(lambda: lens_scene(w=45, h=30, lens=0.3), 1, 5, UNIFORM, "k_li_strat<false, 0>"),
    "lens_nd2": Case(lambda: lens_scene(w=45, h=30, lens=0.3), 2, 5, UNIFORM, "k_li_strat<false, 0>"),
}
LI_KEYS = ("r", "g", "b", "state", "draws", "rays")


def render_desc_of(case):
    return abi.render_desc(case.sx, case.sy, jitter=case.jitter, n_dims=case.nd, max_depth=case.max_depth,
                           light_strategy=case.strategy, mode=abi.PBRT_MODE_THROUGHPUT)


@functools.lru_cache(maxsize=None)
def oracle_film(name):
    case = COMPOSED[name]
    scene = case.scene()
    rc, film, st = O.render(scene.desc, render_desc_of(case), threads=T.THREADS)
    assert rc == 0 and np.isfinite(film).all()
    film.setflags(write=False)
    return film, st


def li_strat(r, case, sb, kb, n, n_tables, nd=None, cursors=None, keys=LI_KEYS):
    """li_stratified_device into fresh padded outputs; returns {key: the first n}."""
    nd = case.nd if nd is None else nd
    c1, c2 = abi.camera_cursors(nd) if cursors is None else cursors
    ob = {k: padded(r, n, G.LI_DTYPES[k]) for k in keys}
    rc = r.li_stratified_device({k: sb[k] for k in G.RAY_KEYS}, {k: sb[k] for k in G.RNG_KEYS}, n, ob, kb, n_tables,
                                case.sx * case.sy, nd, c1, c2, max_depth=case.max_depth, light_strategy=case.strategy)
    assert rc == 0, (rc, r.last_error())
    return {k: head(b, n) for k, b in ob.items()}, ob


def compose(r, case, ranges=None, ts=16):
    """frame_samples_stratified, li_stratified_device, film_add over tile ranges on padded buffers:
    (film, closest, shadow, the Li outputs of the last range)."""
    ns = case.sx * case.sy - 1
    nt = r.num_tiles(ts)
    fb = padded(r, r.hgt * r.w * 3, np.float64)
    closest = shadow = 0
    for i, (b, e) in enumerate(ranges or [(0, nt)]):
        n, npx, sb, kb = strat_samples(r, case.sx, case.sy, case.nd, case.jitter, ts, b, e, G.SAMPLE_REQUIRED)
        before = len(r.launches(outside=True))
        got, ob = li_strat(r, case, sb, kb, n, npx)
        assert names_since(r, before) == [case.kernel]
        rec = r.launches(outside=True)[-1]
        assert rec.block == (64, 1, 1) and rec.grid == ((n + 255) // 256, 1, 1) and rec.lds == 0
        fs = dict(pfilm_x=sb["pfilm_x"], pfilm_y=sb["pfilm_y"], r=ob["r"], g=ob["g"], b=ob["b"])
        assert r.film_add(fs, ns, fb, b, e, ts, clear=i == 0) == 0, r.last_error()
        closest += int((got["rays"] & 0xFFFF).sum())
        shadow += int((got["rays"] >> 16).sum())
        start, inc = head(sb["state"], n), head(sb["inc"], n)
        assert np.array_equal(got["state"], R.pcg_advance(start, inc, got["draws"]))   # draws counts PCG32 draws only
    film = head(fb, r.hgt * r.w * 3).reshape(r.hgt, r.w, 3)
    assert Q.status(r) == Q.CLEAN
    return film, closest, shadow, got


@pytest.mark.parametrize("name", sorted(COMPOSED))
def test_composed_frame_is_the_oracles_and_the_librarys(name):
    case = COMPOSED[name]
    ofilm, ost = oracle_film(name)
    scene = case.scene()
    with G.Renderer(scene) as r:
        film, closest, shadow, _ = compose(r, case)
        assert np.array_equal(bits(film), bits(ofilm)), int((bits(film) != bits(ofilm)).sum())
        assert (closest, shadow) == (ost.closest_rays, ost.shadow_rays)
        # (Power: every pick has pdf 0; max_depth 1: the path ends at its first closest-hit query)
        assert film.any() or case.strategy == POWER or case.max_depth == 1
        lfilm, lst = r.render(render_desc_of(case))   # the library's own THROUGHPUT frame, AUTO kernel
        assert np.array_equal(bits(film), bits(lfilm)), int((bits(film) != bits(lfilm)).sum())
        assert (closest, shadow) == (lst.rays_closest, lst.rays_shadow) and lst.paths_traced == ost.paths
        # render_samples_stratified: the same frame in at least three tile ranges
        spp = case.sx * case.sy
        budget = (G.STRAT_BYTES_PER_SAMPLE * (spp - 1) + 8 * case.nd * spp) * 16 * 16 * 2   # two tiles a range
        rfilm, info = r.render_samples_stratified(case.sx, case.sy, case.nd, case.jitter, case.max_depth, case.strategy,
                                                  budget_bytes=budget, count_rays=True)
        assert info["ranges"] >= 3 and info["samples"] == ost.paths
        assert np.array_equal(bits(rfilm), bits(ofilm))
        assert (info["closest_rays"], info["shadow_rays"]) == (ost.closest_rays, ost.shadow_rays)
        assert Q.status(r) == Q.CLEAN


def test_stratified_dimensions_reach_the_paths():
    """The cases are not vacuous: at n_dims 3 the frame differs from n_dims 2 (the bounce-1 uLight turns
    stratified), a path under n_dims 6 draws less than under n_dims 1, and on the glass scene some
    path of depth 10 reads a Russian-roulette value from a table (it ends with fewer draws than its
    closest-hit count allows for a path that drew every roulette value)."""
    f2, f3 = oracle_film("readme_nd2")[0], oracle_film("readme_nd3")[0]
    assert not np.array_equal(bits(f2), bits(f3))
    with G.Renderer(README()) as r:
        d1 = compose(r, COMPOSED["readme_nd1"])[3]["draws"]
        d6 = compose(r, COMPOSED["readme_nd6"])[3]["draws"]
    assert d6.sum() < d1.sum() and (d1 > 0).any()
    case = COMPOSED["glass_nd6"]
    with G.Renderer(case.scene()) as r:
        got = compose(r, case)[3]
    deep = (got["rays"] & 0xFFFF) > 4   # Russian roulette decided from the fifth iteration on
    assert deep.any()


# ------------------------------------------------------- 3. degenerate equality
DEGENERATE_FAMILIES = ("axis", "inside", "scaled", "tmax", "secondary", "degenerate")


@pytest.mark.parametrize("key", list(LR.SCENES))
def test_cursors_at_n_dims_is_li_device(key):
    """first_1d = first_2d = n_dims: no value is stratified. Every output and the panic record equal
    li_device's, which check_li holds equal to the oracle's per-ray Path.Li; n_dims 0 with no arrays too."""
    rng = np.random.default_rng(5)
    with G.Renderer(LR.SCENES[key]()) as r:
        for family in DEGENERATE_FAMILIES:
            b = LR.batch(key, family)
            li, n = TR.check_li(r, key, family)   # li_device against the oracle; the record is read (and cleared)
            o = LR.oracle_li(key, family)
            rb, gb = T.upload_batch(r, b.rays[:n], b.state[:n], b.inc[:n])
            for nd, spp, n_tables in ((3, 4, 5), (0, 0, 0)):
                kb = {}
                if nd:   # tables of poison and indices anywhere: none may be read for a value
                    kb = {"s1d": padded(r, n_tables * nd * spp, np.float64, np.full(n_tables * nd * spp, np.nan)),
                          "table": padded(r, n, np.int32, rng.integers(0, n_tables, n)),
                          "k": padded(r, n, np.int32, rng.integers(0, spp, n))}
                ob = {k: padded(r, n, G.LI_DTYPES[k]) for k in LI_KEYS}
                before = len(r.launches(outside=True))
                rc = r.li_stratified_device(rb, gb, n, ob, kb, n_tables, spp, nd, nd, nd, max_depth=LR.MAX_DEPTH)
                assert rc == 0, r.last_error()
                assert names_since(r, before) == [LR.kernel(key, "k_li_strat")]
                assert Q.status(r) == TR.record_of(o.panic[:n], o.status[:n]), (key, family, nd)
                for k in LI_KEYS:
                    assert head(ob[k], n).tobytes() == li[k].tobytes(), (key, family, nd, k)
        assert Q.status(r) == Q.CLEAN


# ------------------------------------------------------------- 4. cursor shift
@pytest.mark.parametrize("name", ["readme_nd2", "readme_nd4", "glass_nd4", "glass_nd2"])
def test_cursor_shift(name):
    case = COMPOSED.get(name) or COMPOSED["glass_nd4"]._replace(nd=2)
    N, spp = case.nd, case.sx * case.sy
    rng = np.random.default_rng(N)
    with G.Renderer(case.scene()) as r:
        n, npx, sb, kb = strat_samples(r, case.sx, case.sy, N, case.jitter, keys=G.SAMPLE_REQUIRED)
        want, _ = li_strat(r, case, sb, kb, n, npx)   # the oracle-pinned frame's query: cursors (1, 2) at N
        tables = head(kb["s1d"], npx * N * spp).reshape(npx, N, spp)
        shifted = np.concatenate([rng.random((npx, 1, spp)), tables], axis=1)   # row d + 1 = the frame's row d
        kb2 = dict(kb, s1d=padded(r, shifted.size, np.float64, shifted.ravel()))
        got, _ = li_strat(r, case, sb, kb2, n, npx, nd=N + 1, cursors=(2, 3))
        for k in LI_KEYS:
            assert got[k].tobytes() == want[k].tobytes(), (name, k)
        # and a shift that is wrong is seen: cursors (1, 2) on the shifted tables read row 0 and row 1
        other, _ = li_strat(r, case, sb, kb2, n, npx, nd=N + 1, cursors=(1, 2))
        assert any(other[k].tobytes() != want[k].tobytes() for k in ("r", "draws"))
        assert Q.status(r) == Q.CLEAN


# --------------------------------------------------------------- 5. bad indices
def test_out_of_range_indices_touch_no_other_ray():
    case = COMPOSED["readme_nd4"]
    spp = case.sx * case.sy
    with G.Renderer(case.scene()) as r:
        n, npx, sb, kb = strat_samples(r, case.sx, case.sy, case.nd, case.jitter, keys=G.SAMPLE_REQUIRED)
        clean, _ = li_strat(r, case, sb, kb, n, npx)
        table, k = head(kb["table"], n).copy(), head(kb["k"], n).copy()
        bad_t = {0: -1, 7: npx, 300: 2**31 - 1, 301: -2**31, n - 1: npx + 5}
        bad_k = {3: -5, 7: spp, 511: 2**31 - 1, 512: -2**31, n - 2: spp + 1}
        for i, v in bad_t.items():
            table[i] = v
        for i, v in bad_k.items():
            k[i] = v
        # exactly sized arrays: nothing lies behind the last table, index or ray
        exact = {key: r.upload(head(sb[key], n).copy()) for key in G.RAY_KEYS + G.RNG_KEYS}
        kx = {"s1d": r.upload(head(kb["s1d"], npx * case.nd * spp).copy()), "table": r.upload(table), "k": r.upload(k)}
        ob = {key: r.buffer(n, G.LI_DTYPES[key]) for key in LI_KEYS}
        rc = r.li_stratified_device({key: exact[key] for key in G.RAY_KEYS}, {key: exact[key] for key in G.RNG_KEYS}, n, ob,
                                    kx, npx, spp, case.nd, 1, 2, max_depth=case.max_depth, light_strategy=case.strategy)
        assert rc == 0, r.last_error()
        r.query_status()   # (synchronises; an out-of-range ray's path is unspecified, its record too)
        ok = np.ones(n, dtype=bool)
        ok[list(bad_t) + list(bad_k)] = False
        for key in LI_KEYS:
            assert ob[key].download()[:n][ok].tobytes() == clean[key][ok].tobytes(), key
        assert same(kx["table"].download(), table) and same(kx["k"].download(), k)   # the inputs are untouched


# -------------------------------------------------- 6. refusals and ordering
def test_refusals_in_flight_empty_calls_and_the_steady_state():
    case = COMPOSED["readme_nd4"]
    scene = case.scene()
    spp, ns, ts = 4, 3, 16
    rd = abi.render_desc(2, 2)
    with G.Renderer(scene) as r:
        n, npx, sb, kb = strat_samples(r, 2, 2, 4, False)
        want = {k: head(b, n) for k, b in list(sb.items()) + list(kb.items()) if k != "s1d"}
        rays, rngb = {k: sb[k] for k in G.RAY_KEYS}, {k: sb[k] for k in G.RNG_KEYS}
        ob = {k: padded(r, n, G.LI_DTYPES[k]) for k in LI_KEYS}
        before = len(r.launches(outside=True))
        big = {k: padded(r, 8, dt) for k, dt in G.SAMPLE_DTYPES.items()}
        bigk = {"k": padded(r, 8, np.int32), "table": padded(r, 8, np.int32), "s1d": padded(r, 8, np.float64)}

        def samples(buf=sb, kbuf=kb, sx=2, sy=2, nd=4, **kw):
            return r.frame_samples_stratified(buf, kbuf, sx, sy, nd, False, **kw)

        def li(nd=4, c1=1, c2=2, n_tables=npx, spp_=spp, **kw):
            return r.li_stratified_device(rays, rngb, n, ob, kb, n_tables, spp_, nd, c1, c2, **kw)

        for call, code, word in (
                (lambda: samples(nd=0), UNS, "n_dims < 1"),
                (lambda: samples(big, bigk, 4097, 1, 1, tile_end=0), UNS, "4096 samples"),
                (lambda: samples(big, bigk, 64, 64, 3, tile_end=0), UNS, "n_dims * spp > 8192"),
                (lambda: samples(big, bigk, 64, 64, 2, tile_end=0), UNS, "48 KB"),
                (lambda: li(c1=5), INV, "cursor"), (lambda: li(c2=-1), INV, "cursor"),
                (lambda: li(nd=-1, c1=0, c2=0), INV, "n_dims < 0"),
                (lambda: li(max_depth=0), INV, "max_depth"), (lambda: li(max_depth=4096), UNS, "maxDepth"),
                (lambda: li(integrator=abi.PBRT_INTEGRATOR_DIRECT_LIGHTING), UNS, "Path integrator"),
                (lambda: li(light_strategy=7), UNS, "light sample strategy")):
            assert call() == code and word in r.last_error(), (word, r.last_error())
        # what the wrapper cannot pass on: the raw call with a sampler that does not match ns, NULL strat arrays
        L = G.lib()
        fd, sm = abi.frame_desc(ts, ns, 0, 6), abi.strat_sampler_desc(3, 3, 4)
        os_ = G._soa(abi.FrameSamplesSoA, [(k, sb[k], None) for k in G.SAMPLE_REQUIRED])
        ss = G._soa(abi.StratSamplesSoA, [(k, kb[k], None) for k in ("k", "table", "s1d")])
        assert L.pbrt_gpu_frame_samples_stratified_device(r.h, C.byref(fd), C.byref(sm), C.byref(os_), C.byref(ss)) == INV
        assert "ns != sampler_x * sampler_y - 1" in r.last_error()
        sm = abi.strat_sampler_desc(2, 2, 4, reserved=1)
        assert L.pbrt_gpu_frame_samples_stratified_device(r.h, C.byref(fd), C.byref(sm), C.byref(os_), C.byref(ss)) == INV
        sm = abi.strat_sampler_desc(2, 2, 4)
        assert L.pbrt_gpu_frame_samples_stratified_device(r.h, C.byref(fd), C.byref(sm), C.byref(os_), None) == INV
        assert L.pbrt_gpu_frame_samples_stratified_device(r.h, C.byref(fd), C.byref(sm), C.byref(os_),
                                                          C.byref(abi.StratSamplesSoA())) == INV
        rs, gs, rad = G._li_soas(r, "test", rays, rngb, n, ob)
        d = abi.li_desc(5)
        assert L.pbrt_gpu_li_stratified_device(r.h, C.byref(d), C.byref(rs), C.byref(gs), n, C.byref(rad), None) == INV
        st = abi.StratSoA()
        st.n_tables, st.spp, st.n_dims, st.first_1d, st.first_2d = npx, spp, 4, 1, 2
        assert L.pbrt_gpu_li_stratified_device(r.h, C.byref(d), C.byref(rs), C.byref(gs), n, C.byref(rad), C.byref(st)) == INV
        assert "NULL" in r.last_error()
        # empty calls are PBRT_OK
        assert r.li_stratified_device(rays, rngb, 0, ob, kb, npx, spp, 4, 1, 2) == 0
        for b, e in ((0, 0), (3, 3), (6, 6)):
            assert samples(tile_begin=b, tile_end=e) == 0
        # a render in flight: both calls are refused and the render is left alone
        rc_e, efilm, _ = O.render(scene.desc, rd, threads=T.THREADS)
        r.render_async(rd)
        rcs = [samples(), li()]
        r.synchronize()
        assert rcs == [INV, INV] and "in flight" in r.last_error() and rc_e == 0
        assert np.array_equal(bits(r.film()), bits(efilm))
        assert names_since(r, before) == []   # nothing above launched anything
        for k, b in ob.items():
            assert (b.download() == T.SENTINEL[b.dtype]).all(), k
        for k in want:   # nor wrote anything
            assert same(head(dict(sb, **kb)[k], n), want[k]), k
        # the steady state: one launch a call, no allocation
        free = []
        for _ in range(3):
            before = len(r.launches(outside=True))
            assert samples() == 0 and li() == 0
            assert names_since(r, before) == ["k_strat_pixels", "k_li_strat<false, 0>"]
            assert Q.status(r) == Q.CLEAN
            free.append(hip_free_bytes())
        assert free[1] == free[2], free

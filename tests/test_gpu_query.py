"""Device-resident ray queries on the GPU (pbrt_gpu_intersect[_p]_device,
pbrt_gpu_camera_rays_device, pbrt_gpu_query_status, pbrt_gpu_buffer_*) against
the CPU oracle, bit for bit. numpy and ctypes only: the device memory is the
context's own (DeviceBuffer), no other runtime holds a handle to it.

Every buffer a test hands to a query is 64 elements longer than the query and
pre-filled with a sentinel; the tail must come back unchanged.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import pbrtgpu as G
from pbrtgpu import abi

pytestmark = pytest.mark.gpu

PAD = 64
SENTINEL = {np.dtype(np.float64): -7.25e77, np.dtype(np.int32): -123456, np.dtype(np.uint8): 0xA5}
HIT_KEYS = tuple(G.HIT_DTYPES)   # hit, t_max, prim, px, py, pz, nx, ny, nz: the oracle's column order
INF = float("inf")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def random_rays(n, seed):   # tests/test_gpu_parity.py's generator
    rng = np.random.default_rng(seed)
    o = rng.uniform(-60, 140, size=(n, 3))
    o[:, 1] = rng.uniform(-5, 120, size=n)
    d = rng.normal(size=(n, 3))
    tmax = np.where(rng.uniform(size=n) < 0.2, rng.uniform(1, 200, size=n), np.inf)
    return np.concatenate([o, d, tmax[:, None]], axis=1)


# ------------------------------------------------------------------ buffers
def padded(r, n, dtype, data=None):
    """A buffer of n + PAD elements, all sentinel, then data in its first n."""
    dtype = np.dtype(dtype)
    host = np.full(n + PAD, SENTINEL[dtype], dtype=dtype)
    if data is not None:
        host[:n] = data
    return r.upload(host)


def head(buf, n):
    """The first n elements; the PAD elements after them must still be the sentinel."""
    host = buf.download()
    assert host.size == n + PAD
    assert (host[n:] == SENTINEL[buf.dtype]).all(), "a query wrote past its n elements"
    return host[:n]


def upload_rays(r, rays, tmax=True):
    n = rays.shape[0]
    bufs = {k: padded(r, n, np.float64, rays[:, i]) for i, k in enumerate(G.RAY_KEYS)}
    if tmax:
        bufs["tmax"] = padded(r, n, np.float64, rays[:, 6])
    return bufs


def hit_buffers(r, n, keys=HIT_KEYS):
    return {k: padded(r, n, G.HIT_DTYPES[k]) for k in keys}


def rows(hits, n):
    """Downloaded hits as the oracle's (n, 9) rows."""
    return np.stack([head(hits[k], n).astype(np.float64) for k in HIT_KEYS], axis=1)


def closest(r, rays, n=None):
    """intersect_device of all outputs; returns the (n, 9) rows. Inputs are checked to be untouched."""
    n = rays.shape[0] if n is None else n
    rb, hb = upload_rays(r, rays), hit_buffers(r, n)
    assert r.intersect_device(rb, n, hb) == 0
    got = rows(hb, n)
    for i, k in enumerate(G.RAY_KEYS + ("tmax",)):
        assert same_bits(head(rb[k], n), rays[:n, i])
    return got


def any_hit(r, rays):
    n = rays.shape[0]
    rb, occ = upload_rays(r, rays), padded(r, n, np.uint8)
    assert r.intersect_p_device(rb, n, occ) == 0
    return head(occ, n)


def status(r):
    rc, rec = r.query_status()
    return rc, int(rec.panics), int(rec.first_ray), int(rec.panic_kind)


CLEAN = (0, 0, -1, abi.PBRT_PANIC_NONE)


# ------------------------------------------------------------ oracle camera
PBRT_VOP_NORMALIZED = 14   # include/pbrt_diag.h


def oracle_camera_rays(desc, window, offset):
    """camera_ray with lens_radius == 0 from the oracle's own exports, operation
    for operation: raster -> camera point, normalise, camera -> world ray."""
    L = O.lib()
    x0, y0, x1, y1 = window
    cam = desc.camera
    out = np.zeros(((x1 - x0) * (y1 - y0), 7))
    D3 = C.c_double * 3
    pc, pe, dn, oo, od = D3(), D3(), D3(), D3(), D3()
    i = 0
    for y in range(y0, y1):
        for x in range(x0, x1):
            L.oracle_transform_point(C.byref(cam.raster_to_camera), D3(x + offset[0], y + offset[1], 0.0),
                                     D3(0, 0, 0), pc, pe)
            assert L.oracle_vec_op(PBRT_VOP_NORMALIZED, pc, None, 0.0, dn) == 0
            L.oracle_transform_ray(C.byref(cam.camera_to_world), D3(0, 0, 0), dn, oo, od)
            out[i] = list(oo) + list(od) + [INF]
            i += 1
    return out


def full_window(scene):
    return (0, 0, int(scene.desc.film.res_x), int(scene.desc.film.res_y))


def device_camera_rays(r, window, **kw):
    n = (window[2] - window[0]) * (window[3] - window[1])
    out = {k: padded(r, n, np.float64) for k in G.RAY_KEYS + ("tmax",)}
    got = r.camera_rays(window, out=out, **kw)
    assert set(got) == set(out)
    return np.stack([head(out[k], n) for k in G.RAY_KEYS + ("tmax",)], axis=1)


# ------------------------------------------------------------------- scenes
@pytest.fixture(scope="module")
def readme():
    scene = G.Scene.readme(64, 64)
    with G.Renderer(scene) as r:
        yield scene, r


@functools.lru_cache(maxsize=None)
def readme_case(n):
    """(rays, oracle closest rows, oracle any-hit flags) of random_rays(n, 3) on the README scene."""
    scene = G.Scene.readme(64, 64)
    rays = random_rays(n, 3)
    want = O.intersect(scene.desc, rays, closest=True)
    wocc = O.intersect(scene.desc, rays, closest=False)
    for a in (rays, want, wocc):
        a.setflags(write=False)
    return rays, want, wocc


def spheres_scene():
    rng = np.random.default_rng(7)
    s = G.Scene()
    m = s.add_matte((0.5, 0.5, 0.5))
    for _ in range(100):
        c = rng.uniform(-10, 10, 3)
        rad = rng.uniform(.3, 1.2)
        s.add_primitive(s.add_sphere(G.translate(*c), rad), m)
    s.add_point_light(G.translate(0, 20, 0), (100, 100, 100))
    s.set_film(40, 24)
    s.set_camera(G.look_at((0, 0, 30), (0, 0, 0), (0, 1, 0)), fov=50)
    return s.build(max_prims_in_node=1)


def fidelity_scene(octant):   # tests/test_panic_fidelity.py's scene
    s = G.Scene()
    m = s.add_matte((0.5, 0.5, 0.5))
    floor = s.add_disk(G.mul(G.translate(0, 0, 0), G.rotate(0, 90)), 0.0, 100.0)
    s.add_primitive(floor, m)
    c = [o * 5.77e159 for o in octant]
    big = s.add_sphere(G.translate(*c), 5e159)
    s.add_primitive(big, m)
    light = s.add_sphere(G.translate(0, 5, 0), 0.5)
    s.add_area_light((5, 5, 5), light)
    s.set_film(32, 32)
    s.set_camera(G.look_at((0, 20, 20), (0, 0, 0), (0, 1, 0)), fov=60)
    return s.build(max_prims_in_node=1)


def camera_scene(lens=0.0, focal=20.0):
    s = G.Scene()
    m = s.add_matte((0.5, 0.5, 0.5))
    s.add_primitive(s.add_sphere(G.translate(0, 0, 0), 3.0), m)
    s.add_primitive(s.add_disk(G.mul(G.translate(0, -3, 0), G.rotate(0, 90)), 0.0, 6.0), m)
    s.add_point_light(G.translate(0, 20, 0), (100, 100, 100))
    s.set_film(33, 17)
    s.set_camera(G.look_at((0, 4, 12), (0, 0, 0), (0, 1, 0)), lens=lens, focal=focal, fov=60)
    return s.build()


# ------------------------------------------------- 1. wave and block edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 20_000])
def test_wave_and_block_edges(readme, n):
    _, r = readme
    rays, want, wocc = readme_case(n)
    got = closest(r, rays)
    occ = any_hit(r, rays)
    assert status(r) == CLEAN
    hit_fraction = want[:, 0].mean()
    print(f"n={n}: oracle hit fraction {hit_fraction:.3f}")
    if n == 257:
        assert round(hit_fraction, 3) == 0.642   # both outcomes occur
    assert same_bits(got, want), int((bits(got) != bits(want)).any(axis=1).sum())
    assert np.array_equal(occ.astype(bool), wocc.astype(bool))
    assert set(np.unique(occ)) <= {0, 1}
    rc, host = r.intersect(rays)   # the host-array path returns the same values
    assert rc == 0 and same_bits(got, host)


# ---------------------------------------------------- 2. optional outputs
def test_optional_outputs(readme):
    _, r = readme
    n = 257
    rays, want, _ = readme_case(n)
    rb = upload_rays(r, rays)
    hb = hit_buffers(r, n, ("hit", "prim"))
    unused = padded(r, n, np.float64)   # a t_max buffer that is not passed
    assert r.intersect_device(rb, n, hb) == 0
    assert np.array_equal(head(hb["hit"], n), want[:, 0].astype(np.uint8))
    assert np.array_equal(head(hb["prim"], n), want[:, 2].astype(np.int32))
    assert (unused.download() == SENTINEL[unused.dtype]).all()
    # tmax omitted on input is +Inf
    inf_rays = rays.copy()
    inf_rays[:, 6] = INF
    explicit = closest(r, inf_rays)
    rb6, hb2 = upload_rays(r, inf_rays, tmax=False), hit_buffers(r, n)
    assert r.intersect_device(tuple(rb6[k] for k in G.RAY_KEYS), n, hb2) == 0
    assert same_bits(rows(hb2, n), explicit)
    assert same_bits(explicit, O.intersect(G.Scene.readme(64, 64).desc, inf_rays, closest=True))
    assert status(r) == CLEAN


# ----------------------------------------------------------- 3. stack walk
def test_stack_walk_over_a_large_tree():
    scene = spheres_scene()
    assert scene.desc.n_nodes == 199   # above kLdsNodes: the [64]-stack walk
    win = full_window(scene)
    rays = oracle_camera_rays(scene.desc, win, (0.5, 0.5))
    want = O.intersect(scene.desc, rays, closest=True)
    wocc = O.intersect(scene.desc, rays, closest=False)
    hitf, prims = want[:, 0].mean(), len(set(want[:, 2]))
    print(f"960 primary rays: hit fraction {hitf:.3f}, {prims} distinct values of prim")
    assert rays.shape[0] == 960 and round(hitf, 3) == 0.168
    assert prims == 21   # 20 primitives and the -1 of a miss
    with G.Renderer(scene) as r:
        assert same_bits(device_camera_rays(r, win), rays)
        got = closest(r, rays)
        occ = any_hit(r, rays)
        assert status(r) == CLEAN
    assert same_bits(got, want), int((bits(got) != bits(want)).any(axis=1).sum())
    assert np.array_equal(occ.astype(bool), wocc.astype(bool))


# --------------------------------------------------------------- 4. meshes
@pytest.mark.parametrize("spheres", [True, False])
def test_meshes(spheres):
    scene = G.Scene.heightfield(48, 32, quads=8, seed=1, spheres=spheres)
    d = scene.desc
    assert d.n_meshes == 1 and d.n_prims == (21 if spheres else 0)   # False: the kMeshOnly kernels
    win = full_window(scene)
    rays = oracle_camera_rays(d, win, (0.5, 0.5))
    want = O.intersect(d, rays, closest=True)
    wocc = O.intersect(d, rays, closest=False)
    hit, prim = want[:, 0] == 1, want[:, 2]
    analytic, tris, miss = int((hit & (prim < d.n_prims)).sum()), int((hit & (prim >= d.n_prims)).sum()), int((~hit).sum())
    print(f"spheres={spheres}: {analytic} analytic hits, {tris} triangle hits, {miss} misses")
    if spheres:
        assert (analytic, tris, miss) == (7, 1070, 459)
    else:
        assert analytic == 0 and round(hit.mean(), 2) == 0.70
    with G.Renderer(scene) as r:
        got = closest(r, rays)
        occ = any_hit(r, rays)
        assert status(r) == CLEAN
    assert same_bits(got, want), int((bits(got) != bits(want)).any(axis=1).sum())
    assert np.array_equal(occ.astype(bool), wocc.astype(bool))
    n_tris = int(d.meshes[0].n_triangles)
    assert ((got[hit, 2] >= 0) & (got[hit, 2] < d.n_prims + n_tris)).all()   # prim = n_prims + triangle


# --------------------------------------------------------- 5. panic record
def panic_rays():
    d = np.random.default_rng(5).normal(size=(200, 3))
    d[:50] = np.abs(d[:50])
    d[0] = (1, 1, 1)
    o = np.tile((0.0, 1.0, 0.0), (200, 1))
    return np.concatenate([o, d, np.full((200, 1), INF)], axis=1)


def check_panics(r, scene, rays, expect=None):
    want = O.intersect(scene.desc, rays, closest=True)
    wocc = O.intersect(scene.desc, rays, closest=False)
    nan = np.isnan(want[:, 0])
    assert np.array_equal(nan, np.isnan(wocc))   # the same rays panic in any-hit
    count, first = int(nan.sum()), int(np.argmax(nan))
    print(f"oracle: {count} panics from ray {first}, {int((want[:, 0] == 1).sum())} hits, "
          f"{int((want[:, 0] == 0).sum())} misses")
    if expect:
        assert (count, first, int((want[:, 0] == 1).sum()), int((want[:, 0] == 0).sum())) == expect
    n = rays.shape[0]
    got = closest(r, rays)
    assert status(r) == (abi.PBRT_E_REF_PANIC, count, first, abi.PBRT_PANIC_EFLOAT)
    assert status(r) == CLEAN   # the status call cleared the record
    miss = np.tile([0.0, INF, -1.0, 0, 0, 0, 0, 0, 0], (count, 1))
    assert same_bits(got[nan], miss)                # a panic reads as a miss with the ray's own TMax
    assert same_bits(got[~nan], want[~nan])
    occ = any_hit(r, rays)
    assert status(r) == (abi.PBRT_E_REF_PANIC, count, first, abi.PBRT_PANIC_EFLOAT)
    assert (occ[nan] == 0).all() and np.array_equal(occ[~nan].astype(bool), wocc[~nan].astype(bool))
    assert n == 200
    return first


def test_panic_record():
    scene = fidelity_scene((1, 1, 1))
    rays = panic_rays()
    with G.Renderer(scene) as r:
        assert status(r) == CLEAN   # before any query
        assert check_panics(r, scene, rays, expect=(52, 0, 73, 75)) == 0
        moved = np.concatenate([rays[50:], rays[:50]])   # the first 50 rows at the end
        first = check_panics(r, scene, moved)
        assert first > 0   # first_ray follows the oracle's new smallest index
        # two queries, one record: the counts add, the smallest index wins
        closest(r, rays)
        closest(r, moved)
        rc, count, first_both, kind = status(r)
        assert (rc, count, first_both, kind) == (abi.PBRT_E_REF_PANIC, 104, 0, abi.PBRT_PANIC_EFLOAT)


# ----------------------------------------------------------- 6. camera rays
@pytest.mark.parametrize("offset", [(0.5, 0.5), (0.25, 0.75)])
@pytest.mark.parametrize("window", [None, (5, 3, 30, 11)])
def test_camera_rays_match_the_oracle(window, offset):
    scene = camera_scene()
    win = full_window(scene) if window is None else window
    want = oracle_camera_rays(scene.desc, win, offset)
    with G.Renderer(scene) as r:
        got = device_camera_rays(r, win, film_offset=offset)
        assert status(r) == CLEAN
    assert same_bits(got[:, :6], want[:, :6])
    assert (got[:, 6] == INF).all()


def test_camera_window_outside_the_film_is_invalid():
    scene = camera_scene()
    with G.Renderer(scene) as r:
        for win in ((0, 0, 34, 17), (0, 0, 33, 18), (-1, 0, 5, 5), (5, 5, 5, 6), (6, 5, 5, 6)):
            with pytest.raises(G.PbrtError) as e:
                r.camera_rays(win)
            assert e.value.code == abi.PBRT_E_INVALID
        # the library refuses them too (valid arrays, so the window is what it objects to)
        bufs = [(k, padded(r, 33 * 17, np.float64), np.float64) for k in G.RAY_KEYS]
        out = G._soa(abi.RaySoAOut, bufs)
        for win in ((0, 0, 34, 17), (0, 0, 33, 18), (-1, 0, 5, 5), (5, 5, 5, 6), (6, 5, 5, 6)):
            d = abi.CameraRaysDesc(*win, 0.5, 0.5, 0.5, 0.5, 0.0)
            assert G.lib().pbrt_gpu_camera_rays_device(r.h, C.byref(d), C.byref(out)) == abi.PBRT_E_INVALID
        d = abi.CameraRaysDesc(0, 0, 33, 17, 0.5, 0.5, 0.5, 0.5, 0.0)
        assert G.lib().pbrt_gpu_camera_rays_device(r.h, C.byref(d), C.byref(out)) == 0   # tmax NULL: not written
        out.dz = None
        assert G.lib().pbrt_gpu_camera_rays_device(r.h, C.byref(d), C.byref(out)) == abi.PBRT_E_INVALID
        assert status(r) == CLEAN
        for _, b, _ in bufs:
            head(b, 33 * 17)


def test_library_argument_validation(readme):
    """PBRT_E_INVALID before any device call; n == 0 is PBRT_OK and launches nothing."""
    _, r = readme
    L, n = G.lib(), 65
    rays, want, _ = readme_case(n)
    rb, hb = upload_rays(r, rays), hit_buffers(r, n)
    rs = G._soa(abi.RaySoA, [(k, b, np.float64) for k, b in rb.items()])
    hs = G._soa(abi.HitSoA, [(k, b, G.HIT_DTYPES[k]) for k, b in hb.items()])
    occ = C.c_void_p(hb["hit"].ptr)
    assert L.pbrt_gpu_intersect_device(r.h, None, n, C.byref(hs)) == abi.PBRT_E_INVALID
    assert L.pbrt_gpu_intersect_device(r.h, C.byref(rs), n, None) == abi.PBRT_E_INVALID
    assert L.pbrt_gpu_intersect_p_device(r.h, C.byref(rs), n, None) == abi.PBRT_E_INVALID
    assert L.pbrt_gpu_intersect_device(r.h, C.byref(rs), 2**31, C.byref(hs)) == abi.PBRT_E_INVALID
    assert L.pbrt_gpu_intersect_p_device(r.h, C.byref(rs), 2**31, occ) == abi.PBRT_E_INVALID
    no_hit = G._soa(abi.HitSoA, [("t_max", hb["t_max"], np.float64)])
    assert L.pbrt_gpu_intersect_device(r.h, C.byref(rs), n, C.byref(no_hit)) == abi.PBRT_E_INVALID
    for k in G.RAY_KEYS:   # every ray pointer but tmax is required
        bad = G._soa(abi.RaySoA, [(q, b, np.float64) for q, b in rb.items() if q != k])
        assert L.pbrt_gpu_intersect_device(r.h, C.byref(bad), n, C.byref(hs)) == abi.PBRT_E_INVALID, k
        assert L.pbrt_gpu_intersect_p_device(r.h, C.byref(bad), n, occ) == abi.PBRT_E_INVALID, k
    assert L.pbrt_gpu_intersect_device(r.h, C.byref(rs), 0, C.byref(hs)) == 0
    assert L.pbrt_gpu_intersect_p_device(r.h, C.byref(rs), 0, occ) == 0
    assert status(r) == CLEAN
    for b in hb.values():   # none of the above wrote anything
        assert (b.download() == SENTINEL[b.dtype]).all()
    assert L.pbrt_gpu_intersect_device(r.h, C.byref(rs), n, C.byref(hs)) == 0
    assert same_bits(rows(hb, n), want)


def test_primary_hits():
    scene = camera_scene()
    rays = oracle_camera_rays(scene.desc, full_window(scene), (0.5, 0.5))
    want = O.intersect(scene.desc, rays, closest=True)
    hitf = want[:, 0].mean()
    print(f"primary hit fraction {hitf:.3f}")
    assert round(hitf, 3) == 0.123 and set(want[want[:, 0] == 1, 2]) == {0.0, 1.0}   # and background
    with G.Renderer(scene) as r:
        ph = r.primary_hits()
        n = ph["n"]
        assert n == 33 * 17
        got = np.stack([ph["hits"][k].download().astype(np.float64) for k in HIT_KEYS], axis=1)
        assert same_bits(got, want)
        assert same_bits(np.stack([ph["rays"][k].download() for k in G.RAY_KEYS], axis=1), rays[:, :6])
        again = r.primary_hits()   # one allocation per window size
        assert all(again["hits"][k] is ph["hits"][k] for k in HIT_KEYS)
        sub = r.primary_hits(window=(5, 3, 30, 11))
        wsub = O.intersect(scene.desc, oracle_camera_rays(scene.desc, (5, 3, 30, 11), (0.5, 0.5)), closest=True)
        assert same_bits(np.stack([sub["hits"][k].download().astype(np.float64) for k in HIT_KEYS], axis=1), wsub)
        assert status(r) == CLEAN


def test_thin_lens_camera_rays():
    """The oracle exports no lens sampling, so not bit for bit: every origin lies
    on the lens, and every ray passes through its pinhole ray's focal-plane point."""
    radius, focal, lens = 0.5, 12.0, (0.3, 0.8)
    pin_scene, lens_scene = camera_scene(), camera_scene(lens=radius, focal=focal)
    win = full_window(pin_scene)
    with G.Renderer(pin_scene) as r:
        pin = device_camera_rays(r, win)
    with G.Renderer(lens_scene) as r:
        got = device_camera_rays(r, win, lens=lens)
    c2w = np.array([list(row) for row in lens_scene.desc.camera.camera_to_world.m.m])
    w2c = np.array([list(row) for row in lens_scene.desc.camera.camera_to_world.m_inv.m])
    o_cam = got[:, :3] @ w2c[:3, :3].T + w2c[:3, 3]
    assert (np.hypot(o_cam[:, 0], o_cam[:, 1]) <= radius * (1 + 1e-12)).all() and np.abs(o_cam[:, 2]).max() < 1e-9
    assert np.hypot(o_cam[:, 0], o_cam[:, 1]).min() > 0.1   # the lens sample moved them off the pinhole
    d_cam = pin[:, 3:6] @ w2c[:3, :3].T
    d_cam /= np.linalg.norm(d_cam, axis=1, keepdims=True)
    pf = (d_cam * (focal / d_cam[:, 2:3])) @ c2w[:3, :3].T + c2w[:3, 3]   # focal-plane points, world space
    v = pf - got[:, :3]
    dn = got[:, 3:6] / np.linalg.norm(got[:, 3:6], axis=1, keepdims=True)
    dist = np.linalg.norm(v - (v * dn).sum(axis=1, keepdims=True) * dn, axis=1)
    assert (dist <= 1e-9 * np.linalg.norm(v, axis=1)).all(), dist.max()
    assert (got[:, 6] == INF).all()


# ------------------------------------------------ 7. coexistence with frames
def test_queries_between_frames(readme):
    scene, r = readme
    rd = abi.render_desc(2, 2)
    rc, ofilm, _ = O.render(scene.desc, rd, threads=8)
    assert rc == 0
    n = 257
    rays, want, _ = readme_case(n)
    film1, _ = r.render(rd)
    got = closest(r, rays)
    film2, _ = r.render(rd)
    assert same_bits(film1, ofilm) and same_bits(film2, ofilm)
    assert same_bits(got, want)
    # a query while a frame is in flight is refused and leaves the frame alone
    rb, hb = upload_rays(r, rays), hit_buffers(r, n)
    r.render_async(rd)
    rc_q = r.intersect_device(rb, n, hb)
    rc_p = r.intersect_p_device(rb, n, hb["hit"])
    rc_s, _ = r.query_status()
    r.synchronize()
    assert (rc_q, rc_p, rc_s) == (abi.PBRT_E_INVALID,) * 3
    assert same_bits(r.film(), ofilm)
    assert (hb["hit"].download() == SENTINEL[np.dtype(np.uint8)]).all()   # nothing was enqueued
    assert r.intersect_device(rb, n, hb) == 0 and same_bits(rows(hb, n), want)
    assert status(r) == CLEAN


# ------------------------------------------------------------ 8. lifetimes
def test_buffers_die_with_their_renderer():
    r = G.Renderer(G.Scene.readme(32, 16))
    a, b = r.buffer(100), r.upload(np.arange(10, dtype=np.int32))
    assert np.array_equal(b.download(), np.arange(10)) and not a.closed
    other = G.Renderer(G.Scene.readme(32, 16))
    with pytest.raises(G.PbrtError):   # a buffer of another renderer never reaches the library
        other.intersect_p_device((a,) * 6, 10, other.buffer(10, np.uint8))
    other.close()
    r.close()
    assert a.closed and b.closed
    for use in (lambda: a.upload(np.zeros(1)), lambda: b.download(), lambda: a.ptr,
                lambda: r.buffer(4), lambda: G.check_buffers(r, 1, [("a", a, np.float64)])):
        with pytest.raises(G.PbrtError):
            use()
    a.close()   # silent
    del a, b    # silent


def test_many_buffers_and_leftovers():
    with G.Renderer(G.Scene.readme(32, 16)) as r:
        for i in range(100):
            r.buffer(1 + i, (np.float64, np.int32, np.uint8)[i % 3])   # dropped at once: freed by __del__
        keep = [r.buffer(1000) for _ in range(3)]   # left open: freed with the context
        x = np.linspace(0, 1, 1000)
        keep[1].upload(x[:10], offset=990)
        assert same_bits(keep[1].download()[990:], x[:10])
        with pytest.raises(G.PbrtError):
            keep[1].upload(x[:11], offset=990)
        rc = G.lib().pbrt_gpu_buffer_download(keep[0]._h, 8 * 999, x.ctypes.data, 16)   # the library's own range check
        assert rc == abi.PBRT_E_INVALID
    assert all(b.closed for b in keep)

"""The camera-start wave route (kernel="wave_cam", PBRT_KERNEL_WAVE_CAM) against
the oracle, on the uint64 view of the fp64 film: renders whose camera ray
belongs to the sample -- Stratified without sampled dimensions and
sampler.RandomSampler (n_dims = 0: pFilm, pLens and the time are PCG32 draws),
and a thin lens with one sampled dimension (pLens is a draw). AUTO keeps these
on the serial kernel (tests/test_gpu_parity.py, tests/test_gpu_edges.py pin
that); here every render asks for the route and asserts that it ran.

The oracle restates every piece on its own (n_dims = 0, ORACLE_FLAG_RANDOM_SAMPLER,
the thin lens, Mode B): no reference test covers them, parity is pinned
oracle-vs-device.
"""
import functools
import math
import os

import numpy as np
import pytest

import oracle_lib as O
import pbrtgpu as G
from pbrtgpu import abi

pytestmark = pytest.mark.gpu

ORACLE_FLAG_RANDOM_SAMPLER = 2
THREADS = min(16, os.cpu_count() or 1)
CAM = abi.PBRT_KERNEL_WAVE_CAM
MB = abi.PBRT_MODE_THROUGHPUT


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def copy_rd(rd, **kw):
    out = abi.RenderDesc.from_buffer_copy(rd)
    for k, v in kw.items():
        setattr(out, k, v)
    return out


def random_desc(ns, **kw):
    rd = abi.render_desc(**kw)
    G.lib().pbrt_random_sampler(ns, G.C.byref(rd))
    return rd


def oracle(scene, rd, flags=0):
    rc, film, st = O.render(scene.desc, rd, threads=THREADS, flags=flags)
    assert rc == 0 and np.isfinite(film).all()
    return film, st


def cam_render(scene, rd):
    with G.Renderer(scene, kernel="wave_cam") as r:
        film, st = r.render(rd)
    assert st.kernel == CAM
    return film, st


def check(scene, rd, flags=0):
    """device (wave_cam) vs oracle: the film bit for bit, and the statistics"""
    of, ost = oracle(scene, rd, flags)
    film, st = cam_render(scene, rd)
    assert np.array_equal(bits(film), bits(of))
    assert st.paths_traced == ost.paths and st.camera_samples == ost.camera_samples
    assert st.rays_closest == ost.closest_rays and st.rays_shadow == ost.shadow_rays
    return of, st


def lens_scene(w=48, h=32, lens=0.4, focal=12.0, crop=(0, 0, 1, 1), filter_radius=1.0):
    """tests/test_gpu_edges.py's edge_scene (a floor, three spheres, a disk, an
    area light and a point light) with its thin lens, crop window and filter radius"""
    s = G.Scene()
    chk = s.add_checker((0.2, 0, 0), (0, 0, 0.2), 0, 0, (1, 1, 1), (0.18, 0.18, 0.18))
    red, green, blue = s.add_matte((0.7, 0.1, 0.1)), s.add_matte((0.1, 0.7, 0.1)), s.add_matte((0.1, 0.1, 0.7))
    s.add_primitive(s.add_disk(G.rotate(0, 90), 0.0, 100.0), chk)
    for (x, m) in ((-2.5, red), (2.5, green)):
        s.add_primitive(s.add_sphere(G.translate(0, 0, 0), 2.0), m, G.translate(x, 2.0, 0.0))
    s.add_primitive(s.add_sphere(G.translate(0, 0, 0), 1.5), blue, G.translate(0.0, 1.5, -4.0))
    s.add_primitive(s.add_disk(G.translate(0, 1.0, 3), 0.0, 1.0), red)
    s.add_area_light((6, 6, 6), s.add_sphere(G.translate(0, 9, 2), 0.75))
    s.add_point_light(G.translate(-6, 10, 8), (60, 60, 60))
    s.set_film(w, h, crop=crop, filter_radius=(filter_radius, filter_radius))
    s.set_camera(G.look_at((0, 6, 14), (0, 1.5, 0), (0, 1, 0)), lens=lens, focal=focal, fov=55)
    return s.build(max_prims_in_node=1)


def efloat_scene(look):
    """tests/test_panic_fidelity.py's scene: a sphere of radius 5e159 about 1e160
    away in the (1, 1, -1) octant; a ray that reaches its leaf box overflows
    EFloat in Sphere.Intersect (efloat.go:102-111). `look`: the camera's target."""
    s = G.Scene()
    m = s.add_matte((0.5, 0.5, 0.5))
    s.add_primitive(s.add_disk(G.mul(G.translate(0, 0, 0), G.rotate(0, 90)), 0.0, 100.0), m)
    s.add_primitive(s.add_sphere(G.translate(5.77e159, 5.77e159, -5.77e159), 5e159), m)
    s.add_area_light((5, 5, 5), s.add_sphere(G.translate(0, 5, 0), 0.5))
    s.set_film(32, 32)
    s.set_camera(G.look_at((0, 20, 20), look, (0, 1, 0)), fov=60)
    return s.build(max_prims_in_node=1)


# ---------------------------------------------------------------- 1. RandomSampler
@pytest.mark.parametrize("ns", [2, 5, 16])
def test_random_sampler_exact(ns):
    scene = G.Scene.readme(64, 48)   # 12 tiles of 16
    rd = random_desc(ns, max_depth=5)
    assert (rd.sampler_x, rd.sampler_y, rd.n_dims) == (ns, 1, 0)
    of, st = check(scene, rd, flags=ORACLE_FLAG_RANDOM_SAMPLER)
    assert of.max() > 0 and st.paths_traced == 64 * 48 * (ns - 1)


# ---------------------------------------------------- 2. Stratified with n_dims = 0
@pytest.mark.parametrize("jitter", [False, True])
def test_stratified_no_sampled_dims(jitter):
    check(G.Scene.readme(64, 48), abi.render_desc(3, 3, jitter=jitter, n_dims=0, max_depth=5))


@pytest.mark.parametrize("rr", [1.0, 0.0])
def test_cornell_depth_8(rr):
    """rr_threshold 0: Russian roulette never runs (path.go:139: maxComponent < threshold)"""
    check(G.Scene.cornell(48, 32), abi.render_desc(3, 3, n_dims=0, max_depth=8, rr_threshold=rr))


@pytest.mark.parametrize("max_depth", [1, 2])
def test_shallow_paths(max_depth):
    """maxDepth 1: the camera ray is queried and nothing is traced beyond it (path.go:66)"""
    of, st = check(G.Scene.readme(64, 48), abi.render_desc(2, 2, n_dims=0, max_depth=max_depth))
    assert (of.max() > 0) == (max_depth > 1)


def test_one_sample_traces_nothing():
    """Sample 0 of a pixel is never traced (sampler.go:29-34, #2)"""
    of, st = check(G.Scene.readme(64, 48), abi.render_desc(1, 1, n_dims=0, max_depth=5))
    assert st.paths_traced == 0 and not of.any()


# ------------------------------------------------------------------- 3. thin lens
@functools.lru_cache(maxsize=None)
def pinhole_film(n_dims, xs, ys, jitter):
    film, _ = oracle(lens_scene(lens=0.0), abi.render_desc(xs, ys, jitter=jitter, n_dims=n_dims, max_depth=5))
    return film


@pytest.mark.parametrize("n_dims,xs,ys,jitter", [(0, 3, 3, False), (1, 3, 3, False), (1, 6, 5, True)])
def test_thin_lens(n_dims, xs, ys, jitter):
    """n_dims 1: pFilm is the stratified (0,0), pLens two draws; 6 x 5 jittered
    samples: StartPixel's pcg_bounded picks meet rejections"""
    of, _ = check(lens_scene(), abi.render_desc(xs, ys, jitter=jitter, n_dims=n_dims, max_depth=5))
    assert not np.array_equal(of, pinhole_film(n_dims, xs, ys, jitter))


# ------------------------------------------------------------------------ 4. film
@pytest.mark.parametrize("tile_size", [13, 8, 16])
def test_ragged_tiles(tile_size):
    check(G.Scene.readme(45, 30), abi.render_desc(2, 2, n_dims=0, max_depth=5, tile_size=tile_size))


@pytest.mark.parametrize("radius", [0.5, 1.5, 2.7])
def test_filter_radius_and_crop(radius):
    """per-sample footprints of up to 6 x 6 film pixels; a crop window offsets every tile"""
    scene = lens_scene(w=64, h=40, lens=0.0, crop=(0.25, 0.1, 0.8, 0.9), filter_radius=radius)
    assert scene.desc.film.crop_min_x > 0 and scene.desc.film.crop_min_y > 0
    check(scene, abi.render_desc(2, 2, n_dims=0, max_depth=5))
    check(scene, abi.render_desc(2, 2, n_dims=0, max_depth=5, tile_size=8))


# ------------------------------------------------------------ 5. tiles and groups
def test_tile_subsets():
    scene = G.Scene.readme(80, 48)   # 5 x 3 tiles of 16
    rd = abi.render_desc(2, 2, n_dims=0, max_depth=5)
    full, _ = check(scene, rd)
    margin = int(math.ceil(scene.desc.film.filter_radius_x + 0.5))   # reach of a neighbour tile's samples
    for sub in (dict(tile_begin=1, tile_stride=3), dict(tile_begin=3, tile_end=11)):
        srd = copy_rd(rd, **sub)
        part, st = check(scene, srd)
        end = sub.get("tile_end", 15)
        tiles = range(sub["tile_begin"], end, sub.get("tile_stride", 1))
        assert st.tiles_rendered == len(tiles)
        for t in tiles:   # the pixels only this tile's samples reach: the full frame's bits
            x0, y0 = (t % 5) * 16 + margin, (t // 5) * 16 + margin
            x1, y1 = (t % 5) * 16 + 16 - margin, (t // 5) * 16 + 16 - margin
            assert np.array_equal(bits(part[y0:y1, x0:x1]), bits(full[y0:y1, x0:x1])), t


def test_group_of_two_members():
    scene = G.Scene.readme(80, 48)
    rd = random_desc(4, max_depth=5)
    of, ost = oracle(scene, rd, flags=ORACLE_FLAG_RANDOM_SAMPLER)
    with G.RendererGroup(scene, [0, 0], kernel="wave_cam") as g:
        film, st = g.render(rd)
    assert st.kernel == CAM and st.paths_traced == ost.paths
    assert np.array_equal(bits(film), bits(of))


# ------------------------------------------------------------------ 6. panic sites
@pytest.mark.parametrize("look,max_depth,bounce", [((0, 0, 0), 3, 2), ((20, 40, 0), 3, 1)])
def test_panic_sites(look, max_depth, bounce):
    """the EFloat-overflow sphere: reached by bounce-2 rays off the floor, or
    (camera turned towards it) by the camera ray itself"""
    sc = efloat_scene(look)
    rd = abi.render_desc(2, 2, n_dims=0, max_depth=max_depth)
    rc, _, ost = O.render(sc.desc, rd, threads=4)
    assert rc == abi.PBRT_E_REF_PANIC and ost.panic_kind == abi.PBRT_PANIC_EFLOAT and ost.panic_bounce == bounce
    with G.Renderer(sc, kernel="wave_cam") as r:
        with pytest.raises(G.PbrtError) as ei:
            r.render(rd)
    st = ei.value.stats
    assert ei.value.code == abi.PBRT_E_REF_PANIC and st.kernel == CAM
    assert (st.panic_kind, st.panic_tile, st.panic_pixel_x, st.panic_pixel_y, st.panic_sample, st.panic_bounce) == \
        (ost.panic_kind, ost.panic_tile, ost.panic_px, ost.panic_py, ost.panic_sample, ost.panic_bounce)


# ------------------------------------------------------------------- 7. THROUGHPUT
@pytest.mark.parametrize("scene_name", ["readme", "cornell"])
@pytest.mark.parametrize("ns", [4, 16])
def test_throughput_mode(scene_name, ns):
    scene = G.Scene.readme(64, 48) if scene_name == "readme" else G.Scene.cornell(48, 32)
    check(scene, abi.render_desc(ns, 1, n_dims=0, max_depth=5, mode=MB))


def test_throughput_mode_thin_lens():
    check(lens_scene(), abi.render_desc(3, 3, jitter=True, n_dims=1, max_depth=5, mode=MB))


# ----------------------------------------------------------------------- 8. frames
def test_three_frames_of_one_context():
    """the second frame launches its chains in the first one's measured order:
    the schedule may differ between frames, the films may not"""
    scene = G.Scene.readme(64, 48)
    rd = random_desc(8, max_depth=5)
    of, _ = oracle(scene, rd, flags=ORACLE_FLAG_RANDOM_SAMPLER)
    sources = []
    with G.Renderer(scene, kernel="wave_cam") as r:
        for _ in range(3):
            film, st = r.render(rd)
            assert st.kernel == CAM and np.array_equal(bits(film), bits(of))
            sources.append(r.schedule_source())
    assert sources[2] == "learned"


def test_cancel_in_the_chain_then_render_again():
    """k_chain_cam keeps k_chain_ci's cancel exit: a cancel from another thread
    ends a frame of seconds (1080p, RandomSampler(256)) within 0.25 s, and the
    context's next render is exact (tests/test_cancel.py's contract)"""
    import threading
    import time

    scene = G.Scene.readme(1920, 1080)
    small = random_desc(4, max_depth=5, tile_end=32)
    with G.Renderer(scene, kernel="wave_cam") as r:
        r.render_async(random_desc(256, max_depth=10))
        t_cancel = []

        def fire():
            t_cancel.append(time.time())
            G.lib().pbrt_gpu_cancel(r.h)

        timer = threading.Timer(0.3, fire)
        timer.start()
        with pytest.raises(G.PbrtError) as ei:
            r.synchronize()
        t_done = time.time()
        timer.join()
        assert ei.value.code == abi.PBRT_E_CANCELLED and ei.value.stats.kernel == CAM
        assert t_done - t_cancel[0] < 0.25
        film, st = r.render(small)
    of, _ = oracle(scene, small, flags=ORACLE_FLAG_RANDOM_SAMPLER)
    assert st.kernel == CAM and np.array_equal(bits(film), bits(of))


# ----------------------------------------------------------- 9. one larger frame
def test_larger_frame():
    scene = G.Scene.readme(640, 360)
    check(scene, random_desc(16, max_depth=10), flags=ORACLE_FLAG_RANDOM_SAMPLER)


# -------------------------------------------------------------------- 10. refusals
DL = abi.PBRT_INTEGRATOR_DIRECT_LIGHTING
REFUSALS = {
    "n_dims_4": lambda: (G.Scene.readme(32, 32), abi.render_desc(2, 2, n_dims=4)),
    "n_dims_1_pinhole": lambda: (G.Scene.readme(32, 32), abi.render_desc(2, 2, n_dims=1)),
    "direct_lighting": lambda: (G.Scene.readme(32, 32), abi.render_desc(2, 2, n_dims=0, integrator=DL)),
    "glass": lambda: (G.Scene.readme_glass(32, 32), abi.render_desc(2, 2, n_dims=0)),
    "mesh": lambda: (G.Scene.heightfield(32, 32, quads=24, seed=1, spheres=True), abi.render_desc(2, 2, n_dims=0)),
    "panic_fidelity": lambda: (G.Scene.readme(32, 32),
                               abi.render_desc(2, 2, n_dims=0, flags=abi.PBRT_FLAG_PANIC_FIDELITY)),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(name):
    scene, rd = REFUSALS[name]()
    with G.Renderer(scene, kernel="wave_cam") as r:
        with pytest.raises(G.PbrtError) as ei:
            r.render(rd)
        assert ei.value.code == abi.PBRT_E_UNSUPPORTED
        assert "camera-start" in str(ei.value)   # the message names the route and the reason

"""Device groups (pbrt_gpu_group, include/pbrt_gpu.h): a frame split over
several members and merged on the leader in tile-index order is, bit for bit,
the oracle's film of the WHOLE frame -- which a sum of per-shard films is not
(the precondition each case asserts first, with the oracle alone). Device lists
repeat ordinal 0, so every path but the cross-device copy runs on one GPU;
[0, 1] joins when two GPUs are visible.
"""
import functools
import os
import threading
import time

import numpy as np
import pytest

import oracle_lib as O
import pbrtgpu as G
from pbrtgpu import abi

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
DEVICE_LISTS = [[0], [0, 0], [0, 0, 0], [0, 0, 0, 0, 0], [0, 1]]


def two_gpus():
    import torch
    return torch.cuda.device_count() >= 2


def device_params():
    return [pytest.param(d, id="dev" + "".join(map(str, d))) for d in DEVICE_LISTS]


def need(devices):
    if len(set(devices)) > 1 and not two_gpus():
        pytest.skip("one GPU visible")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def oracle(scene, rd):
    rc, film, st = O.render(scene.desc, rd, threads=THREADS)
    assert rc == 0
    return film, st


def copy_rd(rd, **kw):
    out = abi.RenderDesc.from_buffer_copy(rd)
    for k, v in kw.items():
        setattr(out, k, v)
    return out


def shard_sum_differs(scene, rd, full, n):
    """The precondition: adding the n shard films (tile k -> shard k mod n) in
    shard order gives another film than adding the tile films in tile order."""
    acc = np.zeros_like(full)
    for r in range(n):
        part, _ = oracle(scene, copy_rd(rd, tile_begin=r, tile_stride=n))
        acc += part
    return int(np.count_nonzero(np.any(bits(acc) != bits(full), axis=-1)))


def wide_filter_scene():
    """Matte spheres over a disk, seen from above so that lit surface lies where
    four tiles meet; BoxFilter radius (2.7, 1.5) and a crop window (4 x 2 ragged tiles)."""
    rng = np.random.default_rng(6)
    s = G.Scene()
    mats = [s.add_matte(tuple(rng.uniform(0.2, 0.9, 3))) for _ in range(3)]
    s.add_primitive(s.add_disk(G.mul(G.translate(0, -1, 0), G.rotate(0, 90)), 0.0, 50.0), mats[0])
    for i in range(12):
        c = (rng.uniform(-6, 6), rng.uniform(-0.5, 4), rng.uniform(-6, 6))
        s.add_primitive(s.add_sphere(G.translate(*c), rng.uniform(0.4, 1.2)), mats[i % 3])
    s.add_point_light(G.translate(0, 8, 0), (40, 40, 40))
    s.add_distant_light(G.translate(0, 0, 0), (0.6, 0.6, 0.6), (1, 2, 1))
    s.set_film(64, 48, crop=(0.1, 0.2, 0.9, 0.8), filter_radius=(2.7, 1.5))
    s.set_camera(G.look_at((0, 14, 8), (0, 0, 0), (0, 1, 0)), fov=50)
    return s.build()


def panic_scene():
    """A point light so bright that EstimateDirect returns > 10 on the first lit
    hit: UniformSampleOneLight panics (integrator.go:73-75)."""
    s = G.Scene()
    chk = s.add_matte((0.8, 0.8, 0.8))
    d = s.add_disk(G.mul(G.translate(0, 0, 0), G.rotate(0, 90)), 0.0, 100.0)
    s.add_primitive(d, chk)
    s.add_point_light(G.translate(0, 5, 0), (1e5, 1e5, 1e5))
    s.set_film(32, 32)
    s.set_camera(G.look_at((0, 20, 20), (0, 0, 0), (0, 1, 0)), fov=60)
    return s.build()


# name -> (scene, render desc); the oracle's film of each is computed once (case())
CASES = {
    "readme_64x48": lambda: (G.Scene.readme(64, 48), abi.render_desc(2, 2)),
    "readme_80x48": lambda: (G.Scene.readme(80, 48), abi.render_desc(3, 3)),
    "readme_45x30_t13": lambda: (G.Scene.readme(45, 30), abi.render_desc(2, 2, tile_size=13)),
    "readme_32x16": lambda: (G.Scene.readme(32, 16), abi.render_desc(2, 2)),
    "subset": lambda: (G.Scene.readme(80, 48), abi.render_desc(2, 2, tile_begin=1, tile_stride=2)),
    "wide_filter_crop": lambda: (wide_filter_scene(), abi.render_desc(2, 2)),
    "throughput": lambda: (G.Scene.readme(64, 48), abi.render_desc(2, 2, mode=abi.PBRT_MODE_THROUGHPUT)),
    "direct_lighting": lambda: (G.Scene.readme(64, 48),
                                abi.render_desc(2, 2, integrator=abi.PBRT_INTEGRATOR_DIRECT_LIGHTING)),
    "glass": lambda: (G.Scene.readme_glass(64, 40), abi.render_desc(2, 2)),
    "mesh": lambda: (G.Scene.heightfield(48, 32, quads=24, seed=1, spheres=True), abi.render_desc(2, 2)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    scene, rd = CASES[name]()
    film, st = oracle(scene, rd)
    film.setflags(write=False)
    return scene, rd, film, st


@functools.lru_cache(maxsize=None)
def precondition(name, n):
    scene, rd, film, _ = case(name)
    return shard_sum_differs(scene, rd, film, n)


def n_tiles(scene, rd):
    f = scene.desc.film
    ts = rd.tile_size
    return ((f.crop_max_x - f.crop_min_x + ts - 1) // ts) * ((f.crop_max_y - f.crop_min_y + ts - 1) // ts)


def check_group(name, devices, kernel="auto", frames=1, each_frame=None):
    scene, rd, ofilm, ost = case(name)
    with G.RendererGroup(scene, devices, kernel=kernel) as g:
        assert len(g) == len(devices)
        for frame in range(frames):
            film, st = g.render(rd)
            if each_frame:
                each_frame(g, frame)
            assert np.array_equal(bits(film), bits(ofilm)), name
            assert (st.paths_traced, st.rays_closest, st.rays_shadow) == (ost.paths, ost.closest_rays, ost.shadow_rays)
            members = [g.member_stats(i) for i in range(len(devices))]
            assert sum(m.tiles_rendered for m in members) == st.tiles_rendered == ost.tiles
    return film, st, members


# ------------------------------------------------------------ 1. bit-exact merge
@pytest.mark.parametrize("devices", device_params())
@pytest.mark.parametrize("name", ["readme_64x48", "readme_80x48", "readme_45x30_t13"])
def test_group_film_is_the_full_frame_bit_for_bit(name, devices):
    need(devices)
    scene, rd, ofilm, ost = case(name)
    if len(devices) > 1:   # what makes this test able to fail: the shard sum is another film
        assert precondition(name, len(devices)) >= 1
    film, st, members = check_group(name, devices)
    assert st.tiles_rendered == n_tiles(scene, rd)
    with G.Renderer(scene, device=0) as r:
        plain, pst = r.render(rd)
    assert np.array_equal(bits(film), bits(plain))
    assert st.kernel == pst.kernel and st.camera_samples == pst.camera_samples


# ------------------------------------------------------------ 2. steady state
def test_three_frames_on_one_group_stay_bit_exact():
    """From the second frame on every member runs the slot order it learned from
    its own previous frame (pbrt_gpu_schedule_source of the member contexts)."""
    learned = 2   # PBRT_SCHED_LEARNED (include/pbrt_diag.h)
    assert G.Renderer.SCHEDULE_SOURCES[learned] == "learned"
    seen = []

    def sources(g, frame):
        seen.append([g.member_schedule_source(i) for i in range(3)])

    check_group("readme_80x48", [0, 0, 0], frames=3, each_frame=sources)
    assert all(s != learned for s in seen[0])
    assert seen[1] == [learned] * 3 and seen[2] == [learned] * 3


# ------------------------------------------------------------ 3. empty member
def test_member_without_tiles():
    _, _, members = check_group("readme_32x16", [0, 0, 0])
    assert [m.tiles_rendered for m in members] == [1, 1, 0]


# ------------------------------------------------------------ 4. caller subset
def test_caller_subset_is_split_further():
    scene, rd, _, _ = case("subset")
    _, st, members = check_group("subset", [0, 0, 0])
    assert st.tiles_rendered == n_tiles(scene, rd) // 2 == 7
    assert [m.tiles_rendered for m in members] == [3, 2, 2]


# ------------------------------------------------------------ 5. wide filter and crop
def test_wide_filter_and_crop_window():
    assert precondition("wide_filter_crop", 3) >= 1
    check_group("wide_filter_crop", [0, 0, 0])


# ------------------------------------------------------------ 6. other pipelines
@pytest.mark.parametrize("name,kernel", [("throughput", "auto"), ("direct_lighting", "auto"), ("glass", "auto"),
                                         ("mesh", "auto"), ("readme_64x48", "serial")])
def test_other_pipelines_over_three_members(name, kernel):
    scene, rd, _, _ = case(name)
    film, st, _ = check_group(name, [0, 0, 0], kernel=kernel)
    with G.Renderer(scene, device=0, kernel=kernel) as r:   # the members ran the pipeline a plain context runs
        plain, pst = r.render(rd)
    assert st.kernel == pst.kernel and np.array_equal(bits(film), bits(plain))
    if kernel == "serial":
        assert st.kernel == abi.PBRT_KERNEL_SERIAL


# ------------------------------------------------------------ 7. staging path
def test_staging_copy_path(monkeypatch):
    monkeypatch.setenv("PBRT_GROUP_STAGE", "1")
    check_group("readme_45x30_t13", [0, 0, 0])


def test_two_gpus_staged(monkeypatch):
    need([0, 1])
    monkeypatch.setenv("PBRT_GROUP_STAGE", "1")
    check_group("readme_80x48", [0, 1])


# ------------------------------------------------------------ 8. panic
def test_panic_is_the_lowest_panicking_tile():
    scene = panic_scene()
    rd = abi.render_desc(2, 2)
    rc, _, ost = O.render(scene.desc, rd, threads=1)
    assert rc == abi.PBRT_E_REF_PANIC and ost.panic_kind == abi.PBRT_PANIC_LD_GT_10
    with G.RendererGroup(scene, [0, 0, 0]) as g:
        with pytest.raises(G.PbrtError) as ei:
            g.render(rd)
    st = ei.value.stats
    assert ei.value.code == abi.PBRT_E_REF_PANIC
    assert st.panic_kind == abi.PBRT_PANIC_LD_GT_10
    assert (st.panic_tile, st.panic_pixel_x, st.panic_pixel_y, st.panic_sample, st.panic_bounce) == (
        ost.panic_tile, ost.panic_px, ost.panic_py, ost.panic_sample, ost.panic_bounce)


# ------------------------------------------------------------ 9. cancel
def test_cancel_stops_every_member_and_the_next_frame_is_exact():
    """config C's frame (Cornell, 1080p, Stratified(16,16), Path(8)) is ~10 s of
    chains over three members on one GPU, one after the other: a cancel 0.4 s
    in stops the member in flight and keeps the other two from starting."""
    sc = G.Scene.cornell(1920, 1080)
    small = abi.render_desc(2, 2, max_depth=8, tile_end=48)
    with G.RendererGroup(sc, [0, 0, 0]) as g:
        g.cancel()   # nothing in flight: a no-op
        g.render_async(abi.render_desc(16, 16, max_depth=8))
        t_cancel = []

        def fire():
            t_cancel.append(time.time())
            g.cancel()

        timer = threading.Timer(0.4, fire)
        timer.start()
        result = {}

        def wait():
            try:
                g.synchronize()
                result["code"] = 0
            except G.PbrtError as e:
                result["code"] = e.code
            result["t"] = time.time()

        waiter = threading.Thread(target=wait, daemon=True)
        waiter.start()
        waiter.join(60)   # the render's own time limit: a frame that ignores the cancel takes ~10 s
        timer.join()
        assert not waiter.is_alive(), "synchronize did not return"
        assert result["code"] == abi.PBRT_E_CANCELLED
        # twice the bound tests/test_cancel.py sets for one context: the member in flight stops as
        # there, and the two that have not started only have to be skipped
        assert result["t"] - t_cancel[0] < 0.5, "the frame ran on past the cancel"
        film, st = g.render(small)   # the cancel died with its frame
        assert st.tiles_rendered == 48
    ofilm, _ = oracle(sc, small)
    assert np.array_equal(bits(film), bits(ofilm))

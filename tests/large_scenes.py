"""Scenes beyond the sizes k_paths_ci and the LDS-staged kernels take: more than
16 lights, more than 64 BVH nodes (host-side builder only: no GPU needed to build one).

crowd() is material_scene's floor, camera and lights with n small spheres
standing on the floor: 61 primitives, 121 BVH nodes at n = 60. Its oracle film
is non-black in about 0.9 of its pixels (four materials) or all of them
(Matte), where many_spheres_scene's is black in four pixels of five at a few
samples per pixel.
"""
import functools
import os
from collections import namedtuple

import numpy as np

import oracle_lib as O
import pbrtgpu as G
from pbrtgpu import abi
from scenes import material_scene, readme_lights_scene


def crowd(n=60, seed=7, w=48, h=32, kinds=("matte", "mirror", "glass", "oren"), lights=2, bright=False,
          lens=0.0, focal=20.0):
    """kinds: the spheres' materials, in turn. lights: the area light, the point
    light and lights - 2 more point lights on a ring. bright: the point light
    at 1e5, whose estimates exceed 10 (the reference panics: Ld > 10).
    lens, focal: a thin lens."""
    rng = np.random.default_rng(seed)
    s = G.Scene()
    chk = s.add_checker((0.2, 0, 0), (0, 0, 0.2), 0, 0, (1, 1, 1), (0.18, 0.18, 0.18))
    s.add_primitive(s.add_disk(G.rotate(0, 90), 0.0, 100.0), chk)
    mk = {"matte": lambda: s.add_matte((0.6, 0.1, 0.1)), "mirror": lambda: s.add_mirror(),
          "glass": lambda: s.add_glass(), "oren": lambda: s.add_matte((0.5, 0.6, 0.4), sigma=30.0)}
    mats = [mk[k]() for k in kinds]
    for i in range(n):
        r = rng.uniform(0.3, 0.7)
        s.add_primitive(s.add_sphere(G.translate(0, 0, 0), r), mats[i % len(mats)],
                        G.translate(rng.uniform(-6, 6), r, rng.uniform(-6, 5)))
    s.add_area_light((6, 6, 6), s.add_sphere(G.translate(0, 9, 2), 0.75))
    s.add_point_light(G.translate(-6, 10, 8), (1e5,) * 3 if bright else (60, 60, 60))
    for i in range(lights - 2):
        a = 2 * np.pi * i / max(1, lights - 2)
        s.add_point_light(G.translate(8 * np.cos(a), 8 + 0.1 * i, 8 * np.sin(a)), (20 + i, 20, 24))
    s.set_film(w, h)
    s.set_camera(G.look_at((0, 7, 12), (0, 1.5, 0), (0, 1, 0)), lens=lens, focal=focal, fov=55)
    return s.build(max_prims_in_node=1)


# ---- the renders of tests/test_gpu_large_scenes.py, checked on the host by
# tests/test_large_scenes_host.py: name -> Render. `point` says what the render is
# there for: "nodes" (n_nodes > 64), "lights" (n_lights > 16), "lights16" (the
# largest count k_paths_ci still takes) or "small" (an LDS-staged tree, few lights).
Render = namedtuple("Render", "scene rd point random panics", defaults=(0, False))

MATTE = ("matte",)
TP = dict(mode=abi.PBRT_MODE_THROUGHPUT)
KX = dict(spp_x=2, spp_y=2, n_dims=4, max_depth=8)
CAM0 = dict(spp_x=2, spp_y=2, n_dims=0, max_depth=5)

RENDERS = {
    # Mirror / Glass / OrenNayar on 121 nodes, THROUGHPUT mode: no chain, k_mb_setup<true> and the kX wavefront
    "kx_tp": Render(crowd, dict(KX, **TP), "nodes"),
    "kx_tp_s33_d12": Render(crowd, dict(KX, spp_x=3, spp_y=3, max_depth=12, **TP), "nodes"),
    # more than 16 lights
    "matte_l16": Render(lambda: crowd(kinds=MATTE, lights=16), KX, "lights16"),
    "matte_l17": Render(lambda: crowd(kinds=MATTE, lights=17), KX, "lights"),
    "matte_l20": Render(lambda: crowd(kinds=MATTE, lights=20), KX, "lights"),
    "matte_l64": Render(lambda: crowd(kinds=MATTE, lights=64), KX, "lights"),
    "matte_l2": Render(lambda: crowd(kinds=MATTE), KX, "nodes"),
    "matte_l20_tp": Render(lambda: crowd(kinds=MATTE, lights=20), dict(KX, **TP), "lights"),
    "readme_l20": Render(lambda: readme_lights_scene(32, 32, extra=16), KX, "lights"),
    "kx_small_l20": Render(lambda: crowd(n=4, lights=20), KX, "lights"),   # four materials on an LDS-staged tree
    "kx_l20_tp": Render(lambda: crowd(lights=20), dict(KX, **TP), "lights"),
    "bright_l20": Render(lambda: crowd(n=4, kinds=MATTE, lights=20, bright=True), KX, "lights", panics=True),
    # the camera-start route with more than 16 lights (an LDS-staged tree)
    "cam_l20": Render(lambda: readme_lights_scene(32, 32, extra=16), CAM0, "lights"),
    "cam_l20_s33": Render(lambda: readme_lights_scene(32, 32, extra=16), dict(CAM0, spp_x=3, spp_y=3), "lights"),
    "cam_l20_random5": Render(lambda: readme_lights_scene(32, 32, extra=16), dict(max_depth=5), "lights", random=5),
    "cam_l64": Render(lambda: crowd(n=4, kinds=MATTE, lights=64), CAM0, "lights"),
    "cam_l20_tp": Render(lambda: readme_lights_scene(32, 32, extra=16), dict(CAM0, **TP), "lights"),
    # small scenes, whose kernels must not change
    "small_kx": Render(material_scene, KX, "small"),
    "small_readme": Render(lambda: G.Scene.readme(45, 30), KX, "small"),
}

ORACLE_FLAG_RANDOM_SAMPLER = 2
THREADS = min(16, os.cpu_count() or 1)


def make_rd(name):
    r = RENDERS[name]
    rd = abi.render_desc(**r.rd)
    if r.random:
        G.lib().pbrt_random_sampler(r.random, G.C.byref(rd))
    return rd


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(rc, film, stats) of the oracle for RENDERS[name]: computed once per process,
    shared by the tests, never written to."""
    r = RENDERS[name]
    scene = r.scene()   # (owns the descriptor's arrays: alive until the oracle returns)
    rc, film, st = O.render(scene.desc, make_rd(name), threads=THREADS,
                            flags=ORACLE_FLAG_RANDOM_SAMPLER if r.random else 0)
    film.setflags(write=False)
    return rc, film, st

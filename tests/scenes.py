"""Scene builders shared by the tests and tests/golden/make_golden.py (host-side
pbrt_sb_* builder only: no GPU needed to build a scene)."""
import numpy as np

import pbrtgpu as G


def material_scene(kind="both", w=32, h=24, rough=0.0, area=True, kt=(0.5, 0.5, 0.5), sigma=0.0,
                   glass_kr=(0.5, 0.5, 0.5)):
    """A floor, a glass sphere, a mirror sphere and a matte sphere, lit by a
    point light and an area-light sphere. kind: "both" | "matte" (the two
    special spheres matte) | "black" (the two special spheres black matte)."""
    s = G.Scene()
    chk = s.add_checker((0.2, 0, 0), (0, 0, 0.2), 0, 0, (1, 1, 1), (0.18, 0.18, 0.18))
    floor = s.add_disk(G.rotate(0, 90), 0.0, 100.0)
    s.add_primitive(floor, chk)
    red = s.add_matte((0.6, 0.1, 0.1), sigma=sigma)
    if kind == "both":
        glass = s.add_glass(kr=glass_kr, kt=kt, u_roughness=rough, v_roughness=0.5 * rough)   # server.go:80-87
        mirror = s.add_mirror()
    elif kind == "matte":
        glass = mirror = s.add_matte((0.5, 0.5, 0.5))
    else:
        glass = mirror = s.add_matte((0.0, 0.0, 0.0))
    for (x, z, m) in ((-2.5, 0.0, glass), (2.5, 0.0, mirror), (0.0, -4.0, red)):
        sph = s.add_sphere(G.translate(0, 0, 0), 2.0)
        s.add_primitive(sph, m, G.translate(x, 2.0, z))
    if area:
        light = s.add_sphere(G.translate(0, 9, 2), 0.75)
        s.add_area_light((6, 6, 6), light)
    s.add_point_light(G.translate(-6, 10, 8), (60, 60, 60))
    s.set_film(w, h)
    s.set_camera(G.look_at((0, 7, 12), (0, 1.5, 0), (0, 1, 0)), fov=55)
    return s.build(max_prims_in_node=1)


def many_spheres_scene(n=90, seed=5, w=64, h=48):
    """test_gpu_parity.py's scene of n Matte spheres: a BVH beyond the 64
    LDS-staged nodes, so k_chain_ci walks with the [64] stack and the paths run
    on the path wavefront."""
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
    s.set_film(w, h)
    s.set_camera(G.look_at((0, 5, 14), (0, 0, 0), (0, 1, 0)), fov=50)
    return s.build()


def readme_lights_scene(w=32, h=32, extra=8):
    """The README scene (4 lights) with `extra` more point lights on a ring above
    the spheres: with 12 lights 8 pixels' light lanes no longer fit one wave
    (8 * 12 > 64), so k_paths_ci runs 4 pixels per wave."""
    s = G.Scene.readme(w, h)
    for i in range(extra):
        a = 2.0 * np.pi * i / extra
        s.add_point_light(G.translate(40.0 + 25.0 * np.cos(a), 30.0 + 2.0 * i, 40.0 + 25.0 * np.sin(a)),
                          (300.0 + 40.0 * i, 300.0, 340.0 - 20.0 * i))
    return s.build(2)


def mesh_material_scene(material, w=40, h=32):
    """A small triangle mesh (a tilted 4x4-quad grid) made of `material`
    ("glass" | "mirror" | "oren"), over the checker floor, beside a matte
    sphere; include/pbrt_gpu.h lets a mesh take any material."""
    s = G.Scene()
    chk = s.add_checker((0.2, 0, 0), (0, 0, 0.2), 0, 0, (1, 1, 1), (0.18, 0.18, 0.18))
    s.add_primitive(s.add_disk(G.rotate(0, 90), 0.0, 100.0), chk)
    m = {"glass": lambda: s.add_glass(), "mirror": lambda: s.add_mirror(),
         "oren": lambda: s.add_matte((0.5, 0.6, 0.4), sigma=30.0)}[material]()
    n = 4
    xs = np.linspace(-3.0, 3.0, n + 1)
    p = np.array([(x, 1.0 + 0.4 * x + 0.3 * z, z) for z in xs for x in xs], dtype=np.float32)
    idx = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i, (j + 1) * (n + 1) + i + 1
            idx += [(a, b, d), (a, d, c)]
    s.add_mesh(p, np.array(idx, dtype=np.int32), m)
    s.add_primitive(s.add_sphere(G.translate(0, 0, 0), 1.5), s.add_matte((0.6, 0.1, 0.1)), G.translate(0, 1.5, -4))
    s.add_point_light(G.translate(-6, 10, 8), (60, 60, 60))
    s.add_area_light((6, 6, 6), s.add_sphere(G.translate(0, 9, 2), 0.75))
    s.set_film(w, h)
    s.set_camera(G.look_at((0, 7, 12), (0, 1.5, 0), (0, 1, 0)), fov=55)
    return s.build(max_prims_in_node=1)

"""The edge shapes of tests/test_gpu_edges.py on every render route: the scene and the
renders of tests/test_gpu_edges_routes.py (host-side builder and the oracle: no GPU).

edge_crowd() holds edge_scene(partial=True, disk_edges=True, neg_scale=True,
two_sided=True)'s shapes, their materials taken in turn from `kinds` (so a holed disk is
a Mirror and a partial sphere Glass), filler spheres until the tree has more than 64
nodes, and one more area light on a partial sphere (z_max < r, phi_max < 360) that
stands on the floor: the floor points below it lie inside its radius, where
Sphere.Sample takes its inside-the-sphere branch, and its area is phi_max * radius *
(z_max - z_min). edges=False is the same scene with every edge flag off (full
spheres, whole disks, no mirroring, a one-sided light on a plain sphere, a full light
sphere): the oracle's film must differ from it, or the edges are not in view.
"""
import functools
from collections import namedtuple

import numpy as np

import oracle_lib as O
import pbrtgpu as G
from adversarial_rays import proper
from pbrtgpu import abi

MATTE = ("matte",)
KINDS4 = ("matte", "mirror", "glass", "oren")
THREADS = 16


def edge_crowd(kinds=KINDS4, lights=2, lens=0.0, crop=(0, 0, 1, 1), filter_radius=1.0, edges=True, fill=30, seed=9,
               w=48, h=32, partial_light=True):
    """lights: the reversed two-sided area light, the point light and lights - 2 more point
    lights on a ring; the partial-sphere area light comes on top. fill: filler spheres (0: the
    small tree of at most 64 nodes). partial_light=False leaves the partial-sphere light out."""
    rng = np.random.default_rng(seed)
    s = G.Scene()
    mk = {"matte": lambda: s.add_matte((0.6, 0.1, 0.1)), "mirror": lambda: s.add_mirror(),
          "glass": lambda: s.add_glass(), "oren": lambda: s.add_matte((0.5, 0.6, 0.4), sigma=30.0)}
    mats = [mk[k]() for k in kinds]
    turn = iter(range(1000))

    def mat():
        return mats[next(turn) % len(mats)]

    if edges:
        # (edge_scene's order: NewBVH's partition panics on some orders of the same primitives)
        floor_m, ring_m, cap_m, band_m, under_m = mat(), mat(), mat(), mat(), mat()   # the cap: Glass, the ring: Mirror
        s.add_primitive(s.add_disk(G.rotate(0, 90), 0.0, 30.0, inner=3.0, phi_max=300.0), floor_m)   # the floor: holed
        ring = s.add_disk(G.mul(G.translate(0, 3, -4), G.rotate(2, 30)), 0.0, 4.0, inner=1.5, phi_max=250.0)
        s.add_primitive(ring, ring_m)
        s.add_primitive(s.add_disk(G.rotate(0, 90), -0.5, 40.0), under_m)                            # seen through the hole
        cap = s.add_sphere(G.rotate(0, -90), 2.0, z_min=-1.0, z_max=1.2, phi_max=270.0)
        s.add_primitive(cap, cap_m, G.translate(-2.5, 2.0, 0.0))
        band = s.add_sphere(G.rotate(0, -90), 2.0, z_min=-0.6, z_max=0.9, phi_max=200.0, reverse=True)
        s.add_primitive(band, band_m, G.translate(2.5, 2.0, 0.0))
        s.add_primitive(s.add_sphere(G.scale(1, 1, -1), 1.5), mat(), G.mul(G.translate(0.0, 1.5, -4.0), G.scale(-1, 1, 1)))
        s.add_primitive(s.add_disk(G.mul(G.translate(0, 1.0, 3), G.scale(-1, 1, 1)), 0.0, 1.0), mat())
        s.add_area_light((6, 6, 6), s.add_sphere(G.translate(0, 9, 2), 0.75, reverse=True), two_sided=True)
        # the light on a partial sphere, standing on the floor at the right: the floor below it is inside its radius
        if partial_light:
            light = s.add_sphere(proper(G.mul(G.translate(5.0, 0.75, 3.0), G.rotate(0, -90))), 1.5,
                                 z_min=-1.0, z_max=1.2, phi_max=250.0)
            s.add_area_light((0.3, 0.25, 0.2), light)
    else:
        s.add_primitive(s.add_disk(G.rotate(0, 90), 0.0, 30.0), mat())
        s.add_primitive(s.add_disk(G.mul(G.translate(0, 3, -4), G.rotate(2, 30)), 0.0, 4.0), mat())
        s.add_primitive(s.add_disk(G.rotate(0, 90), -0.5, 40.0), mat())
        for x in (-2.5, 2.5):
            s.add_primitive(s.add_sphere(G.rotate(0, -90), 2.0), mat(), G.translate(x, 2.0, 0.0))
        s.add_primitive(s.add_sphere(G.translate(0, 0, 0), 1.5), mat(), G.translate(0.0, 1.5, -4.0))
        s.add_primitive(s.add_disk(G.translate(0, 1.0, 3), 0.0, 1.0), mat())
        s.add_area_light((6, 6, 6), s.add_sphere(G.translate(0, 9, 2), 0.75))
        s.add_area_light((0.3, 0.25, 0.2), s.add_sphere(proper(G.mul(G.translate(5.0, 0.75, 3.0), G.rotate(0, -90))), 1.5))
    for i in range(fill):
        r = rng.uniform(0.3, 0.6)
        s.add_primitive(s.add_sphere(G.translate(0, 0, 0), r), mat(),
                        G.translate(rng.uniform(-7, 7), r, rng.uniform(2, 7)))
    s.add_point_light(G.translate(-6, 10, 8), (60, 60, 60))
    for i in range(lights - 2):
        a = 2 * np.pi * i / max(1, lights - 2)
        s.add_point_light(G.translate(8 * np.cos(a), 8 + 0.1 * i, 8 * np.sin(a)), (20 + i, 20, 24))
    s.set_film(w, h, crop=crop, filter_radius=(filter_radius, filter_radius))
    s.set_camera(G.look_at((0, 6, 14), (0, 1.5, 0), (0, 1, 0)), lens=lens, focal=12.0, fov=55)
    return s.build(max_prims_in_node=1)


def disk_light_scene():
    """An annular disk as an area light's shape: the device takes spheres only."""
    s = G.Scene()
    s.add_primitive(s.add_disk(G.rotate(0, 90), 0.0, 30.0), s.add_matte((0.5, 0.5, 0.5)))
    s.add_area_light((6, 6, 6), s.add_disk(G.mul(G.translate(0, 5, 0), G.rotate(0, 90)), 0.0, 2.0, inner=1.0, phi_max=300.0))
    s.set_film(16, 16)
    s.set_camera(G.look_at((0, 6, 14), (0, 1.5, 0), (0, 1, 0)), fov=55)
    return s.build(max_prims_in_node=1)


# name -> (scene arguments, render_desc arguments); every render is 48x32, 2x2 spp, max_depth 5
E = dict(spp_x=2, spp_y=2, max_depth=5)
TP = dict(mode=abi.PBRT_MODE_THROUGHPUT)
DL = dict(integrator=abi.PBRT_INTEGRATOR_DIRECT_LIGHTING)
Render = namedtuple("Render", "scene rd")
RENDERS = {
    # the large tree (more than 64 nodes)
    "matte": Render(dict(kinds=MATTE), E),
    "matte_tp": Render(dict(kinds=MATTE), dict(E, **TP)),
    "kx": Render(dict(kinds=KINDS4), E),
    "kx_tp": Render(dict(kinds=KINDS4), dict(E, **TP)),
    "matte_l20": Render(dict(kinds=MATTE, lights=20), E),
    "dl_matte": Render(dict(kinds=MATTE), dict(E, **DL)),
    "dl_kx": Render(dict(kinds=KINDS4), dict(E, **DL)),
    "cam": Render(dict(kinds=MATTE), dict(E, n_dims=0)),
    "cam_tp": Render(dict(kinds=MATTE), dict(E, n_dims=0, **TP)),
    "cam_lens": Render(dict(kinds=MATTE, lens=0.3), dict(E, n_dims=1)),
    "cam_crop": Render(dict(kinds=MATTE, crop=(0.25, 0.1, 0.8, 0.9), filter_radius=1.5), dict(E, n_dims=0)),
    # the small tree: the edge shapes alone, four materials
    "small_kx": Render(dict(kinds=KINDS4, fill=0), E),
    "small_kx_tp": Render(dict(kinds=KINDS4, fill=0), dict(E, **TP)),
}


def scene(name, edges=True):
    return edge_crowd(edges=edges, **RENDERS[name].scene)


def make_rd(name):
    return abi.render_desc(**RENDERS[name].rd)


@functools.lru_cache(maxsize=None)
def oracle(name, edges=True):
    """(rc, film, stats) of the oracle for RENDERS[name] (edges=False: the same scene with the
    edge flags off): computed once per process, never written to."""
    sc = scene(name, edges)   # (owns the descriptor's arrays: alive until the oracle returns)
    rc, film, st = O.render(sc.desc, make_rd(name), threads=THREADS)
    film.setflags(write=False)
    return rc, film, st

"""Renders of trees beyond 64 BVH nodes on the routes that took only LDS-staged
trees: the kX chain (Mirror / Glass / OrenNayar, EXACT mode) and the camera-start
route. The scene is tests/large_scenes.py's crowd(): 61 primitives, 121 nodes
(crowd_mesh(): the same with a triangle mesh).

RENDERS is read by tests/test_gpu_large_trees.py (against the oracle, on the GPU)
and tests/test_large_trees_host.py (every render is a fit witness; no GPU).
"""
import functools

import numpy as np

import large_scenes as L
import oracle_lib as O
import pbrtgpu as G
from large_scenes import CAM0, KX, MATTE, TP, Render, crowd
from pbrtgpu import abi


def crowd_mesh(n=60, seed=7, w=48, h=32, quads=4):
    """crowd()'s floor, camera, lights and n spheres of its four materials (121 BVH nodes
    at n = 60), plus a Matte triangle mesh: a bumpy quads x quads patch standing among the
    spheres, so that a traversal goes on into the mesh after the [64]-stack walk."""
    rng = np.random.default_rng(seed)
    s = G.Scene()
    chk = s.add_checker((0.2, 0, 0), (0, 0, 0.2), 0, 0, (1, 1, 1), (0.18, 0.18, 0.18))
    s.add_primitive(s.add_disk(G.rotate(0, 90), 0.0, 100.0), chk)
    mats = [s.add_matte((0.6, 0.1, 0.1)), s.add_mirror(), s.add_glass(), s.add_matte((0.5, 0.6, 0.4), sigma=30.0)]
    for i in range(n):
        r = rng.uniform(0.3, 0.7)
        s.add_primitive(s.add_sphere(G.translate(0, 0, 0), r), mats[i % len(mats)],
                        G.translate(rng.uniform(-6, 6), r, rng.uniform(-6, 5)))
    g = np.linspace(-2.5, 2.5, quads + 1)
    p = np.array([(x, 1.6 + 0.5 * np.sin(1.7 * x) * np.cos(1.3 * z), z) for z in g for x in g], dtype=np.float32)
    v = lambda i, j: j * (quads + 1) + i   # noqa: E731
    idx = [t for j in range(quads) for i in range(quads)
           for t in ((v(i, j), v(i + 1, j), v(i + 1, j + 1)), (v(i, j), v(i + 1, j + 1), v(i, j + 1)))]
    s.add_mesh(p, np.array(idx, dtype=np.int32), s.add_matte((0.2, 0.3, 0.7)))
    s.add_area_light((6, 6, 6), s.add_sphere(G.translate(0, 9, 2), 0.75))
    s.add_point_light(G.translate(-6, 10, 8), (60, 60, 60))
    s.set_film(w, h)
    s.set_camera(G.look_at((0, 7, 12), (0, 1.5, 0), (0, 1, 0)), fov=55)
    return s.build(max_prims_in_node=1)


RENDERS = {
    # ---- A: Mirror / Glass / OrenNayar, EXACT: k_chain_ci<kW, 64, true, ...> and the kX path wavefront
    "kx_exact": Render(crowd, KX, "nodes"),
    "kx_exact_s33_d12": Render(crowd, dict(KX, spp_x=3, spp_y=3, max_depth=12), "nodes"),
    "kx_exact_nd2": Render(crowd, dict(KX, n_dims=2), "nodes"),   # the bounce-1 light sample is a draw per sample
    "kx_exact_nd1": Render(crowd, dict(KX, n_dims=1), "nodes"),
    "kx_exact_norr": Render(crowd, dict(KX, rr_threshold=0.0), "nodes"),
    # glass only, 7 sampled dimensions, depth 12: meant to put Russian-roulette draws on stratified dimensions
    "kx_exact_glass": Render(lambda: crowd(kinds=("glass",)), dict(KX, spp_x=3, spp_y=3, n_dims=7, max_depth=12),
                             "nodes"),
    "kx_exact_l20": Render(lambda: crowd(lights=20), KX, "nodes"),
    # the same with a triangle mesh in the scene: mesh_walk_mixed after the stack walk
    "kx_exact_mesh": Render(crowd_mesh, KX, "nodes"),
    "kx_exact_bright": Render(lambda: crowd(bright=True), KX, "nodes", panics=True),
    # ---- B: the camera-start route (Matte): k_chain_cam_stack / k_cam_setup and k_paths_cam_stack<P, kMB>
    "cam_nodes": Render(lambda: crowd(kinds=MATTE), CAM0, "nodes"),
    "cam_nodes_s33": Render(lambda: crowd(kinds=MATTE), dict(CAM0, spp_x=3, spp_y=3), "nodes"),
    "cam_nodes_random5": Render(lambda: crowd(kinds=MATTE), dict(max_depth=5), "nodes", random=5),
    # a thin lens and one sampled dimension: StartPixel, and s1d[0][k] as the time
    "cam_nodes_lens": Render(lambda: crowd(kinds=MATTE, lens=0.3), dict(CAM0, n_dims=1), "nodes"),
    "cam_nodes_tp": Render(lambda: crowd(kinds=MATTE), dict(CAM0, **TP), "nodes"),
    "cam_nodes_l20": Render(lambda: crowd(kinds=MATTE, lights=20), CAM0, "nodes"),
    "cam_nodes_s66": Render(lambda: crowd(kinds=MATTE, w=16, h=16), dict(CAM0, spp_x=6, spp_y=6), "nodes"),   # P = 4
    "cam_nodes_bright": Render(lambda: crowd(kinds=MATTE, bright=True), CAM0, "nodes", panics=True),
}

A_RENDERS = [n for n in RENDERS if n.startswith("kx_") and not RENDERS[n].panics]
B_RENDERS = [n for n in RENDERS if n.startswith("cam_") and not RENDERS[n].panics]


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
    rc, film, st = O.render(scene.desc, make_rd(name), threads=L.THREADS,
                            flags=L.ORACLE_FLAG_RANDOM_SAMPLER if r.random else 0)
    film.setflags(write=False)
    return rc, film, st

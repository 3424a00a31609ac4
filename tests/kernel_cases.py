"""The coverage table: one small case per compiled kernel that must launch it.

A case is a scene, render_desc arguments, Renderer options and environment
knobs; `covers` lists the kernels of the manifest (tests/kernel_manifest.py)
the case is responsible for. COVERAGE inverts that: kernel -> case. A kernel
that no log can see is in EXEMPT, with the existing test that launches it.
tests/test_kernel_manifest.py (no GPU) holds COVERAGE + EXEMPT equal to the
manifest; tests/test_gpu_kernel_coverage.py renders every case twice against
the oracle and finds the kernels in the launch log.

The launch decision each case steers is frame_route.h's (chain_launch, paths_ci_pixels,
cam_pixels_per_wave, the route): the arguments render.hip's launch_ci, launch_paths,
enqueue_cam and the serial launch give their kernel selectors (chain_kernel,
paths_ci_kernel, paths_cam_kernel, serial_kernel), and paths_wavefront; the comment
of a case says which condition selects its kernel.
"""
from collections import namedtuple

import pbrtgpu as G
from launch_checks import chain as ci
from pbrtgpu import abi
from scenes import many_spheres_scene, material_scene, readme_lights_scene

CI, WAVE, DL, SERIAL, CAM = (abi.PBRT_KERNEL_WAVE_CI, abi.PBRT_KERNEL_WAVE, abi.PBRT_KERNEL_WAVE_DL,
                             abi.PBRT_KERNEL_SERIAL, abi.PBRT_KERNEL_WAVE_CAM)

SCENES = {
    "readme45x30": lambda: G.Scene.readme(45, 30),   # 6 tiles of 16 px, ragged
    "readme45x46": lambda: G.Scene.readme(45, 46),   # 9 ragged tiles: a multiple of neither 2 nor 4
    "readme32x32": lambda: G.Scene.readme(32, 32),
    "readme16x16": lambda: G.Scene.readme(16, 16),   # one tile
    "lights12": lambda: readme_lights_scene(32, 32, extra=8),   # 12 lights: 4 pixels per k_paths_ci wave
    "glass48x32": lambda: G.Scene.readme_glass(48, 32),         # Glass + Mirror: the kX kernels
    "mesh48x32": lambda: G.Scene.heightfield(48, 32, quads=8, seed=1),   # a mesh and no analytic primitive
    "mesh33": lambda: G.Scene.heightfield(32, 32, quads=33, seed=2),     # 2178 triangles: the sort pads to 4096 keys
    "spheres90": lambda: many_spheres_scene(90, 5),             # 181 BVH nodes: beyond the 64 LDS-staged ones
    "dl_matte": lambda: material_scene("matte"),
    "dl_glass": lambda: material_scene("both"),
}

# scene, render_desc arguments, Renderer options, environment, expected st.kernel,
# kernels the case must launch in a frame (either of the two), kernels it must
# launch in the learned (second) frame, kernels it must launch outside a frame
Case = namedtuple("Case", "scene rd opts env family covers learned outside", defaults=((), ()))


S22 = dict(spp_x=2, spp_y=2)
SPWIN = dict(spp_x=11, spp_y=11, jitter=False, max_depth=3)   # 121 spp, no jitter: the windowed StartPixel
TP = dict(mode=abi.PBRT_MODE_THROUGHPUT)
DLI = dict(spp_x=2, spp_y=2, max_depth=3, integrator=abi.PBRT_INTEGRATOR_DIRECT_LIGHTING)
NOSAMP = dict(n_dims=0, max_depth=5)   # no sampled dimension: the camera ray belongs to the sample (wave_cam)


def waves(w, eu=None, **more):
    env = {"PBRT_CI_WAVES": str(w)}
    if eu:
        env["PBRT_CI_EU"] = str(eu)
    env.update(more)
    return env


CASES = {
    # ---- the Matte chain on an LDS-staged tree; the frame's other kernels ride on the first case:
    # frame 1 probes (k_tile_cost, the sort, k_order_of_keys), frame 2 runs the completion-driven
    # path stage behind k_gate
    "ci_w1_eu3": Case("readme45x30", S22, {}, waves(1, 3), CI,
                      (ci(1), "k_wf_primary<false>", "k_tile_cost<false>", "k_bitonic_local", "k_order_of_keys",
                       "k_paths_ci<8, false, false>", "k_film", "k_panic_reduce", "k_merge_film"),
                      learned=("k_gate",)),
    "ci_w1_eu2": Case("readme45x30", S22, {}, waves(1, 2), CI, (ci(1, eu=2),)),
    "ci_w2": Case("readme45x30", S22, {}, waves(2), CI, (ci(2),)),
    "ci_w4": Case("readme45x30", S22, {}, waves(4), CI, (ci(4),)),
    "ci_w8": Case("readme45x30", S22, {}, waves(8), CI, (ci(8),)),
    # ---- n_nodes > kLdsNodes: the [64]-stack walk, and the paths on the path wavefront
    "stack_w1_eu3": Case("spheres90", S22, {}, waves(1, 3), CI,
                         (ci(1, 64), "k_pw_cache<false>", "k_pw_start<false, false>", "k_pw_trace<false>",
                          "k_pw_shade<false>", "k_pw_shadow<false>", "k_pw_panics")),
    "stack_w1_eu2": Case("spheres90", S22, {}, waves(1, 2), CI, (ci(1, 64, eu=2),)),
    "stack_w2": Case("spheres90", S22, {}, waves(2), CI, (ci(2, 64),)),
    "stack_w4": Case("spheres90", S22, {}, waves(4), CI, (ci(4, 64),)),
    "stack_w8": Case("spheres90", S22, {}, waves(8), CI, (ci(8, 64),)),
    # ---- rp.sp_window: the serial StartPixel's sample count, without jitter
    "spwin_w1_eu3": Case("readme16x16", SPWIN, {}, waves(1, 3), CI, (ci(1, spwin=True),)),
    "spwin_w1_eu2": Case("readme16x16", SPWIN, {}, waves(1, 2), CI, (ci(1, eu=2, spwin=True),)),
    "spwin_w2": Case("readme16x16", SPWIN, {}, waves(2), CI, (ci(2, spwin=True),)),
    "spwin_w4": Case("readme16x16", SPWIN, {}, waves(4), CI, (ci(4, spwin=True),)),
    "spwin_w8": Case("readme16x16", SPWIN, {}, waves(8), CI, (ci(8, spwin=True),)),
    # ---- mesh_only: n_prims == 0; its paths run the kMeshOnly wavefront kernels
    "mesh_w1": Case("mesh48x32", S22, {}, waves(1), CI, (ci(1, -1), "k_pw_trace<true>", "k_pw_shadow<true>")),
    "mesh_w2": Case("mesh48x32", S22, {}, waves(2), CI, (ci(2, -1),)),
    "mesh_w4": Case("mesh48x32", S22, {}, waves(4), CI, (ci(4, -1),)),
    "mesh_w8": Case("mesh48x32", S22, {}, waves(8), CI, (ci(8, -1),)),
    # ---- non_matte: kX. One wave runs the per-lane (kMulti) code; ci_waves clamps kX to 4 waves
    "kx_w1": Case("glass48x32", S22, {}, waves(1), CI,
                  (ci(1, kx=True, multi=True), "k_wf_primary<true>", "k_tile_cost<true>", "k_paths_ci<8, false, true>")),
    "kx_w2": Case("glass48x32", S22, {}, waves(2), CI, (ci(2, kx=True),)),
    "kx_w4_p4": Case("glass48x32", S22, {}, waves(4, PBRT_PATHS_CI="4"), CI, (ci(4, kx=True), "k_paths_ci<4, false, true>")),
    # ---- opts.lanes_per_wave = 2 or 4: several tiles per wave (kMulti)
    "multi_eu3": Case("readme45x46", S22, dict(lanes_per_wave=2), {"PBRT_CI_EU": "3"}, CI, (ci(1, multi=True),)),
    "multi_eu2": Case("readme45x46", S22, dict(lanes_per_wave=4), {"PBRT_CI_EU": "2"}, CI, (ci(1, eu=2, multi=True),)),
    "multi_stack_eu3": Case("spheres90", S22, dict(lanes_per_wave=2), {"PBRT_CI_EU": "3"}, CI, (ci(1, 64, multi=True),)),
    "multi_stack_eu2": Case("spheres90", S22, dict(lanes_per_wave=4), {"PBRT_CI_EU": "2"}, CI,
                            (ci(1, 64, eu=2, multi=True),)),
    "multi_spwin_eu3": Case("readme16x16", SPWIN, dict(lanes_per_wave=2), {"PBRT_CI_EU": "3"}, CI,
                            (ci(1, spwin=True, multi=True),)),
    "multi_spwin_eu2": Case("readme16x16", SPWIN, dict(lanes_per_wave=2), {"PBRT_CI_EU": "2"}, CI,
                            (ci(1, eu=2, spwin=True, multi=True),)),
    "multi_mesh": Case("mesh48x32", S22, dict(lanes_per_wave=4), {}, CI, (ci(1, -1, multi=True),)),
    # ---- a forced heavy/light split: the learned frame runs both instantiations
    "split_heavy4": Case("readme45x30", dict(spp_x=3, spp_y=3), {}, waves(1, 3, PBRT_CI_HEAVY="2"), CI, (),
                         learned=(ci(4), ci(1), "k_gate")),
    "split_heavy8": Case("readme45x30", dict(spp_x=3, spp_y=3), {},
                         waves(2, 3, PBRT_CI_HEAVY="2", PBRT_CI_HEAVY_WAVES="8"), CI, (),
                         learned=(ci(8), ci(1), "k_gate")),
    # ---- k_paths_ci's pixels per wave: 8 * n_lights <= 64, else 4; PBRT_PATHS_CI=2
    "paths_p4": Case("lights12", S22, {}, {}, CI, ("k_paths_ci<4, false, false>",)),
    "paths_p2": Case("readme45x30", S22, {}, {"PBRT_PATHS_CI": "2"}, CI, ("k_paths_ci<2, false, false>",)),
    # ---- THROUGHPUT: k_mb_setup instead of the chain
    "tp_p8": Case("readme45x30", dict(S22, **TP), {}, {}, WAVE, ("k_mb_setup<false>", "k_paths_ci<8, true, false>")),
    "tp_p4": Case("lights12", dict(S22, **TP), {}, {}, WAVE, ("k_paths_ci<4, true, false>",)),
    "tp_p2": Case("readme45x30", dict(S22, **TP), {}, {"PBRT_PATHS_CI": "2"}, WAVE, ("k_paths_ci<2, true, false>",)),
    "tp_kx_p8": Case("glass48x32", dict(S22, **TP), {}, {}, WAVE, ("k_mb_setup<true>", "k_paths_ci<8, true, true>")),
    "tp_kx_p4": Case("glass48x32", dict(S22, **TP), {}, {"PBRT_PATHS_CI": "4"}, WAVE, ("k_paths_ci<4, true, true>",)),
    # ---- PBRT_PATHS_WF=1: the path wavefront on analytic scenes; PBRT_PW_SORT=1: the material sort
    "pw_kx": Case("glass48x32", S22, {}, {"PBRT_PATHS_WF": "1"}, CI,
                  ("k_pw_cache<true>", "k_pw_start<false, true>", "k_pw_shade<true>")),
    "pw_kx_tp": Case("glass48x32", dict(S22, **TP), {}, {"PBRT_PATHS_WF": "1"}, WAVE, ("k_pw_start<true, true>",)),
    "pw_tp_sort": Case("readme45x30", dict(S22, **TP), {}, {"PBRT_PATHS_WF": "1", "PBRT_PW_SORT": "1"}, WAVE,
                       ("k_pw_start<true, false>", "k_pw_scan", "k_pw_scatter")),
    # ---- DirectLighting
    "dl_matte": Case("dl_matte", DLI, {}, {}, DL, ("k_dl_setup", "k_dl_samples<false>", "k_dl_panics")),
    "dl_kx": Case("dl_glass", DLI, {}, {}, DL, ("k_dl_samples<true>",)),
    # ---- the camera-start route: pixels per k_paths_cam wave by spp - 1 (< 8: 64, < 32: 16, else 4;
    # 4 pixels per wave need 33 spp at least: 6x6 on the one-tile image)
    "cam_p64": Case("readme32x32", dict(S22, **NOSAMP), dict(kernel="wave_cam"), {}, CAM,
                    ("k_chain_cam", "k_paths_cam<64, false>", "k_film_cam<false>")),
    "cam_p16": Case("readme32x32", dict(spp_x=3, spp_y=3, **NOSAMP), dict(kernel="wave_cam"), {}, CAM,
                    ("k_paths_cam<16, false>",)),
    "cam_p4": Case("readme16x16", dict(spp_x=6, spp_y=6, **NOSAMP), dict(kernel="wave_cam"), {}, CAM,
                   ("k_paths_cam<4, false>",)),
    "cam_tp_p64": Case("readme32x32", dict(S22, **NOSAMP, **TP), dict(kernel="wave_cam"), {}, CAM,
                       ("k_cam_setup", "k_paths_cam<64, true>", "k_film_cam<true>")),
    "cam_tp_p16": Case("readme32x32", dict(spp_x=3, spp_y=3, **NOSAMP, **TP), dict(kernel="wave_cam"), {}, CAM,
                       ("k_paths_cam<16, true>",)),
    "cam_tp_p4": Case("readme16x16", dict(spp_x=6, spp_y=6, **NOSAMP, **TP), dict(kernel="wave_cam"), {}, CAM,
                      ("k_paths_cam<4, true>",)),
    # ---- the serial kernel: opts.occupancy picks the amdgpu_waves_per_eu build
    "serial_occ1": Case("readme32x32", S22, dict(kernel="serial"), {}, SERIAL, ("k_render_exact<1>",)),
    "serial_occ2": Case("readme32x32", S22, dict(kernel="serial", occupancy=2), {}, SERIAL, ("k_render_exact<2>",)),
    "serial_occ4": Case("readme32x32", S22, dict(kernel="serial", occupancy=4), {}, SERIAL, ("k_render_exact<4>",)),
    "serial_occ8": Case("readme32x32", S22, dict(kernel="serial", occupancy=8), {}, SERIAL, ("k_render_exact<8>",)),
    # ---- outside a frame: the LBVH build of pbrt_gpu_create (2178 triangles: a 4096-key sort, so
    # the global bitonic passes run)
    "mesh_build": Case("mesh33", S22, {}, {}, CI, (),
                       outside=("k_centroids", "k_morton", "k_bitonic_global", "k_gather", "k_karras", "k_up",
                                "k_flatten")),
}

# Ray queries, outside a frame (tests/test_gpu_kernel_coverage.py test_query_kernels): scene -> kernels.
# query_hit's kMeshOnly is n_prims == 0, as the render path chooses. k_query_hit_staged is the diagnostic
# entry of include/pbrt_diag.h (Renderer.intersect_device(staged=True)): LDS-staged trees without a mesh.
QUERY_CASES = {
    "query_analytic": ("readme32x32", ("k_query_camera", "k_query_hit<false, false>", "k_query_hit<true, false>",
                                       "k_intersect", "k_query_hit_staged<false>", "k_query_hit_staged<true>")),
    "query_mesh": ("mesh48x32", ("k_query_hit<false, true>", "k_query_hit<true, true>")),
}

# Kernels no context's log can see: kernel -> (existing test that launches it, why the log cannot).
EXEMPT = {
    "k_probe": ("tests/test_gpu_parity.py::test_device_trig_matches_oracle",
                "pbrt_gpu_probe takes a device ordinal and launches on the null stream: there is no context"),
    "k_merge_film_group": ("tests/test_gpu_group.py (every group render)",
                           "the group launches it on its own stream after its members' frames: it belongs to "
                           "no member context (RendererGroup.member_launches shows the members' frames)"),
}
# nothing reachable from render_enqueue may be exempt
NEVER_EXEMPT_PREFIXES = ("k_chain_", "k_paths_", "k_pw_", "k_dl_", "k_film")
NEVER_EXEMPT_NAMES = {"k_mb_setup", "k_cam_setup", "k_wf_primary", "k_tile_cost", "k_order_of_keys", "k_gate", "k_film",
                      "k_merge_film", "k_panic_reduce", "k_render_exact"}


def may_be_exempt(kernel):
    base = kernel.split("<")[0]
    return not base.startswith(NEVER_EXEMPT_PREFIXES) and base not in NEVER_EXEMPT_NAMES


def coverage():
    """{kernel: case} over CASES and QUERY_CASES; a kernel belongs to one case."""
    out = {}
    for name, c in CASES.items():
        for k in tuple(c.covers) + tuple(c.outside):
            assert k not in out, f"{k} is assigned to {out[k]} and {name}"
            out[k] = name
        for k in c.learned:   # the learned frame's kernels count where no other case owns them
            out.setdefault(k, name)
    for name, (_, kernels) in QUERY_CASES.items():
        for k in kernels:
            assert k not in out, f"{k} is assigned to {out[k]} and {name}"
            out[k] = name
    return out


COVERAGE = coverage()


def pixels(case):
    """Image size and samples per pixel of a case (for the size limits of the table)."""
    d = SCENES[case.scene]().desc
    return int(d.film.res_x), int(d.film.res_y), case.rd.get("spp_x", 8) * case.rd.get("spp_y", 8)


def make_rd(case):
    return abi.render_desc(**case.rd)


"""Rows of the coverage table (tests/kernel_cases.py) for the kernels of trees beyond
64 BVH nodes: the kX stack chains and the camera-start route's stack kernels.

The rows live here and are added to kernel_cases.SCENES / CASES / COVERAGE when this
module is imported: new entries only, no existing entry is read or replaced. pytest
imports every test module of the directory, in name order, before it runs a test,
and this module sorts before tests/test_gpu_kernel_coverage.py (which parametrises
over CASES at import) and tests/test_kernel_manifest.py (which reads COVERAGE when
its tests run). So a run over tests/ sees the rows in both; a run of one of those
two files alone does not, and test_kernel_manifest.py then names the ten kernels
as uncovered. test_this_module_is_imported_first pins the order.

Each case is within the table's own size test (test_kernel_manifest.py): at most
64x48 pixels and 3x3 spp, or 6x6 on the one-tile 16x16 image for a P = 4 path kernel.
"""
import os

import kernel_cases as K
import kernel_manifest as M
from kernel_cases import CAM, CI, NOSAMP, S22, TP, Case, ci, waves
from large_scenes import crowd

SCENES = {
    "crowd48x32": lambda: crowd(),                                     # four materials, 121 BVH nodes
    "crowd_matte48x32": lambda: crowd(kinds=("matte",)),               # Matte, 121 nodes
    "crowd_matte16x16": lambda: crowd(kinds=("matte",), w=16, h=16),   # one tile
}
WAVE_CAM = dict(kernel="wave_cam")
CASES = {
    # non_matte and n_nodes > kLdsNodes: the kX chain with the [64] stack (chain_launch: kx, depth 64)
    "kx_stack_w1": Case("crowd48x32", S22, {}, waves(1), CI, (ci(1, 64, kx=True, multi=True),)),
    "kx_stack_w2": Case("crowd48x32", S22, {}, waves(2), CI, (ci(2, 64, kx=True),)),
    "kx_stack_w4": Case("crowd48x32", S22, {}, waves(4), CI, (ci(4, 64, kx=True),)),
    # the camera-start route, n_nodes > kLdsNodes (enqueue_cam: n_nodes > kLdsNodes); pixels per k_paths_cam_stack
    # wave by spp - 1 (< 8: 64, < 32: 16, else 4)
    "cam_stack_p64": Case("crowd_matte48x32", dict(S22, **NOSAMP), WAVE_CAM, {}, CAM,
                          ("k_chain_cam_stack", "k_paths_cam_stack<64, false>")),
    "cam_stack_p16": Case("crowd_matte48x32", dict(spp_x=3, spp_y=3, **NOSAMP), WAVE_CAM, {}, CAM,
                          ("k_paths_cam_stack<16, false>",)),
    "cam_stack_p4": Case("crowd_matte16x16", dict(spp_x=6, spp_y=6, **NOSAMP), WAVE_CAM, {}, CAM,
                         ("k_paths_cam_stack<4, false>",)),
    "cam_stack_tp_p64": Case("crowd_matte48x32", dict(S22, **NOSAMP, **TP), WAVE_CAM, {}, CAM,
                             ("k_paths_cam_stack<64, true>",)),
    "cam_stack_tp_p16": Case("crowd_matte48x32", dict(spp_x=3, spp_y=3, **NOSAMP, **TP), WAVE_CAM, {}, CAM,
                             ("k_paths_cam_stack<16, true>",)),
    "cam_stack_tp_p4": Case("crowd_matte16x16", dict(spp_x=6, spp_y=6, **NOSAMP, **TP), WAVE_CAM, {}, CAM,
                            ("k_paths_cam_stack<4, true>",)),
}
KERNELS = {k for c in CASES.values() for k in c.covers}

assert not set(SCENES) & set(K.SCENES) and not set(CASES) & set(K.CASES) and not KERNELS & set(K.COVERAGE)
K.SCENES.update(SCENES)
K.CASES.update(CASES)
K.COVERAGE.update({k: name for name, c in CASES.items() for k in c.covers})


def test_this_module_is_imported_first():
    """pytest collects a directory's modules in name order: the rows are in the table before
    test_gpu_kernel_coverage.py parametrises over it."""
    here = os.path.basename(__file__)
    mods = sorted(f for f in os.listdir(os.path.dirname(os.path.abspath(__file__)))
                  if f.startswith("test_") and f.endswith(".py"))
    assert mods.index(here) < mods.index("test_gpu_kernel_coverage.py") < mods.index("test_kernel_manifest.py")


def test_the_rows_are_in_the_table_and_cover_the_new_kernels():
    assert set(CASES) <= set(K.CASES) and set(SCENES) <= set(K.SCENES)
    assert K.coverage() == K.COVERAGE   # the table's own inversion agrees: one case per kernel
    stack = {k for k in M.manifest() if k.startswith(("k_chain_cam_stack", "k_paths_cam_stack"))
             or (k.startswith("k_chain_ci<") and ", 64, true, " in k)}
    assert stack == KERNELS and len(KERNELS) == 10


def test_the_scenes_are_beyond_the_lds_staged_trees():
    for name, make in SCENES.items():
        assert make().desc.n_nodes > 64, name

"""Rows of the coverage table (tests/kernel_cases.py) for the kernels of
pbrt_gpu_path_begin_device and pbrt_gpu_path_step_device: k_path_begin and the four k_path_step.

They are query kernels, launched outside a frame, so they go to QUERY_CASES and
COVERAGE: new entries only, no existing entry is read or replaced (the way
tests/test_li_direct_coverage_rows.py adds k_li_direct's rows). pytest imports every test
module of the directory, in name order, before it runs a test. This module sorts after
tests/test_gpu_kernel_coverage.py, which has by then parametrised its test_query_kernels over
the intersect queries' rows, and every module is imported before
tests/test_kernel_manifest.py's tests read COVERAGE. The test that launches each kernel under a
bit-exact check and finds its name in the launch log is
tests/test_gpu_path_step.py::test_dense_steps_are_li_device (k_path_begin:
test_launch_log_and_no_allocation_on_the_second_batch), whose cases are named here.
"""
import os

import kernel_cases as K
import kernel_manifest as M
import test_gpu_path_step as P
from large_scenes import MATTE, crowd

SCENES = {
    "ps_crowd_matte48x32": lambda: crowd(kinds=MATTE),   # Matte, 121 BVH nodes
    "ps_crowd48x32": lambda: crowd(),                    # four materials, 121 nodes
}
# row -> (scene of the table, kernels, the case of tests/test_gpu_path_step.py that launches them)
ROWS = {
    "path_step_matte": ("readme32x32", ("k_path_step<false, 0>", "k_path_begin"), "readme40x24"),
    "path_step_kx": ("glass48x32", ("k_path_step<true, 0>",), "glass"),
    "path_step_matte_stack": ("ps_crowd_matte48x32", ("k_path_step<false, 64>",), "crowd_matte"),
    "path_step_kx_stack": ("ps_crowd48x32", ("k_path_step<true, 64>",), "crowd_kx"),
}
KERNELS = {k for _, ks, _ in ROWS.values() for k in ks}

assert not set(SCENES) & set(K.SCENES) and not set(ROWS) & set(K.QUERY_CASES) and not KERNELS & set(K.COVERAGE)
K.SCENES.update(SCENES)
K.QUERY_CASES.update({name: (scene, ks) for name, (scene, ks, _) in ROWS.items()})
K.COVERAGE.update({k: name for name, (_, ks, _) in ROWS.items() for k in ks})


def test_this_module_is_imported_after_the_query_test_is_parametrised():
    here = os.path.basename(__file__)
    mods = sorted(f for f in os.listdir(os.path.dirname(os.path.abspath(__file__)))
                  if f.startswith("test_") and f.endswith(".py"))
    assert mods.index("test_gpu_kernel_coverage.py") < mods.index(here)


def test_the_rows_cover_the_path_step_kernels_and_name_their_gpu_cases():
    assert K.coverage() == K.COVERAGE   # the table's own inversion agrees: one case per kernel
    unit = {k for k, u in M.manifest().items() if u == "k_path_step.hip"}
    assert unit == KERNELS and len(KERNELS) == 5
    assert {k for k in M.manifest() if k.startswith("k_path_step<")} == KERNELS - {"k_path_begin"}
    assert len({k for k in M.manifest() if k.startswith("k_li<")}) == 4   # the prefixes other tests count
    assert len({k for k in M.manifest() if k.startswith("k_li_direct<")}) == 4
    for name, (scene, ks, case) in ROWS.items():
        assert case in P.CASE_NAMES and P.KERNEL[case] == ks[0], name   # the GPU case asserts this name in its launch log
    assert K.SCENES["ps_crowd48x32"]().desc.n_nodes > 64 and K.SCENES["ps_crowd_matte48x32"]().desc.n_nodes > 64
    assert K.SCENES["readme32x32"]().desc.n_nodes <= 64 and K.SCENES["glass48x32"]().desc.n_nodes <= 64

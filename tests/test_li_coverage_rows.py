"""Rows of the coverage table (tests/kernel_cases.py) for the four k_li kernels of
pbrt_gpu_li_device.

They are query kernels, launched outside a frame, so they go to QUERY_CASES and
COVERAGE: new entries only, no existing entry is read or replaced (the way
tests/test_coverage_rows_large_trees.py adds its rows). pytest imports every test
module of the directory, in name order, before it runs a test. This module sorts
after tests/test_gpu_kernel_coverage.py, which has by then parametrised its
test_query_kernels over the intersect queries' rows (that test runs camera rays and
intersections, not Li), and every module is imported before
tests/test_kernel_manifest.py's tests read COVERAGE. The test that launches each
kernel under a bit-exact check and finds its name in the launch log is
tests/test_gpu_li.py::test_film_of_li_is_the_oracles, whose cases are named here.
"""
import os

import kernel_cases as K
import kernel_manifest as M
import test_gpu_li as T
from large_scenes import MATTE, crowd

SCENES = {
    "li_crowd_matte48x32": lambda: crowd(kinds=MATTE),   # Matte, 121 BVH nodes
    "li_crowd48x32": lambda: crowd(),                    # four materials, 121 nodes
}
# row -> (scene of the table, kernels, the case of tests/test_gpu_li.py that launches them)
ROWS = {
    "li_matte": ("readme32x32", ("k_li<false, 0>",), "readme40x24"),
    "li_kx": ("glass48x32", ("k_li<true, 0>",), "glass"),
    "li_matte_stack": ("li_crowd_matte48x32", ("k_li<false, 64>",), "crowd_matte"),
    "li_kx_stack": ("li_crowd48x32", ("k_li<true, 64>",), "crowd_kx"),
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


def test_the_rows_cover_the_li_kernels_and_name_their_gpu_cases():
    assert K.coverage() == K.COVERAGE   # the table's own inversion agrees: one case per kernel
    assert {k for k in M.manifest() if k.startswith("k_li<")} == KERNELS and len(KERNELS) == 4
    for name, (scene, ks, case) in ROWS.items():
        assert T.CASES[case].kernel == ks[0], name   # the GPU case asserts this name in its launch log
        assert M.manifest()[ks[0]] == "k_li.hip"
    assert K.SCENES["li_crowd48x32"]().desc.n_nodes > 64 and K.SCENES["li_crowd_matte48x32"]().desc.n_nodes > 64
    assert K.SCENES["readme32x32"]().desc.n_nodes <= 64 and K.SCENES["glass48x32"]().desc.n_nodes <= 64

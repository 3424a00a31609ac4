"""Rows of the coverage table (tests/kernel_cases.py) for the four k_li_direct kernels of
pbrt_gpu_direct_li_device.

They are query kernels, launched outside a frame, so they go to QUERY_CASES and
COVERAGE: new entries only, no existing entry is read or replaced (the way
tests/test_li_coverage_rows.py adds k_li's rows). pytest imports every test module of
the directory, in name order, before it runs a test. This module sorts after
tests/test_gpu_kernel_coverage.py, which has by then parametrised its
test_query_kernels over the intersect queries' rows, and every module is imported
before tests/test_kernel_manifest.py's tests read COVERAGE. The test that launches each
kernel under a bit-exact check and finds its name in the launch log is
tests/test_gpu_direct_li.py::test_film_of_direct_li_is_the_oracles, whose cases are
named here.
"""
import os

import kernel_cases as K
import kernel_manifest as M
import test_gpu_direct_li as T
from large_scenes import MATTE, crowd

SCENES = {
    "dli_crowd_matte48x32": lambda: crowd(kinds=MATTE),   # Matte, 121 BVH nodes
    "dli_crowd48x32": lambda: crowd(),                    # four materials, 121 nodes
}
# row -> (scene of the table, kernels, the case of tests/test_gpu_direct_li.py that launches them)
ROWS = {
    "direct_li_matte": ("readme32x32", ("k_li_direct<false, 0>",), "readme40x24"),
    "direct_li_kx": ("glass48x32", ("k_li_direct<true, 0>",), "glass"),
    "direct_li_matte_stack": ("dli_crowd_matte48x32", ("k_li_direct<false, 64>",), "crowd_matte"),
    "direct_li_kx_stack": ("dli_crowd48x32", ("k_li_direct<true, 64>",), "crowd_kx"),
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


def test_the_rows_cover_the_direct_li_kernels_and_name_their_gpu_cases():
    assert K.coverage() == K.COVERAGE   # the table's own inversion agrees: one case per kernel
    assert {k for k in M.manifest() if k.startswith("k_li_direct<")} == KERNELS and len(KERNELS) == 4
    assert len({k for k in M.manifest() if k.startswith("k_li<")}) == 4
    for name, (scene, ks, case) in ROWS.items():
        assert T.CASES[case].kernel == ks[0], name   # the GPU case asserts this name in its launch log
        assert (case, 5, T.ALL) in T.ORACLE_RUNS and (case, 5, T.ONE) in T.ORACLE_RUNS
        assert M.manifest()[ks[0]] == "k_li_direct.hip"
    assert K.SCENES["dli_crowd48x32"]().desc.n_nodes > 64 and K.SCENES["dli_crowd_matte48x32"]().desc.n_nodes > 64
    assert K.SCENES["readme32x32"]().desc.n_nodes <= 64 and K.SCENES["glass48x32"]().desc.n_nodes <= 64

"""Rows of the coverage table (tests/kernel_cases.py) for the five kernels of
go-pbrt_amd/csrc/k_strat.hip: k_strat_pixels and k_li_strat<false / true, 0 / 64>.

They are launched outside a frame, so they go to QUERY_CASES and COVERAGE the way
tests/test_open_frame_coverage_rows.py adds the k_film_q rows: new entries only,
from a module that sorts after tests/test_gpu_kernel_coverage.py (whose
test_query_kernels is parametrised over the intersect queries by then; it does
not run these calls). The tests that launch each kernel under a bit-exact check
and find its name in the launch log are tests/test_gpu_strat.py's, named here.
"""
import os
import re

import kernel_cases as K
import kernel_manifest as M

# row -> (scene of the table, kernels, the test of tests/test_gpu_strat.py that launches them,
#         how that test names the kernel: a literal, or the case table's entry it asserts)
ROWS = {
    "strat_pixels": ("readme45x30", ("k_strat_pixels",), "test_tables_and_samples_are_the_references"),
    "li_strat_matte": ("readme45x30", ("k_li_strat<false, 0>",), "test_composed_frame_is_the_oracles_and_the_librarys"),
    "li_strat_kx": ("glass48x32", ("k_li_strat<true, 0>",), "test_composed_frame_is_the_oracles_and_the_librarys"),
    "li_strat_stack": ("spheres90", ("k_li_strat<false, 64>", "k_li_strat<true, 64>"),
                       "test_composed_frame_is_the_oracles_and_the_librarys"),
}
KERNELS = {k for _, ks, _ in ROWS.values() for k in ks}

assert not set(ROWS) & set(K.QUERY_CASES) and not KERNELS & set(K.COVERAGE)
K.QUERY_CASES.update({name: (scene, ks) for name, (scene, ks, _) in ROWS.items()})
K.COVERAGE.update({k: name for name, (_, ks, _) in ROWS.items() for k in ks})


def test_this_module_is_imported_after_the_query_test_is_parametrised():
    here = os.path.basename(__file__)
    mods = sorted(f for f in os.listdir(os.path.dirname(os.path.abspath(__file__)))
                  if f.startswith("test_") and f.endswith(".py"))
    assert mods.index("test_gpu_kernel_coverage.py") < mods.index(here)


def test_the_rows_cover_the_unit_and_name_their_gpu_tests():
    assert K.coverage() == K.COVERAGE   # the table's own inversion agrees: one case per kernel
    assert {k for k, u in M.manifest().items() if u == "k_strat.hip"} == KERNELS and len(KERNELS) == 5
    src = open(os.path.join(M.REPO, "tests", "test_gpu_strat.py")).read()
    for name, (scene, ks, test) in ROWS.items():
        assert scene in K.SCENES and f"def {test}(" in src, name
        for k in ks:
            assert f'"{k}"' in src, k   # the GPU test asserts this name in its launch log
    # every case of the composed-frame test names the instantiation it must find in the log
    body = src[src.index("COMPOSED = {"):src.index("LI_KEYS =")]
    assert set(re.findall(r'"(k_li_strat<\w+, \d+>)"', body)) == KERNELS - {"k_strat_pixels"}
    assert "names_since(r, before) == [case.kernel]" in src

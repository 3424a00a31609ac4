"""Rows of the coverage table (tests/kernel_cases.py) for the five kernels of
go-pbrt_amd/csrc/k_film_q.hip: k_frame_samples, k_film_add_tiles<false / true>,
k_film_add_merge and k_film_rgba8.

They are launched outside a frame, so they go to QUERY_CASES and COVERAGE the
way tests/test_li_coverage_rows.py adds the k_li rows: new entries only, from a
module that sorts after tests/test_gpu_kernel_coverage.py (whose
test_query_kernels is parametrised over the intersect queries by then; it does
not run these calls). The tests that launch each kernel under a bit-exact
check and find its name in the launch log are tests/test_gpu_open_frame.py's,
named here.
"""
import os

import kernel_cases as K
import kernel_manifest as M

# row -> (scene of the table, kernels, the test of tests/test_gpu_open_frame.py that launches them)
ROWS = {
    "frame_samples": ("readme45x30", ("k_frame_samples",), "test_samples_are_the_references"),
    "film_add_lds": ("readme45x30", ("k_film_add_tiles<true>", "k_film_add_merge"), "test_film_add_is_the_numpy_film"),
    "film_add_direct": ("readme45x30", ("k_film_add_tiles<false>",), "test_film_add_is_the_numpy_film"),
    "film_rgba8": ("readme32x32", ("k_film_rgba8",), "test_rgba8_is_the_hosts"),
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
    assert {k for k, u in M.manifest().items() if u == "k_film_q.hip"} == KERNELS and len(KERNELS) == 5
    src = open(os.path.join(M.REPO, "tests", "test_gpu_open_frame.py")).read()
    for name, (scene, ks, test) in ROWS.items():
        assert scene in K.SCENES and f"def {test}(" in src, name
        for k in ks:
            assert f'"{k}"' in src, k   # the GPU test asserts this name in its launch log

"""The manifest of compiled kernels against the launch log's names and the coverage table.

No GPU: the manifest is read from the sources (tests/kernel_manifest.py), the
log's names from the library's static pointer-to-name table
(pbrt_gpu_kernel_names), the table from tests/kernel_cases.py. An explicit
instantiation added to a unit without a name entry, or without a covering
case, fails here.
"""
import os
import re

import pytest

import kernel_cases as K
import kernel_manifest as M
import pbrtgpu as G

MANIFEST = M.manifest()


def test_manifest_reads_every_family():
    """The parser finds the families render_kernels.h declares (a regex that silently matched
    nothing would make every equality below vacuous)."""
    fam = {}
    for k in MANIFEST:
        fam.setdefault(k.split("<")[0], []).append(k)
    decl = open(os.path.join(M.AMD, "csrc", "render_kernels.h")).read()
    declared = set(re.findall(r"__global__\s+void\s+(\w+)\s*\(", decl))
    assert declared and declared <= set(fam), sorted(declared - set(fam))
    assert set(fam["k_render_exact"]) == {f"k_render_exact<{n}>" for n in (1, 2, 4, 8)}   # the serial launch's four
    assert len(fam["k_chain_ci"]) > 20
    for k in fam["k_chain_ci"]:   # every argument spelled
        assert re.fullmatch(r"k_chain_ci<(1|2|4|8), (-1|0|64), (true|false), (0|2), (true|false), (true|false)>", k), k
    assert MANIFEST["k_probe"] == "diag.hip" and MANIFEST["k_flatten"] == "mesh_bvh.hip"


def test_parser_on_a_synthetic_unit(tmp_path):
    """Comments, template definitions, declarations and inactive preprocessor branches are not kernels."""
    src = tmp_path / "unit.hip"
    src.write_text("""
        // template __global__ void k_commented<1>(int a);
        template <int N, bool B>
        __global__ __launch_bounds__(64) void k_tmpl(int a) { }
        __global__ void k_declared(int a);
        __global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(2, 8))) void k_plain(int a,
                                                                                                    void (*f)(int)) {
        }
        #if PBRT_MESH_WIDE
        __global__ void k_off(int a) { }
        #else
        __global__ void k_on(int a) { }
        #endif
        #ifdef SOME_DIAG
        template __global__ void k_tmpl<9, true>(int a);
        #endif
        template __global__ void k_tmpl<1,false>(int a);
        template __global__ void k_tmpl< 2 , true >(int a);
    """)
    inst, plain = M.unit_kernels(str(src))
    assert inst == ["k_tmpl<1, false>", "k_tmpl<2, true>"] and plain == ["k_plain", "k_on"]
    src.write_text("#if PBRT_UNKNOWN_SWITCH\n__global__ void k(int a) { }\n#endif\n")
    with pytest.raises(ValueError):
        M.unit_kernels(str(src))


def test_log_names_are_the_manifest():
    """The names pbrt_gpu_launch_log can produce are exactly the compiled kernels."""
    names = G.kernel_names()
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)
    assert set(names) == set(MANIFEST), (sorted(set(MANIFEST) - set(names)), sorted(set(names) - set(MANIFEST)))


def test_table_plus_exemptions_is_the_manifest():
    covered, exempt = set(K.COVERAGE), set(K.EXEMPT)
    assert not covered & exempt, sorted(covered & exempt)
    missing, unknown = set(MANIFEST) - covered - exempt, (covered | exempt) - set(MANIFEST)
    assert not missing, f"compiled kernels with no covering case in tests/kernel_cases.py: {sorted(missing)}"
    assert not unknown, f"the table names kernels the library does not compile: {sorted(unknown)}"


def test_exemptions_name_a_test_and_nothing_of_a_frame():
    for k, (test, why) in K.EXEMPT.items():
        assert K.may_be_exempt(k), f"{k} is reachable from render_enqueue"
        path = test.split("::")[0].split(" ")[0]
        assert os.path.exists(os.path.join(M.REPO, path)), test
        if "::" in test:
            assert f"def {test.split('::')[1]}(" in open(os.path.join(M.REPO, path)).read(), test
        assert why
    assert not K.may_be_exempt("k_merge_film") and not K.may_be_exempt("k_film_cam<true>")
    assert not K.may_be_exempt("k_chain_ci<1, 0, false, 0, false, false>") and K.may_be_exempt("k_merge_film_group")


def test_cases_are_small_and_their_knobs_exist():
    """At most 64x48 pixels and 3x3 spp (on the one-tile 16x16 image: the windowed StartPixel's
    11x11 without jitter, and the 6x6 that k_paths_cam<4> needs, which runs from 33 spp);
    every knob a case sets is one Knobs::from_env reads, every option one the Renderer takes."""
    host = open(os.path.join(M.AMD, "csrc", "knobs.h")).read()
    knobs = set(re.findall(r'getenv\("(PBRT_\w+)"\)', host)) | set(re.findall(r'ival\("(PBRT_\w+)"', host))
    assert len(knobs) >= 27
    for name, c in K.CASES.items():
        w, h, spp = K.pixels(c)
        assert w <= 64 and h <= 48, name
        assert spp <= 9 or (spp == 121 and (w, h) == (16, 16) and c.rd.get("jitter") is False) or \
            (spp == 36 and (w, h) == (16, 16)), (name, spp)
        assert set(c.env) <= knobs, (name, sorted(set(c.env) - knobs))
        assert set(c.opts) <= {"lanes_per_wave", "occupancy", "kernel"}, name
        assert c.scene in K.SCENES
    for name, (scene, _) in K.QUERY_CASES.items():
        assert scene in K.SCENES, name


def test_every_launch_goes_through_the_log():
    """No unit launches a kernel past launch_logged(), but the group's merge (no member context)."""
    raw = {}
    for path in M.makefile_units():
        text = M.strip_comments(open(path).read())
        n = len(re.findall(r"hipLaunchKernelGGL\s*\(|<<<|hipLaunchKernel\s*\(|hipModuleLaunchKernel", text))
        if n:
            raw[os.path.basename(path)] = n
    assert raw == {"group.hip": 1}, raw
    assert "k_merge_film_group" in K.EXEMPT

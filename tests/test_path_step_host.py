"""The host side of pbrt_gpu_path_begin_device / pbrt_gpu_path_step_device without a GPU.

- go-pbrt_amd/csrc/path_query.h (the argument checks, the queue rules, the grids) as a
  stand-alone program under ASan + UBSan: tests/path_query_check.cpp.
- The selector of the four k_path_step kernels by its launch-log names, and that the new
  names keep clear of the k_li< and k_li_direct< prefixes other tests count.
"""
import os
import re
import subprocess

import pbrtgpu as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ("ox", "oy", "oz", "dx", "dy", "dz", "lr", "lg", "lb", "br", "bg", "bb", "eta_scale", "state", "inc", "draws",
         "rays", "bounces", "status")


def test_path_query_header_under_sanitizers(tmp_path):
    exe = tmp_path / "pqc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(REPO, "tests", "path_query_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"checks=(\d+) bad=(\d+)", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) > 250
    cases = {ln.split()[1]: int(ln.split()[2]) for ln in r.stdout.splitlines() if ln.startswith("case ")}
    invalid = {"begin_null_ctx", "begin_null_rays", "begin_null_rng", "begin_null_paths", "begin_n_2_31",
               "begin_in_flight", "begin_in_flight_n0", "begin_null_rng_state", "begin_null_rng_inc",
               "step_null_ctx", "step_null_desc", "step_null_paths", "step_n_2_31", "step_in_flight",
               "step_in_flight_n0", "step_depth_0", "step_depth_negative", "step_reserved",
               "step_in_null_index", "step_in_null_count", "step_out_null_index", "step_out_null_count",
               "step_alias_same_struct", "step_alias_copy", "step_alias_index", "step_alias_count"}
    invalid |= {f"begin_null_ray_{k}" for k in G.RAY_KEYS}
    invalid |= {f"{call}_null_state_{k}" for call in ("begin", "step") for k in STATE}   # every pointer but tmax
    assert {k for k, v in cases.items() if v == G.abi.PBRT_E_INVALID} == invalid
    assert {k for k, v in cases.items() if v == G.abi.PBRT_E_UNSUPPORTED} == {"rough_glass", "direct_lighting",
                                                                             "depth_2049", "strategy_3"}
    assert {k for k, v in cases.items() if v == 0} == {"begin_valid", "begin_valid_n0", "begin_valid_nmax",
                                                       "begin_with_tmax", "step_valid", "step_valid_n0",
                                                       "step_valid_nmax", "step_valid_in", "step_valid_out",
                                                       "step_valid_in_out", "supported", "depth_2048"}
    assert set(STATE) | {"tmax"} == set(G.PATH_DTYPES)
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("kernel ")]
    assert len(rows) == 2 * 2 * 7


def test_selector_has_the_four_kernels_the_table_can_ask_for():
    """path_step_kernel (kernel_select.hip) by its launch-log names; null for what is not compiled."""
    want = set()
    for kx in (0, 1):
        for depth in (0, 64):
            name = f"k_path_step<{'true' if kx else 'false'}, {depth}>"
            assert G.kernel_choice("k_path_step", kx, depth) == name
            want.add(name)
    assert G.kernel_choice("k_path_step", 0, 32) is None and G.kernel_choice("k_path_step", 1, -1) is None
    names = G.kernel_names()
    assert {n for n in names if n.startswith("k_path_step<")} == want and "k_path_begin" in names
    assert len({n for n in names if n.startswith("k_li<")}) == 4   # the new names keep clear of the prefixes
    assert len({n for n in names if n.startswith("k_li_direct<")}) == 4   # that other tests count


def test_bytes_per_path_are_the_headers():
    assert G.PATH_BYTES == 141
    hdr = open(os.path.join(REPO, "include", "pbrt_gpu.h")).read()
    assert "141 bytes a path, 133 without tmax" in hdr
    q = open(os.path.join(REPO, "go-pbrt_amd", "csrc", "path_query.h")).read()
    assert "kBytesPerPath = 141" in q

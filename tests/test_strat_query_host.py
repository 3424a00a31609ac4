"""The host side of pbrt_gpu_frame_samples_stratified_device and
pbrt_gpu_li_stratified_device without a GPU: go-pbrt_amd/csrc/strat_query.h as a
stand-alone program under ASan + UBSan (tests/strat_query_check.cpp). The program
checks every refusal with its text, the pixel and table counts against a literal
enumeration, the cursors and draws after the camera sample and the StartPixel
form of the shapes the GPU tests run; this module holds its case list complete
and its counts equal to tests/strat_reference.py's frame().
"""
import os
import re
import subprocess
from collections import namedtuple

import pytest

import strat_reference as S
from pbrtgpu import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Film = namedtuple("Film", "res_x res_y crop_min_x crop_min_y crop_max_x crop_max_y")


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sqc") / "sqc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(REPO, "tests", "strat_query_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_strat_query_header_under_sanitizers(output):
    m = re.search(r"checks=(\d+) bad=(\d+)", output)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) > 400
    cases = {ln.split()[1]: int(ln.split()[2]) for ln in output.splitlines() if ln.startswith("case ")}
    invalid = {k for k, v in cases.items() if v == abi.PBRT_E_INVALID}
    unsupported = {k for k, v in cases.items() if v == abi.PBRT_E_UNSUPPORTED}
    assert invalid == {
        "samples_null_ctx", "samples_null_desc", "samples_null_sampler", "samples_null_out", "samples_null_strat",
        "samples_in_flight", "samples_tile_size_0", "samples_ns_0", "samples_clear_flag", "samples_frame_reserved",
        "samples_end_past_the_film", "samples_begin_negative", "samples_sampler_x_0", "samples_sampler_y_negative",
        "samples_sampler_reserved", "samples_ns_is_spp", "samples_ns_short", "samples_spp_2_32", "samples_null_ray_array",
        "samples_null_pfilm", "samples_null_state", "samples_null_k", "samples_null_table", "samples_null_s1d",
        "samples_order_in_flight_first", "samples_order_sampler_before_pointers", "samples_order_frame_first",
        "li_null_ctx", "li_in_flight", "li_null_strat", "li_n_2_31", "li_desc_reserved", "li_depth_0", "li_null_ray_array",
        "li_null_radiance", "li_strat_reserved", "li_n_dims_negative", "li_first_1d_beyond", "li_first_1d_negative",
        "li_first_2d_beyond", "li_first_2d_negative", "li_null_s1d", "li_null_table", "li_null_k", "li_spp_0",
        "li_n_tables_0", "li_n_dims_0_cursor_1", "li_order_in_flight_before_strat", "li_order_desc_first"}
    assert unsupported == {"samples_n_dims_0", "samples_n_dims_negative", "samples_tile_257", "samples_spp_4097",
                           "samples_lds_beyond_48k", "samples_n_dims_times_spp", "li_direct_lighting", "li_rough_glass"}
    assert {k for k, v in cases.items() if v == 0} == {
        "samples_valid", "samples_valid_empty", "samples_valid_jitter", "samples_spp_4096", "li_valid", "li_valid_n0",
        "li_valid_cursors_at_n_dims", "li_valid_cursors_at_0", "li_valid_n_dims_0"}


def test_counts_cursors_and_forms(output):
    counts = dict(re.findall(r"count (\d+x\d+ tile \d+) -> (\d+) pixels", output))
    assert counts == {"45x30 tile 16": "1350", "17x5 tile 4": "85", "16x16 tile 16": "256"}
    for (w, h, ts) in ((45, 30, 16), (17, 5, 4), (16, 16, 16)):   # the reference's frame has as many tables
        fr = S.frame(Film(w, h, 0, 0, w, h), 1, 2, 1, False, tile_size=ts)
        assert str(fr.tables.shape[0]) == counts[f"{w}x{h} tile {ts}"] and len(fr.k) == fr.tables.shape[0]
    cursors = {int(a): (int(b), int(c), int(d)) for a, b, c, d in re.findall(r"cursor (\d) -> (\d) (\d) draws (\d)", output)}
    assert cursors == {0: (0, 0, 5), 1: (1, 1, 2), 2: (1, 2, 0), 3: (1, 2, 0), 4: (1, 2, 0), 5: (1, 2, 0)}
    for nd, (c1, c2, draws) in cursors.items():
        assert (c1, c2) == abi.camera_cursors(nd) and draws == S.camera_draws(nd)
    forms = dict(re.findall(r"plan (\w+) form (\d)", output))
    assert forms == {"s2x2_nd4": "0", "s3x3_nd1_jitter": "0", "s1x2_nd2": "0", "s8x8_nd4": "0", "s11x11_nd4_windowed": "2",
                     "s11x11_nd4_kx_serial": "1", "s6x6_nd4_jitter_buffered": "0", "s7x7_nd4_jitter_serial": "1"}
    kernels = re.findall(r"kernel (\d) (\d+) -> (\d) (\d+) (\d+)", output)
    assert len(kernels) == 8 and all((kx == nm and int(depth) == (64 if int(nodes) > 64 else 0))
                                     for nm, nodes, kx, depth, _ in kernels)

"""The host side of pbrt_gpu_frame_samples_device, pbrt_gpu_film_add_device and
pbrt_gpu_film_rgba8_device without a GPU.

- go-pbrt_amd/csrc/film_query.h (the frame layout, the argument checks and the
  refusals) as a stand-alone program under ASan + UBSan: tests/film_query_check.cpp.
  It checks the layout against a literal enumeration of its own and lists every
  PBRT_E_INVALID and PBRT_E_UNSUPPORTED case of the three calls.
- The same program prints the layout of a film; it must be the order of
  tests/li_reference.py's samples(), which the GPU tests compare the device's
  samples with: offsets of tiles, counts of ranges, the tile, pixel index and
  raster position of every element.
- The ctypes structs against the header, the new knob, the coverage rows.
"""
import ctypes as C
import os
import re
import subprocess
from collections import namedtuple

import numpy as np
import pytest

import li_reference as R
import pbrtgpu as G
from pbrtgpu import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Film = namedtuple("Film", "res_x res_y crop_min_x crop_min_y crop_max_x crop_max_y")


def cropped(w, h, crop):
    """Film.CroppedPixelBounds (film.go:55-60) of a crop window."""
    return Film(w, h, int(np.ceil(w * crop[0])), int(np.ceil(h * crop[1])), int(np.ceil(w * crop[2])),
                int(np.ceil(h * crop[3])))


FILMS = {
    "40x24": (Film(40, 24, 0, 0, 40, 24), 16),
    "45x30_tile13": (Film(45, 30, 0, 0, 45, 30), 13),
    "80x48": (Film(80, 48, 0, 0, 80, 48), 16),
    "crop64x40_tile8": (cropped(64, 40, (0.25, 0.1, 0.8, 0.9)), 8),
    "crop64x40_tile16": (cropped(64, 40, (0.25, 0.1, 0.8, 0.9)), 16),
}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fqc") / "fqc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(REPO, "tests", "film_query_check.cpp")], check=True)
    return str(exe)


def test_film_query_header_under_sanitizers(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"checks=(\d+) bad=(\d+)", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) > 100000
    cases = {ln.split()[1]: int(ln.split()[2]) for ln in r.stdout.splitlines() if ln.startswith("case ")}
    null_fields = {f"pbrt_frame_samples_soa_null_{k}" for k in G.SAMPLE_REQUIRED} | \
        {f"pbrt_film_samples_soa_null_{k}" for k in G.FILM_KEYS}
    invalid = {"null_ctx", "null_desc", "tile_size_0", "tile_size_negative", "ns_0", "ns_negative",
               "samples_clear_flag", "unknown_flag", "reserved", "begin_negative", "end_before_begin",
               "end_past_the_film", "more_than_2_31", "in_flight", "in_flight_empty", "ns_2_20_in_flight",
               "samples_null_out", "film_null_samples", "film_null_film", "rgba8_null_ctx", "rgba8_null_film",
               "rgba8_null_rgba", "rgba8_misaligned_rgba", "rgba8_misaligned_film", "rgba8_w_0", "rgba8_h_negative",
               "rgba8_2_31_pixels", "rgba8_huge", "rgba8_in_flight"} | null_fields
    unsupported = {"tile_size_257", "ns_2_20", "radius_is_the_tile", "radius_0", "radius_negative", "radius_nan",
                   "radius_beyond_a_tile_of_8"}
    assert {k for k, v in cases.items() if v == abi.PBRT_E_INVALID} == invalid
    assert {k for k, v in cases.items() if v == abi.PBRT_E_UNSUPPORTED} == unsupported
    assert {k for k, v in cases.items() if v == 0} == {
        "valid", "valid_single_tile", "valid_empty", "valid_empty_at_end", "valid_clear", "valid_largest",
        "valid_one_row_of_1080p", "samples_ignore_the_filter", "radius_below_the_tile", "samples_valid",
        "samples_valid_without_optional", "film_valid", "rgba8_valid", "rgba8_valid_largest"}


@pytest.mark.parametrize("name", sorted(FILMS))
def test_layout_is_the_reference_order(checker, name):
    """Offsets, counts and the inverse map against li_reference.samples(): one sample per pixel
    (spp 2), so element g of the layout is the g-th sample of the reference's order."""
    film, ts = FILMS[name]
    out = subprocess.run([checker, "layout"] + [str(v) for v in film] + [str(ts)], capture_output=True, text=True,
                         check=True).stdout.splitlines()
    assert out[0] == f"tiles {R.num_tiles(film, ts)}"
    before = np.array([[int(v) for v in ln.split()[1:]] for ln in out if ln.startswith("tile ")])
    px = np.array([[int(v) for v in ln.split()[1:]] for ln in out if ln.startswith("px ")])
    s = R.samples(film, 2, tile_size=ts)
    n = len(s.k)
    assert n == (film.crop_max_x - film.crop_min_x) * (film.crop_max_y - film.crop_min_y) == px.shape[0]
    assert np.array_equal(px[:, 0], np.arange(n))
    assert np.array_equal(px[:, 1], s.tile) and np.array_equal(px[:, 2], s.pi)
    assert np.array_equal(px[:, 3], s.px) and np.array_equal(px[:, 4], s.py)
    nt = R.num_tiles(film, ts)
    assert np.array_equal(before[:, 0], np.arange(nt + 1))
    # pixels before tile t: the samples of the tiles below it; the last row is the whole film
    want = np.concatenate([[0], np.cumsum(np.bincount(s.tile, minlength=nt))])
    assert np.array_equal(before[:, 1], want)
    # the formula of the header: ty * ts * W + tx * ts * h(ty)
    W, H = film.crop_max_x - film.crop_min_x, film.crop_max_y - film.crop_min_y
    ntx = (W + ts - 1) // ts
    for t in range(nt):
        tx, ty = t % ntx, t // ntx
        assert before[t, 1] == ty * ts * W + tx * ts * min(ts, H - ty * ts)
    # a range's count with ns samples a pixel, empty and single-tile ranges among them
    for b, e in ((0, nt), (0, 0), (nt, nt), (1, 1), (1, 2), (nt - 1, nt), (1, nt - 1)):
        assert (before[e, 1] - before[b, 1]) * 3 == 3 * int(((s.tile >= b) & (s.tile < e)).sum())
    x0, y0, x1, y1 = R.tile_bounds(film, ts, nt - 1)
    assert before[nt, 1] - before[nt - 1, 1] == (x1 - x0) * (y1 - y0)   # the last tile, ragged where the film is


def test_the_cropped_film_is_the_scene_builders():
    """The crop bounds this module restates are the film's the GPU tests render (no device needed)."""
    from test_gpu_wave_cam import lens_scene
    scene = lens_scene(w=64, h=40, lens=0.0, crop=(0.25, 0.1, 0.8, 0.9))
    f = scene.desc.film
    assert Film(f.res_x, f.res_y, f.crop_min_x, f.crop_min_y, f.crop_max_x, f.crop_max_y) == FILMS["crop64x40_tile8"][0]
    w, h = f.crop_max_x - f.crop_min_x, f.crop_max_y - f.crop_min_y
    assert (w, h) == (36, 32) and f.crop_min_x % 8 == 0 and f.crop_min_y % 8   # ragged in x at tiles 8 and 16


def test_structs_and_symbols():
    """The ctypes structs are the header's: sizes by the fields the header lists, and every entry
    point is exported and declared."""
    assert C.sizeof(abi.FrameDesc) == 32 and abi.FrameDesc.tile_begin.offset == 8 and abi.FrameDesc.flags.offset == 24
    assert C.sizeof(abi.FrameSamplesSoA) == 13 * 8 and C.sizeof(abi.FilmSamplesSoA) == 5 * 8
    assert [n for n, _ in abi.FrameSamplesSoA._fields_] == ["ox", "oy", "oz", "dx", "dy", "dz", "tmax", "pfilm_x",
                                                             "pfilm_y", "state", "inc", "px", "py"]
    hdr = open(os.path.join(REPO, "include", "pbrt_gpu.h")).read()
    body = re.search(r"typedef struct pbrt_frame_samples_soa \{(.*?)\}", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\*(\w+)", body) == [n for n, _ in abi.FrameSamplesSoA._fields_]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct pbrt_frame_desc \{(.*?)\}", hdr, re.S).group(1), flags=re.S)
    assert re.findall(r"(\w+)[,;]", body) == [n for n, _ in abi.FrameDesc._fields_]
    L = G.lib()
    for sym in abi.FRAME_SYMBOLS:
        assert hasattr(L, sym), sym
    assert f"PBRT_FILM_ADD_CLEAR = {abi.PBRT_FILM_ADD_CLEAR}" in hdr
    assert G.FRAME_BYTES_PER_SAMPLE == 104
    # NULL arguments are refused before anything touches a device
    assert L.pbrt_gpu_frame_count(None, None) == -abi.PBRT_E_INVALID
    assert L.pbrt_gpu_frame_samples_device(None, None, None) == abi.PBRT_E_INVALID
    assert L.pbrt_gpu_film_add_device(None, None, None, None) == abi.PBRT_E_INVALID
    assert L.pbrt_gpu_film_rgba8_device(None, None, 4, 4, None) == abi.PBRT_E_INVALID
    assert L.pbrt_gpu_film_scratch_bytes(None) == 0


def test_kernels_are_named_and_the_knob_is_read():
    names = set(G.kernel_names())
    assert {"k_frame_samples", "k_film_add_tiles<false>", "k_film_add_tiles<true>", "k_film_add_merge",
            "k_film_rgba8"} <= names
    knobs = open(os.path.join(REPO, "go-pbrt_amd", "csrc", "knobs.h")).read()
    assert 'getenv("PBRT_FILM_ADD")' in knobs

"""The camera-sample mapping of the camera-start wave route (PBRT_KERNEL_WAVE_CAM)
on the host: go-pbrt_amd/csrc/cam_sample.h, the header k_chain_cam, k_paths_cam
and k_film_cam draw their CameraSample with, built as a stand-alone program
under ASan + UBSan and checked against the oracle's PCG32 floats
(GetCameraSample, pkg/sampler/sampler.go:75-80: pFilm, pLens, time):

- n_dims = 0 consumes floats 0..4 as (film x, film y, lens x, lens y, time);
- n_dims = 1 consumes floats 0, 1 as the lens point; pFilm is the stratified
  (0,0) and the time is the pixel's stratified value (not a draw);
- n_dims >= 2 consumes nothing.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import oracle_lib as O
from pbrtgpu import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_camera_sample_header_matches_the_oracle_stream(tmp_path):
    exe = tmp_path / "wcc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-o", str(exe), os.path.join(REPO, "tests", "wave_cam_check.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == 3 * 4
    seen = set()
    for row in rows:
        seed, nd, draws, time_drawn = (int(v) for v in row[:4])
        vals = np.array([int(v, 16) for v in row[4:9]], dtype=np.uint64).view(np.float64)
        nxt = int(row[9])
        fl = (C.c_double * 8)()
        O.lib().oracle_pcg_floats(seed, 8, fl)
        raw = (C.c_uint32 * 8)()
        O.lib().oracle_pcg_stream(seed, 8, raw)
        want = np.zeros(5)
        if nd == 0:
            want[:] = list(fl)[:5]
            assert (draws, time_drawn) == (5, 1)
        elif nd == 1:
            want[2:4] = list(fl)[:2]
            assert (draws, time_drawn) == (2, 0)
        else:
            assert (draws, time_drawn) == (0, 0)
        assert np.array_equal(vals.view(np.uint64), want.view(np.uint64)), (seed, nd)
        assert nxt == raw[draws], (seed, nd)   # the stream stands right after the camera sample
        seen.add((seed, nd))
    assert seen == {(s, d) for s in (0, 1, 7) for d in (0, 1, 2, 3)}


def test_kernel_request_value():
    assert abi.PBRT_KERNEL_WAVE_CAM == 6
    hdr = open(os.path.join(REPO, "include", "pbrt_gpu.h")).read()
    m = re.search(r"PBRT_KERNEL_WAVE_CAM\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == 6
    import pbrtgpu as G
    assert G.Renderer.KERNELS["wave_cam"] == 6

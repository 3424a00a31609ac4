"""Device groups (pbrt_gpu_group, include/pbrt_gpu.h) without a GPU: argument
validation happens before any device call, and the tile mapping shared by the
host split and the merge kernel (go-pbrt_amd/csrc/group_map.h) partitions every
tile subset over 1..8 members with dense slots. CPU only."""
import ctypes as C
import os
import re
import subprocess

import pytest

import pbrtgpu as G
from pbrtgpu import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def create(scene_ref, devices, n):
    h = C.c_void_p(0xdead)   # must be cleared on failure
    opts = abi.GpuOpts()
    rc = G.lib().pbrt_gpu_group_create(scene_ref, C.byref(opts), devices, n, C.byref(h))
    return rc, h.value


@pytest.fixture(scope="module")
def scene():
    return G.Scene.readme(32, 16)


def test_null_scene_is_invalid():
    rc, h = create(None, (C.c_int32 * 1)(0), 1)
    assert rc == abi.PBRT_E_INVALID and not h


def test_null_devices_is_invalid(scene):
    rc, h = create(C.byref(scene.desc), None, 1)
    assert rc == abi.PBRT_E_INVALID and not h


@pytest.mark.parametrize("n", [0, abi.PBRT_GROUP_MAX + 1])
def test_member_count_out_of_range_is_invalid(scene, n):
    rc, h = create(C.byref(scene.desc), (C.c_int32 * 16)(), n)
    assert rc == abi.PBRT_E_INVALID and not h


def test_negative_ordinal_is_invalid(scene):
    rc, h = create(C.byref(scene.desc), (C.c_int32 * 3)(0, -1, 0), 3)
    assert rc == abi.PBRT_E_INVALID and not h


def test_null_out_is_invalid(scene):
    opts = abi.GpuOpts()
    rc = G.lib().pbrt_gpu_group_create(C.byref(scene.desc), C.byref(opts), (C.c_int32 * 1)(0), 1, None)
    assert rc == abi.PBRT_E_INVALID


def test_python_wrapper_raises_on_a_bad_device_list(scene):
    for devices in ([], [0] * 9, [0, -2]):
        with pytest.raises(G.PbrtError) as e:
            G.RendererGroup(scene, devices)
        assert e.value.code == abi.PBRT_E_INVALID


def test_null_group_calls_are_harmless():
    L = G.lib()
    assert L.pbrt_gpu_group_size(None) == 0
    assert L.pbrt_gpu_group_member(None, 0) is None
    assert L.pbrt_gpu_group_film_device(None) is None
    assert L.pbrt_gpu_group_synchronize(None, None) == abi.PBRT_E_INVALID
    L.pbrt_gpu_group_cancel(None)
    L.pbrt_gpu_group_destroy(None)
    assert L.pbrt_gpu_group_last_error(None) == b"null group"


def test_tile_mapping_partitions_every_subset(tmp_path):
    """group_map.h as a stand-alone host program under ASan + UBSan."""
    exe = tmp_path / "gmc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(REPO, "tests", "group_map_check.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"cases=(\d+) tiles=(\d+) bad=(\d+)", r.stdout)
    assert m and int(m.group(3)) == 0
    assert int(m.group(1)) == 40 * 4 * 3 * 3 * 8 and int(m.group(2)) > 100000

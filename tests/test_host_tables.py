"""The host code that decides what the kernels read, checked without a GPU:
go-pbrt_amd/csrc/scene_tables.h, schedule.h and knobs.h, built as a stand-alone
program under ASan + UBSan (tests/host_tables_check.cpp), each property against
brute force written in the check:

- dev_order: for trees of 1, 3 and 7 nodes, a left-deep chain of 70 interior
  nodes and random trees of 199 and 201 nodes (n leaves make 2 n - 1 nodes), every
  octant's table is a recursive near-first walk, every skip field is the index just
  past the subtree, kOrdOverflow sits exactly on interior nodes with 64 or more far
  children pending, and the leaf lists are the leaves in that order; cycles, an
  offset past the nodes, shared children and forests are refused without a read
  out of bounds; no nodes is accepted;
- cull_groups: group boxes are the exact unions of their members, the G + 1 masks
  of every octant partition the leaf positions, large leaves and singletons are
  tested unconditionally, and G = 0 beyond kLdsNodes nodes, beyond 32 leaves and
  below cull_min (more than kMaxCullGroups groups would take 34 leaves: the check
  holds the bound itself, 32 leaves in 16 groups);
- validate_scene: one accepted scene, and one refusal per rule with its code;
- learn_order: a permutation, costs non-increasing, ties in index order, the heavy
  count, its two caps on either side of ci_wps * n_simd tiles, the override; the
  process cache's keying and its restart when full;
- Knobs::from_env: the defaults and the clamped or ignored values.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scene_tables_schedule_and_knobs(tmp_path):
    exe = tmp_path / "htc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-o", str(exe), os.path.join(REPO, "tests", "host_tables_check.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [ln[:2] for ln in lines] == [["ok", "dev_order"], ["ok", "cull_groups"], ["ok", "validate_scene"],
                                        ["ok", "schedule"], ["ok", "knobs"]]
    checks = {ln[1]: int(ln[2]) for ln in lines}
    # 8 octants x (3 fields + the leaf list) over some 2800 nodes; 200 random schedules of up to 400 slots
    assert checks["dev_order"] > 50000 and checks["schedule"] > 50000
    assert checks["cull_groups"] > 500 and checks["validate_scene"] >= 30 and checks["knobs"] >= 15


def test_the_host_headers_include_no_hip():
    """knobs.h, scene_tables.h, schedule.h and bvh_tables.h take the public headers and the standard library only;
    render_params.h and frame_route.h besides those only each other and the headers above."""
    csrc = os.path.join(REPO, "go-pbrt_amd", "csrc")
    allowed = {"../../include/pbrt_gpu.h", "../../include/pbrt_scene.h", "../../include/pbrt_diag.h", "bvh_tables.h"}
    for name in ("knobs.h", "scene_tables.h", "schedule.h", "bvh_tables.h"):
        for line in open(os.path.join(csrc, name)):
            if line.startswith("#include"):
                inc = line.split()[1]
                assert inc.startswith("<") and "hip" not in inc or inc.strip('"') in allowed, (name, line)
    inc = [ln.split()[1] for ln in open(os.path.join(csrc, "bvh_tables.h")) if ln.startswith("#include")]
    assert inc == ["<cstdint>"]
    # render_params.h (host and device): the standard library alone; frame_route.h: besides the public
    # headers, knobs.h, bvh_tables.h and render_params.h
    inc = [ln.split()[1] for ln in open(os.path.join(csrc, "render_params.h")) if ln.startswith("#include")]
    assert inc == ["<cstdint>"]
    allowed = {"../../include/pbrt_gpu.h", "../../include/pbrt_scene.h", "knobs.h", "bvh_tables.h", "render_params.h"}
    for line in open(os.path.join(csrc, "frame_route.h")):
        if line.startswith("#include"):
            inc = line.split()[1]
            assert inc.startswith("<") and "hip" not in inc or inc.strip('"') in allowed, line

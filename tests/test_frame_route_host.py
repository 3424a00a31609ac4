"""The rules that decide what a frame launches, checked without a GPU:
go-pbrt_amd/csrc/frame_route.h and render_params.h, built as a stand-alone program
under ASan + UBSan (tests/frame_route_check.cpp), each property against brute force
written in the check or against a recorded value, never against the function's own
output:

- layouts: every offset of L, Lci and Lcam is 16-byte aligned, the regions are
  disjoint and `total` / `staging` is the end of the last one, for n_dims 0, 1, 2, 5,
  spp 1 .. 4096, with and without jitter; Lci's three branches on both sides of
  PBRT_CI_STAGE_KB; ci_layout's ring aliasing the staging (G == 1), after it (G > 1),
  twice after it (next-pixel speculation), `pcs` aligned and the caches sized by G;
- render_params: n_slots against a loop that counts tiles around the edges of begin,
  end and stride; sp_serial and sp_window flip at the byte counts PBRT_SP_SERIAL_KB
  and PBRT_SP_WINDOW_KB state;
- check_render and the route: one case per refusal with its code and exact text (the
  texts of render.hip's prepare() before the rules moved), every Route value, every
  PBRT_KERNEL_* request against a render no wave kernel takes, each shared condition
  first in either route's order;
- ci_waves, ci_stride, ci_split: both sides of slots and 2 * slots, every branch of the
  split, the nb / 16 cap, heavy >= nb, the override, kX and mesh-only never splitting on
  one GPU; the path chunks partition [0, nb) in K chunks or fewer; the buffers' carving;
- recorded launches: for cases of tools/dump_launch_logs.py, the chain and path launches
  (template arguments, grid, block, dynamic LDS) are the lines of
  profiles/frame_route/launches_parent.json, copied into the check as literals; the
  static LDS the 3-waves/SIMD rule reads is kernel_resources_parent.json's.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frame_route_rules(tmp_path):
    exe = tmp_path / "frc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-o", str(exe), os.path.join(REPO, "tests", "frame_route_check.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [ln[:2] for ln in lines] == [["ok", "layouts"], ["ok", "render_params"], ["ok", "route"],
                                        ["ok", "chain_rules"], ["ok", "recorded"]]
    checks = {ln[1]: int(ln[2]) for ln in lines}
    # 4 n_dims x 6 spp x 2 jitter renders of three layouts; 252 tile ranges; some 40 refusals and 30 routes;
    # 8 tile counts x 16 chunk counts; 50 recorded frames of two or more launches
    assert checks["layouts"] > 1000 and checks["render_params"] > 700 and checks["route"] > 150
    assert checks["chain_rules"] > 1000 and checks["recorded"] > 300


def test_the_recorded_launches_are_the_parent_dumps():
    """Every launch line the check holds as a literal stands in the committed parent dump."""
    import json
    import re

    dump = json.load(open(os.path.join(REPO, "profiles", "frame_route", "launches_parent.json")))
    lines = set()

    def walk(x):
        for e in x:
            if isinstance(e, list):
                walk(e[1])
            else:
                lines.add(re.sub(r" s\d$", "", e))

    for case in dump.values():
        for frame in case["frames"]:
            walk(frame["launches"])
    lines |= {re.sub(r" lds \d+$", "", ln) for ln in lines if ln.startswith("k_paths_ci<")}
    src = open(os.path.join(REPO, "tests", "frame_route_check.cpp")).read()
    src = src[src.index("static void check_recorded()"):]
    literals = re.findall(r'"(k_[a-z_]+(?:<[^">]*>)? \[[^"]*)"', src)
    assert len(literals) > 100
    for lit in literals:
        assert lit in lines, lit

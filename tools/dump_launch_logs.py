#!/usr/bin/env python3
"""Dump what every render route launches, to compare two builds of the host code.

Per case, on one fresh context: two frames (the cold one, then the learned one).
Per frame: the launch log in order ("kernel [grid x block] lds <dynamic LDS bytes>
s<stream>"; a block of launches that repeats is written once with its count), st.kernel, st.batches, st.paths_traced and the ray counts, the schedule
source, the heavy count of pbrt_gpu_tile_ticks and a hash of the film's bytes. Everything a frame launches is
decided on the host, so two builds that enqueue the same frame give the same file,
byte for byte:

    PBRT_GPU_LIB=<library of the other build> python tools/dump_launch_logs.py --out a.json
    python tools/dump_launch_logs.py --out b.json && cmp a.json b.json

The heavy count of a learned frame whose split is not forced comes from measured
chain times: a case whose two dumps of ONE build differ is timing-dependent; pin it
with PBRT_CI_HEAVY or leave it out (--skip).

Cases: every row of tests/kernel_cases.py (with the rows of
tests/test_coverage_rows_large_trees.py), the routes of tests/edge_routes.py as
tests/test_gpu_edges_routes.py runs them, the forced split under the knobs that
change its choreography, a multi-wave shard with and without its 8-wave tiles, and
a frame of several batches on the chain and the camera-start route.
"""
import argparse
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-pbrt_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import edge_routes as R  # noqa: E402
import kernel_cases as K  # noqa: E402
import pbrtgpu as G  # noqa: E402
import test_coverage_rows_large_trees  # noqa: E402,F401  (adds its rows to K.CASES)
from pbrtgpu import abi  # noqa: E402

KNOB_PREFIXES = ("PBRT_CI_", "PBRT_PATHS_", "PBRT_PW_", "PBRT_SP_", "PBRT_CULL_", "PBRT_GATE_", "PBRT_WAVE_BUFFER_")
SMALL_BUFFER = {"PBRT_WAVE_BUFFER_GB": "0.000001"}   # below one tile's records: one tile per batch


def cases():
    """name -> (scene factory, render_desc, Renderer options, environment)"""
    out = {}
    for name, c in K.CASES.items():
        out[name] = (K.SCENES[c.scene], K.make_rd(c), c.opts, c.env)
    cam = dict(kernel="wave_cam")
    routes = [("matte", {}, {}), ("matte_tp", {}, {}), ("kx", {}, {"PBRT_CI_WAVES": "1"}),
              ("kx", {}, {"PBRT_CI_WAVES": "4"}), ("kx_tp", {}, {}), ("matte_l20", {}, {}), ("dl_matte", {}, {}),
              ("dl_kx", {}, {}), ("cam", cam, {}), ("cam_tp", cam, {}), ("cam_lens", cam, {}), ("cam_crop", cam, {}),
              ("kx", dict(kernel="serial"), {}), ("small_kx", {}, {}), ("small_kx", {}, {"PBRT_PATHS_WF": "1"}),
              ("small_kx", dict(lanes_per_wave=2), {}), ("small_kx_tp", {}, {})]
    for name, opts, env in routes:
        tag = "edge_" + "_".join([name] + [f"{k}{v}" for k, v in sorted(opts.items())] +
                                 [f"{k[5:].lower()}{v}" for k, v in sorted(env.items())])
        out[tag] = (lambda name=name: R.scene(name), R.make_rd(name), opts, env)
    split = K.CASES["split_heavy4"]
    for knob in ("PBRT_PATHS_OVERLAP=0", "PBRT_PATHS_OVERLAP_ALL=0", "PBRT_GATE_HOLD=1", "PBRT_CI_LIGHT_KW=1"):
        k, v = knob.split("=")
        out["split_heavy4_" + k[5:].lower() + v] = (K.SCENES[split.scene], K.make_rd(split), split.opts,
                                                     dict(split.env, **{k: v}))
    readme64 = lambda: G.Scene.readme(64, 64)   # 16 tiles at 2 waves each: a shard that fits the wave slots
    out["shard_w2_split8"] = (readme64, abi.render_desc(2, 2), {}, {"PBRT_CI_WAVES": "2"})
    out["shard_w2_split8_off"] = (readme64, abi.render_desc(2, 2), {}, {"PBRT_CI_WAVES": "2", "PBRT_CI_SPLIT8": "0"})
    # the one-wave Matte chain's build left to its rule (no PBRT_CI_EU): 256 spp (config C's sampler: the
    # windowed StartPixel's staging still leaves 12 workgroups on a CU) and a tree beyond LDS (whose
    # static LDS does not)
    out["spp256_w1"] = (K.SCENES["readme16x16"], abi.render_desc(16, 16, max_depth=3), {}, {"PBRT_CI_WAVES": "1"})
    out["stack_w1_auto"] = (K.SCENES["spheres90"], abi.render_desc(2, 2), {}, {"PBRT_CI_WAVES": "1"})
    two_tiles = lambda: G.Scene.readme(32, 16)
    out["batches_chain"] = (two_tiles, abi.render_desc(2, 2), {}, SMALL_BUFFER)
    out["batches_cam"] = (two_tiles, abi.render_desc(**dict(K.S22, **K.NOSAMP)), cam, SMALL_BUFFER)
    return out


def only_these_knobs(env):
    for k in list(os.environ):
        if k.startswith(KNOB_PREFIXES):
            del os.environ[k]
    os.environ["PBRT_CI_ORDER_CACHE"] = "0"   # every context learns its own schedule
    os.environ.update(env)


def launch_line(rec):
    dims = lambda d: str(d[0]) if d[1:] == (1, 1) else "x".join(map(str, d))
    return f"{rec.name} [{dims(rec.grid)} x {dims(rec.block)}] lds {rec.lds} s{rec.stream}"


def fold(lines):
    """The list with every immediate repetition of a block of up to 8 lines written once, as
    [count, block] (the wavefront's passes, the path chunks, a frame's batches): lossless, and
    a function of the list alone."""
    out, i = [], 0
    while i < len(lines):
        best = (1, 1)   # (period, count)
        for p in range(1, 9):
            k = 1
            while lines[i + k * p:i + (k + 1) * p] == lines[i:i + p]:
                k += 1
            if k > 1 and k * p > best[0] * best[1]:
                best = (p, k)
        p, k = best
        out.append([k, lines[i:i + p]] if k > 1 else lines[i])
        i += p * k
    return out


def run_case(scene, rd, opts, env, frames=2):
    only_these_knobs(env)   # (a context reads its knobs when it is created)
    out = []
    with G.Renderer(scene(), **opts) as r:
        for _ in range(frames):
            film, st = r.render(rd)
            _, heavy = r.tile_ticks()
            log = r.launches()
            out.append({"launches": fold([launch_line(rec) for rec in log]), "n_launches": len(log),
                        "overflow": r.launch_overflow,
                        "film_sha256": hashlib.sha256(film.tobytes()).hexdigest()[:16],
                        "kernel": st.kernel, "batches": st.batches, "paths_traced": st.paths_traced,
                        "camera_samples": st.camera_samples, "rays_closest": st.rays_closest,
                        "rays_shadow": st.rays_shadow, "schedule": r.schedule_source(), "heavy": int(heavy),
                        "overlap_slots": r.overlap_slots()})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", nargs="*", help="these cases only")
    ap.add_argument("--skip", nargs="*", default=[], help="cases to leave out (timing-dependent ones)")
    args = ap.parse_args()
    table = cases()
    pick = [n for n in (args.only or table) if n not in args.skip]
    dump = {}
    for name in pick:
        scene, rd, opts, env = table[name]
        dump[name] = {"opts": opts, "env": env, "frames": run_case(scene, rd, opts, env)}
        print(name, [f["n_launches"] for f in dump[name]["frames"]], flush=True)
    with open(args.out, "w") as f:   # one line per case
        rows = [f"{json.dumps(name)}: {json.dumps(dump[name], sort_keys=True)}" for name in sorted(dump)]
        f.write("{\n" + ",\n".join(rows) + "\n}\n")
    print(f"{len(dump)} cases -> {args.out} (library {G.build_id()})")


if __name__ == "__main__":
    main()

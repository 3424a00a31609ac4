"""The stratified public pieces against the library's own frame, and
li_stratified_device against li_device.

  composed  config B's render desc (README 1920x1080, Stratified(8, 8, false, 4),
            Path(10), Uniform) in THROUGHPUT mode, composed as
            Renderer.render_samples_stratified composes it: per ascending tile range
            sized to --budget-gb, frame_samples_stratified, li_stratified_device at the
            cursors after the camera sample and film_add into a device film, buffers
            allocated once. Wall time from the first enqueue until
            pbrt_gpu_query_status returns, median of --repeats after --warmup; then
            the same frame with the stream synchronised after every stage, which
            gives the three stages' shares.
  frame     the same desc by pbrt_gpu_render_async (AUTO kernel): wall time to the end
            of synchronize and the frame's own device-event times. Same process, same
            build. The two films are compared bit for bit on every run of the tool.
            The library frame traces one camera ray per pixel and caches bounce 1;
            the composed frame traces one per sample.
  li        2 M rays (the first --li-rays samples of the composed frame's first
            ranges) and their streams through li_device and through
            li_stratified_device with both cursors at n_dims: the cost of the per-ray
            table pointer and indices when no stratified value is read. The outputs
            are compared bit for bit.

One GPU process; every step runs under a time limit of its own (SIGALRM), and the
process ends at the first step that fails or overruns.

    python tools/strat_frame_bench.py [--out profiles/strat_query/strat_frame_bench.json] [--small]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-pbrt_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import pbrtgpu as G  # noqa: E402
from open_frame_bench import stats, step, sync  # noqa: E402
from pbrtgpu import abi  # noqa: E402


def composed(scene, sx, sy, nd, args):
    spp = sx * sy
    ns = spp - 1
    c1, c2 = abi.camera_cursors(nd)
    with G.Renderer(scene) as r:
        ranges = r.frame_ranges_stratified(spp, nd, 16, int(args.budget_gb * 2**30))
        cap = max(n for _, _, n in ranges)
        sb = {k: r.buffer(cap, G.SAMPLE_DTYPES[k]) for k in G.SAMPLE_REQUIRED}
        ob = {k: r.buffer(cap) for k in ("r", "g", "b")}
        kb = {k: r.buffer(cap, np.int32) for k in G.STRAT_SAMPLE_KEYS}
        kb["s1d"] = r.buffer((cap // ns) * nd * spp)
        film = r.buffer(r.hgt * r.w * 3)
        rays, rng = {k: sb[k] for k in G.RAY_KEYS}, {k: sb[k] for k in G.RNG_KEYS}
        fs = dict(pfilm_x=sb["pfilm_x"], pfilm_y=sb["pfilm_y"], r=ob["r"], g=ob["g"], b=ob["b"])
        stage = {"samples": [], "li": [], "film_add": []}

        def run(split):
            acc = dict.fromkeys(stage, 0.0)
            for i, (b, e, n) in enumerate(ranges):
                t0 = time.perf_counter()
                assert r.frame_samples_stratified(sb, kb, sx, sy, nd, False, b, e) == 0, r.last_error()
                if split:
                    sync(r)
                t1 = time.perf_counter()
                assert r.li_stratified_device(rays, rng, n, ob, kb, n // ns, spp, nd, c1, c2, max_depth=10) == 0, r.last_error()
                if split:
                    sync(r)
                t2 = time.perf_counter()
                assert r.film_add(fs, ns, film, b, e, clear=i == 0) == 0, r.last_error()
                if split:
                    sync(r)
                t3 = time.perf_counter()
                acc["samples"] += t1 - t0
                acc["li"] += t2 - t1
                acc["film_add"] += t3 - t2
            sync(r)
            if split:
                for k in stage:
                    stage[k].append(acc[k])

        whole = []
        for i in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            run(False)
            if i >= args.warmup:
                whole.append(time.perf_counter() - t0)
        for i in range(args.warmup + args.repeats):
            run(True)
        for k in stage:
            stage[k] = stage[k][args.warmup:]
        names = sorted({rec.name for rec in r.launches(outside=True)})
        out_film = film.download().reshape(r.hgt, r.w, 3)

        # li_stratified_device against li_device on the rays and streams the buffers hold (the last range's)
        n_li = min(args.li_rays, ranges[-1][2])
        ob2 = {k: r.buffer(n_li, dt) for k, dt in G.LI_DTYPES.items()}
        ob3 = {k: r.buffer(n_li, dt) for k, dt in G.LI_DTYPES.items()}
        t_plain, t_strat = [], []
        for i in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            assert r.li_device(rays, rng, n_li, ob2, max_depth=10) == 0, r.last_error()
            sync(r)
            t1 = time.perf_counter()
            assert r.li_stratified_device(rays, rng, n_li, ob3, kb, ranges[-1][2] // ns, spp, nd, nd, nd, max_depth=10) == 0
            sync(r)
            t2 = time.perf_counter()
            if i >= args.warmup:
                t_plain.append(t1 - t0)
                t_strat.append(t2 - t1)
        equal = all(ob2[k].download().tobytes() == ob3[k].download().tobytes() for k in ob2)
    samples = sum(n for _, _, n in ranges)
    out = {"kernels": names, "ranges": len(ranges), "samples": samples, "bytes_per_sample": G.STRAT_BYTES_PER_SAMPLE,
           "table_bytes_per_pixel": 8 * nd * spp, "whole": stats(whole), "stages": {k: stats(v) for k, v in stage.items()},
           "ns_per_sample": {k: float(np.median(v)) / samples * 1e9 for k, v in stage.items()}}
    li = {"rays": n_li, "li_device": stats(t_plain), "li_stratified_device_cursors_at_n_dims": stats(t_strat),
          "outputs_equal": bool(equal), "stratified_over_plain": float(np.median(t_strat)) / float(np.median(t_plain))}
    print(json.dumps(out), flush=True)
    print(json.dumps(li), flush=True)
    return out, li, out_film


def library_frame(scene, sx, sy, nd, args):
    rd = abi.render_desc(sx, sy, n_dims=nd, max_depth=10, mode=abi.PBRT_MODE_THROUGHPUT)
    wall, res = [], []
    with G.Renderer(scene) as r:
        for i in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            r.render_async(rd)
            st = r.synchronize()
            t1 = time.perf_counter()
            if i >= args.warmup:
                wall.append(t1 - t0)
                res.append((st.kernel_ms, st.paths_ms, int(st.paths_traced), int(st.kernel)))
        film = r.film()
        names = sorted({rec.name for rec in r.launches()})
    out = {"kernels": names, "paths": res[0][2], "kernel": res[0][3], "wall": stats(wall),
           "kernel_ms": float(np.median([k for k, _, _, _ in res])), "paths_ms": float(np.median([p for _, p, _, _ in res]))}
    print(json.dumps(out), flush=True)
    return out, film


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--budget-gb", type=float, default=1.0, help="sample arrays and tables of one tile range")
    ap.add_argument("--li-rays", type=int, default=2 * 1000 * 1000)
    ap.add_argument("--limit", type=int, default=200, help="seconds a step may take")
    ap.add_argument("--small", action="store_true", help="a tiny film (a functional check of the tool)")
    args = ap.parse_args()
    w, h, sx, sy, nd = (1920, 1080, 8, 8, 4) if not args.small else (64, 48, 2, 2, 4)
    if args.small:
        args.budget_gb = (112 * 3 + 8 * 16) * 256 * 3 / 2**30   # three tiles a range
    scene = G.Scene.readme(w, h)
    frame, lib_film = step("frame", args.limit, lambda: library_frame(scene, sx, sy, nd, args))
    comp, li, film = step("composed", args.limit, lambda: composed(scene, sx, sy, nd, args))
    comp["film_is_the_library_frames"] = bool(np.array_equal(film.view(np.uint64), lib_film.view(np.uint64)))
    comp["whole_over_frame_wall"] = comp["whole"]["median_ms"] / frame["wall"]["median_ms"]
    res = {"what": "a frame composed of frame_samples_stratified, li_stratified_device and film_add in tile ranges against "
                   f"the library's THROUGHPUT frame of the same desc (README {w}x{h}, Stratified({sx}, {sy}, false, {nd}), "
                   "Path(10)); and li_stratified_device with its cursors at n_dims against li_device on the same rays",
           "build_id": G.build_id(), "warmup": args.warmup, "repeats": args.repeats, "budget_gb": args.budget_gb,
           "frame": frame, "composed": comp, "li": li}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({"whole_over_frame_wall": comp["whole_over_frame_wall"],
                      "film_is_the_library_frames": comp["film_is_the_library_frames"],
                      "stratified_over_plain": li["stratified_over_plain"], "outputs_equal": li["outputs_equal"]}))
    if not (comp["film_is_the_library_frames"] and li["outputs_equal"]):
        sys.exit(1)


if __name__ == "__main__":
    main()

"""A frame composed of the public stages against the library's own frame, and the
tail of a request (film to RGBA8 bytes on the host) on the device against the host.

  composed  README 1920x1080, 64 samples a pixel (63 traced), Path(10), THROUGHPUT
            with n_dims = 0, composed as Renderer.render_samples composes it: per
            ascending tile range sized to --budget-gb, frame_samples, li_device and
            film_add into a device film, buffers allocated once. Wall time from the
            first enqueue until pbrt_gpu_query_status returns, median of --repeats
            after --warmup; then the same frame with the stream synchronised after
            every stage, which gives the three stages' shares. Both gather kernels
            of film_add (PBRT_FILM_ADD=lds / direct, a context each).
  frame     the same render by pbrt_gpu_render_async on the camera-start route
            (kernel="wave_cam"): wall time to the end of synchronize, and the
            frame's own device-event times. Same process, same build. The two
            films are compared bit for bit.
  tail      after one EXACT and one THROUGHPUT frame of config B (Stratified(8, 8),
            Path(10)) into a caller's device film: film_rgba8 + a download of the
            8 MB image, against a download of the 50 MB film + pbrt_film_to_rgba8
            on the host; copy and conversion apart. The bytes are compared.

One GPU process; every step runs under a time limit of its own (SIGALRM), and the
process ends at the first step that fails or overruns.

    python tools/open_frame_bench.py [--out profiles/open_frame/open_frame_bench.json] [--small]
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-pbrt_amd"))
import pbrtgpu as G  # noqa: E402
from pbrtgpu import abi  # noqa: E402


class StepTimeout(Exception):
    pass


def step(name, limit_s, fn):
    """fn() under a time limit of its own."""
    def fire(signum, frame):
        raise StepTimeout(f"step '{name}' ran longer than {limit_s} s")
    signal.signal(signal.SIGALRM, fire)
    signal.alarm(limit_s)
    try:
        return fn()
    finally:
        signal.alarm(0)


def stats(ts):
    return {"median_ms": float(np.median(ts)) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3, "repeats": len(ts)}


def sync(r):
    rc, rec = r.query_status()
    assert rc == 0, (rc, rec.panics)


def composed(variant, scene, spp, args):
    """The composed frame on a context created under PBRT_FILM_ADD=variant."""
    os.environ["PBRT_FILM_ADD"] = variant
    ns = spp - 1
    with G.Renderer(scene) as r:
        ranges = r.frame_ranges(ns, 16, int(args.budget_gb * 2**30))
        cap = max(n for _, _, n in ranges)
        sb = {k: r.buffer(cap, G.SAMPLE_DTYPES[k]) for k in G.SAMPLE_REQUIRED}
        ob = {k: r.buffer(cap) for k in ("r", "g", "b")}
        film = r.buffer(r.hgt * r.w * 3)
        rays, rng = {k: sb[k] for k in G.RAY_KEYS}, {k: sb[k] for k in G.RNG_KEYS}
        fs = dict(pfilm_x=sb["pfilm_x"], pfilm_y=sb["pfilm_y"], r=ob["r"], g=ob["g"], b=ob["b"])
        stage = {"samples": [], "li": [], "film_add": []}

        def run(split):
            acc = dict.fromkeys(stage, 0.0)
            for i, (b, e, n) in enumerate(ranges):
                t0 = time.perf_counter()
                assert r.frame_samples(sb, ns, b, e) == 0, r.last_error()
                if split:
                    sync(r)
                t1 = time.perf_counter()
                assert r.li_device(rays, rng, n, ob, max_depth=10) == 0, r.last_error()
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
        scratch = r.film_scratch_bytes()
    samples = sum(n for _, _, n in ranges)
    out = {"variant": variant, "kernels": names, "ranges": len(ranges), "samples": samples,
           "bytes_per_sample": G.FRAME_BYTES_PER_SAMPLE, "array_bytes": cap * G.FRAME_BYTES_PER_SAMPLE,
           "film_scratch_bytes": scratch, "whole": stats(whole), "stages": {k: stats(v) for k, v in stage.items()},
           "ns_per_sample": {k: float(np.median(v)) / samples * 1e9 for k, v in stage.items()}}
    print(json.dumps(out), flush=True)
    return out, out_film


def library_frame(scene, spp, args):
    rd = abi.render_desc(max_depth=10, mode=abi.PBRT_MODE_THROUGHPUT)
    G.lib().pbrt_random_sampler(spp, G.C.byref(rd))
    wall, res = [], []
    with G.Renderer(scene, kernel="wave_cam") as r:
        for i in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            r.render_async(rd)
            st = r.synchronize()
            t1 = time.perf_counter()
            assert st.kernel == abi.PBRT_KERNEL_WAVE_CAM
            if i >= args.warmup:
                wall.append(t1 - t0)
                res.append((st.kernel_ms, st.paths_ms, int(st.paths_traced)))
        film = r.film()
        names = [rec.name for rec in r.launches()]
    out = {"kernels": names, "paths": res[0][2], "wall": stats(wall),
           "kernel_ms": float(np.median([k for k, _, _ in res])), "paths_ms": float(np.median([p for _, p, _ in res]))}
    print(json.dumps(out), flush=True)
    return out, film


def tail(scene, args):
    """Film to RGBA8 bytes on the host: device conversion + small download against big download + host conversion."""
    out = {}
    L, dp, bp = G.lib(), G.C.POINTER(G.C.c_double), G.C.POINTER(G.C.c_uint8)
    with G.Renderer(scene) as r:
        film = r.buffer(r.hgt * r.w * 3)
        rgba = r.buffer(r.hgt * r.w * 4, np.uint8)
        # host arrays allocated and touched once, as a server keeps them: a fresh 50 MB array per
        # request would add its page faults to the copy
        got, host_film, want = np.zeros(rgba.n, np.uint8), np.zeros(film.n), np.zeros(rgba.n, np.uint8)
        for mode, key in ((abi.PBRT_MODE_EXACT, "exact"), (abi.PBRT_MODE_THROUGHPUT, "throughput")):
            rd = abi.render_desc(8, 8, max_depth=10, mode=mode)
            r.render_async(rd, film.ptr)
            r.synchronize()
            dev_conv, dev_copy, host_copy, host_conv = [], [], [], []
            for i in range(args.warmup + args.repeats):
                t0 = time.perf_counter()
                r.film_rgba8(film, rgba)
                sync(r)
                t1 = time.perf_counter()
                assert L.pbrt_gpu_buffer_download(rgba._h, 0, got.ctypes.data, got.nbytes) == 0
                t2 = time.perf_counter()
                assert L.pbrt_gpu_buffer_download(film._h, 0, host_film.ctypes.data, host_film.nbytes) == 0
                t3 = time.perf_counter()
                assert L.pbrt_film_to_rgba8(host_film.ctypes.data_as(dp), r.w, r.hgt, want.ctypes.data_as(bp)) == 0
                t4 = time.perf_counter()
                assert np.array_equal(got, want)
                if i >= args.warmup:
                    dev_conv.append(t1 - t0)
                    dev_copy.append(t2 - t1)
                    host_copy.append(t3 - t2)
                    host_conv.append(t4 - t3)
            dev = [a + b for a, b in zip(dev_conv, dev_copy)]
            host = [a + b for a, b in zip(host_copy, host_conv)]
            out[key] = {"device": dict(stats(dev), convert_ms=float(np.median(dev_conv)) * 1e3,
                                       download_ms=float(np.median(dev_copy)) * 1e3, bytes=int(rgba.nbytes)),
                        "host": dict(stats(host), download_ms=float(np.median(host_copy)) * 1e3,
                                     convert_ms=float(np.median(host_conv)) * 1e3, bytes=int(film.nbytes)),
                        "host_over_device": float(np.median(host)) / float(np.median(dev))}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--budget-gb", type=float, default=1.0, help="sample arrays of one tile range")
    ap.add_argument("--limit", type=int, default=150, help="seconds a step may take")
    ap.add_argument("--small", action="store_true", help="a tiny film (a functional check of the tool)")
    args = ap.parse_args()
    w, h, spp = (1920, 1080, 64) if not args.small else (64, 48, 4)
    if args.small:
        args.budget_gb = 104 * 3 * 256 * 3 / 2**30   # three tiles a range
    scene = G.Scene.readme(w, h)
    frame, lib_film = step("frame", args.limit, lambda: library_frame(scene, spp, args))
    comp = {}
    for variant in ("lds", "direct"):
        comp[variant], film = step(f"composed {variant}", args.limit, lambda: composed(variant, scene, spp, args))
        comp[variant]["film_is_the_library_frames"] = bool(np.array_equal(film.view(np.uint64), lib_film.view(np.uint64)))
        comp[variant]["whole_over_frame_wall"] = comp[variant]["whole"]["median_ms"] / frame["wall"]["median_ms"]
        comp[variant]["li_over_frame_paths_ms"] = comp[variant]["stages"]["li"]["median_ms"] / frame["paths_ms"]
    os.environ.pop("PBRT_FILM_ADD", None)
    t = step("tail", args.limit, lambda: tail(scene, args))
    res = {"what": "a frame composed of frame_samples, li_device and film_add in tile ranges against the wave_cam frame "
                   f"of the same render (README {w}x{h}, {spp} spp, Path(10), THROUGHPUT n_dims 0); and film to RGBA8 "
                   "bytes on the host by the device conversion against the host conversion, config B",
           "build_id": G.build_id(), "warmup": args.warmup, "repeats": args.repeats, "budget_gb": args.budget_gb,
           "frame": frame, "composed": comp, "tail": t}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({v: {k: c[k] for k in ("whole_over_frame_wall", "li_over_frame_paths_ms",
                                            "film_is_the_library_frames")} for v, c in comp.items()}))


if __name__ == "__main__":
    main()

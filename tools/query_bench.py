"""Throughput of the ray-query paths of the C ABI, in Mrays/s:

  host      pbrt_gpu_intersect: host SoA arrays in and out (repack, allocate,
            copy both ways, synchronise, every call);
  device    pbrt_gpu_intersect_device on rays already resident in DeviceBuffers;
  chained   pbrt_gpu_camera_rays_device + pbrt_gpu_intersect_device on its
            output (primary-ray sets only).

Ray sets: the README scene at 1920x1080 with its 2 073 600 primary rays and
with 2^22 random rays (tests/test_gpu_parity.py's generator), and the
707-quad height field (config D's mesh) with its own primary rays.

The ABI exposes no events on the context's stream, so a repeat is host wall
time from the first enqueue until pbrt_gpu_query_status returns (it
synchronises the stream); the host path is wall time of the call. Median of
--repeats timed repeats after --warmup untimed ones. numpy and ctypes only.

    python tools/query_bench.py [--out profiles/query/query_bench.json] [--small]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-pbrt_amd"))
import pbrtgpu as G  # noqa: E402
from pbrtgpu import abi  # noqa: E402


def random_rays(n, seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-60, 140, size=(n, 3))
    o[:, 1] = rng.uniform(-5, 120, size=n)
    d = rng.normal(size=(n, 3))
    tmax = np.where(rng.uniform(size=n) < 0.2, rng.uniform(1, 200, size=n), np.inf)
    return np.concatenate([o, d, tmax[:, None]], axis=1)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def host_call(r, cols):
    """pbrt_gpu_intersect over prepared host arrays (no numpy work in the timed call)."""
    n = cols[0].size
    dp = C.POINTER(C.c_double)
    soa = abi.RaySoA(*[c.ctypes.data_as(dp) for c in cols])
    hit, tmax, prim = np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.int32)
    pn = [np.zeros(n) for _ in range(6)]
    hs = abi.HitSoA(hit.ctypes.data_as(C.POINTER(C.c_uint8)), tmax.ctypes.data_as(dp),
                    prim.ctypes.data_as(C.POINTER(C.c_int32)), *[a.ctypes.data_as(dp) for a in pn])
    keep = (cols, hit, tmax, prim, pn)

    def call():
        rc = G.lib().pbrt_gpu_intersect(r.h, C.byref(soa), n, C.byref(hs))
        assert rc == 0, rc
        return keep
    return call, hit


def measure(name, scene, rays, window, args):
    """rays: (n, 7) host rays, or None for the primary rays of window."""
    out = {"set": name, "paths": {}}
    with G.Renderer(scene) as r:
        if rays is None:
            cam = r.camera_rays(window)
            r.query_status()
            cols = [cam[k].download() for k in G.RAY_KEYS + ("tmax",)]
        else:
            cols = [np.ascontiguousarray(rays[:, k]) for k in range(7)]
        n = cols[0].size
        out["rays"] = n
        rb = {k: r.upload(c) for k, c in zip(G.RAY_KEYS + ("tmax",), cols)}
        hb = {k: r.buffer(n, dt) for k, dt in G.HIT_DTYPES.items()}

        def device():
            assert r.intersect_device(rb, n, hb) == 0
            assert r.query_status()[0] == 0

        def chained():
            r.camera_rays(window, out=rb)
            assert r.intersect_device(rb, n, hb) == 0
            assert r.query_status()[0] == 0

        host, host_hit = host_call(r, cols)
        paths = [("host", host), ("device", device)] + ([("chained", chained)] if rays is None else [])
        for pname, fn in paths:
            ts = timed(fn, args.warmup, args.repeats)
            med = float(np.median(ts))
            out["paths"][pname] = {"median_ms": med * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3,
                                   "mrays_per_s": n / med / 1e6, "repeats": len(ts)}
        out["hit_fraction"] = float(host_hit.mean())
        out["same_hits"] = bool(np.array_equal(hb["hit"].download(), host_hit))
    out["device_over_host"] = out["paths"]["device"]["mrays_per_s"] / out["paths"]["host"]["mrays_per_s"]
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="tiny ray sets (a functional check of the tool)")
    args = ap.parse_args()
    w, h, nrand, quads = (1920, 1080, 1 << 22, 707) if not args.small else (64, 48, 1 << 12, 8)
    readme = G.Scene.readme(w, h)
    sets = [measure(f"readme {w}x{h} primary", readme, None, (0, 0, w, h), args),
            measure(f"readme {w}x{h} random 2^{nrand.bit_length() - 1}", readme, random_rays(nrand, 3), None, args)]
    field = G.Scene.heightfield(w, h, quads=quads, seed=1)
    sets.append(measure(f"heightfield {quads} quads {w}x{h} primary", field, None, (0, 0, w, h), args))
    res = {"what": "ray queries, Mrays/s: host arrays (pbrt_gpu_intersect) against device-resident arrays "
                   "(pbrt_gpu_intersect_device, alone and chained after pbrt_gpu_camera_rays_device); wall time "
                   "to the end of pbrt_gpu_query_status, median of the timed repeats",
           "build_id": G.build_id(), "warmup": args.warmup, "repeats": args.repeats, "sets": sets,
           "device_not_slower_than_host": all(s["device_over_host"] >= 1.0 for s in sets)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "sets"}))


if __name__ == "__main__":
    main()

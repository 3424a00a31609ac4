"""Rate of pbrt_gpu_li_device (k_li), in ns per path, against the path stage of a frame.

  li      pbrt_gpu_camera_rays_device + pbrt_gpu_li_device on the 2 073 600 primary
          rays of a 1920x1080 scene (max_depth 10, Uniform lights, every ray on a
          PCG32 stream of its own), buffers resident in DeviceBuffers: host wall time
          from the first enqueue until pbrt_gpu_query_status returns (it synchronises
          the stream), median of --repeats timed repeats after --warmup untimed ones;
  frame   paths_ms / paths_traced of a THROUGHPUT frame of the README scene on the
          camera-start route (kernel="wave_cam", pbrt_random_sampler(64), Path(10)):
          the same path_step work behind k_paths_cam<64, true>, timed by the frame's
          own device events. Median over the same number of frames, same process.

Scenes: README (k_li<false, 0>) and readme_glass (k_li<true, 0>). The figure to
read is li ns/path over frame ns/path of the README scene (DESIGN.md section 6.1
expects at most 1.25). One GPU process; every step runs under a time limit of its
own (SIGALRM), and the process ends at the first step that fails or overruns.

    python tools/li_bench.py [--out profiles/li_query/li_bench.json] [--small]
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


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def li_rate(name, scene, w, h, args):
    n = w * h
    rng = np.random.default_rng(11)
    state = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    inc = rng.integers(0, 2**63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    with G.Renderer(scene) as r:
        rb = {k: r.buffer(n) for k in G.RAY_KEYS + ("tmax",)}
        gb = {"state": r.upload(state), "inc": r.upload(inc)}
        ob = {k: r.buffer(n, dt) for k, dt in G.LI_DTYPES.items()}

        def run():
            r.camera_rays((0, 0, w, h), out=rb)
            assert r.li_device(rb, gb, n, ob, max_depth=10) == 0, r.last_error()
            rc, rec = r.query_status()
            assert rc == 0, (rc, rec.panics)

        ts = timed(run, args.warmup, args.repeats)
        kernel = [rec.name for rec in r.launches(outside=True) if rec.name.startswith("k_li")][-1]
        draws, rays = ob["draws"].download(), ob["rays"].download()
        lum = ob["g"].download()
    med = float(np.median(ts))
    out = {"set": name, "kernel": kernel, "paths": n, "median_ms": med * 1e3, "min_ms": min(ts) * 1e3,
           "max_ms": max(ts) * 1e3, "ns_per_path": med / n * 1e9, "mpaths_per_s": n / med / 1e6, "repeats": len(ts),
           "mean_draws": float(draws.mean()), "mean_closest_rays": float((rays & 0xFFFF).mean()),
           "mean_shadow_rays": float((rays >> 16).mean()), "mean_g": float(lum.mean())}
    print(json.dumps(out), flush=True)
    return out


def frame_rate(name, scene, ns, args):
    rd = abi.render_desc(max_depth=10, mode=abi.PBRT_MODE_THROUGHPUT)
    G.lib().pbrt_random_sampler(ns, G.C.byref(rd))
    res = []
    with G.Renderer(scene, kernel="wave_cam") as r:
        for i in range(args.warmup + args.repeats):
            r.render_async(rd)
            st = r.synchronize()
            assert st.kernel == abi.PBRT_KERNEL_WAVE_CAM
            if i >= args.warmup:
                res.append((st.paths_ms, st.kernel_ms, int(st.paths_traced)))
        kernel = [rec.name for rec in r.launches() if rec.name.startswith("k_paths_cam")][-1]
    pm = float(np.median([p for p, _, _ in res]))
    paths = res[0][2]
    out = {"set": name, "kernel": kernel, "paths": paths, "paths_ms": pm, "min_paths_ms": min(p for p, _, _ in res),
           "max_paths_ms": max(p for p, _, _ in res), "kernel_ms": float(np.median([k for _, k, _ in res])),
           "ns_per_path": pm / paths * 1e6, "repeats": len(res)}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds a step may take")
    ap.add_argument("--small", action="store_true", help="tiny sets (a functional check of the tool)")
    args = ap.parse_args()
    w, h, ns = (1920, 1080, 64) if not args.small else (64, 48, 4)
    readme, glass = G.Scene.readme(w, h), G.Scene.readme_glass(w, h)
    frame = step("frame", args.limit, lambda: frame_rate(f"readme {w}x{h} wave_cam THROUGHPUT random({ns}) Path(10)",
                                                        readme, ns, args))
    li = [step("li readme", args.limit, lambda: li_rate(f"readme {w}x{h} primary", readme, w, h, args)),
          step("li glass", args.limit, lambda: li_rate(f"readme_glass {w}x{h} primary", glass, w, h, args))]
    ratio = li[0]["ns_per_path"] / frame["ns_per_path"]
    res = {"what": "pbrt_gpu_li_device (camera_rays + li_device, wall time to the end of query_status, median) against "
                   "paths_ms / paths of a THROUGHPUT wave_cam frame (device events, median), ns per path",
           "build_id": G.build_id(), "warmup": args.warmup, "repeats": args.repeats, "frame": frame, "li": li,
           "li_over_frame_readme": ratio, "li_over_frame_glass_scene": li[1]["ns_per_path"] / frame["ns_per_path"],
           "expected_at_most": 1.25, "within_expectation": bool(ratio <= 1.25)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("frame", "li")}))


if __name__ == "__main__":
    main()

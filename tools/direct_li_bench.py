"""Rates of pbrt_gpu_direct_li_device (k_li_direct) and of the DirectLighting frame composed of it.

  rays    direct_li_device (both strategies) and li_device on the same 2 073 600 primary
          rays of a 1920x1080 scene, max_depth 10, every ray on a PCG32 stream of its
          own, buffers resident in DeviceBuffers: host wall time from the enqueue until
          pbrt_gpu_query_status returns (it synchronises the stream), median of
          --repeats timed repeats after --warmup untimed ones. Scenes: README
          (k_li_direct<false, 0>) and readme_glass (k_li_direct<true, 0>). The figure to
          read is direct (UNIFORM_SAMPLE_ONE) over li: on a Matte scene it does a prefix
          of Path.Li's first bounce.
  grid    the same direct query with PBRT_DIRECT_LI_GRID at each value of --grids (a
          context of its own each: the knob is read when a context is created).
  frame   README 1080p, pbrt_random_sampler(64) (63 traced samples a pixel),
          DirectLighting(10), THROUGHPUT: the frame as Renderer.render_samples composes it
          within 1 GiB (wall time, film download included) against pbrt_gpu_render of the
          same render desc (wall time of Renderer.render), and the two films bit for bit;
          then the composed frame alone with PBRT_DIRECT_LI_GRID at each value of
          --frame-grids. With --render-only the composed frame is left out, for a library
          of an earlier build (PBRT_GPU_LIB).

One GPU process; every step runs under a time limit of its own (SIGALRM), and the
process ends at the first step that fails or overruns.

    python tools/direct_li_bench.py [--out profiles/direct_li/direct_li_bench.json] [--small]
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

ALL, ONE = abi.PBRT_DL_UNIFORM_SAMPLE_ALL, abi.PBRT_DL_UNIFORM_SAMPLE_ONE
DIRECT = abi.PBRT_INTEGRATOR_DIRECT_LIGHTING


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


def summary(ts, n):
    med = float(np.median(ts))
    return {"median_ms": med * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3, "ns_per_ray": med / n * 1e9,
            "repeats": len(ts)}


def ray_rates(name, scene, w, h, args, with_li=True):
    n = w * h
    rng = np.random.default_rng(11)
    state = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    inc = rng.integers(0, 2**63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    out = {"set": name, "rays": n}
    with G.Renderer(scene) as r:
        rb = {k: r.buffer(n) for k in G.RAY_KEYS + ("tmax",)}
        gb = {"state": r.upload(state), "inc": r.upload(inc)}
        ob = {k: r.buffer(n, dt) for k, dt in G.LI_DTYPES.items()}
        r.camera_rays((0, 0, w, h), out=rb)

        def query(call, **desc):
            def run():
                assert call(rb, gb, n, ob, max_depth=10, **desc) == 0, r.last_error()
                rc, rec = r.query_status()
                assert rc == 0, (rc, rec.panics)
            res = summary(timed(run, args.warmup, args.repeats), n)
            rec = r.launches(outside=True)[-1]
            rays, draws = ob["rays"].download(), ob["draws"].download()
            res.update(kernel=rec.name, grid=rec.grid[0], mean_draws=float(draws.mean()),
                       mean_closest_rays=float((rays & 0xFFFF).mean()), mean_shadow_rays=float((rays >> 16).mean()),
                       mean_g=float(ob["g"].download().mean()))
            return res

        out["direct_all"] = query(r.direct_li_device, dl_strategy=ALL)
        out["direct_one"] = query(r.direct_li_device, dl_strategy=ONE)
        out["scratch_bytes"] = int(r.direct_li_scratch_bytes())
        if with_li:
            out["li"] = query(r.li_device)
            out["direct_one_over_li"] = out["direct_one"]["median_ms"] / out["li"]["median_ms"]
            out["direct_all_over_li"] = out["direct_all"]["median_ms"] / out["li"]["median_ms"]
    print(json.dumps(out), flush=True)
    return out


def frame_desc(ns):
    rd = abi.render_desc(integrator=DIRECT, max_depth=10, dl_strategy=ALL, mode=abi.PBRT_MODE_THROUGHPUT)
    G.lib().pbrt_random_sampler(ns, G.C.byref(rd))
    return rd


def frames(scene, ns, args, composed_only=False):
    """pbrt_random_sampler(ns): ns samples a pixel, of which sample 0 is never traced; render_samples(ns) is that frame."""
    out = {"set": f"README random({ns}) DirectLighting(10) THROUGHPUT",
           "PBRT_DIRECT_LI_GRID": os.environ.get("PBRT_DIRECT_LI_GRID", "")}
    rd = frame_desc(ns)
    with G.Renderer(scene) as r:
        films = {}
        if not args.render_only:
            def composed():
                films["composed"], films["info"] = r.render_samples(ns, max_depth=10, integrator=DIRECT,
                                                                    dl_strategy=ALL, budget_bytes=1 << 30)
            out["composed"] = summary(timed(composed, args.warmup, args.repeats), films["info"]["samples"])
            out["composed"].update(films["info"])
            out["composed"]["grid"] = max(rec.grid[0] for rec in r.launches(outside=True)
                                          if rec.name.startswith("k_li_direct"))
        if composed_only:
            print(json.dumps(out), flush=True)
            return out

        def render():
            films["render"], films["stats"] = r.render(rd)
        out["render"] = summary(timed(render, min(args.warmup, 1), args.render_repeats), int(r.w * r.hgt * ns))
        out["render"].update(kernel_ms=float(films["stats"].kernel_ms), paths=int(films["stats"].paths_traced),
                             kernels=sorted({rec.name for rec in r.launches()}))
        if not args.render_only:
            a, b = films["composed"].view(np.uint64), films["render"].view(np.uint64)
            out["films_differ_in"] = int((a != b).sum())
            out["films_bit_identical"] = bool(np.array_equal(a, b))
            out["render_over_composed"] = out["render"]["median_ms"] / out["composed"]["median_ms"]
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--render-repeats", type=int, default=7, help="timed pbrt_gpu_render frames (the serial kernel)")
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--grids", default="", help="comma-separated PBRT_DIRECT_LI_GRID values to sweep")
    ap.add_argument("--frame-grids", default="", help="PBRT_DIRECT_LI_GRID values to sweep on the composed frame")
    ap.add_argument("--no-rays", action="store_true")
    ap.add_argument("--no-frames", action="store_true")
    ap.add_argument("--render-only", action="store_true", help="pbrt_gpu_render's frame alone (an earlier build)")
    ap.add_argument("--small", action="store_true", help="tiny sets (a functional check of the tool)")
    args = ap.parse_args()
    w, h, ns = (1920, 1080, 64) if not args.small else (64, 48, 4)
    res = {"what": "direct_li_device and li_device on the same primary rays (wall time to the end of query_status, "
                   "median), and the composed DirectLighting frame against pbrt_gpu_render of the same render desc",
           "build_id": G.build_id(), "lib": os.path.relpath(G.LIB_PATH, REPO), "warmup": args.warmup,
           "repeats": args.repeats}
    readme = G.Scene.readme(w, h)
    if not args.render_only and not args.no_rays:
        glass = G.Scene.readme_glass(w, h)
        res["rays"] = [step("rays readme", args.limit, lambda: ray_rates(f"readme {w}x{h} primary", readme, w, h, args)),
                       step("rays glass", args.limit, lambda: ray_rates(f"readme_glass {w}x{h} primary", glass, w, h, args))]
        res["grid_sweep"] = []
        for g in [int(v) for v in args.grids.split(",") if v]:
            os.environ["PBRT_DIRECT_LI_GRID"] = str(g)
            for nm, sc in (("readme", readme), ("readme_glass", glass)):
                res["grid_sweep"].append(step(f"grid {g} {nm}", args.limit, lambda: ray_rates(
                    f"{nm} {w}x{h} primary, PBRT_DIRECT_LI_GRID={g}", sc, w, h, args, with_li=False)))
        os.environ.pop("PBRT_DIRECT_LI_GRID", None)
    if not args.no_frames:
        res["frame"] = step("frames", 4 * args.limit, lambda: frames(readme, ns, args))
        res["frame_grid_sweep"] = []
        for g in [int(v) for v in args.frame_grids.split(",") if v]:
            os.environ["PBRT_DIRECT_LI_GRID"] = str(g)
            res["frame_grid_sweep"].append(step(f"frame grid {g}", args.limit, lambda: frames(readme, ns, args, True)))
        os.environ.pop("PBRT_DIRECT_LI_GRID", None)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print("done")


if __name__ == "__main__":
    main()

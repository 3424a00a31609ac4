"""Cost of stepping Path.Li one bounce at a time (pbrt_gpu_path_begin_device +
pbrt_gpu_path_step_device, k_path_step) against the one launch of pbrt_gpu_li_device (k_li).

The README scene at 1920x1080, one frame_samples range of the whole frame at one sample a
pixel (2 073 600 rays on the frame's own PCG32 streams), max_depth 10, Uniform lights,
buffers resident in DeviceBuffers. Three measurements, alternated within every repeat so
that a drift of the shared host lands on all of them, after --warmup untimed rounds:

  li        li_device: host wall time from the enqueue until pbrt_gpu_query_status returns
            (it synchronises the stream);
  stepped   path_begin + max_depth path_steps through ping-pong queues, enqueued back to
            back, wall time until query_status returns;
  per step  the same sequence with a query_status after begin and after every step: the
            time of each step alone (it includes one stream synchronisation), and the
            count of its out queue, the paths still alive.

Median, minimum and maximum over --repeats are reported. The stepped results are checked
against li_device's bits before anything is timed. Bytes: what a step must move for the
paths it advances, from the state's layout (path_query.h: 141 B a path) -- per advanced
path the gather of its state but the radiance sum, and its queue entry (121 B), the scatter of the stream, the
counters and the status (21 B), the radiance sum read and written where a term is added
(at most 48 B), and per surviving path the next ray, the throughput and the out-queue entry
(92 B) -- over the step's time, against the 8.0 TB/s HBM peak of the MI355X.

One GPU process; every stage runs under a time limit of its own (SIGALRM), and the process
ends at the first stage that fails or overruns.

    python tools/path_step_bench.py [--out profiles/path_step/path_step_bench.json] [--small]
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

HBM_PEAK = 8.0e12            # bytes / s (spec)
GATHER, SCATTER, L_RW, SURVIVOR = 121, 21, 48, 92   # bytes: see the module docstring
MAX_DEPTH = 10


class StageTimeout(Exception):
    pass


def stage(name, limit_s, fn):
    """fn() under a time limit of its own."""
    def fire(signum, frame):
        raise StageTimeout(f"stage '{name}' ran longer than {limit_s} s")
    signal.signal(signal.SIGALRM, fire)
    signal.alarm(limit_s)
    try:
        return fn()
    finally:
        signal.alarm(0)


def sync(r):
    rc, rec = r.query_status()
    assert rc == 0, (rc, rec.panics)


def spread(ts):
    return {"median_ms": float(np.median(ts)) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


def step_bytes(advanced, survivors):
    return advanced * (GATHER + SCATTER + L_RW) + survivors * SURVIVOR


def run(w, h, args):
    scene = G.Scene.readme(w, h)
    with G.Renderer(scene) as r:
        n = r.frame_count(1)
        sb = {k: r.buffer(n, G.SAMPLE_DTYPES[k]) for k in G.SAMPLE_REQUIRED}
        assert r.frame_samples(sb, 1) == 0, r.last_error()
        rb, gb = {k: sb[k] for k in G.RAY_KEYS}, {k: sb[k] for k in G.RNG_KEYS}
        ob = {k: r.buffer(n, dt) for k, dt in G.LI_DTYPES.items()}
        pb = r.path_buffers(n)
        qs = [r.path_queue(n), r.path_queue(n)]
        sync(r)

        def li():
            assert r.li_device(rb, gb, n, ob, max_depth=MAX_DEPTH) == 0, r.last_error()
            sync(r)

        def one_step(k):
            rc = r.path_step(pb, n, None if k == 0 else qs[k % 2], qs[(k + 1) % 2], max_depth=MAX_DEPTH)
            assert rc == 0, r.last_error()

        def stepped():
            assert r.path_begin(rb, gb, n, pb) == 0, r.last_error()
            for k in range(MAX_DEPTH):
                one_step(k)
            sync(r)

        def per_step():
            t0 = time.perf_counter()
            assert r.path_begin(rb, gb, n, pb) == 0, r.last_error()
            sync(r)
            ts, alive = [time.perf_counter() - t0], []
            for k in range(MAX_DEPTH):
                t0 = time.perf_counter()
                one_step(k)
                sync(r)
                ts.append(time.perf_counter() - t0)
                alive.append(int(qs[(k + 1) % 2]["count"].download()[0]))
            return ts, alive

        # the same bits, before anything is timed
        li()
        stepped()
        for a, o in (("lr", "r"), ("lg", "g"), ("lb", "b"), ("state", "state"), ("draws", "draws"), ("rays", "rays")):
            assert pb[a].download().tobytes() == ob[o].download().tobytes(), a
        for _ in range(args.warmup):
            li(), stepped(), per_step()
        t_li, t_st, t_ps, alive = [], [], [], None
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            li()
            t_li.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            stepped()
            t_st.append(time.perf_counter() - t0)
            ts, al = per_step()
            assert alive is None or al == alive   # the set is determined
            t_ps.append(ts)
            alive = al
        kernels = sorted({rec.name for rec in r.launches(outside=True) if rec.name.startswith(("k_li", "k_path"))})
        mean_closest = float((ob["rays"].download() & 0xFFFF).mean())
    t_ps = np.array(t_ps)
    advanced = [n] + alive[:-1]
    steps = []
    for k in range(MAX_DEPTH):
        s = spread(t_ps[:, k + 1].tolist())
        b = step_bytes(advanced[k], alive[k])
        t = s["median_ms"] * 1e-3
        steps.append({"step": k + 1, "advanced": advanced[k], "alive_after": alive[k], **s, "bytes": b,
                      "bytes_per_advanced_path": b / max(advanced[k], 1), "achieved_gb_per_s": b / t / 1e9,
                      "hbm_floor_ms": b / HBM_PEAK * 1e3, "share_of_hbm_peak": b / HBM_PEAK / t})
    li_s, st_s = spread(t_li), spread(t_st)
    return {"scene": f"readme {w}x{h}, frame_samples ns=1", "paths": n, "max_depth": MAX_DEPTH, "kernels": kernels,
            "mean_closest_rays": mean_closest, "li_device": li_s, "stepped_with_queues": st_s,
            "stepped_over_li": st_s["median_ms"] / li_s["median_ms"], "begin": spread(t_ps[:, 0].tolist()),
            "steps": steps, "sum_of_step_medians_ms": sum(s["median_ms"] for s in steps),
            "path_steps": int(sum(advanced)), "bytes_all_steps": int(sum(s["bytes"] for s in steps))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds the measurement may take")
    ap.add_argument("--small", action="store_true", help="a tiny frame (a functional check of the tool)")
    args = ap.parse_args()
    w, h = (1920, 1080) if not args.small else (64, 48)
    res = stage("path_step_bench", args.limit, lambda: run(w, h, args))
    res = {"what": "pbrt_gpu_li_device against path_begin + max_depth path_steps with ping-pong queues: host wall "
                   "time to the end of query_status, median / min / max over the repeats, alternated; per-step times "
                   "include one stream synchronisation each; bytes from the state layout against the 8.0 TB/s HBM peak",
           "build_id": G.build_id(), "warmup": args.warmup, "repeats": args.repeats, **res}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "steps"}))
    for s in res["steps"]:
        print(json.dumps(s))


if __name__ == "__main__":
    main()

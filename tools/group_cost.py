"""Cost of a device group (pbrt_gpu_group) against a plain context, config B
(README scene, 1920x1080, Stratified(8,8), Path(10)), in one process:

    python tools/group_cost.py [--devices 0] [--steps 8] [--warmup 3] [--stage]

One JSON line: the plain context's frame (render_async + synchronize, host wall
time, median of --steps after --warmup) and its merge_ms; the group's frame over
--devices (render_async + synchronize), its merge_ms, per-member kernel_ms,
total_ms (host wall time of the member's frame inside its worker thread; the
group's total_ms minus the slowest worker's sum is the cost of the threads and
the merge) and merge_ms; and whether the two films are bit-identical. --stage
sets PBRT_GROUP_STAGE=1 (the merge reads staging copies on the leader).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "go-pbrt_amd"))


def frames(start, wait, steps, warmup):
    wall, stats = [], None
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        start()
        stats = wait()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    return wall, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--devices", default="0", help="comma-separated HIP ordinals, e.g. 0,1 or 0,0,0")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stage", action="store_true")
    a = ap.parse_args()
    if a.stage:
        os.environ["PBRT_GROUP_STAGE"] = "1"
    import numpy as np

    import pbrtgpu as G
    from pbrtgpu import abi

    devices = [int(x) for x in a.devices.split(",")]
    scene = G.Scene.readme(1920, 1080)
    rd = abi.render_desc(8, 8)
    with G.Renderer(scene, device=devices[0]) as r:
        pw, pst = frames(lambda: r.render_async(rd), r.synchronize, a.steps, a.warmup)
        pfilm = r.film()
    with G.RendererGroup(scene, devices) as g:
        gw, gst = frames(lambda: g.render_async(rd), g.synchronize, a.steps, a.warmup)
        gfilm = g.film()
        members = [g.member_stats(i) for i in range(len(devices))]
    print(json.dumps({
        "config": "B", "devices": devices, "staged": bool(a.stage), "steps": a.steps, "warmup": a.warmup,
        "plain_frame_ms": statistics.median(pw), "plain_frame_ms_min_max": [min(pw), max(pw)],
        "plain_merge_ms": pst.merge_ms, "plain_kernel_ms": pst.kernel_ms,
        "group_frame_ms": statistics.median(gw), "group_frame_ms_min_max": [min(gw), max(gw)],
        "group_merge_ms": gst.merge_ms, "group_kernel_ms": gst.kernel_ms,
        "group_total_ms": gst.total_ms,
        "member_kernel_ms": [m.kernel_ms for m in members],
        "member_total_ms": [m.total_ms for m in members],   # each member's enqueue + synchronize, host wall time
        "member_merge_ms": [m.merge_ms for m in members],   # each member's own k_merge_film
        "member_tiles": [int(m.tiles_rendered) for m in members],
        "films_bit_identical": bool(np.array_equal(pfilm.view(np.uint64), gfilm.view(np.uint64))),
    }))


if __name__ == "__main__":
    main()

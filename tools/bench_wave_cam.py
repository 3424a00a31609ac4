"""Frame time of the camera-start wave route (kernel="wave_cam") on renders with
per-sample camera rays, timed as bench.py times a step: render_async_into a
device-resident film + synchronize per frame, warm-up frames first.

    python tools/bench_wave_cam.py --kernel wave_cam --mode exact      [--runs 3 --warmup 1]
    python tools/bench_wave_cam.py --kernel auto     --mode exact      # the serial kernel, for the ratio

The render is the README scene at 1920x1080, pbrt_random_sampler(64), Path(10).
Prints one JSON line: the timed frames (host wall clock, ms) and each frame's
kernels_ms / chain_ms / paths_ms from the device events. PBRT_GPU_LIB selects
another build of the library (e.g. the parent commit's, for kernel="auto").
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-pbrt_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", default="wave_cam", choices=["wave_cam", "auto", "serial"])
    ap.add_argument("--mode", default="exact", choices=["exact", "throughput"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--ns", type=int, default=64, help="RandomSampler(ns)")
    ap.add_argument("--max-depth", type=int, default=10)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    import torch

    import pbrtgpu as G
    from pbrtgpu import abi

    scene = G.Scene.readme(args.width, args.height)
    rd = abi.render_desc(max_depth=args.max_depth,
                         mode=abi.PBRT_MODE_THROUGHPUT if args.mode == "throughput" else abi.PBRT_MODE_EXACT)
    G.lib().pbrt_random_sampler(args.ns, C.byref(rd))
    dev = torch.device("cuda", 0)
    film = torch.zeros((args.height, args.width, 3), dtype=torch.float64, device=dev)
    frames = []
    with G.Renderer(scene, device=0, kernel=args.kernel) as r:
        torch.cuda.synchronize()

        def step():
            r.render_async(rd, film.data_ptr())
            return r.synchronize()

        for _ in range(args.warmup):
            step()
        for _ in range(args.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = step()
            ms = (time.perf_counter() - t0) * 1e3
            frames.append({"frame_ms": ms, "kernels_ms": st.kernel_ms, "chain_ms": st.chain_ms,
                           "paths_ms": st.paths_ms, "merge_ms": st.merge_ms, "kernel": int(st.kernel),
                           "paths": int(st.paths_traced), "schedule": r.schedule_source()})
    mean = sum(f["frame_ms"] for f in frames) / len(frames)
    print(json.dumps({"label": args.label, "kernel_request": args.kernel, "mode": args.mode,
                      "render": f"README {args.width}x{args.height}, RandomSampler({args.ns}), Path({args.max_depth})",
                      "library": os.environ.get("PBRT_GPU_LIB", "default"), "build_id": G.build_id(),
                      "mean_frame_ms": mean, "frames": frames}))


if __name__ == "__main__":
    main()

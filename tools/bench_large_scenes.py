"""Frame time of the wave routes on scenes beyond 16 lights and on scenes beyond 64
BVH nodes (Mirror / Glass / OrenNayar, and the camera-start route), timed as bench.py
times a step: render_async_into a device-resident film + synchronize per frame, warm-up
frames first.

    python tools/bench_large_scenes.py --workload a --mode throughput   [--runs 3 --warmup 1]
    python tools/bench_large_scenes.py --workload b
    python tools/bench_large_scenes.py --workload c --kernel wave_cam
    python tools/bench_large_scenes.py --workload d --kernel wave_cam   [--mode throughput]
    PBRT_GPU_LIB=<the parent commit's library> python tools/bench_large_scenes.py --workload b

Workloads, all at 1920x1080 with Path(10):
  a  tests/large_scenes.py crowd(n=60), four materials (121 BVH nodes), Stratified(8,8).
     Both modes run the wave pipeline (EXACT: the kX chain with the [64] stack).
     At this size the reference panics on it (Ld > 10 on an OrenNayar sphere): the
     frame is the reference's up to the panic and the JSON line carries the panic
     site; a frame that ends at a panic is no yardstick, use a3 for timings.
  a3 the same without OrenNayar (Matte, Mirror, Glass), which renders whole
  b  the README scene plus 16 point lights (20 lights), Stratified(8,8)
  c  the same scene under pbrt_random_sampler(64): per-sample camera rays
     (kernel wave_cam; auto and serial run the serial kernel)
  d  crowd(n=60), Matte (121 BVH nodes), under pbrt_random_sampler(64): the
     camera-start route's stack kernels (kernel wave_cam; auto and serial run the
     serial kernel)
Prints one JSON line: the timed frames (host wall clock, ms), each frame's
kernels_ms / chain_ms / paths_ms from the device events, st.kernel and the
frame's chain and path kernels from the launch log. PBRT_GPU_LIB selects another
build of the library (the parent commit's, for the yardstick).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-pbrt_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=["a", "a3", "b", "c", "d"])
    ap.add_argument("--kernel", default="auto", choices=["auto", "serial", "wave_ci", "wave_cam"])
    ap.add_argument("--mode", default="exact", choices=["exact", "throughput"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    import torch

    import pbrtgpu as G
    from large_scenes import crowd
    from pbrtgpu import abi
    from scenes import readme_lights_scene

    mode = abi.PBRT_MODE_THROUGHPUT if args.mode == "throughput" else abi.PBRT_MODE_EXACT
    w, h = args.width, args.height
    if args.workload == "a":
        scene, rd, what = crowd(w=w, h=h), abi.render_desc(8, 8, max_depth=10, mode=mode), "crowd(60), four materials"
    elif args.workload == "a3":
        scene, rd = crowd(w=w, h=h, kinds=("matte", "mirror", "glass")), abi.render_desc(8, 8, max_depth=10, mode=mode)
        what = "crowd(60), Matte / Mirror / Glass"
    elif args.workload == "b":
        scene, rd = readme_lights_scene(w, h, extra=16), abi.render_desc(8, 8, max_depth=10, mode=mode)
        what = "README + 16 point lights"
    elif args.workload == "c":
        scene, rd = readme_lights_scene(w, h, extra=16), abi.render_desc(max_depth=10, mode=mode)
        G.lib().pbrt_random_sampler(64, C.byref(rd))
        what = "README + 16 point lights, RandomSampler(64)"
    else:
        scene, rd = crowd(w=w, h=h, kinds=("matte",)), abi.render_desc(max_depth=10, mode=mode)
        G.lib().pbrt_random_sampler(64, C.byref(rd))
        what = "crowd(60), Matte, RandomSampler(64)"
    dev = torch.device("cuda", 0)
    film = torch.zeros((h, w, 3), dtype=torch.float64, device=dev)
    frames = []
    with G.Renderer(scene, device=0, kernel=args.kernel) as r:
        torch.cuda.synchronize()

        def step():
            r.render_async(rd, film.data_ptr())
            try:
                return r.synchronize()
            except G.PbrtError as e:   # the reference panics on this render: the frame ran up to the panic
                if e.code != abi.PBRT_E_REF_PANIC:
                    raise
                return e.stats

        for _ in range(args.warmup):
            step()
        for _ in range(args.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = step()
            ms = (time.perf_counter() - t0) * 1e3
            frames.append({"frame_ms": ms, "kernels_ms": st.kernel_ms, "chain_ms": st.chain_ms,
                           "paths_ms": st.paths_ms, "merge_ms": st.merge_ms, "kernel": int(st.kernel),
                           "paths": int(st.paths_traced), "schedule": r.schedule_source(),
                           "panic": [int(v) for v in (st.panic_kind, st.panic_tile, st.panic_pixel_x, st.panic_pixel_y,
                                                      st.panic_sample, st.panic_bounce)] if st.panic_kind else None})
        launched = sorted({rec.name for rec in r.launches()
                           if rec.name.startswith(("k_chain_", "k_paths_", "k_pw_s", "k_render_exact", "k_mb_", "k_cam_"))})
    ms = [f["frame_ms"] for f in frames]
    print(json.dumps({"label": args.label, "workload": args.workload, "kernel_request": args.kernel, "mode": args.mode,
                      "render": f"{what}, {w}x{h}, Path(10)", "nodes": int(scene.desc.n_nodes),
                      "lights": int(scene.desc.n_lights), "library": os.environ.get("PBRT_GPU_LIB", "default"),
                      "build_id": G.build_id(), "min_frame_ms": min(ms), "max_frame_ms": max(ms),
                      "mean_frame_ms": sum(ms) / len(ms), "kernels": launched, "frames": frames}))


if __name__ == "__main__":
    main()

"""The exact launch sequence of a frame on every route: which kernel, on which stream, in which order.

render.hip's frame stages (chain_stage and its four ways of issuing the
k_chain_ci launches, path_stage, enqueue_cam, launch_films) decide every launch on
the host. Each case renders two frames on one context (the cold frame, then the
learned one) and holds each frame's launch log, as ordered (kernel name, stream)
pairs, equal to a literal; every film is the oracle's bit for bit. The literals were
recorded from the build before the stages became functions
(profiles/enqueue_stages/launches_parent.json, tools/dump_launch_logs.py): nothing
here is derived from the code under test.

The stream choreography of a learned frame (render.hip, above overlap_arm):
  stream 0  the heavy chain launch of a split; the films and the merge
  stream 3  k_gate, then the light chain launch (an unsplit frame: its one chain launch)
  stream 2  the path stage in chunks of halving size, each behind a k_gate; without
            the overlap (PBRT_PATHS_OVERLAP=0, or the re-render after a k_gate stall)
            stream 2 runs the light chain launch and the paths follow on stream 0
"""
import numpy as np
import pytest

import kernel_cases as K
import oracle_lib as O
import pbrtgpu as G
from pbrtgpu import abi
from test_gpu_kernel_coverage import THREADS, bits, only_these_knobs, oracle_film

pytestmark = pytest.mark.gpu


def s0(*names):
    return [(n, 0) for n in names]


CI1, CI4 = "k_chain_ci<1, 0, false, 0, false, false>", "k_chain_ci<4, 0, false, 0, false, false>"
P8 = "k_paths_ci<8, false, false>"
PROBE = s0("k_wf_primary<false>", "k_tile_cost<false>", "k_bitonic_local", "k_order_of_keys")
FILMS = s0("k_film", "k_panic_reduce")
MERGE = s0("k_merge_film")
COLD = PROBE + s0(CI1, P8) + FILMS + MERGE          # the probe, one chain launch, the paths after it
CHUNKS = [("k_gate", 2), (P8, 2)] * 4               # 6 tiles in chunks of 3, 1, 1, 1 (PBRT_PATHS_OVERLAP=5 halvings at most)
SPLIT_OVERLAP = (s0("k_wf_primary<false>", CI4) + [("k_gate", 3), (CI1, 3)] + CHUNKS + FILMS + MERGE)
SPLIT_PLAIN = s0("k_wf_primary<false>", CI4) + [(CI1, 2)] + s0(P8) + FILMS + MERGE
PW_PASS = s0("k_pw_trace<false>", "k_pw_shade<false>", "k_pw_shadow<false>")
STACK = (s0("k_chain_ci<1, 64, false, 0, false, false>", "k_pw_cache<false>", "k_pw_start<false, false>") + PW_PASS * 9 +
         s0("k_pw_panics") + FILMS + MERGE)
CAM = s0("k_chain_cam", "k_paths_cam<64, false>", "k_film_cam<false>", "k_panic_reduce")
ONE_TILE = {"PBRT_WAVE_BUFFER_GB": "0.000001"}      # below one tile's records: one tile per batch

# name -> (row of kernel_cases.CASES, knobs on top of the row's, [frame 0, frame 1], overlap slots of frame 1)
CASES = {
    # the probe frame, then the unsplit frame with the completion-driven path stage: the chain on stream 3
    "ci_w1_eu3": ("ci_w1_eu3", {}, [COLD, s0("k_wf_primary<false>") + [(CI1, 3)] + CHUNKS + FILMS + MERGE], 6),
    "split_heavy4": ("split_heavy4", {}, [COLD, SPLIT_OVERLAP], 6),
    "split_heavy4_no_overlap": ("split_heavy4", {"PBRT_PATHS_OVERLAP": "0"}, [COLD, SPLIT_PLAIN], 0),
    # the light launch waits for the path stage: k_gate stalls, and the logged frame is the re-render
    "split_heavy4_gate_hold": ("split_heavy4", {"PBRT_GATE_HOLD": "1"}, [COLD, SPLIT_PLAIN], 0),
    "tp_p8": ("tp_p8", {}, [s0("k_mb_setup<false>", "k_paths_ci<8, true, false>") + FILMS + MERGE] * 2, 0),
    "dl_matte": ("dl_matte", {}, [s0("k_wf_primary<false>", "k_dl_setup", "k_dl_samples<false>", "k_dl_panics") +
                                  FILMS + MERGE] * 2, 0),
    "cam_p64": ("cam_p64", {}, [CAM + MERGE] * 2, 0),
    # the path wavefront: trace, shade, shadow once per bounce after the first (max_depth - 1 = 9)
    "stack_w1_eu3": ("stack_w1_eu3", {}, [PROBE + STACK, s0("k_wf_primary<false>") + STACK], 0),
    "serial_occ1": ("serial_occ1", {}, [s0("k_render_exact<1>") + MERGE] * 2, 0),
}
# a frame of two batches (32x16: two tiles, one per batch): the per-batch sequence repeats, every
# chain launch runs in launch order (no probe, no learned order), one tile at 4 waves
BATCHES = {
    "batches_chain": ({}, K.S22, (s0("k_wf_primary<false>", CI4, P8) + FILMS) * 2 + MERGE, abi.PBRT_KERNEL_WAVE_CI),
    "batches_cam": (dict(kernel="wave_cam"), dict(K.S22, **K.NOSAMP), CAM * 2 + MERGE, abi.PBRT_KERNEL_WAVE_CAM),
}


def sequence(log):
    return [(rec.name, rec.stream) for rec in log]


def test_the_wavefront_passes_are_the_bounces():
    assert K.make_rd(K.CASES["stack_w1_eu3"]).max_depth - 1 == 9
    assert len(CHUNKS) // 2 <= 5   # Knobs::paths_overlap


@pytest.mark.parametrize("name", list(CASES))
def test_frame_sequence(name, monkeypatch):
    row, env, want, overlap_slots = CASES[name]
    case = K.CASES[row]
    only_these_knobs(monkeypatch, dict(case.env, **env))
    ofilm, opaths = oracle_film(case.scene, tuple(sorted(case.rd.items())))
    with G.Renderer(K.SCENES[case.scene](), **case.opts) as r:
        for frame in range(2):
            film, st = r.render(K.make_rd(case))
            got = sequence(r.launches())
            print(f"{name} frame {frame}: {got}")
            assert st.kernel == case.family and st.paths_traced == opaths, (frame, st.kernel, st.paths_traced)
            assert np.array_equal(bits(film), bits(ofilm)), (frame, int((film != ofilm).sum()))
            assert got == want[frame], frame
        assert r.launch_overflow == 0 and r.overlap_slots() == overlap_slots


@pytest.mark.parametrize("name", list(BATCHES))
def test_two_batches(name, monkeypatch):
    opts, rd_args, want, family = BATCHES[name]
    only_these_knobs(monkeypatch, ONE_TILE)
    scene = G.Scene.readme(32, 16)
    rc, ofilm, ost = O.render(scene.desc, abi.render_desc(**rd_args), threads=THREADS)
    assert rc == 0 and ofilm.max() > 0
    opaths = ost.paths
    with G.Renderer(scene, **opts) as r:
        for frame in range(2):
            film, st = r.render(abi.render_desc(**rd_args))
            got = sequence(r.launches())
            print(f"{name} frame {frame}: {got}")
            assert st.kernel == family and st.batches == 2 and st.paths_traced == opaths, (frame, st.kernel, st.batches)
            assert np.array_equal(bits(film), bits(ofilm)), (frame, int((film != ofilm).sum()))
            assert got == want, frame
            assert r.schedule_source() == "launch order" and r.overlap_slots() == 0, frame

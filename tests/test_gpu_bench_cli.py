"""bench.py's command line on the GPU: a plain run and --dump-outputs.

One small run of the benchmark itself (config B's scene at 96x64,
Stratified(2,2), 2 timed steps): the result line carries the headline fields
and ms_per_step for the steps asked for, the legs that belong to --full are
absent, and DIR/film.npy is the film of the last timed EXACT frame: bit for
bit the oracle's.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from pbrtgpu import abi

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, S = 96, 64, 2


def test_plain_run_result_line_and_dumped_film(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--width", str(W), "--height", str(H), "--spp", str(S), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["unit"] == "Mpaths/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert res["steps"] == 2 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["metric"]
    paths = W * H * (S * S - 1)
    assert res["config"]["paths_per_frame"] == paths
    # value is the timed steps' paths over their time
    assert res["value"] == pytest.approx(paths / (res["ms_per_step"] * 1e-3) / 1e6, rel=1e-9)
    assert r.stderr.count("] exact step ") == 2 and r.stderr.count("] exact warmup ") == 1
    assert not {"side_mode", "rpc", "cpu_baseline"} & set(res)
    assert os.listdir(out) == ["film.npy"]
    film = np.load(out / "film.npy")
    assert film.dtype == np.float64 and film.shape == (H, W, 3)
    sc = O.OracleScene.readme(W, H)
    rc, ofilm, ost = O.render(sc.desc, abi.render_desc(S, S, max_depth=10), threads=4)
    assert rc == 0 and ost.paths == paths
    assert np.array_equal(film.view(np.uint64), ofilm.view(np.uint64))

"""pbrtgpu.hip_runtimes() and the message of a failed create.

A torch wheel for ROCm carries its own copy of the HIP runtime. Whether a
process ends up with one runtime or two depends on what is loaded first
(INTEGRATION.md section 4), so each case runs in a fresh child interpreter.
Loading the libraries needs no GPU and no case touches one: the failing create
is a stand-in that returns PBRT_E_HIP, as the real one does when its runtime
finds no device."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = "import sys, json; sys.path.insert(0, %r)\n" % os.path.join(REPO, "go-pbrt_amd")
REPORT = """
import pbrtgpu as G
from pbrtgpu import abi
scene = G.Scene.readme(16, 16)
real = G.lib().pbrt_gpu_create
out = {"runtimes": G.hip_runtimes(), "torch": "torch" in sys.modules}
for code in (abi.PBRT_E_HIP, abi.PBRT_E_INVALID):
    G.lib().pbrt_gpu_create = lambda *a, code=code: code
    try:
        G.Renderer(scene)
        out[str(code)] = None
    except G.PbrtError as e:
        out[str(code)] = [e.code, str(e)]
G.lib().pbrt_gpu_create = real
real = G.lib().pbrt_gpu_group_create
G.lib().pbrt_gpu_group_create = lambda *a: abi.PBRT_E_HIP
try:
    G.RendererGroup(scene, [0, 0])
    out["group"] = None
except G.PbrtError as e:
    out["group"] = [e.code, str(e)]
G.lib().pbrt_gpu_group_create = real
print(json.dumps(out))
"""


def child(order):
    first = {"library_only": "import pbrtgpu; pbrtgpu.lib()\n",
             "library_then_torch": "import pbrtgpu; pbrtgpu.lib()\nimport torch\n",
             "torch_then_library": "import torch\nimport pbrtgpu; pbrtgpu.lib()\n"}[order]
    run = subprocess.run([sys.executable, "-c", PRELUDE + first + REPORT], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    return json.loads(run.stdout.strip().splitlines()[-1])


def test_library_alone_maps_one_runtime():
    out = child("library_only")
    assert not out["torch"] and len(out["runtimes"]) == 1
    assert "libamdhip64" in os.path.basename(out["runtimes"][0])
    code, msg = out["2"]
    assert code == 2 and "no GPU visible" in msg and "HIP runtimes" not in msg
    code, msg = out["group"]
    assert code == 2 and "no GPU visible" in msg and "HIP runtimes" not in msg


def test_library_before_torch_maps_two_and_create_says_so():
    out = child("library_then_torch")
    rts = out["runtimes"]
    assert out["torch"] and len(rts) == 2 and len({os.path.realpath(p) for p in rts}) == 2
    assert any(os.sep + "torch" + os.sep in p for p in rts)
    code, msg = out["2"]
    assert code == 2 and "2 HIP runtimes" in msg and "import torch before" in msg
    assert all(p in msg for p in rts)
    code, msg = out["group"]
    assert code == 2 and "pbrt_gpu_group_create" in msg and "2 HIP runtimes" in msg
    # another status is not blamed on the runtimes
    code, msg = out["1"]
    assert code == 1 and "HIP runtimes" not in msg and "no GPU visible" not in msg


def test_torch_before_library_shares_torchs_runtime():
    out = child("torch_then_library")
    assert out["torch"] and len(out["runtimes"]) == 1
    assert os.sep + "torch" + os.sep in out["runtimes"][0]
    code, msg = out["2"]
    assert code == 2 and "no GPU visible" in msg and "HIP runtimes" not in msg

"""Register and scratch budget of the one-wave Matte k_chain_ci kernels.

csrc/k_chain_1.hip is compiled device-only to assembly with the Makefile's
FLAGS (read from the Makefile, not repeated here), and the kernels' resource
metadata is read through tools/kernel_resources.py. Metadata only: no
instruction is looked at.

k_chain_ci<1, 0, false, 0, false> (config B's light tiles, built for 3
waves/SIMD) had 168 VGPRs and 128 B/lane of scratch while the tile's state was
per-lane; with one tile per wave a compile-time fact and the group's state in
scalar registers it has 44, and with the trajectory's start state written to
its ring entry at issue and no per-lane pixel index 32 (BOUND below, what the
final kernel reached: the BSDF's reflectance across one bounce's draws and
one dword of the cursor, stored and loaded once per bounce, no longer per
traversal step). The 2-waves/SIMD builds stay free of scratch.
"""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMD = os.path.join(REPO, "go-pbrt_amd")

BOUND = 32   # B/lane (the parent: 128; one tile per wave and scalar group state alone: 44)


def makefile_var(name):
    text = open(os.path.join(AMD, "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M)
    assert m, name
    return m.group(1).split()


def find_hipcc():
    cand = makefile_var("HIPCC")[0]
    return cand if os.access(cand, os.X_OK) else shutil.which("hipcc")


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    hipcc = find_hipcc()
    if not hipcc:
        pytest.skip("no hipcc")
    asm = str(tmp_path_factory.mktemp("asm") / "k_chain_1.s")
    subprocess.run([hipcc, "--offload-arch=" + makefile_var("ARCH")[0], *makefile_var("FLAGS"), "--cuda-device-only",
                    "-S", "-o", asm, os.path.join(AMD, "csrc", "k_chain_1.hip")], check=True, cwd=AMD)
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), asm, "k_chain_ci"],
                         check=True, capture_output=True, text=True).stdout
    return json.loads(out)


def kernel(resources, targs):
    hits = [v for k, v in resources.items() if k.endswith("<" + targs + ">")]
    assert len(hits) == 1, (targs, sorted(resources))
    return hits[0]


def test_three_wave_matte_chain_fits_its_registers(resources):
    k = kernel(resources, "1, 0, false, 0, false, false")
    print(k)
    assert k["arch_vgpr"] <= 168
    assert k["waves_per_simd_by_registers"] >= 3
    assert k["scratch_bytes_per_lane"] <= BOUND


def test_two_wave_build_has_no_scratch(resources):
    for targs in ("1, 0, false, 2, false, false", "1, 64, false, 2, false, false", "1, 0, false, 2, true, false"):
        k = kernel(resources, targs)
        print(targs, k)
        assert k["scratch_bytes_per_lane"] == 0

"""The PCG32 jump tables and helpers of the chain kernel's issue step on the host:
go-pbrt_amd/csrc/pcg_jump.h, built as a stand-alone program under ASan + UBSan
(tests/pcg_steps_check.cpp). Everything is integer arithmetic mod 2^64, so every
comparison is exact:

- step[k] (k = 0..127) and mid[j] (128 j steps) against literal LCG steps, over
  300 random (state, odd inc) pairs;
- pcg_advance_near == pcg_advance == literal steps for n in {0, 1, 126, 127, 128,
  129, 255, 1023, 1024, 1025, 2^20 + 3, random}, and the two helpers against
  each other for random 64-bit n;
- the state k_chain_ci carries at `nxt`: 8 x 4000 random "issue cs * m
  candidates" and "reset to the head, d draws past a walked entry" updates (d
  above 127 included), each followed by a comparison with pcg_advance from the
  origin, and the lanes' table steps from their wave's base;
- pcg_skip(k) against k literal steps, k = 0..5.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pcg_step_tables_and_carried_state(tmp_path):
    exe = tmp_path / "psc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-o", str(exe), os.path.join(REPO, "tests", "pcg_steps_check.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert [ln.split()[:2] for ln in lines] == [["ok", "tables"], ["ok", "advance_near"], ["ok", "carried"], ["ok", "skip"]]
    carried = lines[2].split()
    assert int(carried[2]) >= 8 * 4000
    # both paths of the reset and the generic path of the issue were compared
    assert int(carried[4]) >= 50 and int(carried[6]) >= 50 and int(carried[8]) >= 1
    assert int(lines[3].split()[2]) == 300 * 6

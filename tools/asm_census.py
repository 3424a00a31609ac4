"""Census of a kernel's fp64 divisions and inlined Go-math polynomials, by source
line, from device assembly with line tables:

    make -C go-pbrt_amd asm FLAGS="<Makefile FLAGS> -gline-tables-only"
    python tools/asm_census.py go-pbrt_amd/build/asm/k_chain_1.s "k_chain_ci<1, 0, false, 0, false, false>" \
        > profiles/<dir>/census_<name>.json

Every instruction is attributed to the `.loc file line col` in force where it
stands (the innermost inlined callee's own line). Per kernel:
  valu_static     v_* instructions
  div_f64_sites   v_div_fmas_f64 (one per fp64 division expansion) by "file:line"
  inlined_copies  xatan: divisions on xatan's lines of csrc/gomath.h; sin_poly,
                  cos_poly: v_mul_f64 at the polynomial's leading product (the
                  `*` after its first coefficient), one per inlined copy
The lines are found in go-pbrt_amd/csrc/gomath.h as it stands beside the
assembly (--gomath to name another copy, as for a parent build).
"""
import argparse
import collections
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import demangle_short  # noqa: E402

LEAD = {"sin_poly": "1.58962301576546568060e-10 *", "cos_poly": "-1.13585365213876817300e-11 *"}


def gomath_marks(path):
    src = open(path).read().split("\n")
    marks = {}
    for name, lit in LEAD.items():
        (ln,) = [i for i, s in enumerate(src) if lit in s]
        marks[name] = (ln + 1, src[ln].index(lit) + len(lit))   # 1-based line, column of the `*`
    start = next(i for i, s in enumerate(src) if "double xatan(" in s)
    end = next(i for i in range(start, len(src)) if src[i].startswith("}"))
    marks["xatan"] = (start + 1, end + 1)
    return marks


def census(asm, wanted, marks):
    files, out = {}, {}
    name, cur, loc = None, None, None
    for line in open(asm):
        m = re.match(r"\s+\.file\s+(\d+) \"[^\"]*\" \"([^\"]+)\"", line)
        if m:
            files[m.group(1)] = os.path.basename(m.group(2))
            continue
        m = re.match(r"(_Z\w+):", line)
        if m:
            n = demangle_short(m.group(1))
            name = n if n in wanted else None
            if name:
                cur = out[name] = {"valu_static": 0, "div_f64_sites": collections.Counter(),
                                   "inlined_copies": dict.fromkeys(("xatan", "sin_poly", "cos_poly"), 0)}
            continue
        if name is None:
            continue
        if re.match(r"\.Lfunc_end", line):
            name = None
            continue
        m = re.match(r"\s+\.loc\s+(\d+) (\d+) (\d+)", line)
        if m:
            loc = (files.get(m.group(1), m.group(1)), int(m.group(2)), int(m.group(3)))
            continue
        m = re.match(r"\s+(v_\w+)", line)
        if not m or loc is None:
            continue
        op = m.group(1)
        cur["valu_static"] += 1
        in_gomath = loc[0] == "gomath.h"
        if op.startswith("v_div_fmas_f64"):
            cur["div_f64_sites"]["%s:%d" % loc[:2]] += 1
            if in_gomath and marks["xatan"][0] <= loc[1] <= marks["xatan"][1]:
                cur["inlined_copies"]["xatan"] += 1
        if op.startswith("v_mul_f64") and in_gomath:
            for poly in LEAD:
                if loc[1:] == marks[poly]:
                    cur["inlined_copies"][poly] += 1
    for v in out.values():
        v["div_f64_total"] = sum(v["div_f64_sites"].values())
        v["div_f64_sites"] = dict(sorted(v["div_f64_sites"].items(),
                                         key=lambda kv: (kv[0].split(":")[0], int(kv[0].split(":")[1]))))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("kernels", nargs="+", help="names as tools/kernel_resources.py prints them")
    ap.add_argument("--gomath", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                     "go-pbrt_amd", "csrc", "gomath.h"))
    a = ap.parse_args()
    res = census(a.asm, set(a.kernels), gomath_marks(a.gomath))
    missing = set(a.kernels) - set(res)
    if missing:
        sys.exit("not in %s: %s" % (a.asm, sorted(missing)))
    json.dump(res, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()

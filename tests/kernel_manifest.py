"""The manifest of the device kernels libpbrt_gpu.so compiles, read from the sources.

render_kernels.h only declares the kernels, so a template kernel links only if a
unit instantiates it explicitly, and every such line spells all its arguments.
The manifest is therefore:
- every `template __global__ void NAME<...>(` line (an explicit instantiation),
- every non-template `__global__` definition,
over the units the Makefile's default target builds (SRC), with the default
build's preprocessor conditions applied. Names are canonical: the template name
with every argument, ", " between arguments, no namespace, no parameter list:
`k_chain_ci<1, 0, false, 0, false, false>`; the spelling of the launch log
(pbrt_gpu_launch_log) and of tools/kernel_resources.py. Nothing is generated
or cached: every caller derives the manifest from the tree.
"""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMD = os.path.join(REPO, "go-pbrt_amd")

# Macros the default build leaves at their default (the Makefile passes only
# -DPBRT_BUILD_ID); `#if NAME` on any other name is an error here, so that a new
# conditional around a kernel cannot silently drop it from the manifest.
DEFAULT_MACROS = {"PBRT_MESH_WIDE": 0}   # csrc/pbrt_mesh.h


def makefile_units(makefile=os.path.join(AMD, "Makefile")):
    """The .hip units of the Makefile's SRC (with KSRC expanded), as absolute paths."""
    text = open(makefile).read().replace("\\\n", " ")
    var = {}
    for m in re.finditer(r"^(\w+)\s*:?=\s*(.*)$", text, re.M):
        var[m.group(1)] = m.group(2)

    def expand(v):
        return re.sub(r"\$\((\w+)\)", lambda m: expand(var.get(m.group(1), "")), v)

    units = [u for u in expand(var["SRC"]).split() if u.endswith(".hip")]
    assert units, "no units in the Makefile's SRC"
    return [os.path.join(AMD, u) for u in units]


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def preprocess(text, macros=DEFAULT_MACROS):
    """The lines of `text` the default build compiles (conditionals only; no expansion)."""
    out, stack = [], []   # stack of (taken_now, any_branch_taken, parent_active)
    for line in text.split("\n"):
        m = re.match(r"\s*#\s*(ifdef|ifndef|if|elif|else|endif)\b(.*)", line)
        active = all(t for t, _, _ in stack)
        if not m:
            out.append(line if active else "")
            continue
        kind, arg = m.group(1), m.group(2).strip()
        if kind in ("ifdef", "ifndef", "if"):
            if kind == "ifdef":
                cond = arg in macros
            elif kind == "ifndef":
                cond = arg not in macros
            else:
                mm = re.fullmatch(r"(!?)\s*(\w+)", arg)
                if not mm or mm.group(2) not in macros:
                    raise ValueError(f"kernel_manifest: cannot evaluate '#if {arg}' (add the macro to DEFAULT_MACROS)")
                cond = bool(macros[mm.group(2)]) != bool(mm.group(1))
            stack.append((cond, cond, active))
        elif kind == "else":
            _, anyt, par = stack.pop()
            stack.append((not anyt, True, par))
        elif kind == "elif":
            raise ValueError("kernel_manifest: #elif is not handled")
        else:
            stack.pop()
        out.append("")
    assert not stack, "unbalanced preprocessor conditionals"
    return "\n".join(out)


def canonical(name, args=None):
    if args is None:
        return name
    return name + "<" + ", ".join(a.strip() for a in args.split(",")) + ">"


def unit_kernels(path):
    """(explicit instantiations, non-template definitions) of one unit, canonical names."""
    text = preprocess(strip_comments(open(path).read()))
    inst, plain = [], []
    for m in re.finditer(r"\b__global__\b", text):
        before = text[:m.start()].rstrip()
        after = text[m.end():]
        if re.search(r"\btemplate$", before):   # `template __global__ void NAME<...>(`: explicit instantiation
            mm = re.match(r"\s*void\s+(\w+)\s*<([^>]*)>\s*\(", after)
            assert mm, f"{path}: unreadable explicit instantiation near offset {m.start()}"
            inst.append(canonical(mm.group(1), mm.group(2)))
            continue
        if re.search(r"\btemplate\s*<[^;{}]*>$", before):   # a template's definition or declaration
            continue
        mm = re.match(r"(?:\s*__launch_bounds__\s*\([^)]*\)|\s*__attribute__\s*\(\(.*?\)\)\))*\s*void\s+(\w+)\s*\(", after,
                      flags=re.S)
        assert mm, f"{path}: unreadable __global__ function near offset {m.start()}"
        depth, i = 1, mm.end()
        while depth:   # to the end of the parameter list
            depth += {"(": 1, ")": -1}.get(after[i], 0)
            i += 1
        if after[i:].lstrip().startswith("{"):   # a definition (a declaration ends in ';')
            plain.append(mm.group(1))
    return inst, plain


def manifest():
    """{canonical kernel name: unit file name} of every kernel the default build compiles."""
    out = {}
    for path in makefile_units():
        inst, plain = unit_kernels(path)
        for k in inst + plain:
            assert k not in out, f"{k} compiled twice: {out[k]} and {os.path.basename(path)}"
            out[k] = os.path.basename(path)
    return out


if __name__ == "__main__":
    for k, u in sorted(manifest().items()):
        print(f"{u:16s} {k}")

"""Checks on a context's launch log (Renderer.launches(), pbrt_gpu_launch_log),
shared by the coverage test and the chain tests that name an instantiation."""
import re

# kernels launched as one wave of 64 lanes per workgroup (dim3(kWave) at their launch sites)
ONE_WAVE = {"k_paths_ci", "k_paths_cam", "k_chain_cam", "k_cam_setup", "k_mb_setup", "k_wf_primary", "k_dl_setup",
            "k_dl_samples", "k_tile_cost", "k_gate", "k_render_exact", "k_intersect", "k_pw_cache", "k_pw_start",
            "k_pw_trace", "k_pw_shade", "k_pw_shadow"}


def names(launches):
    return {rec.name for rec in launches}


def check_invariants(launches, lds_per_block, overflow=0):
    """What must hold for every record of a log:
    - the name resolved, and so did the kernel's attributes;
    - the grid is positive;
    - k_chain_ci<kW, ...> runs 64 * kW lanes per workgroup, the one-wave kernels 64;
    - dynamic plus static LDS is within the device's limit per workgroup."""
    assert overflow == 0, f"the log overflowed by {overflow} records"
    for rec in launches:
        assert rec.name != "?", rec
        assert all(g >= 1 for g in rec.grid) and all(b >= 1 for b in rec.block), rec
        assert rec.stream in (0, 2, 3), rec
        base = rec.name.split("<")[0]
        if base == "k_chain_ci":
            kw = int(re.match(r"k_chain_ci<(\d+),", rec.name).group(1))
            assert rec.block == (64 * kw, 1, 1), rec
        elif base in ONE_WAVE:
            assert rec.block == (64, 1, 1), rec
        assert rec.lds_static != 0xFFFFFFFF, ("hipFuncGetAttributes failed", rec)
        assert rec.lds + rec.lds_static <= lds_per_block, (rec, rec.lds_static, lds_per_block)


def chain(kw, depth=0, kx=False, eu=0, spwin=False, multi=False):
    """k_chain_ci<kW, kDepth, kX, kEu, kSpWin, kMulti> as the log spells it. eu=None leaves
    the register build open ("[02]": where ci_eu3_fits decides it from the device's LDS),
    which makes the result a pattern for assert_chain."""
    b = lambda v: "true" if v else "false"   # noqa: E731
    return f"k_chain_ci<{kw}, {depth}, {b(kx)}, {'[02]' if eu is None else eu}, {b(spwin)}, {b(multi)}>"


def assert_chain(launches, pattern, what=""):
    """The frames launched the k_chain_ci instantiation `pattern` names (a regular expression
    over the canonical name; chain() builds it). A learned frame may add the heavy tiles'
    instantiation beside it, so other chain launches are allowed."""
    got = sorted(n for n in names(launches) if n.startswith("k_chain_ci<"))
    assert any(re.fullmatch(pattern, n) for n in got), f"{what}: k_chain_ci launches {got}, expected {pattern}"


def assert_launched(launches, expected, what=""):
    """Every kernel of `expected` is in the log."""
    missing = sorted(set(expected) - names(launches))
    assert not missing, f"{what}: not launched: {missing}; the log has {sorted(names(launches))}"

"""The kernel selectors (kernel_select.hip) against the manifest of compiled kernels. No GPU.

Every launch of a templated family takes its kernel from one host function
(chain_kernel, paths_ci_kernel, paths_cam_kernel, serial_kernel), which returns
the instantiation with exactly the arguments asked for, or nothing. Each test
sweeps a family's whole argument domain through pbrt_diag_kernel_choice: the
answers are exactly the family's compiled kernels (tests/kernel_manifest.py),
each spelled with the very arguments of the question. So an instantiation that
is compiled but cannot be selected fails here, one that can be selected but is
not compiled fails here, and no question is answered with a neighbouring
instantiation (<8, 0, true, ...> is nothing, not <4, 0, true, ...>).
"""
import itertools

import kernel_manifest as M
import pbrtgpu as G

MANIFEST = M.manifest()
BOOL = (False, True)


def tf(b):
    return "true" if b else "false"


def family(*prefixes):
    return {k for k in MANIFEST if k.startswith(prefixes)}


def sweep(fam, domain, spell):
    """{question: answer} of the selector over `domain`; every answer is the question's own spelling."""
    chosen = {}
    for q in domain:
        got = G.kernel_choice(fam, *q)
        if got is not None:
            assert got == spell(*q), (q, got)
            chosen[q] = got
    return chosen


def test_chain_kernels():
    domain = list(itertools.product((1, 2, 4, 8), (-1, 0, 64), BOOL, (0, 2), BOOL, BOOL))
    assert len(domain) == 192
    chosen = sweep("k_chain_ci", domain,
                   lambda w, d, kx, eu, sw, mu: f"k_chain_ci<{w}, {d}, {tf(kx)}, {eu}, {tf(sw)}, {tf(mu)}>")
    want = family("k_chain_ci<")
    assert len(want) == 32
    assert set(chosen.values()) == want, (sorted(want - set(chosen.values())), sorted(set(chosen.values()) - want))
    assert len(chosen) == 32
    assert G.kernel_choice("k_chain_ci", 8, 0, True, 0, False, False) is None   # kX runs 4 waves at most
    assert G.kernel_choice("k_chain_ci", 3, 0, False, 0, False, False) is None
    assert G.kernel_choice("k_chain_ci", 1, 0, False, 3, False, False) is None   # eu 3 is the default build, 0


def test_paths_ci_kernels():
    domain = list(itertools.product((2, 4, 8), BOOL, BOOL))
    chosen = sweep("k_paths_ci", domain, lambda p, mb, kx: f"k_paths_ci<{p}, {tf(mb)}, {tf(kx)}>")
    want = family("k_paths_ci<")
    assert len(want) == 10 and set(chosen.values()) == want and len(chosen) == 10
    for mb in BOOL:   # kX: 4 or 8 pixels per wave
        assert (2, mb, True) not in chosen
    assert G.kernel_choice("k_paths_ci", 16, False, False) is None


def test_paths_cam_kernels():
    domain = list(itertools.product((4, 16, 64), BOOL, BOOL))
    chosen = sweep("k_paths_cam", domain,
                   lambda p, mb, stack: f"k_paths_cam{'_stack' if stack else ''}<{p}, {tf(mb)}>")
    want = family("k_paths_cam<", "k_paths_cam_stack<")
    assert len(want) == 12 and set(chosen.values()) == want and len(chosen) == 12
    assert G.kernel_choice("k_paths_cam", 8, False, False) is None


def test_serial_kernels():
    chosen = sweep("k_render_exact", [(n,) for n in range(0, 17)], lambda n: f"k_render_exact<{n}>")
    want = family("k_render_exact<")
    assert len(want) == 4 and set(chosen.values()) == want and set(chosen) == {(1,), (2,), (4,), (8,)}


def test_unknown_family_or_argument_count():
    assert G.kernel_choice("k_film") is None
    assert G.kernel_choice("k_chain_ci", 1, 0, False, 0, False) is None
    assert G.kernel_choice("k_render_exact", 1, 2) is None


def test_the_selected_names_are_log_names():
    """The selectors' answers are names the launch log produces (one table names both)."""
    names = set(G.kernel_names())
    assert family("k_chain_ci<", "k_paths_ci<", "k_paths_cam", "k_render_exact<") <= names

"""The caller-ray families of tests/li_rays.py on the oracle alone (no GPU), so that
tests/test_gpu_li_rays.py cannot pass vacuously: each family contains what it names, the counts
are pinned, and outside the families made to panic the rows the device test compares in full are
at least 99 % of a family.

What the reference makes of these rays (oracle_path_li restates path.go and reflection.go):

- wo := ray.Direction goes unnormalised into the BSDF (SURVEY #8). A first hit on Matte or Mirror
  does not notice; on OrenNayar the sines are taken of an unnormalised vector and L changes; on
  smooth Glass the Fresnel term reads |wo.z| as a cosine, so a direction of another length picks
  reflection or transmission differently: there even the 2^k copies of a ray, whose hit point is
  the ray's bit for bit, draw another number of values. The draws and ray counts of the 2^k copies
  equal the ray's on every first hit that is not Glass.
- UniformSampleOneLight panics on Ld > 10 for some first hits of the scenes with the area light
  (diffuse.go's wi is unnormalised too, SURVEY #12): a few rows of axis, poles and sweeps.
"""
import numpy as np
import pytest

import adversarial_rays as A
import li_rays as LR
import oracle_lib as O
from pbrtgpu import abi

KEYS = list(LR.SCENES)
UNCAPPED = ("huge", "degenerate")
CAP = 0.01

# (rays, first-ray hits, paths of >= 2 iterations, paths that ran iteration 4 (Russian roulette applies), panics, rows whose L has a NaN,
#  distinct draw counts) of oracle_path_li at max_depth 5
PINNED = {
    "small": {
        "axis": (5592, 1335, 1285, 412, 1, 0, 6),
        "poles": (1120, 960, 954, 257, 0, 0, 6),
        "disk_plane": (255, 87, 87, 27, 0, 0, 6),
        "inside": (384, 308, 306, 62, 0, 0, 6),
        "sweeps": (1095, 410, 402, 78, 0, 0, 6),
        "huge": (4032, 1857, 1134, 334, 1570, 684, 6),
        "degenerate": (705, 201, 104, 26, 217, 96, 6),
        "random": (2000, 48, 48, 7, 0, 0, 5),
        "scaled": (240, 240, 240, 25, 0, 0, 5),
        "tmax": (228, 46, 46, 3, 0, 0, 4),
        "secondary": (304, 144, 144, 29, 0, 0, 6),
        "state": (250, 93, 65, 117, 0, 0, 7),
    },
    "large": {
        "axis": (11676, 4364, 4297, 1516, 0, 0, 6),
        "poles": (4320, 4160, 4141, 1101, 0, 0, 6),
        "disk_plane": (493, 149, 148, 57, 0, 0, 6),
        "inside": (1344, 1268, 1259, 228, 0, 0, 6),
        "sweeps": (3600, 1226, 1215, 340, 0, 0, 6),
        "huge": (4536, 2170, 1177, 356, 1618, 840, 6),
        "degenerate": (769, 224, 103, 27, 220, 119, 6),
        "random": (2000, 35, 35, 12, 0, 0, 6),
        "scaled": (240, 240, 240, 40, 0, 0, 5),
        "tmax": (228, 42, 42, 8, 0, 0, 3),
        "secondary": (300, 166, 165, 24, 0, 0, 6),
        "state": (250, 89, 61, 116, 0, 0, 7),
    },
    "small_kx": {
        "axis": (5592, 1333, 1289, 350, 22, 0, 13),
        "poles": (1120, 960, 956, 295, 0, 0, 13),
        "disk_plane": (255, 87, 87, 33, 0, 0, 9),
        "inside": (384, 308, 308, 48, 0, 0, 10),
        "sweeps": (1095, 408, 401, 79, 2, 0, 12),
        "huge": (4032, 1857, 1542, 344, 1608, 386, 16),
        "degenerate": (705, 201, 156, 30, 217, 68, 11),
        "random": (2000, 48, 48, 8, 0, 0, 7),
        "scaled": (240, 240, 230, 78, 0, 0, 9),
        "tmax": (133, 21, 21, 6, 0, 0, 6),
        "secondary": (336, 173, 173, 32, 0, 0, 11),
        "state": (250, 78, 60, 120, 0, 0, 13),
    },
    "large_kx": {
        "axis": (11676, 4358, 4304, 1635, 35, 0, 17),
        "poles": (4320, 4160, 4154, 1732, 3, 0, 15),
        "disk_plane": (493, 149, 148, 62, 0, 0, 10),
        "inside": (1344, 1268, 1262, 204, 0, 0, 14),
        "sweeps": (3600, 1217, 1208, 289, 9, 0, 13),
        "huge": (4536, 2165, 1548, 389, 1652, 599, 18),
        "degenerate": (769, 224, 167, 37, 220, 95, 10),
        "random": (2000, 35, 35, 8, 0, 0, 8),
        "scaled": (240, 240, 240, 93, 0, 0, 14),
        "tmax": (228, 50, 50, 22, 0, 0, 8),
        "secondary": (324, 185, 184, 46, 0, 0, 13),
        "state": (250, 95, 72, 119, 0, 0, 14),
    },
}
# secondary at max_depth 12: (paths of >= 5 iterations, the longest path)
PINNED_DEEP = {
    "small": (2, 7),
    "large": (2, 5),
    "small_kx": (5, 7),
    "large_kx": (4, 6),
}
# scaled: per first-hit material (groups, groups whose x3 copy has other bits in L, groups whose 2^k copies draw or trace otherwise)
PINNED_SCALED = {
    "small": {'matte': (48, 6, 0)},
    "large": {'matte': (48, 9, 0)},
    "small_kx": {'glass': (12, 2, 9), 'matte': (12, 2, 0), 'mirror': (12, 0, 0), 'oren_nayar': (12, 4, 0)},
    "large_kx": {'glass': (12, 9, 10), 'matte': (12, 1, 0), 'mirror': (12, 11, 0), 'oren_nayar': (12, 3, 0)},
}
# secondary: (origins on a surface, of those: rays that meet the origin's own primitive, at t < 1e-6;
#             origins inside Glass, of those after one iteration: left the glass, reflected inside it, ended)
PINNED_SECONDARY = {
    "small": (240, 85, 9, 0, 0, 0, 0),
    "large": (228, 111, 42, 0, 0, 0, 0),
    "small_kx": (240, 85, 9, 40, 32, 3, 5),
    "large_kx": (228, 111, 42, 30, 23, 1, 6),
}


def first_hits(key, family):
    b, one = LR.batch(key, family), LR.oracle_steps(key, family)[0]
    d0 = 0 if b.start is None else b.start.draws.astype(np.uint32)
    return (one.draws != d0) & (one.status != O.PANICKED)   # every interaction draws its BSDF sample


def figures(key, family):
    end = LR.oracle_li(key, family)
    n = LR.batch(key, family).rays.shape[0]
    b0 = 0 if LR.batch(key, family).start is None else LR.batch(key, family).start.bounces
    its = end.bounces - b0
    four = (end.bounces >= 4) & (b0 < 4)   # the path ran its fourth iteration: Russian roulette applies from there on
    return (n, int(first_hits(key, family).sum()), int((its >= 2).sum()), int(four.sum()),
            int((end.status == O.PANICKED).sum()), int(np.isnan(end.L).any(axis=1).sum()), len(set(end.draws.tolist())))


@pytest.mark.parametrize("key", KEYS)
def test_scenes(key):
    scene, twin = LR.SCENES[key](), LR.SCENES[LR.MATTE_TWIN[key]]()
    d, t = scene.desc, twin.desc
    assert (d.n_prims, d.n_nodes) == (t.n_prims, t.n_nodes) and d.n_meshes == 0
    for i in range(d.n_nodes):   # the same tree: the geometry of the pinned adversarial scenes
        assert bytes(d.nodes[i]) == bytes(t.nodes[i]), i
    assert (d.n_nodes > 64) == (LR.DEPTH[key] == 64)
    kinds = LR.material_kinds(scene)
    if LR.KX[key]:
        assert set(kinds) == {LR.MATTE, LR.MIRROR, LR.GLASS, LR.OREN} and min(kinds.count(k) for k in set(kinds)) >= d.n_prims // 4
        assert [d.lights[i].type for i in range(d.n_lights)] == [abi.PBRT_LIGHT_POINT, abi.PBRT_LIGHT_DIFFUSE_AREA]
    else:
        assert set(kinds) == {LR.MATTE} and d.n_lights == 1


@pytest.mark.parametrize("key", KEYS)
def test_ray_budget(key):
    sizes = {f: LR.batch(key, f).rays.shape for f in LR.ALL}
    total = sum(s[0] for s in sizes.values())
    print(key, total, sizes)
    assert all(s[1] == 7 for s in sizes.values()) and total <= 30_000
    akey = {"small": "small1", "large": "large"}[LR.MATTE_TWIN[key]]
    moved = A.rays(akey, "disk_plane").shape[0] - sizes["disk_plane"][0]
    for f in A.FAMILIES:   # adversarial_rays' own rows; the disk-centre rays counted with `degenerate`
        assert sizes[f][0] == A.rays(akey, f).shape[0] + {"disk_plane": -moved, "degenerate": moved}.get(f, 0), f
    assert 0 < moved < 32


@pytest.mark.parametrize("family", LR.ALL)
@pytest.mark.parametrize("key", KEYS)
def test_pinned_counts_and_caps(key, family):
    got = figures(key, family)
    print(f'        "{family}": {got},')
    assert got == PINNED[key][family]
    n, hits, two, four, panics, nan_rows, draws = got
    assert hits > 0 and two > 0 and four > 0 and draws >= 3
    end = LR.oracle_li(key, family)
    assert (end.status != O.ALIVE).all()
    bad = (end.status == O.PANICKED) | np.isnan(end.L).any(axis=1)
    if family == "tmax":   # the NaN and negative TMax rows are degenerate's kind
        t = LR.batch(key, family).rays[:, 6]
        bad &= ~(np.isnan(t) | (t < 0))
    if family not in UNCAPPED:
        assert bad.sum() <= CAP * n, (int(bad.sum()), n)
    else:
        assert panics > 0 and nan_rows > 0 and panics + nan_rows < n   # both kinds, and rows that are neither


@pytest.mark.parametrize("key", KEYS)
def test_secondary_deep(key):
    end = LR.oracle_li(key, "secondary", LR.DEEP)
    got = (int((end.bounces >= 5).sum()), int(end.bounces.max()))
    print(f'    "{key}": {got},')
    assert got == PINNED_DEEP[key] and got[0] > 0


@pytest.mark.parametrize("key", KEYS)
def test_scaled(key):
    scene = LR.SCENES[key]()
    b, end = LR.batch(key, "scaled"), LR.oracle_li(key, "scaled")
    g = LR.N_SCALED
    rays = b.rays.reshape(-1, g, 7)
    for j, f in enumerate(LR.SCALES):   # the copies: d times f, the same origin and stream
        assert np.array_equal(rays[:, 1 + j, 3:6], rays[:, 0, 3:6] * f) and np.array_equal(rays[:, 1 + j, :3], rays[:, 0, :3])
        fin = np.isfinite(rays[:, 0, 6])
        assert np.array_equal(rays[fin, 1 + j, 6], rays[fin, 0, 6] / f) and np.isinf(rays[~fin, 1 + j, 6]).all()
    assert np.array_equal(b.state.reshape(-1, g), np.repeat(b.state[::g, None], g, axis=1))
    kinds = LR.scaled_kinds(scene)
    L = end.L.reshape(-1, g, 3).view(np.uint64)
    count = np.stack([end.draws, end.closest, end.shadow], axis=1).reshape(-1, g, 3)
    pow2 = [0] + [1 + j for j, f in enumerate(LR.SCALES) if f != 3.0]
    x3 = 1 + LR.SCALES.index(3.0)
    got = {}
    for k in sorted(set(kinds)):
        sel = kinds == k
        other = (count[sel][:, pow2] != count[sel][:, :1]).any(axis=(1, 2))
        got[str(k)] = (int(sel.sum()), int((L[sel, 0] != L[sel, x3]).any(axis=1).sum()), int(other.sum()))
        if k != LR.GLASS:
            assert not other.any(), k
    print(f'    "{key}": {got},')
    assert got == PINNED_SCALED[key]
    assert (first_hits(key, "scaled").reshape(-1, g)[:, pow2]).all()   # a power of two keeps the hit
    # and the whole first iteration's counts, on Glass too: there only the lobe picked may differ, which
    # shows from the second iteration on
    one = LR.oracle_steps(key, "scaled")[0]
    count1 = np.stack([one.draws, one.closest, one.shadow], axis=1).reshape(-1, g, 3)
    assert (count1[:, pow2] == count1[:, :1]).all() and (count1[:, :, 1] == 1).all()
    if LR.KX[key]:
        assert got[LR.GLASS][1] > 0 and got[LR.OREN][1] > 0 and got[LR.GLASS][2] > 0


@pytest.mark.parametrize("key", KEYS)
def test_tmax(key):
    b, end = LR.batch(key, "tmax"), LR.oracle_li(key, "tmax")
    g = LR.N_TMAX
    t = b.rays[:, 6].reshape(-1, g)
    assert (t[:, A.SWEEP_N:A.SWEEP_N + 3] == np.array(LR.TMAX_EXTRA[:3])).all() and np.isnan(t[:, -1]).all()
    hit = first_hits(key, "tmax").reshape(-1, g)
    L = end.L.reshape(-1, g, 3)
    sweeps = hit[:, :A.SWEEP_N]
    assert t.shape[0] >= 6
    assert (sweeps.sum(axis=1) >= 1).all() and (sweeps.sum(axis=1) < A.SWEEP_N).all()   # both sides of the decision
    lit = L.max(axis=2) > 0
    assert np.array_equal(lit[:, :A.SWEEP_N], sweeps)   # L differs across it: a hit is lit, a miss black
    assert not hit[:, A.SWEEP_N:].any()   # TMax 0, a denormal, negative, NaN: misses


@pytest.mark.parametrize("key", KEYS)
def test_secondary(key):
    scene = LR.SCENES[key]()
    rows, where, prim = LR._secondary(scene)
    d = rows[:, 3:6]
    assert ((d == 0) & ~np.signbit(d)).any() and ((d == 0) & np.signbit(d)).any()
    norm = np.linalg.norm(d, axis=1)
    assert (np.abs(norm - 1) < 1e-12).any() and (norm > 2).any() and (norm < 0.5).any()
    assert set(where) == {LR.ON_SURFACE, LR.AT_CENTRE, LR.INSIDE, LR.IN_DISK_PLANE}
    w = O.intersect(scene.desc, rows)
    on = where == LR.ON_SURFACE
    own = on & (w[:, 0] == 1) & (w[:, 2] == prim)
    kinds = np.array(LR.material_kinds(scene))
    ing = (where == LR.INSIDE) & (kinds[prim] == LR.GLASS)
    one = LR.oracle_steps(key, "secondary")[0]
    left = ing & (one.status == O.ALIVE) & (one.eta_scale != 1)
    stayed = ing & (one.status == O.ALIVE) & (one.eta_scale == 1)
    got = (int(on.sum()), int(own.sum()), int((own & (w[:, 1] < 1e-6)).sum()), int(ing.sum()), int(left.sum()), int(stayed.sum()),
           int((ing & (one.status != O.ALIVE)).sum()))
    print(f'    "{key}": {got},')
    assert got == PINNED_SECONDARY[key]
    # both outcomes of self-intersection: a ray from a surface point meets its own surface at once, or leaves it
    assert got[2] > 0 and got[0] - got[2] > 0
    if LR.KX[key]:
        assert got[4] > 0 and got[5] > 0
        assert np.isin(one.eta_scale[left], (1.5 * 1.5, 1 / (1.5 * 1.5))).all()


@pytest.mark.parametrize("key", KEYS)
def test_state(key):
    b = LR.batch(key, LR.STATE)
    s = b.start
    n = b.rays.shape[0]
    assert n >= 200 and len(LR.EDITS) == 10
    kind = np.array([LR.EDITS[i % len(LR.EDITS)] for i in range(n)])
    assert (s.eta_scale[kind == "eta_quarter"] == 0.25).all() and (s.eta_scale[kind == "eta_four"] == 4.0).all()
    assert (s.beta[kind == "beta_channels", 0] == 0).all() and (s.L[kind == "L_preloaded"].min(axis=1) > 0).all()
    assert (s.bounces[kind == "at_max_depth"] == LR.MAX_DEPTH).all() and (s.bounces[kind == "beyond_max_depth"] > LR.MAX_DEPTH).all()
    assert set(s.bounces[kind == "as_is"]) == {1, 2, 3} and (s.draws > 0).all() and (s.closest > 0).all()
    one = LR.oracle_steps(key, LR.STATE)[0]
    # a path at or beyond max_depth ends in its next iteration having asked one closest hit and drawn nothing
    late = np.isin(kind, ("at_max_depth", "beyond_max_depth"))
    assert (one.status[late] == O.ENDED).all() and np.array_equal(one.closest[late], s.closest[late].astype(np.uint32) + 1)
    assert np.array_equal(one.draws[late], s.draws[late].astype(np.uint32))
    # Russian roulette reads the caller's etaScale (path.go:145-146: rrBeta = beta * etaScale): the same rows from
    # etaScale 1 make another decision, on a Matte scene too
    desc = LR.SCENES[key]().desc
    for k in ("rr_early_eta_quarter", "rr_early_eta_four"):
        sel = kind == k
        unit = O.PathStart(*[np.array(getattr(s, f)[sel]) if f != "eta_scale" else np.ones(int(sel.sum())) for f in O.PathStart._fields])
        plain = O.path_li(desc, b.rays[sel], b.state[sel], b.inc[sel], max_depth=LR.MAX_DEPTH, k=1, start=unit)
        differ = (plain.draws != one.draws[sel]) | (plain.beta.view(np.uint64) != one.beta[sel].view(np.uint64)).any(axis=1)
        print(key, k, int(sel.sum()), "rows,", int(differ.sum()), "decide otherwise from etaScale 1")
        assert differ.any(), k
    # a preloaded L is kept: nothing is ever subtracted
    pre = kind == "L_preloaded"
    assert (LR.oracle_li(key, LR.STATE).L[pre] >= s.L[pre]).all()

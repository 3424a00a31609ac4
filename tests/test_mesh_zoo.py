"""The oracle's mesh code on tests/mesh_zoo.py's families, CPU only: before the
GPU tests (tests/test_gpu_mesh_zoo.py) compare the device with the oracle on
these inputs, the oracle itself is pinned on them:

  * closest hit and any-hit against brute force over every kept triangle under
    the rule "smallest (t, global index), t < TMax" (test_mesh.brute_ties);
  * each family does what it is named for (exact counts, read from the brute
    force, and the floors below them);
  * the triangle test against exact rational arithmetic;
  * relations that need no second implementation (appended copies, power-of-two
    scaling, the reverse flag);
  * the mesh cache key (oracle_mesh.c mesh_key) tells apart two scenes that
    differ only in their index buffers.
"""
import functools
import gc
from fractions import Fraction

import numpy as np
import pytest

import mesh_zoo as Z
import oracle_lib as O
from pbrtgpu import abi
from test_mesh import brute_ties

NAMES = ["grid_ties[6]", "grid_ties[24]", "duplicates[two_meshes]", "duplicates[shuffled]", "duplicates[soup]",
         "duplicates[x2]",
         "duplicates[x9]", "duplicates[x65]", "degenerates[interleaved]", "degenerates[all]",
         "degenerates[collinear]", "degenerates[between]", "tiny[1]", "tiny[2]", "tiny[3]", "tiny[5]",
         "cluster[outlier]", "cluster[star]", "scaled[2^40]", "scaled[2^-40]", "scaled[2^100]", "scaled[2^-100]",
         "multi", "soup", "tmax_edge", "subnormal", "mixed_tie"]

MAX_PAIRS = 12_000_000   # brute-force (ray, triangle) tests per family; rays are subsampled above it


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def brute(name):
    """Brute force over the kept triangles of Case `name`, in global indices:
    (ray rows used, t, gid (-1: miss), triangles at the winning t)."""
    c = Z.query_cases()[name]
    kept = np.flatnonzero(c.kept)
    tris = c.tris_in.astype(np.float64)[kept]
    take = np.arange(c.rays.shape[0])
    if take.size * max(len(tris), 1) > MAX_PAIRS:
        take = take[:: -(-take.size * len(tris) // MAX_PAIRS)]
    res = brute_ties(tris, c.rays[take])
    t = np.array([r[0] for r in res])
    g = np.array([kept[r[1]] if r[1] >= 0 else -1 for r in res], dtype=np.int64)
    k = np.array([r[2] for r in res], dtype=np.int64)
    for a in (take, t, g, k):
        a.setflags(write=False)
    return take, t, g, k


# ------------------------------------------------------ 1. brute force
@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_brute_force(name):
    c = Z.query_cases()[name]
    take, t, g, _ = brute(name)
    rays = c.rays[take]
    hit = g >= 0
    desc = c.scene().desc
    assert desc.n_prims == 0
    got = O.intersect(desc, rays, closest=True)
    occ = O.intersect(desc, rays, closest=False)
    assert not np.isnan(got).any()
    assert np.array_equal(got[:, 0] == 1, hit)
    assert np.array_equal(got[hit, 1], t[hit]) and np.array_equal(got[hit, 2].astype(np.int64), g[hit])
    assert same_bits(got[~hit, 1], rays[~hit, 6]) and (got[~hit, 2] == -1).all()
    assert np.array_equal(occ == 1, hit)   # any-hit: brute force finds a hit with t < TMax
    if not c.has_mixed:
        return
    # with analytic primitives in the scene: a triangle wins with the brute
    # force's (t, index); an analytic primitive wins only at or in front of it
    # (a triangle at exactly an analytic primitive's t loses: TMax is exclusive)
    desc = c.scene(mixed=True).desc
    n_prims = desc.n_prims
    assert n_prims >= 1
    got = O.intersect(desc, rays, closest=True)
    occ = O.intersect(desc, rays, closest=False)
    assert not np.isnan(got).any()
    analytic = (got[:, 0] == 1) & (got[:, 2] < n_prims)
    assert analytic.any()
    assert (got[analytic, 1] <= t[analytic]).all()
    tri = ~analytic
    assert np.array_equal(got[tri, 0] == 1, hit[tri])
    w = tri & hit
    assert np.array_equal(got[w, 1], t[w]) and np.array_equal(got[w, 2].astype(np.int64), n_prims + g[w])
    assert (occ[hit] == 1).all() and np.array_equal(occ[tri] == 1, hit[tri])


def test_names_cover_the_zoo():
    assert set(NAMES) == set(Z.query_cases())
    for name, c in Z.query_cases().items():
        assert c.tris_in.shape[0] <= 4000 and c.rays.shape[0] <= 20_000, name


# ------------------------------------- 2. each family does what it names
# (rays, rays hit, rays with two or more triangles at the winning t, input
# triangles dropped as zero-area), read from the brute force
COUNTS = {
    "grid_ties[6]": (676, 676, 572, 0),
    "grid_ties[24]": (9604, 9604, 9212, 0),
    "duplicates[two_meshes]": (676, 676, 676, 0),
    "duplicates[shuffled]": (676, 676, 676, 0),
    "duplicates[soup]": (6300, 4498, 4498, 0),
    "duplicates[x2]": (484, 180, 180, 0),
    "duplicates[x9]": (484, 180, 180, 0),
    "duplicates[x65]": (484, 180, 180, 0),
    "degenerates[interleaved]": (676, 676, 572, 72),
    "degenerates[all]": (676, 0, 0, 10),
    "degenerates[collinear]": (1500, 834, 0, 60),
    "degenerates[between]": (676, 464, 295, 10),
    "tiny[1]": (676, 24, 0, 0),
    "tiny[2]": (676, 36, 12, 0),
    "tiny[3]": (676, 56, 16, 0),
    "tiny[5]": (676, 80, 32, 0),
    "cluster[outlier]": (1000, 995, 0, 0),
    "cluster[star]": (400, 393, 29, 0),
    "scaled[2^40]": (6300, 4973, 0, 0),
    "scaled[2^-40]": (6300, 4973, 0, 0),
    "scaled[2^100]": (6300, 4973, 0, 0),
    "scaled[2^-100]": (6300, 4973, 0, 0),
    "multi": (1500, 457, 0, 0),
    "soup": (6300, 4973, 0, 0),
    "tmax_edge": (3000, 1500, 0, 0),
    "subnormal": (6300, 4972, 0, 0),
    "mixed_tie": (336, 216, 184, 0),
}


@pytest.mark.parametrize("name", NAMES)
def test_family_counts(name):
    c = Z.query_cases()[name]
    take, t, g, k = brute(name)
    assert take.size == c.rays.shape[0]   # nothing in the zoo needs subsampling
    counts = (take.size, int((g >= 0).sum()), int((k >= 2).sum()), int((~c.kept).sum()))
    print(f'    "{name}": {counts},')
    assert counts == COUNTS[name]
    # the oracle's own tree holds exactly the kept triangles
    assert O.mesh_counts(c.scene().desc) == (c.kept.size, int(c.kept.sum()))


def test_grid_ties_floor():
    for n in (6, 24):
        take, _, g, k = brute(f"grid_ties[{n}]")
        assert (k >= 2).sum() * 2 >= take.size and k.max() == 6
        assert (g >= 0).all()


def test_duplicates_floor_and_first_copy():
    for name, first in (("two_meshes", 72), ("shuffled", 72), ("soup", 200), ("x2", 1), ("x9", 1), ("x65", 1)):
        _, _, g, k = brute(f"duplicates[{name}]")
        hit = g >= 0
        assert hit.any() and (k[hit] >= 2).all()   # every hit ray ties
        assert (g[hit] < first).all()              # and the first copy wins
    assert brute("duplicates[x65]")[3].max() == 65


def test_degenerates_floor():
    for name in ("interleaved", "collinear"):
        c = Z.degenerates()[name]
        _, _, g, _ = brute(f"degenerates[{name}]")
        n_kept = int(c.kept.sum())
        assert (~c.kept).sum() >= 0.4 * c.kept.size
        assert (g >= n_kept).any()   # a winner's global index counts the dropped triangles
    c = Z.degenerates()["all"]
    assert not c.kept.any() and (brute("degenerates[all]")[2] == -1).all()
    c = Z.degenerates()["between"]
    first = c.mesh_first
    _, _, g, _ = brute("degenerates[between]")
    assert not c.kept[first[1]:first[2]].any()
    assert ((g >= 0) & (g < first[1])).any() and (g >= first[2]).any()   # both valid meshes win somewhere


def test_bare_triangle_test_never_hits_a_zero_area_triangle():
    """The dropping rule cannot be seen in a hit: orc_triangle_hit itself
    rejects every zero-area triangle of the zoo (det == 0, or t <= deltaT with
    a det that is rounding noise), also the collinear ones aimed at from
    general directions. Dropping is pinned through the device tree's counts
    (tests/test_gpu_mesh_zoo.py) and through gid here."""
    for name in ("interleaved", "collinear", "all", "between"):
        c = Z.degenerates()[name]
        dropped = c.tris_in.astype(np.float64)[~c.kept]
        for r in c.rays:
            assert not O.triangle_hits(dropped, r)[0].any()


def test_tmax_edge_floor():
    c = Z.tmax_edge()
    take, t, g, _ = brute("tmax_edge")
    m = take.size // 2
    assert m == 1500
    at, above = g[:m] >= 0, g[m:] >= 0
    both = ~at & above & (t[m:] == c.rays[:m, 6])   # a miss at TMax == t, that hit again one ulp above
    print(f"tmax_edge: both outcomes on {int(both.sum())} of {m} rays")
    assert both.sum() >= 0.9 * m


def test_cluster_floor():
    take, _, g, _ = brute("cluster[outlier]")
    assert ((g >= 0) & (g < 300)).sum() * 2 >= take.size and (g == 300).sum() >= 1
    c = Z.cluster()["star"]
    p = c.meshes[0][0].reshape(-1, 3, 3)
    cen = (p[:, 0] + p[:, 1] + p[:, 2]) * np.float32(1.0 / 3.0)   # k_centroids' float32 arithmetic
    assert cen.dtype == np.float32 and (cen == 0).all()
    assert brute("cluster[star]")[3].max() == 24   # a ray through the centroid hits all 24 at one point


def test_mixed_tie_floor():
    c = Z.mixed_tie()
    desc = c.scene(mixed=True).desc
    got = O.intersect(desc, c.rays, closest=True)
    hit = got[:, 0] == 1
    _, _, g, _ = brute("mixed_tie")
    disk, tri = hit & (got[:, 2] == 0), hit & (got[:, 2] >= 1)
    assert disk.any() and tri.any() and (~hit).any()
    assert (got[hit, 1] == 4.0).all()
    assert (disk & (g >= 0)).sum() > 50   # coplanar ties: the analytic primitive wins them
    assert not (tri & ~(g >= 0)).any()


def test_subnormal_floor():
    c = Z.subnormal()
    p = c.tris_in
    tiny = np.float32(2.0 ** -126)
    sub = ((np.abs(p) < tiny) & (p != 0)).any(axis=1)
    _, _, g, _ = brute("subnormal")
    n = int(sub[g[g >= 0]].sum())
    print(f"subnormal: {int(sub.sum())} triangles with a subnormal coordinate, {n} winning hits on them")
    assert n >= 1


# ------------------------------------------ 3. exact triangle reference
def F3(a):
    return [Fraction(float(x)) for x in a]


def sub(a, b):
    return [x - y for x, y in zip(a, b)]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def exact_hit(v, ray):
    """Moeller-Trumbore in exact rationals: (t, b0, b1, b2), or None when the
    ray is parallel to the triangle's plane. No rounding anywhere."""
    v0, v1, v2, o, d = F3(v[0:3]), F3(v[3:6]), F3(v[6:9]), F3(ray[0:3]), F3(ray[3:6])
    e1, e2 = sub(v1, v0), sub(v2, v0)
    pv = cross(d, e2)
    det = dot(e1, pv)
    if det == 0:
        return None
    tv = sub(o, v0)
    qv = cross(tv, e1)
    b1, b2 = dot(tv, pv) / det, dot(d, qv) / det
    return dot(e2, qv) / det, 1 - b1 - b2, b1, b2


def exact_pairs():
    """About 2 000 (triangle, ray) pairs: rays of grid_ties, soup and scaled,
    each with the triangle the oracle says it hits and with a random other."""
    rng = np.random.default_rng(71)
    pairs = []
    for c, n_rays, rows in ((Z.grid_ties()[6], 60, None), (Z.soup(), 600, slice(0, 5700)),
                            (Z.scaled()[100], 170, slice(0, 5700)), (Z.scaled()[-100], 170, slice(0, 5700))):
        tris = c.tris_in.astype(np.float64)
        idx = np.arange(c.rays.shape[0])[rows if rows is not None else slice(None)]
        pick = rng.choice(idx, n_rays, replace=False)
        want = O.intersect(c.scene().desc, c.rays[pick], closest=True)
        for r, w in zip(c.rays[pick], want):
            if w[0] == 1:
                pairs.append((tris[int(w[2])], r))
            pairs.append((tris[rng.integers(0, len(tris))], r))
    return pairs


def test_triangle_hit_against_exact_rationals():
    """orc_triangle_hit against exact Moeller-Trumbore on 1 805 pairs: with
    every exact barycentric and the exact t above 2^-20 (t relative to the
    largest origin-to-vertex distance over |d|) it must hit; with a barycentric
    below -2^-20 or t < 0 it must miss; the pairs between are excluded.
    Measured: 710 must-hit, 992 must-miss, 103 excluded (5.7 %; the grid's rays
    run through edges and vertices, where an exact barycentric is 0);
    max |t - t_exact| / t_exact = 8.5e-15 and max |b - b_exact| = 2.99e-11 (a
    barycentric's error grows with the ray's distance over the triangle's
    size; the soup's triangles go down to 1e-3). The bounds are 16 x these: room for
    another libm or compiler, not for another formula."""
    T_MEASURED, B_MEASURED = 8.5e-15, 2.99e-11
    eps = Fraction(1, 2 ** 20)
    n_hit = n_miss = n_excluded = 0
    t_err = b_err = 0.0
    pairs = exact_pairs()
    for v, r in pairs:
        hit, t, b0, b1, b2 = O.triangle_hit(v, r)
        ex = exact_hit(v, r)
        if ex is None:
            assert not hit   # parallel to the plane
            n_miss += 1
            continue
        te, be = ex[0], ex[1:]
        far = max(np.linalg.norm(v[3 * k:3 * k + 3] - r[0:3]) for k in range(3)) / np.linalg.norm(r[3:6])
        if min(be) > eps and te > eps * Fraction(far):
            assert hit, (v, r)
            n_hit += 1
            t_err = max(t_err, abs(float((Fraction(t) - te) / te)))
            b_err = max(b_err, max(abs(float(Fraction(b) - e)) for b, e in zip((b0, b1, b2), be)))
        elif min(be) < -eps or te < 0:
            assert not hit, (v, r)
            n_miss += 1
        else:
            n_excluded += 1
    print(f"{len(pairs)} pairs: {n_hit} must-hit, {n_miss} must-miss, {n_excluded} excluded "
          f"({100 * n_excluded / len(pairs):.1f} %); max t error {t_err:.3g}, max barycentric error {b_err:.3g}")
    assert len(pairs) >= 1700 and n_hit >= 500 and n_miss >= 500
    assert n_excluded <= 0.10 * len(pairs)
    assert t_err <= 16 * T_MEASURED and b_err <= 16 * B_MEASURED


# ------------------------------------------------------- 4. relations
RELATION_CASES = ["grid_ties[6]", "duplicates[two_meshes]", "degenerates[between]", "soup", "multi"]


def render_desc_of(name):
    return abi.render_desc(2, 2, max_depth=5)


@pytest.mark.parametrize("name", RELATION_CASES)
def test_appended_copies_change_nothing(name):
    """An exact copy of every mesh, appended with another material and the
    opposite flag, loses every tie: all hit rows and the film stay bit-equal."""
    c = Z.query_cases()[name]
    mixed = c.has_mixed
    base = c.scene(mixed=mixed, size=(40, 32))
    twice = c.scene(mixed=mixed, size=(40, 32), meshes=c.with_copies())
    assert twice.desc.n_meshes == 2 * base.desc.n_meshes
    for closest in (True, False):
        assert same_bits(O.intersect(base.desc, c.rays, closest), O.intersect(twice.desc, c.rays, closest))
    if c.view is None:
        return
    rd = render_desc_of(name)
    rc1, film1, st1 = O.render(base.desc, rd, threads=4)
    rc2, film2, st2 = O.render(twice.desc, rd, threads=4)
    assert rc1 == 0 and rc2 == 0 and st1.paths == st2.paths
    assert film1.max() > 0 and same_bits(film1, film2)
    # the copies in front do change it (they win the ties with their own material)
    front = c.scene(mixed=mixed, size=(40, 32), meshes=c.with_copies()[len(c.meshes):] + c.meshes)
    rc3, film3, _ = O.render(front.desc, rd, threads=4)
    assert rc3 == 0 and not same_bits(film1, film3)


def unscale(rows, k):
    """Hit rows of a scene scaled by 2^k, scaled back: t and p by 2^-k."""
    out = rows.copy()
    f = np.ldexp(1.0, -k)
    hit = out[:, 0] == 1
    out[hit, 1] *= f
    out[:, 3:6] *= f
    return out


def scaled_tmax_back(rows, rays, k):
    """A miss reports the ray's own TMax, which was scaled too."""
    out = unscale(rows, k)
    miss = out[:, 0] != 1
    out[miss, 1] = rays[miss, 6]
    return out


@pytest.mark.parametrize("k", [40, -40, 100, -100])
def test_power_of_two_scaling(k):
    s, c = Z.soup(), Z.scaled()[k]
    want = O.intersect(s.scene().desc, s.rays, closest=True)
    got = O.intersect(c.scene().desc, c.rays, closest=True)
    assert same_bits(scaled_tmax_back(got, s.rays, k), want)
    assert np.array_equal(O.intersect(c.scene().desc, c.rays, closest=False),
                          O.intersect(s.scene().desc, s.rays, closest=False))


def flip(meshes, i):
    return [(p, idx, m, (not r) if j == i else r) for j, (p, idx, m, r) in enumerate(meshes)]


def test_reverse_flag_changes_the_film_and_the_normal():
    c = Z.multi()
    assert c.meshes[0][2] == "glass"   # a dielectric: which side is inside depends on the normal
    base = c.scene(mixed=True, size=(40, 32))
    flipped = c.scene(mixed=True, size=(40, 32), meshes=flip(c.meshes, 0))
    rd = render_desc_of("multi")
    rc1, film1, _ = O.render(base.desc, rd, threads=4)
    rc2, film2, _ = O.render(flipped.desc, rd, threads=4)
    assert rc1 == 0 and rc2 == 0 and not same_bits(film1, film2)
    a, b = O.intersect(base.desc, c.rays, True), O.intersect(flipped.desc, c.rays, True)
    n_prims, first = base.desc.n_prims, c.mesh_first
    on0 = (a[:, 0] == 1) & (a[:, 2] >= n_prims) & (a[:, 2] < n_prims + first[1])
    assert on0.sum() > 50
    assert same_bits(a[:, :6], b[:, :6]) and same_bits(a[~on0], b[~on0])
    assert same_bits(b[on0, 6:9], -a[on0, 6:9])   # mesh_rev flips the normal of that mesh's hits only


# ------------------------------------------------- 5. the mesh cache key
def test_cache_key_sees_the_index_buffer():
    """Two scenes of equal vertices, counts and (after a free) very likely
    equal addresses, differing only in their indices, built and queried in
    turn: each answers for its own triangles."""
    p, idx = Z.grid(6)
    rays = Z.grid_rays(6, dirs=Z.GRID_DIRS[:1])
    halves = (idx[:36], idx[36:])
    want = []
    for h in halves:
        res = brute_ties(p[h].reshape(-1, 9).astype(np.float64), rays)
        want.append(np.array([r[1] for r in res]))
    assert not np.array_equal(want[0] >= 0, want[1] >= 0)
    for turn in range(8):
        k = turn % 2
        s = Z.build_scene([(p, halves[k], "matte", False)])
        got = O.intersect(s.desc, rays, closest=True)
        assert np.array_equal(got[:, 2].astype(np.int64), want[k]), turn
        del s
        gc.collect()

"""The oracle's sphere and disk hits against tests/analytic_reference.py, a brute-force
reference written from the geometry (no GPU): on every decided ray the hit flag and
the primitive are equal, t, p and n agree within TOL, the any-hit flag is the
closest-hit flag and the oracle does not panic.

Families: analytic_reference's `aimed`, `offsets` and `shadowing`, and
adversarial_rays' `inside`, `random` and `axis`. All but `axis` are decidable ray for
ray (asserted: 0 undecided); of `axis` the decided rays are compared and the number of
the others is pinned.

TOL. Measured on the CPU over all six families and three scenes (10 500 to 19 100
decided rays per scene), the largest gap between the oracle and the reference was

    t   2.85e-14   relative to |t| + |o| / |d|
    p   2.49e-14   relative to the root box's diagonal
    n   2.22e-16   as 1 - |n . n_ref| (and the signs agreed on every ray)

TOL is FACTOR = 50 times each maximum: the oracle's t carries EFloat's float64
rounding and the rounding of the float64 inverse matrices, which may differ by a few
ulps on other rays; a mistaken root, clip or transform shows at 1e-6 or more.
"""
import numpy as np
import pytest

import adversarial_rays as A
import analytic_reference as R

SCENE_KEYS = list(A.SCENES)
MEASURED = {"t": 2.85e-14, "p": 2.49e-14, "n": 2.22e-16}
FACTOR = 50
TOL = {k: FACTOR * v for k, v in MEASURED.items()}
UNDECIDED_AXIS = {"small1": 490, "small4": 646, "large": 1060}


def same_as_reference(scene, rays, ref, rows, occ, what):
    """The assertions on decided rays, for the oracle's rows and for any device walk's: returns the largest gaps."""
    d = ref.decided
    rows, occ, rays = rows[d], np.asarray(occ)[d], rays[d]
    ref = R.Hits(*[a[d] for a in ref])
    assert not np.isnan(rows[:, 0]).any(), (what, "a decided ray panics")
    hit = rows[:, 0] == 1
    assert np.array_equal(hit, ref.hit), (what, np.flatnonzero(hit != ref.hit)[:5], rays[hit != ref.hit][:2])
    assert np.array_equal(rows[hit, 2].astype(int), ref.prim[hit]), (what, rays[hit][rows[hit, 2] != ref.prim[hit]][:2])
    assert np.array_equal(occ == 1, ref.hit), (what, "any-hit differs from closest-hit")
    gt, gp, gn, sign = R.gaps(scene, rays, ref, rows)
    worst = {"t": float(gt.max(initial=0)), "p": float(gp.max(initial=0)), "n": float(gn.max(initial=0))}
    print(f"{what}: {int(d.sum())} decided of {d.size}, {int(hit.sum())} hits, largest gaps {worst}")
    assert sign.all(), (what, "a normal points to the other side", rays[hit][~sign][:2])
    for k in TOL:
        assert worst[k] <= TOL[k], (what, k, worst[k], TOL[k])
    return worst


def test_tolerance_is_the_measured_maximum_times_the_factor():
    assert FACTOR == 50 and all(TOL[k] == 50 * MEASURED[k] for k in MEASURED) and max(TOL.values()) < 1e-10


@pytest.mark.parametrize("family", R.COMPARED)
@pytest.mark.parametrize("key", SCENE_KEYS)
def test_oracle_against_reference(key, family):
    ref = R.reference(key, family)
    want, wocc = R.oracle(key, family)
    undecided = int((~ref.decided).sum())
    if family == "axis":
        assert undecided == UNDECIDED_AXIS[key]
    else:
        assert undecided == 0, R.rays(key, family)[~ref.decided][:3]
    same_as_reference(A.SCENES[key](), R.rays(key, family), ref, want, wocc, f"{key} {family}")


@pytest.mark.parametrize("key", SCENE_KEYS)
def test_ray_budget(key):
    sizes = {f: R.rays(key, f).shape[0] for f in R.FAMILIES}
    print(key, sizes)
    assert sum(sizes.values()) <= 12_000


@pytest.mark.parametrize("key", SCENE_KEYS)
def test_aimed_reaches_every_primitive_through_both_roots(key):
    scene = A.SCENES[key]()
    ref = R.reference(key, "aimed")
    shapes = A.shapes(scene)
    index = R.aimed_index(scene)
    assert [a.prim for a in index] == [s.prim for s in shapes]
    assert sum(1 for s in shapes if R.has_removed_part(s)) >= 3
    for sh, aim in zip(shapes, index):
        own = ref.decided & ref.hit & (ref.prim == sh.prim)
        assert own.sum() >= 32, (sh.prim, int(own.sum()))
        if sh.kind == "sphere":
            assert (own & (ref.root == 1)).sum() >= 8, (sh.prim, "far root")
            assert (own & (ref.root == 0)).sum() >= 8, (sh.prim, "near root")
        assert (aim.removed > 0) == R.has_removed_part(sh)
        if aim.removed:
            sl = slice(aim.start + aim.kept, aim.start + aim.kept + aim.removed)
            missed = ref.decided[sl] & ~(ref.hit[sl] & (ref.prim[sl] == sh.prim))
            assert missed.sum() >= 8, (sh.prim, int(missed.sum()))
    tmax = R.rays(key, "aimed")[:, 6]
    assert np.isfinite(tmax).sum() >= len(shapes) * 16


@pytest.mark.parametrize("key", SCENE_KEYS)
def test_offsets_are_decided_on_both_sides_of_every_boundary(key):
    scene = A.SCENES[key]()
    ref = R.reference(key, "offsets")
    index = R.offsets_index(scene)
    assert len(index) * len(R.OFFSETS) == ref.hit.size
    # the sweeps are adversarial_rays' own, one for one
    assert [(s.name, s.prim) for s in index] == [(s.name, s.prim) for s in A.sweep_index(scene)]
    assert {s.name for s in index} == {"tangent", "tmax_t0", "tmax_t1", "cross", "z_min", "z_max", "phi_max", "phi_seam",
                                       "radius", "inner_radius"}
    plus = [i for i, s in enumerate(R.OFFSETS) if s > 0]
    minus = [i for i, s in enumerate(R.OFFSETS) if s < 0]
    assert len(plus) == len(minus) == 3
    for sw in index:
        sl = slice(sw.start, sw.start + len(R.OFFSETS))
        assert ref.decided[sl].all(), sw
        own = ref.hit[sl] & (ref.prim[sl] == sw.prim)
        assert not (ref.hit[sl] & ~own).any(), sw     # a sweep's ray can meet its own shape only
        assert len(set(own[plus])) == 1 and len(set(own[minus])) == 1 and own[plus][0] != own[minus][0], (sw, own)


@pytest.mark.parametrize("key", SCENE_KEYS)
def test_shadowing_rays_pass_several_primitives(key):
    """The closest hit is not always the same primitive of a line, and a TMax between two primitives changes the
    any-hit answer."""
    rays, ref = R.rays(key, "shadowing"), R.reference(key, "shadowing")
    lines = {}
    for i, row in enumerate(rays):
        lines.setdefault(tuple(row[1:6]) + (row[0] if row[3] == 0 else None,), []).append(i)
    several = sum(1 for ix in lines.values() if len({int(ref.prim[i]) for i in ix if ref.hit[i]}) >= 2)
    both = sum(1 for ix in lines.values() if len({bool(ref.hit[i]) for i in ix}) == 2)
    print(key, len(lines), several, both)
    assert several >= 8 and both >= 16
    kinds = {A.shapes(A.SCENES[key]())[p].kind for p in set(ref.prim[ref.hit])}
    assert kinds == {"sphere", "disk"}
    if key != "small1":   # the nested disk and the ring are hit through the annular disk's hole
        sh = A.shapes(A.SCENES[key]())
        centre = next(s.centre for s in sh if s.kind == "disk" and s.inner > 0 and s.phi_max < 2 * np.pi)
        nested = {s.prim for s in sh if s.kind == "disk" and np.array_equal(s.centre, centre)}
        assert len(nested) == 3 and nested <= set(ref.prim[ref.hit])


# ----------------------------------------------------- the reference on its own
@pytest.fixture(scope="module")
def hand_scene():
    """A unit sphere at the origin, a unit disk at height 1 over (5, 0, 0) and a 270 degree sector at (10, 0, 0)."""
    import pbrtgpu as G
    s = G.Scene()
    m = s.add_matte((0.5, 0.5, 0.5))
    s.add_primitive(s.add_sphere(G.translate(0, 0, 0), 1.0), m)
    s.add_primitive(s.add_disk(G.translate(5, 0, 0), 1.0, 1.0), m)
    s.add_primitive(s.add_disk(G.translate(10, 0, 0), 0.0, 1.0, phi_max=270.0), m)
    s.add_point_light(G.translate(0, 20, 8), (1, 1, 1))
    s.set_film(4, 4)
    s.set_camera(G.look_at((0, 40, 55), (0, 0, 0), (0, 1, 0)), fov=50)
    return s.build(max_prims_in_node=1)


def _prim_at(scene, x):
    return next(p.index for p in R.primitives(scene) if float(p.M[0, 3]) == x)


def test_reference_on_hand_computed_rays(hand_scene):
    scene = hand_scene
    sphere, disk, sector = _prim_at(scene, 0.0), _prim_at(scene, 5.0), _prim_at(scene, 10.0)
    inf = float("inf")
    rays = np.array([
        [0.6, 0, -3, 0, 0, 1, inf],        # 0 the sphere at z = -0.8: t = 2.2
        [0.6, 0, 0, 0, 0, 2, inf],         # 1 from inside, the far root at z = 0.8: t = 0.4
        [0.6, 0, -3, 0, 0, 1, 3.0],        # 2 TMax between the roots 2.2 and 3.8: the near one
        [0.6, 0, -3, 0, 0, 1, 2.0],        # 3 TMax short of both: a miss
        [0.6, 0, 3, 0, 0, 1, inf],         # 4 both roots behind: a miss
        [5.5, 0, 3, 0, 0, -1, inf],        # 5 the disk at height 1: t = 2
        [5.5, 0.25, 3, 0, 0, -4, inf],     # 6 t = 0.5
        [5.5, 0.25, 3, 0, 0, -4, 0.25],    # 7 TMax short of the plane
        [6.5, 0, 3, 0, 0, -1, inf],        # 8 rho = 1.5: outside the disk
        [9.5, 0.5, 2, 0, 0, -1, inf],      # 9 the sector at phi = 135 degrees: t = 2
        [10.5, -0.5, 2, 0, 0, -1, inf],    # 10 phi = 315 degrees: in the missing quarter
        [8, 0, 0.5, 1, 0, 0, inf],         # 11 parallel to the sector's plane and off it: a decided miss
        [8, 0, 0, 1, 0, 0, inf],           # 12 in the sector's plane, through it: undecided
        [8, 0, 0, -1, 0, 0, 5.0],          # 13 in that plane, away from the sector, TMax short of the sphere: a miss
        [1, 0, -3, 0, 0, 1, inf],          # 14 tangent to the sphere: undecided
        [10.5, 0, 2, 0, 0, -1, inf],       # 15 on the sector's seam phi = 0: undecided
        [10, 0, 2, 0, 0, -1, inf],         # 16 the disk's centre: undecided
        [0, -3, 0, 0, 1, 0, inf],          # 17 through the sphere's centre, in the sector's plane but clear of it: t = 2
    ], dtype=np.float64)
    ref = R.intersect(scene, rays)
    expect_hit = [1, 1, 1, 0, 0, 1, 1, 0, 0, 1, 0, 0, None, 0, None, None, None, 1]
    for i, e in enumerate(expect_hit):
        assert ref.decided[i] == (e is not None), i
        if e is not None:
            assert ref.hit[i] == bool(e), i
    near = {0: (sphere, 2.2, (0.6, 0, -0.8), (0.6, 0, -0.8), 0), 1: (sphere, 0.4, (0.6, 0, 0.8), (0.6, 0, 0.8), 1),
            2: (sphere, 2.2, (0.6, 0, -0.8), (0.6, 0, -0.8), 0), 5: (disk, 2.0, (5.5, 0, 1), (0, 0, -1), 0),
            6: (disk, 0.5, (5.5, 0.25, 1), (0, 0, -1), 0), 9: (sector, 2.0, (9.5, 0.5, 0), (0, 0, -1), 0),
            17: (sphere, 2.0, (0, -1, 0), (0, -1, 0), 0)}
    for i, (prim, t, p, n, root) in near.items():
        assert ref.prim[i] == prim and ref.root[i] == root, i
        assert abs(ref.t[i] - t) < 1e-15 and np.allclose(ref.p[i], p, rtol=0, atol=2e-15), (i, ref.t[i], ref.p[i])
        assert np.allclose(ref.n[i], n, rtol=0, atol=1e-15), (i, ref.n[i])
    for i, e in enumerate(expect_hit):
        if e == 0:
            assert ref.prim[i] == -1 and ref.root[i] == -1 and ref.t[i] == 0 and not ref.p[i].any() and not ref.n[i].any()


def test_reference_inverts_the_transforms_itself():
    """affine_inverse against the matrices of the composite shapes: M Minv = 1 to longdouble's precision, and the
    descriptor's own inverses (not read by the reference) agree to float64's."""
    scene = A.SCENES["small4"]()
    eye = np.eye(4, dtype=R.LD)
    composite = 0
    for pr in R.primitives(scene):
        assert np.abs(pr.M @ pr.Minv - eye).max() < 1e-17
        composite += not np.array_equal(pr.M[:3, :3], eye[:3, :3])
    assert composite >= 5
    assert float(np.finfo(R.LD).eps) < 1e-18   # the platform's longdouble is wider than float64


def test_normal_sign_rule():
    """Outward on spheres (the doubly mirrored one too), inward where reverse is set, object -z on disks."""
    key = "small4"
    scene = A.SCENES[key]()
    ref, rays = R.reference(key, "aimed"), R.rays(key, "aimed")
    prims = R.primitives(scene)
    mirrored = [p.index for p in prims if p.kind == "sphere" and np.linalg.det(np.array(p.M[:3, :3], dtype=float)) > 0
                and float(p.M[2, 2]) == -1.0]
    assert len(mirrored) == 1 and sum(p.reverse for p in prims) == 2
    for pr in prims:
        own = ref.hit & (ref.prim == pr.index)
        centre = np.array(pr.M[:3, 3], dtype=float)
        if pr.kind == "sphere":
            outward = ((ref.p[own] - centre) * ref.n[own]).sum(axis=1)
            assert ((outward < 0) if pr.reverse else (outward > 0)).all(), pr.index
        else:
            minus_z = -np.array(pr.M[:3, 2], dtype=float)   # the matrices here are rotations and translations
            assert np.allclose(ref.n[own], minus_z / np.linalg.norm(minus_z), atol=1e-15), pr.index

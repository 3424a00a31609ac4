"""The adversarial ray families of tests/adversarial_rays.py on the oracle alone (no
GPU), so that tests/test_gpu_adversarial_rays.py cannot pass vacuously: every sweep
straddles its boundary, the families that must not panic do not, NaN stays where it
is expected, every primitive is some ray's closest hit, and the counts are pinned.

Two things differ from what the planning of these tests expected, both the
reference's own behaviour (oracle_intersect restates sphere.go / efloat.go):

- `huge` has hits whose p and n are NaN: an origin 1e90 or more away from a unit
  sphere is a hit (the quadratic's interval contains 0), whose refined hit point
  pHit * radius / Distance(pHit, 0) is 0 * inf. So NaN inside a hit row occurs in
  `huge` as well as in `disk_plane` (the centre rays) and `degenerate`; it is pinned
  there and must be absent everywhere else.
- rays at moderate coordinates can panic, or hit with a NaN normal: a tangent ray
  that starts on the sphere (a = 2, b = c = 0), which the face centre of a sphere's
  bounding box is; a line within 1e-154 radii of a sphere's z axis (x^2 + y^2
  underflows, the pole substitution does not apply). The `axis` and `poles` families
  stay clear of both (the cap of 0 panics holds for them); the rays themselves are
  kept, in `degenerate`, where a panic and a NaN are allowed.
"""
import numpy as np
import pytest

import adversarial_rays as A

SCENE_KEYS = list(A.SCENES)
NO_PANIC = [f for f in A.FAMILIES if f not in ("huge", "degenerate")]
NAN_FAMILIES = ("disk_plane", "degenerate", "huge")

# (hits, misses, panics, distinct primitives hit, hit rows with a NaN element) of the oracle
PINNED = {
    "small1": {
        "axis": (1335, 4257, 0, 16, 0),
        "poles": (960, 160, 0, 12, 0),
        "disk_plane": (88, 168, 0, 5, 1),
        "inside": (308, 76, 0, 14, 0),
        "sweeps": (410, 685, 0, 16, 0),
        "huge": (1857, 605, 1570, 16, 684),
        "degenerate": (200, 287, 217, 14, 95),
        "random": (48, 1952, 0, 11, 0),
    },
    "small4": {
        "axis": (1404, 4572, 0, 18, 0),
        "poles": (960, 160, 0, 12, 0),
        "disk_plane": (152, 360, 0, 5, 19),
        "inside": (308, 76, 0, 14, 0),
        "sweeps": (461, 739, 0, 18, 0),
        "huge": (2182, 748, 1606, 17, 963),
        "degenerate": (206, 325, 219, 15, 101),
        "random": (48, 1952, 0, 11, 0),
    },
    "large": {
        "axis": (4364, 7312, 0, 58, 0),
        "poles": (4160, 160, 0, 52, 0),
        "disk_plane": (168, 344, 0, 7, 19),
        "inside": (1268, 76, 0, 54, 0),
        "sweeps": (1226, 2374, 0, 58, 0),
        "huge": (2170, 748, 1618, 26, 840),
        "degenerate": (205, 325, 220, 15, 100),
        "random": (35, 1965, 0, 19, 0),
    },
}
# (primitives, nodes, leaves)
TREES = {"small1": (16, 31, 16), "small4": (18, 33, 17), "large": (58, 113, 57)}


def counts(want):
    pan = A.panicked(want)
    hit = want[:, 0] == 1
    nan_rows = np.isnan(want[hit]).any(axis=1)
    miss = want[want[:, 0] == 0]
    assert not np.isnan(np.delete(miss, 1, axis=1)).any()   # a miss row is (0, TMax, -1, 0 ...): NaN only as its own TMax
    return int(hit.sum()), int((want[:, 0] == 0).sum()), int(pan.sum()), len(set(want[hit, 2])), int(nan_rows.sum())


@pytest.mark.parametrize("key", SCENE_KEYS)
def test_trees(key):
    d = A.SCENES[key]().desc
    leaves = sum(1 for i in range(d.n_nodes) if d.nodes[i].n_prims > 0)
    print(f"{key}: {d.n_prims} primitives, {d.n_nodes} nodes, {leaves} leaves")
    assert (d.n_prims, d.n_nodes, leaves) == TREES[key]
    if key == "large":
        assert d.n_nodes > 64      # kLdsNodes: the [64]-stack walk only
    else:
        assert d.n_nodes <= 64 and leaves <= 32   # LDS-staged, and the host may form culling groups
    if key != "small1":   # several primitives in a leaf: the leaf_prims loop, n_leaves != n_prims
        assert leaves < d.n_prims and max(d.nodes[i].n_prims for i in range(d.n_nodes)) == 2
    assert d.n_meshes == 0
    # every transform's m_inv is its m's inverse (Transform.Mul's is not where its operands do not commute)
    mats = [d.shapes[i].object_to_world for i in range(d.n_shapes)] + [d.prims[i].prim_to_world for i in range(d.n_prims)
                                                                      if d.prims[i].kind == A.abi.PBRT_PRIM_TRANSFORMED]
    for t in mats:
        m = np.array([list(row) for row in t.m.m])
        mi = np.array([list(row) for row in t.m_inv.m])
        assert np.allclose(m @ mi, np.eye(4), atol=1e-14)


@pytest.mark.parametrize("key", SCENE_KEYS)
def test_the_scene_has_every_edge_shape(key):
    sh = A.shapes(A.SCENES[key]())
    spheres = [s for s in sh if s.kind == "sphere"]
    disks = [s for s in sh if s.kind == "disk"]
    d = A.SCENES[key]().desc
    rev = {i for i in range(d.n_prims) if d.shapes[d.prims[i].shape].reverse_orientation}
    assert len([s for s in spheres if A.partial(s)]) == 2 and len(rev) == 2
    assert any(A.partial(s) and s.prim in rev for s in spheres) and any(not A.partial(s) and s.prim in rev for s in spheres)
    assert any(s.inner > 0 and s.phi_max < 2 * np.pi for s in disks) and any(s.inner == 0 and not A.partial(s) for s in disks)
    assert sum(1 for s in spheres if np.linalg.det(s.M[:3, :3]) > 0 and not s.rigid
               and (np.abs(s.M[:3, :3]) < 1e-9).sum() == 1) == 1   # RotateX . RotateZ: one zero in the matrix
    assert len([s for s in spheres if s.radius == 0.3]) == A.N_ROW
    assert len({tuple(np.round(s.centre, 9)) for s in spheres}) == len(spheres)


@pytest.mark.parametrize("key", SCENE_KEYS)
def test_ray_budget(key):
    sizes = {f: A.rays(key, f).shape for f in A.FAMILIES}
    assert all(s[1] == 7 for s in sizes.values())
    total = sum(s[0] for s in sizes.values())
    print(key, total, sizes)
    assert sizes["random"][0] == 2000 and total <= 30_000


@pytest.mark.parametrize("key", SCENE_KEYS)
def test_every_sweep_straddles_its_boundary(key):
    scene = A.SCENES[key]()
    want, _ = A.oracle(key, "sweeps")
    index = A.sweep_index(scene)
    assert len(index) * A.SWEEP_N == want.shape[0]
    by_name = {}
    for sw in index:
        w = want[sw.start:sw.start + A.SWEEP_N]
        hits, misses = int((w[:, 0] == 1).sum()), int((w[:, 0] == 0).sum())
        by_name.setdefault(sw.name, []).append((sw.prim, hits, misses))
        if sw.prims is None:
            assert hits >= 1 and misses >= 1 and hits + misses == A.SWEEP_N, (sw, hits, misses)
            assert set(w[w[:, 0] == 1, 2]) == {float(sw.prim)}, sw   # a sweep's ray can meet its own shape only
        else:
            assert set(sw.prims) <= set(w[:, 2]), sw
    print(key, by_name)
    sh = A.shapes(scene)
    n_sph = sum(1 for s in sh if s.kind == "sphere")
    part_sph = [s for s in sh if s.kind == "sphere" and A.partial(s)]
    disks = [s for s in sh if s.kind == "disk"]
    have = {k: len(v) for k, v in by_name.items()}
    assert have["tangent"] == n_sph and have["tmax_t1"] == n_sph           # one per sphere
    assert have["tmax_t0"] == len(sh) and have["cross"] == len(sh)         # one per shape
    assert have["z_min"] == len(part_sph) == 2 and have["z_max"] == 2
    n_phi = len(part_sph) + sum(1 for s in disks if A.partial(s))
    assert have["phi_max"] == n_phi and have["phi_seam"] == n_phi
    assert have["radius"] == len(disks) and have["inner_radius"] == sum(1 for s in disks if s.inner > 0)


def test_sweep_values():
    v = A.sweep_values(2.0)
    assert len(v) == A.SWEEP_N == 15 and v[0] == 2.0
    u = np.spacing(2.0)
    assert sorted(v[:7]) == [2 - 8 * u, 2 - 2 * u, 2 - u, 2.0, 2 + u, 2 + 2 * u, 2 + 8 * u]
    assert np.allclose(sorted(abs(x / 2.0 - 1) for x in v[7:]), sorted([1e-15, 1e-12, 1e-9, 1e-6] * 2), rtol=0.2, atol=0)


@pytest.mark.parametrize("family", list(A.FAMILIES))
@pytest.mark.parametrize("key", SCENE_KEYS)
def test_pinned_counts(key, family):
    want, wocc = A.oracle(key, family)
    got = counts(want)
    print(f"{key} {family}: (hits, misses, panics, prims, NaN hit rows) = {got}")
    assert got == PINNED[key][family]
    hits, misses, panics, _, nan_rows = got
    assert hits + misses + panics == A.rays(key, family).shape[0]
    if family in NO_PANIC:
        assert panics == 0
    if family == "huge":   # the `moderate` guard and EFloat's checks: both outcomes
        assert panics >= 1 and hits + misses >= 1
    if family not in NAN_FAMILIES:
        assert nan_rows == 0
    # the oracle's any-hit answers are its closest-hit answers (a panic in one is a panic in the other)
    pan = A.panicked(want)
    assert np.array_equal(pan, np.isnan(wocc))
    assert np.array_equal(want[~pan, 0] == 1, wocc[~pan] == 1)


@pytest.mark.parametrize("key", SCENE_KEYS)
def test_every_primitive_is_some_rays_closest_hit(key):
    seen = set()
    for family in A.FAMILIES:
        want, _ = A.oracle(key, family)
        seen |= set(want[want[:, 0] == 1, 2].astype(int))
    assert seen == set(range(A.SCENES[key]().desc.n_prims))


@pytest.mark.parametrize("key", SCENE_KEYS)
def test_the_families_hold_what_they_name(key):
    """Zero components of both signs, origins on box planes, exact pole lines, in-plane
    disk rays, every TMax of the list, denormal and huge components, NaN and zero directions."""
    scene = A.SCENES[key]()
    ax = A.rays(key, "axis")
    d = ax[:, 3:6]
    assert ((d == 0) & ~np.signbit(d)).any() and ((d == 0) & np.signbit(d)).any()
    assert {float("inf"), 0.0, 5e-324, 1.0} <= set(ax[:, 6])
    lo, hi = A.root_box(scene)
    assert all((ax[:, a] == lo[a]).any() and (ax[:, a] == hi[a]).any() for a in range(3))
    nodes = scene.desc.nodes
    for i in range(scene.desc.n_nodes):   # an origin on a plane of every node, with a zero direction component along it
        on = (ax[:, 0] == nodes[i].bmin[0]) | (ax[:, 0] == nodes[i].bmax[0])
        assert (on & (ax[:, 3] == 0)).any(), i
    hg = A.rays(key, "huge")
    assert (np.abs(hg[:, :3]).max(axis=1) >= 1e300).any() and (np.abs(hg[:, :3]).max(axis=1) < 1e100).any()
    assert (np.abs(hg[:, 3:6]) == 5e-324).any() and (np.abs(hg[:, 3:6]) == 1e-310).any()
    dg = A.rays(key, "degenerate")
    assert (dg[:, 3:6] == 0).all(axis=1).any() and np.isnan(dg[:, :6]).any(axis=1).sum() >= 6
    assert np.isnan(dg[:, 6]).any() and (dg[:, 6] < 0).any()
    sh = [s for s in A.shapes(scene) if s.kind == "sphere" and s.rigid]
    po = A.rays(key, "poles")
    for s in sh:   # on the object-space z axis, exactly
        assert ((po[:, 0] == s.centre[0]) & (po[:, 1] == s.centre[1]) & (po[:, 3] == 0) & (po[:, 4] == 0)).any()

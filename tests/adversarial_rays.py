"""Scenes and ray families aimed at the decision boundaries of the BVH walks and of
the sphere and disk intersection tests (host-side builder and numpy only: no GPU).

Read by tests/test_adversarial_rays_host.py (the families on the oracle alone:
every sweep straddles its boundary, the counts are pinned) and by
tests/test_gpu_adversarial_rays.py (device against oracle, bit for bit).

Scenes: edge_small(1), edge_small(4), edge_large(). The shapes stand far enough
apart that a ray of a sweep, which stays within 2 radii of its shape's centre, can
meet that shape only: where it misses the shape it misses the scene.

A family is a function of the built scene that returns (n, 7) rows of o, d, TMax.
Every family reads the geometry from the scene's descriptor (desc.prims,
desc.shapes, desc.nodes): rays are written in a shape's object space and mapped
to the world with the primitive's own matrices, so t is the object-space t.
"""
import functools
from collections import namedtuple

import numpy as np

import pbrtgpu as G
from pbrtgpu import abi

INF = float("inf")
NAN = float("nan")
DENORM = 5e-324

# ----------------------------------------------------------------------- scenes
N_ROW = 8        # small spheres in a row (the culling groups' leaves)
N_EDGE = 8 + N_ROW   # (the nested disk, where a scene has it, comes after)


def _edge_shapes(s, m, nested):
    """The 16 edge primitives (nested: 18): two rows 8 apart (z = 0 and z = 10) and a row of small spheres
    (z = 20). A composite transform is split between the shape and a TransformedPrimitive
    (or rebuilt from its matrix), so that every m_inv is the inverse of its m: Transform.Mul
    multiplies the inverses in the operands' order (transform.go:179-184), which is the inverse only
    where the operands commute."""
    s.add_primitive(s.add_sphere(G.translate(-12, 0, 0), 1.5), m)                     # a full sphere
    s.add_primitive(s.add_sphere(G.translate(-4, 0, 0), 1.25, reverse=True), m)       # reversed
    # tests/test_gpu_edges.py's partial spheres: z axis up (RotateX(-90))
    cap = s.add_sphere(G.rotate(0, -90), 2.0, z_min=-1.0, z_max=1.2, phi_max=270.0)
    s.add_primitive(cap, m, G.translate(4.0, 0.0, 0.0))
    band = s.add_sphere(G.rotate(0, -90), 2.0, z_min=-0.6, z_max=0.9, phi_max=200.0, reverse=True)
    s.add_primitive(band, m, G.translate(12.0, 0.0, 0.0))
    s.add_primitive(s.add_disk(G.translate(-12, 0, 10), 0.0, 2.0, inner=0.75, phi_max=300.0), m)   # annular, a sector missing
    if nested:
        # a disk and a ring in the annular disk's hole, concentric and in its plane: primitives whose
        # centroids coincide are never split (bvh.go: centroidBounds.pMax[dim] == pMin[dim] makes a
        # leaf), so once the build has two of the three alone in a node they share a leaf
        s.add_primitive(s.add_disk(G.translate(-12, 0, 10), 0.0, 0.5), m)
        s.add_primitive(s.add_disk(G.translate(-12, 0, 10), 0.0, 0.6875, inner=0.5625), m)
    s.add_primitive(s.add_disk(G.rotate(0, 90), 0.5, 2.0), m, G.translate(-4.0, 0.0, 10.0))       # plain, upright
    # a mirrored object-to-world inside a mirrored TransformedPrimitive
    s.add_primitive(s.add_sphere(G.scale(1, 1, -1), 1.5), m, proper(G.mul(G.translate(4.0, 0.0, 10.0), G.scale(-1, 1, 1))))
    # RotateX . RotateZ: no axis of the object space is an axis of the world
    s.add_primitive(s.add_sphere(proper(G.mul(G.rotate(0, 30), G.rotate(2, 40))), 1.5), m, G.translate(12.0, 0.0, 10.0))
    for i in range(N_ROW):
        s.add_primitive(s.add_sphere(G.translate(-10.5 + 3.0 * i, 0, 20), 0.3), m)


def proper(t):
    """t's matrix with its true inverse (pbrt_new_transform)."""
    out = abi.Transform()
    G.lib().pbrt_new_transform(G.C.byref(t.m), G.C.byref(out))
    return out


def _finish(s, max_prims_in_node):
    s.add_point_light(G.translate(0, 20, 8), (100, 100, 100))
    s.set_film(32, 32)
    s.set_camera(G.look_at((0, 40, 55), (0, 0, 16), (0, 1, 0)), fov=50)
    return s.build(max_prims_in_node=max_prims_in_node)


@functools.lru_cache(maxsize=None)
def edge_small(max_prims_in_node=1):
    s = G.Scene()
    _edge_shapes(s, s.add_matte((0.5, 0.5, 0.5)), nested=max_prims_in_node > 1)
    return _finish(s, max_prims_in_node)


@functools.lru_cache(maxsize=None)
def edge_large(seed=11):
    """edge_small's shapes and 40 filler spheres on a jittered 8 x 5 grid behind them (z >= 27):
    58 primitives."""
    rng = np.random.default_rng(seed)
    s = G.Scene()
    m = s.add_matte((0.5, 0.5, 0.5))
    _edge_shapes(s, m, nested=True)
    for j in range(5):
        for i in range(8):
            c = np.array([-10.5 + 3.0 * i, 0.0, 28.0 + 3.0 * j]) + rng.uniform(-0.4, 0.4, 3)
            s.add_primitive(s.add_sphere(G.translate(*c), rng.uniform(0.25, 0.45)), m)
    return _finish(s, 1)


SCENES = {"small1": lambda: edge_small(1), "small4": lambda: edge_small(4), "large": edge_large}

# -------------------------------------------------------------------- geometry
Shape = namedtuple("Shape", "prim kind M rigid radius z_min z_max phi_max height inner centre")


def _mat(t):
    return np.array([[t.m.m[i][j] for j in range(4)] for i in range(4)], dtype=np.float64)


def shapes(scene):
    """One Shape per primitive of the descriptor, in its (BVH) order. M: object to world,
    through the primitive's transform; rigid: M's linear part is the identity (a ray
    keeps its direction's bits, -0.0 included). Sphere: kind "sphere", disk: "disk"."""
    d = scene.desc
    out = []
    for i in range(d.n_prims):
        p = d.prims[i]
        sd = d.shapes[p.shape]
        M = _mat(sd.object_to_world)
        if p.kind == abi.PBRT_PRIM_TRANSFORMED:
            M = _mat(p.prim_to_world) @ M
        kind = "sphere" if sd.type == abi.PBRT_SHAPE_SPHERE else "disk"
        h = sd.height if kind == "disk" else 0.0
        centre = M[:3, :3] @ np.array([0.0, 0.0, h]) + M[:3, 3]
        out.append(Shape(i, kind, M, bool(np.array_equal(M[:3, :3], np.eye(3))), sd.radius, sd.z_min, sd.z_max,
                         sd.phi_max, h, sd.inner_radius, centre))
    return out


def edge_shapes(scene):
    """The edge shapes without the fillers of edge_large (which stand at z >= 27)."""
    return [sh for sh in shapes(scene) if sh.centre[2] < 25]


def partial(sh):
    if sh.kind == "disk":
        return sh.phi_max < 2 * np.pi
    return sh.z_min > -sh.radius or sh.z_max < sh.radius or sh.phi_max < 2 * np.pi


def world(sh, o, d, tmax=INF):
    """An object-space ray of sh as a world-space row."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    if sh.rigid:   # exact: a translation (and the zero signs of d survive)
        return np.concatenate([o + sh.M[:3, 3], d, [tmax]])
    return np.concatenate([sh.M[:3, :3] @ o + sh.M[:3, 3], sh.M[:3, :3] @ d, [tmax]])


def surface_point(sh, phi=None, z=None):
    """A point on the kept part of sh, object space: at azimuth phi (default: a
    twelfth of phi_max, 30 degrees on a full shape) and height z (default: the
    middle of the kept z range) on a sphere; mid-annulus on a disk."""
    phi = sh.phi_max / 12 if phi is None else phi
    if sh.kind == "disk":
        rho = 0.5 * (sh.inner + sh.radius)
        return np.array([rho * np.cos(phi), rho * np.sin(phi), sh.height])
    z = 0.5 * (sh.z_min + sh.z_max) if z is None else z
    rho = np.sqrt(max(sh.radius * sh.radius - z * z, 0.0))
    return np.array([rho * np.cos(phi), rho * np.sin(phi), z])


def root_box(scene):
    n = scene.desc.nodes[0]
    return np.array(list(n.bmin)), np.array(list(n.bmax))


AXES = [np.array(v, dtype=np.float64) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
DIAGONALS = [np.array(v, dtype=np.float64) for v in ((1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1))]


def zero_signs(dirs):
    """Every direction with its zero components as +0.0 and as -0.0."""
    out = []
    for d in dirs:
        out.append(d + 0.0)
        out.append(np.where(d == 0, -0.0, d))
    return out


def _rows(rows):
    a = np.array(rows, dtype=np.float64).reshape(-1, 7)
    a.setflags(write=False)
    return a


# --------------------------------------------------------------------- families
def axis(scene):
    """Axis directions and face diagonals, zero components of both signs: through every
    shape's centre line (a disk's: the line through its mid-annulus point, its centre is
    disk_plane's), TMax inf, the far side and one of 0, 5e-324, 1 in turn; and from origins on the
    planes of every BVH node's box (its two corners; a point of each of its six faces with the
    diagonals, of which four lie in the face's plane) and on the root's faces."""
    rows = []
    dirs = zero_signs(AXES + DIAGONALS)
    for sh in shapes(scene):
        c = sh.centre if sh.kind == "sphere" else world(sh, surface_point(sh), (0, 0, 1))[:3]
        r = sh.radius
        for k, d in enumerate(dirs):
            o = c - 3 * r * d
            far = 3 * r + r / np.linalg.norm(d)
            for tmax in (INF, far, (0.0, DENORM, 1.0)[(sh.prim + k) % 3]):
                rows.append(np.concatenate([o, d, [tmax]]))
    nodes, n_nodes = scene.desc.nodes, scene.desc.n_nodes
    tmaxes = (INF, 0.0, DENORM, 1.0, float(np.linalg.norm(np.subtract(*root_box(scene)))))
    k = 0
    for i in range(scene.desc.n_nodes):
        lo, hi = np.array(list(nodes[i].bmin)), np.array(list(nodes[i].bmax))
        mid = lo + 0.375 * (hi - lo)   # (not the face's centre: on a sphere's box that is a point of the sphere)
        for o in ((lo, hi) if n_nodes <= 64 else (lo, hi)[i % 2:][:1]):   # large trees: one corner per node
            for d in dirs:
                rows.append(np.concatenate([o, d, [INF if k % 3 else tmaxes[(k // 3) % 5]]]))
                k += 1
        for a in range(3):
            for face in ((lo, hi) if n_nodes <= 64 else (lo, hi)[(i + a) % 2:][:1]):   # large trees: one face per axis
                o = mid.copy()
                o[a] = face[a]
                for d in zero_signs(DIAGONALS):
                    rows.append(np.concatenate([o, d, [INF if k % 3 else tmaxes[(k // 3) % 5]]]))
                    k += 1
    lo, hi = root_box(scene)
    mid = lo + 0.375 * (hi - lo)
    for a in range(3):
        for face in (lo, hi):
            o = mid.copy()
            o[a] = face[a]
            for d in dirs:
                for tmax in tmaxes:
                    rows.append(np.concatenate([o, d, [tmax]]))
    return _rows(rows)


def poles(scene):
    """Rays along each sphere's object-space z axis (sphere.go's ph.x == 0 && ph.y == 0
    substitution), from both ends and from the centre, zero components of both signs, and
    lines next to the axis by 1e-17 and 1e-150 radii (x^2 + y^2 does not underflow; where it
    does, the reference's normal is NaN: those lines are in `degenerate`). On the cap and the
    band the pole itself is cut off."""
    rows = []
    for sh in shapes(scene):
        if sh.kind != "sphere":
            continue
        r = sh.radius
        for k, off in enumerate((0.0, -0.0, 1e-17 * r, -1e-17 * r, 1e-150 * r)):
            for oy in (0.0, off):
                for dz in (1.0, -1.0):
                    for z0 in (-3 * r * dz, 0.0):
                        zero = -0.0 if k % 2 else 0.0
                        rows.append(world(sh, (off, oy, z0), (zero, zero, dz)))
                        rows.append(world(sh, (off, oy, z0), (zero, zero, dz), 3 * r))
    return _rows(rows)


def disk_plane(scene):
    """Rays in each disk's plane (d.z == 0 in object space, +0.0 and -0.0), in the
    planes one ulp and a denormal off it, and rays through the disk's exact centre,
    where the oracle's normal is NaN (on the annular disk the centre is the hole)."""
    rows = []
    for sh in shapes(scene):
        if sh.kind != "disk":
            continue
        h, r = sh.height, sh.radius
        heights = (h, np.nextafter(h, INF), np.nextafter(h, -INF), h + DENORM)
        for z in heights:
            for zero in (0.0, -0.0):
                for a in np.radians((0, 30, 90, 135, 180, 270, 300)):
                    c, s = np.cos(a), np.sin(a)
                    rows.append(world(sh, (-3 * r * c, -3 * r * s, z), (c, s, zero)))        # through the axis
                    rows.append(world(sh, (-3 * r * c - s, -3 * r * s + c, z), (c, s, zero)))   # a chord
                rows.append(world(sh, (0.0, 0.0, z), (1.0, 0.0, zero)))                     # from the centre
        for dz in (1.0, -1.0):
            rows.append(world(sh, (0.0, 0.0, h - 2 * dz), (0.0, 0.0, dz)))
            rows.append(world(sh, (-0.0, -0.0, h - 2 * dz), (-0.0, -0.0, dz)))
            rows.append(world(sh, (-dz, -dz, h - dz), (dz, dz, dz)))                        # oblique, through (0, 0, h)
            rows.append(world(sh, (0.0, 0.0, h - 2 * dz), (0.0, 0.0, dz), 2.0))             # TMax at the plane
    return _rows(rows)


def inside(scene, per_sphere=24, seed=21):
    """Origins inside each sphere with random directions; for a partial sphere also its
    centre and origins on its clip planes (the near root is clipped or behind: t1)."""
    rng = np.random.default_rng(seed)
    rows = []
    for sh in shapes(scene):
        if sh.kind != "sphere":
            continue
        r = sh.radius
        origins = []
        for _ in range(per_sphere):
            v = rng.normal(size=3)
            origins.append(v / np.linalg.norm(v) * r * 0.95 * rng.uniform() ** (1 / 3))
        if partial(sh):
            origins += [np.zeros(3)] * 8
            for z in (sh.z_min, sh.z_max):
                rho = np.sqrt(r * r - z * z)
                for _ in range(8):
                    a, q = rng.uniform(0, 2 * np.pi), rho * 0.9 * np.sqrt(rng.uniform())
                    origins.append(np.array([q * np.cos(a), q * np.sin(a), z]))
        for o in origins:
            rows.append(world(sh, o, rng.normal(size=3)))
    return _rows(rows)


# ----------------------------------------------------------------------- sweeps
SWEEP_ULPS = (0, 1, -1, 2, -2, 8, -8)
SWEEP_REL = (1e-15, 1e-12, 1e-9, 1e-6)
SWEEP_N = len(SWEEP_ULPS) + 2 * len(SWEEP_REL)   # 15 rays per sweep


def sweep_values(p0):
    """p0 + k ulp(p0) for k in {0, +-1, +-2, +-8} and p0 (1 +- r) for r in {1e-15, 1e-12, 1e-9, 1e-6}."""
    u = np.spacing(abs(p0))
    return [p0 + k * u for k in SWEEP_ULPS] + [p0 * (1 + s * r) for r in SWEEP_REL for s in (1, -1)]


Sweep = namedtuple("Sweep", "name prim start prims", defaults=(None,))


def _sweeps(scene):
    """(rows, [Sweep]): sweep i is rows[start : start + SWEEP_N]. Each ray starts within 2
    radii of its shape's centre and its TMax ends there, so a miss of the shape is a miss of the scene. prims: a
    sweep across which the closest primitive changes instead (none so far)."""
    rows, index = [], []

    def add(name, sh, p0, ray):
        index.append(Sweep(name, sh.prim, len(rows)))
        for p in sweep_values(p0):
            rows.append(ray(p))

    for sh in shapes(scene):
        r = sh.radius
        hp = surface_point(sh)
        if sh.kind == "sphere":
            # exact where nothing clips: phi = 0 on a full sphere, so o.x = c.x + p under a translation
            phi = sh.phi_max / 12 if partial(sh) else 0.0
            zt = 0.5 * (sh.z_min + sh.z_max) if partial(sh) else 0.0
            c, s = np.cos(phi), np.sin(phi)
            rho = np.sqrt(r * r - zt * zt)
            # tangency: a ray along the z axis at distance p from it; disc = 0 at p = radius
            add("tangent", sh, r, lambda p: world(sh, (p * c, p * s, -2 * r), (0.0, 0.0, 1.0), 4 * r))
            # TMax around the closest hit: o = 2 h, d = -h meets the surface point h at t = 1 (and t = 3)
            h0 = np.array([rho * c, rho * s, zt]) if partial(sh) else np.array([r, 0.0, 0.0])
            add("tmax_t0", sh, 1.0, lambda p: world(sh, 2 * h0, -h0, p))
            # TMax around t1 from the centre: t0 = -1, t1 = 1
            add("tmax_t1", sh, 1.0, lambda p: world(sh, (0.0, 0.0, 0.0), h0, p))
            # the origin moved across the surface along the ray: o = p h, t0 = p - 1 changes sign;
            # TMax 1 keeps t1 = p + 1 out, so "t0.lo <= 0" reads as a miss
            add("cross", sh, 1.0, lambda p: world(sh, p * h0, -h0, 1.0))
            if sh.z_min > -r:
                add("z_min", sh, sh.z_min, lambda p: world(sh, (2 * r * c, 2 * r * s, p), (-r * c, -r * s, 0.0), 2.0))
            if sh.z_max < r:
                add("z_max", sh, sh.z_max, lambda p: world(sh, (2 * r * c, 2 * r * s, p), (-r * c, -r * s, 0.0), 2.0))
            if sh.phi_max < 2 * np.pi:
                def at_phi(p):
                    h = np.array([rho * np.cos(p), rho * np.sin(p), zt])
                    return world(sh, 2 * h, -h, 2.0)   # TMax 2: the far root (t = 3) stays out
                add("phi_max", sh, sh.phi_max, at_phi)
                add("phi_seam", sh, 2 * np.pi, at_phi)
        else:
            down = (0.0, 0.0, -1.0)
            add("tmax_t0", sh, 2.0, lambda p: world(sh, hp + (0, 0, 2), down, p))
            # the origin moved across the plane: above it t = p - 1 > 0, below it the ray leaves
            add("cross", sh, 1.0, lambda p: world(sh, hp + (0, 0, p - 1.0), down, 1.0))
            h = sh.height
            add("radius", sh, r, lambda p: world(sh, (p, 0.0, h + 2), down, 3.0))
            if sh.inner > 0:
                add("inner_radius", sh, sh.inner, lambda p: world(sh, (p, 0.0, h + 2), down, 3.0))
            if sh.phi_max < 2 * np.pi:
                rho = 0.5 * (sh.inner + r)

                def at_phi(p):
                    return world(sh, (rho * np.cos(p), rho * np.sin(p), h + 2), down, 3.0)
                add("phi_max", sh, sh.phi_max, at_phi)
                add("phi_seam", sh, 2 * np.pi, at_phi)
    return _rows(rows), index


def sweeps(scene):
    return _sweeps(scene)[0]


def sweep_index(scene):
    return _sweeps(scene)[1]


# ------------------------------------------------------------- huge, degenerate
HUGE = (1e90, 1e100, 1e150, 1e154, 1e160, 1e300, 1e308)


def huge(scene):
    """Origins and directions of magnitude 1e90 .. 1e308 along the axes and the face
    diagonals, aimed at the first N_EDGE shapes' centres (on some the reference's
    `moderate` guard holds, on others not, and EFloat panics on many), and denormal
    direction components."""
    rows = []
    for sh in edge_shapes(scene):
        c, r = sh.centre, sh.radius
        for u in AXES + DIAGONALS:
            for m in HUGE:
                rows.append(np.concatenate([c - m * u, u, [INF]]))           # a huge origin
                rows.append(np.concatenate([c - 3 * r * u, m * u, [INF]]))   # a huge direction
            rows.append(np.concatenate([c - 1e300 * u, 1e300 * u, [INF]]))
            for tiny in (DENORM, 1e-310):
                rows.append(np.concatenate([c - 3 * r * u, tiny * u, [INF]]))
                rows.append(np.concatenate([c - 3 * r * u, u + tiny * (u == 0), [INF]]))
                rows.append(np.concatenate([c - 3 * r * u, u + tiny * (u == 0), [1e300]]))
    return _rows(rows)


def degenerate(scene):
    """d = (0, 0, 0); one NaN component in d or in o; TMax NaN, negative or -0.0. No loop
    of a walk depends on the ray, so every walk ends; the oracle's answer is the expectation.
    Two more kinds the oracle answers with a panic or a NaN at moderate coordinates: a line
    next to a sphere's z axis by a denormal or 1e-300 (x^2 + y^2 underflows to 0 and the
    ph.x == 0 && ph.y == 0 substitution does not apply: a hit with a NaN normal), and a
    tangent ray from a point of the sphere (a = 2, b = c = 0: EFloat panics)."""
    rows = []
    for sh in edge_shapes(scene):
        sp = surface_point(sh)
        base = world(sh, sp + (0, 0, 2), (0, 0, -1)) if sh.kind == "disk" else world(sh, 2 * sp, -sp)   # hits sh
        if sh.kind == "sphere":
            r = sh.radius
            for off in (DENORM, 1e-300):
                for oy in (0.0, off):
                    for dz in (1.0, -1.0):
                        rows.append(world(sh, (off, oy, -2 * r * dz), (0.0, 0.0, dz)))
                        rows.append(world(sh, (off, oy, 0.0), (-0.0, -0.0, dz)))
            for o, d in (((0, -r, 0), (1, 0, 1)), ((0, r, 0), (1, -0.0, -1)), ((r, 0, 0), (0, 1, 1)), ((0, 0, -r), (1, 1, 0))):
                rows.append(world(sh, o, d))
                rows.append(world(sh, o, d, 1.0))
        for o in (base[:3], sh.centre, world(sh, surface_point(sh), (0, 0, 1))[:3]):
            for zero in (0.0, -0.0):
                rows.append(np.concatenate([o, [zero] * 3, [INF]]))
                rows.append(np.concatenate([o, [zero] * 3, [1.0]]))
        for k in range(6):
            row = base.copy()
            row[k] = NAN
            rows.append(row)
        for tmax in (NAN, -1.0, -INF, -0.0, -DENORM):
            row = base.copy()
            row[6] = tmax
            rows.append(row)
    return _rows(rows)


def random(scene, n=2000, seed=3):
    """The control: tests/test_gpu_query.py's random_rays over this scene's box (origins
    uniform in the root box grown by half its size, normal directions, a fifth of the
    rays with a finite TMax)."""
    rng = np.random.default_rng(seed)
    lo, hi = root_box(scene)
    o = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), size=(n, 3))
    d = rng.normal(size=(n, 3))
    tmax = np.where(rng.uniform(size=n) < 0.2, rng.uniform(1, 40, size=n), np.inf)
    return _rows(np.concatenate([o, d, tmax[:, None]], axis=1))


FAMILIES = {"axis": axis, "poles": poles, "disk_plane": disk_plane, "inside": inside, "sweeps": sweeps, "huge": huge,
            "degenerate": degenerate, "random": random}


@functools.lru_cache(maxsize=None)
def rays(scene_key, family):
    """FAMILIES[family] on SCENES[scene_key]: computed once, read-only."""
    return FAMILIES[family](SCENES[scene_key]())


@functools.lru_cache(maxsize=None)
def oracle(scene_key, family):
    """(closest rows, any-hit flags) of the oracle on rays(scene_key, family): computed once, read-only."""
    import oracle_lib as O
    desc = SCENES[scene_key]().desc
    want = O.intersect(desc, rays(scene_key, family), closest=True)
    wocc = O.intersect(desc, rays(scene_key, family), closest=False)
    want.setflags(write=False)
    wocc.setflags(write=False)
    return want, wocc


def panicked(want):
    """Rows on which the reference panics: NaN in column 0 (oracle_intersect)."""
    return np.isnan(want[:, 0])

"""A brute-force closest-hit and any-hit over the spheres and disks of a scene
descriptor, written from the geometry and independent of the oracle, and ray
families on which its answer does not depend on anybody's rounding.

Read by tests/test_analytic_reference_host.py (the oracle against this reference)
and by tests/test_gpu_analytic_reference.py (every device walk against it, not
through the oracle). numpy and the host-side scene builder only: no GPU.

The reference (intersect). No BVH and no error intervals. Per primitive it composes
the object-to-world matrix in longdouble (the shape's transform inside the
primitive's), inverts it itself (the descriptor's m_inv is not read), maps the ray
to object space (t is unchanged by an affine map) and solves there:

- sphere: the quadratic a t^2 + b t + c = 0, by the cancellation-free form
  q = -(b + sign(b) sqrt(disc)) / 2, roots q / a and c / q, taken in order. A root
  counts if 0 < t <= TMax and its point passes the clips: z >= z_min where
  z_min > -radius, z <= z_max where z_max < radius, phi <= phi_max where
  phi_max < 2 pi, phi = atan2(y, x) brought into [0, 2 pi). The first root that
  counts is the primitive's hit.
- disk: the root of the plane z = height. It counts if 0 < t <= TMax,
  inner <= rho <= radius and, on a sector, phi <= phi_max. A ray parallel to the
  plane never hits.

The closest hit is the smallest t over all primitives; the any-hit flag is whether
any root counts, which is the closest-hit flag.

The normal. The unit geometric normal in world space, M^-T n_obj normalised, with
n_obj the outward normal p / radius of a sphere and (0, 0, -1) of a disk:
sphere.go and disk.go give dpdu x dpdv, which is outward on a sphere (theta_max -
theta_min is negative) and object -z on a disk. interaction.go flips it where
reverseOrientation differs from transformSwapsHandedness; no constructor of the
reference sets transformSwapsHandedness, so the rule is: flipped where `reverse` is
set, and a mirroring transform flips nothing (M^-T keeps a normal on its side of
the surface whatever M's handedness, and the TransformedPrimitive maps the normal
with its own M^-T again). So: outward on spheres, the doubly mirrored one
included, inward where reverse is set, object -z on every disk.

Decidability. intersect also returns `decided`. A ray is undecided if a quantity
that a decision rests on lies within the relative margin EPS of its boundary, on
any primitive whose root in question could be the answer (it is not decidedly
behind a hit that is certain):

- the discriminant against 0, relative to b^2 + |4 a c|;
- a root against 0 and against TMax, relative to |t| + |o| / |d|;
- z against z_min and z_max where they clip, relative to the radius;
- phi against 0, 2 pi and phi_max where phi_max clips, relative to 2 pi;
- on a phi-clipped sphere, rho within 1e-4 radius of the axis (sphere.go moves the
  point there), and on every sphere rho within EPS radius of it (the move is by
  1e-5 radius and the point returned is the moved one);
- rho against both radii of a disk, relative to the radius, and against 0 (the
  reference's normal is NaN at a disk's centre);
- a ray parallel to a disk's plane within EPS |d| whose origin is within EPS of the
  plane and which comes within the disk's radius of its axis for some t in
  [0, TMax] (a parallel ray off the plane, or one that stays clear of the disk, is
  a decided miss);
- the two smallest counting t of different primitives within EPS of each other.

The families (FAMILIES) sit near the boundaries, decidably: `aimed`, `offsets` and
`shadowing`, over the scenes of tests/adversarial_rays.py.
"""
import functools
from collections import namedtuple

import numpy as np

import adversarial_rays as A
from pbrtgpu import abi

LD = np.longdouble
EPS = 1e-9
POLE_ZONE = 1e-4
INF = float("inf")
TWO_PI = 2 * np.pi

Prim = namedtuple("Prim", "index kind M Minv reverse radius z_min z_max phi_max height inner")
Hits = namedtuple("Hits", "hit t prim p n decided root")


# -------------------------------------------------------------------- geometry
def _mat(t):
    return np.array([[t.m.m[i][j] for j in range(4)] for i in range(4)], dtype=LD)


def affine_inverse(M):
    """The inverse of an affine 4x4 (last row 0 0 0 1) in longdouble: the adjugate of its 3x3 over the determinant."""
    a = M[:3, :3]
    cof = np.empty((3, 3), dtype=LD)
    for i in range(3):
        for j in range(3):
            r, c = [k for k in range(3) if k != i], [k for k in range(3) if k != j]
            cof[i, j] = (-1) ** (i + j) * (a[r[0], c[0]] * a[r[1], c[1]] - a[r[0], c[1]] * a[r[1], c[0]])
    det = (a[0] * cof[0]).sum()
    out = np.zeros((4, 4), dtype=LD)
    out[:3, :3] = cof.T / det
    out[:3, 3] = -(out[:3, :3] @ M[:3, 3])
    out[3, 3] = 1
    return out


def primitives(scene):
    """One Prim per primitive of scene.desc, in the descriptor's order."""
    d = scene.desc
    out = []
    for i in range(d.n_prims):
        p = d.prims[i]
        sd = d.shapes[p.shape]
        M = _mat(sd.object_to_world)
        assert np.array_equal(M[3], np.array([0, 0, 0, 1], dtype=LD))
        if p.kind == abi.PBRT_PRIM_TRANSFORMED:
            M = _mat(p.prim_to_world) @ M
        kind = "sphere" if sd.type == abi.PBRT_SHAPE_SPHERE else "disk"
        out.append(Prim(i, kind, M, affine_inverse(M), bool(sd.reverse_orientation), float(sd.radius), float(sd.z_min),
                        float(sd.z_max), float(sd.phi_max), float(sd.height) if kind == "disk" else 0.0,
                        float(sd.inner_radius) if kind == "disk" else 0.0))
    return out


def _norm(v):
    return np.sqrt((v * v).sum(axis=1))


PI_LD = LD(np.pi) + LD(1.2246467991473532e-16)   # pi to longdouble's precision: float64's pi and its remainder


def _phi(x, y):
    phi = np.arctan2(y, x)
    return np.where(phi < 0, phi + 2 * PI_LD, phi)


# status of a candidate root: it certainly counts, certainly does not, or rests on a margin
NO, MAYBE, YES = 0, 1, 2


def _combine(*parts):
    """NO if any part is NO, else MAYBE if any is MAYBE, else YES."""
    out = np.full(parts[0].shape, YES)
    for s in parts:
        out = np.minimum(out, s)
    return out


def _above(x, bound, margin):
    """x >= bound: YES / NO beyond the margin, MAYBE within it."""
    return np.where(x > bound + margin, YES, np.where(x < bound - margin, NO, MAYBE))


def _range_status(t, tmax, scale):
    m = EPS * (np.abs(t) + scale)
    with np.errstate(invalid="ignore"):
        hi = np.where(np.isinf(tmax), YES, _above(-t, -tmax, m))
    return _combine(_above(t, 0, m), hi)


def _phi_status(phi, phi_max):
    if phi_max >= TWO_PI:
        return np.full(phi.shape, YES)
    m = EPS * TWO_PI
    near = (phi < m) | (phi > TWO_PI - m) | (np.abs(phi - phi_max) <= m)   # the seam on either side, and phi_max
    return np.where(near, MAYBE, np.where(phi < phi_max, YES, NO))


def _sphere_roots(pr, o, d, tmax, scale):
    """Per root (near, far): (t, status, object-space point)."""
    r = LD(pr.radius)
    a = (d * d).sum(axis=1)
    b = 2 * (o * d).sum(axis=1)
    c = (o * o).sum(axis=1) - r * r
    disc = b * b - 4 * a * c
    dscale = b * b + np.abs(4 * a * c)
    dstat = np.where(disc > EPS * dscale, YES, np.where(disc < -EPS * dscale, NO, MAYBE))
    with np.errstate(invalid="ignore", divide="ignore"):
        q = -(b + np.where(b < 0, -1, 1) * np.sqrt(np.maximum(disc, 0))) / 2
        ta, tb = q / a, c / q
        tb = np.where(q == 0, ta, tb)
    roots = []
    for t in (np.minimum(ta, tb), np.maximum(ta, tb)):
        p = o + t[:, None] * d
        p = p * (r / _norm(p))[:, None]
        rho = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2)
        parts = [dstat, _range_status(t, tmax, scale)]
        if pr.z_min > -pr.radius:
            parts.append(_above(p[:, 2], pr.z_min, EPS * r))
        if pr.z_max < pr.radius:
            parts.append(_above(-p[:, 2], -pr.z_max, EPS * r))
        if pr.phi_max < TWO_PI:
            parts.append(_phi_status(_phi(p[:, 0], p[:, 1]), pr.phi_max))
            parts.append(np.where(rho < POLE_ZONE * r, MAYBE, YES))
        else:
            parts.append(np.where(rho < EPS * r, MAYBE, YES))
        with np.errstate(invalid="ignore"):
            roots.append((t, _combine(*parts), p))
    return roots


def _disk_roots(pr, o, d, tmax, scale):
    h, r = LD(pr.height), LD(pr.radius)
    dn = _norm(d)
    parallel = np.abs(d[:, 2]) <= EPS * dn
    in_plane = np.abs(o[:, 2] - h) <= EPS * (r + _norm(o) + abs(h))
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (h - o[:, 2]) / d[:, 2]
    t = np.where(parallel, LD(0), t)
    p = o + t[:, None] * d
    p[:, 2] = h
    rho = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2)
    parts = [_range_status(t, tmax, scale), _above(-rho, -r, EPS * r), np.where(rho < EPS * r, MAYBE, YES)]
    if pr.inner > 0:
        parts.append(_above(rho, pr.inner, EPS * r))
    parts.append(_phi_status(_phi(p[:, 0], p[:, 1]), pr.phi_max))
    status = _combine(*parts)
    # a parallel ray: off the plane it misses; in the plane it is undecided where it comes within the radius of the axis
    with np.errstate(invalid="ignore", divide="ignore"):
        ts = np.clip(-(o[:, 0] * d[:, 0] + o[:, 1] * d[:, 1]) / (d[:, 0] ** 2 + d[:, 1] ** 2), 0, tmax)
        nearest = np.sqrt((o[:, 0] + ts * d[:, 0]) ** 2 + (o[:, 1] + ts * d[:, 1]) ** 2)   # of 0 <= t <= TMax to the axis
    status = np.where(parallel, np.where(in_plane & ~(nearest > r * (1 + EPS)), MAYBE, NO), status)
    return [(t, status, p)]


START = 1e-6   # a root this close to 0 (relative) is the starting point of a ray that leaves `start_on`


def intersect(scene, rays, start_on=None):
    """Closest hit of rays (n, 7: o, d, TMax) over scene.desc's primitives: Hits of hit (bool), t, prim (-1 on a miss),
    p, n (world space, float64; zero on a miss), decided (bool) and root (0: a sphere's near root or a disk's, 1: the
    far root; -1 on a miss). The any-hit answer is `hit`.

    start_on: per ray the primitive on whose surface it starts (-1: none), for a ray spawned at a hit point. The root
    of that primitive at the start itself, |t| <= START (|t| + |o| / |d|), does not count and leaves nothing
    undecided; its other root is a root like any. (Geometrically the ray leaves the surface there. The reference's
    disk ends on t <= 0 and its sphere on the error interval of that root, which contains 0; were a render of the
    reference to meet its own surface again, its film would differ from one built on this answer, and show it.)"""
    rays = np.asarray(rays, dtype=np.float64)
    n = rays.shape[0]
    ow, dw, tmax = rays[:, :3].astype(LD), rays[:, 3:6].astype(LD), rays[:, 6].astype(LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = _norm(ow) / _norm(dw)
    best_t = np.full(n, LD(np.inf))
    second_t = np.full(n, LD(np.inf))     # the smallest counting t of another primitive
    maybe_t = np.full(n, LD(np.inf))      # the smallest t of a root that rests on a margin
    best = np.full(n, -1)
    best_root = np.full(n, -1)
    best_p = np.zeros((n, 3), dtype=LD)
    best_n = np.zeros((n, 3), dtype=LD)
    for pr in primitives(scene):
        o = ow @ pr.Minv[:3, :3].T + pr.Minv[:3, 3]
        d = dw @ pr.Minv[:3, :3].T
        roots = (_sphere_roots if pr.kind == "sphere" else _disk_roots)(pr, o, d, tmax, scale)
        found = np.zeros(n, dtype=bool)
        for k, (t, status, p) in enumerate(roots):
            if start_on is not None:
                with np.errstate(invalid="ignore"):
                    at_start = (np.asarray(start_on) == pr.index) & (np.abs(t) <= START * (np.abs(t) + scale))
                status = np.where(at_start, NO, status)
            take = (status == YES) & ~found
            found |= take
            maybe_t = np.where((status == MAYBE) & (t < maybe_t), t, maybe_t)
            new = take & (t < best_t)
            if pr.kind == "sphere":
                n_obj = p / LD(pr.radius)
            else:
                n_obj = np.broadcast_to(np.array([0, 0, -1], dtype=LD), p.shape)
            if pr.reverse:
                n_obj = -n_obj
            nw = n_obj @ pr.Minv[:3, :3]        # M^-T n: rows times Minv
            with np.errstate(invalid="ignore"):
                nw = nw / _norm(nw)[:, None]
            pw = p @ pr.M[:3, :3].T + pr.M[:3, 3]
            second_t = np.where(new, best_t, np.where(take & ~new & (t < second_t), t, second_t))
            best_t = np.where(new, t, best_t)
            best = np.where(new, pr.index, best)
            best_root = np.where(new, k, best_root)
            best_p = np.where(new[:, None], pw, best_p)
            best_n = np.where(new[:, None], nw, best_n)
    hit = best >= 0
    with np.errstate(invalid="ignore"):
        margin = EPS * (np.abs(np.where(hit, best_t, 0)) + scale)
        decided = ~(np.isfinite(maybe_t) & (maybe_t <= best_t + margin)) & ~(hit & (second_t - best_t <= margin))
        decided &= np.isfinite(rays[:, :6]).all(axis=1) & ~np.isnan(rays[:, 6]) & np.isfinite(scale)
    f = np.float64
    return Hits(hit, np.where(hit, best_t, 0).astype(f), best, best_p.astype(f), best_n.astype(f), decided, best_root)


# ---------------------------------------------------------- comparison scaling
def scene_size(scene):
    lo, hi = A.root_box(scene)
    return float(np.linalg.norm(hi - lo))


def gaps(scene, rays, ref, rows):
    """The gaps between (n, 9) closest-hit rows (the oracle's or the device's) and the reference on the rays that
    both call a hit: t relative to |t| + |o| / |d|, p relative to the root box's diagonal, n as 1 - |n . n_ref|, and
    whether the normals' signs agree."""
    both = ref.hit & (rows[:, 0] == 1)
    t, p, n = rows[both, 1], rows[both, 3:6], rows[both, 6:9]
    scale = np.abs(ref.t[both]) + np.linalg.norm(rays[both, :3], axis=1) / np.linalg.norm(rays[both, 3:6], axis=1)
    dot = (n * ref.n[both]).sum(axis=1)
    return (np.abs(t - ref.t[both]) / scale, np.linalg.norm(p - ref.p[both], axis=1) / scene_size(scene),
            1 - np.abs(dot), dot > 0)


# --------------------------------------------------------------------- families
AIMED_KEPT, AIMED_REMOVED = 64, 16
OFFSETS = (1e-6, -1e-6, 1e-4, -1e-4, 1e-2, -1e-2)
Sweep = namedtuple("Sweep", "name prim start")
Aim = namedtuple("Aim", "prim start kept removed")


def has_removed_part(sh):
    """A cut-off cap, a missing sector or a hole."""
    return A.partial(sh) or (sh.kind == "disk" and sh.inner > 0)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _kept_point(sh, rng):
    """A point of the kept surface of sh at least 2 % of its extent inside every clip, object space, and the outward
    normal there (a disk: +z)."""
    full = sh.phi_max >= TWO_PI
    phi = rng.uniform(0, TWO_PI) if full else rng.uniform(0.02, 0.98) * sh.phi_max
    if sh.kind == "disk":
        rho = sh.inner + rng.uniform(0.02, 0.98) * (sh.radius - sh.inner)
        return np.array([rho * np.cos(phi), rho * np.sin(phi), sh.height]), np.array([0.0, 0.0, 1.0])
    z = sh.z_min + rng.uniform(0.02, 0.98) * (sh.z_max - sh.z_min)
    rho = np.sqrt(sh.radius ** 2 - z * z)
    p = np.array([rho * np.cos(phi), rho * np.sin(phi), z])
    return p, p / sh.radius


def _removed_point(sh, rng, k):
    """A point of the part of the full sphere, or of the full disk, that sh's clips remove, as far inside that
    part: the parts in turn (k)."""
    parts = []
    if sh.kind == "disk":
        if sh.inner > 0:
            parts.append("hole")
        if sh.phi_max < TWO_PI:
            parts.append("sector")
        part = parts[k % len(parts)]
        if part == "hole":
            rho, phi = rng.uniform(0.05, 0.95) * sh.inner, rng.uniform(0, TWO_PI)
        else:
            rho = rng.uniform(0.05, 0.95) * sh.radius
            phi = sh.phi_max + rng.uniform(0.05, 0.95) * (TWO_PI - sh.phi_max)
        return np.array([rho * np.cos(phi), rho * np.sin(phi), sh.height]), np.array([0.0, 0.0, 1.0])
    r = sh.radius
    if sh.z_min > -r:
        parts.append("below")
    if sh.z_max < r:
        parts.append("above")
    if sh.phi_max < TWO_PI:
        parts.append("sector")
    part = parts[k % len(parts)]
    phi = rng.uniform(0.05, 0.95) * sh.phi_max
    z = sh.z_min + rng.uniform(0.05, 0.95) * (sh.z_max - sh.z_min)
    if part == "below":
        z = -r + rng.uniform(0.1, 0.95) * (sh.z_min + r)
    elif part == "above":
        z = sh.z_max + rng.uniform(0.05, 0.9) * (r - sh.z_max)
    else:
        phi = sh.phi_max + rng.uniform(0.05, 0.95) * (TWO_PI - sh.phi_max)
    rho = np.sqrt(r * r - z * z)
    p = np.array([rho * np.cos(phi), rho * np.sin(phi), z])
    return p, p / r


def _outside_origin(sh, rng, target, normal):
    """target + (2 .. 6 radii) along a direction at least 0.25 to the normal (a disk: on either side)."""
    while True:
        u = _unit(rng)
        c = u @ normal
        if sh.kind == "disk" and abs(c) >= 0.25 or sh.kind == "sphere" and c >= 0.25:
            return target + rng.uniform(2, 6) * sh.radius * u


def _far_root(sh, o, d):
    """The far root of the full sphere on the ray o + t d that meets it at t = 1 (float64: it only places a TMax)."""
    a, b, c = d @ d, 2 * (o @ d), o @ o - sh.radius ** 2
    return c / a   # the product of the roots, one of which is 1


def _aimed(scene, seed=5):
    rng = np.random.default_rng(seed)
    rows, index = [], []
    for sh in A.shapes(scene):
        removed = AIMED_REMOVED if has_removed_part(sh) else 0
        index.append(Aim(sh.prim, len(rows), AIMED_KEPT, removed))
        for k in range(AIMED_KEPT):
            target, normal = _kept_point(sh, rng)
            tmax = INF
            if sh.kind == "sphere" and k % 4 == 0:      # from inside: the far root
                o = _unit(rng) * sh.radius * 0.9 * rng.uniform() ** (1 / 3)
            else:
                o = _outside_origin(sh, rng, target, normal)
                if k % 4 == 1:                          # TMax between the two roots (a disk: past its one)
                    tmax = 0.5 * (1 + _far_root(sh, o, target - o)) if sh.kind == "sphere" else 1.5
            rows.append(A.world(sh, o, target - o, tmax))
        for k in range(removed):
            target, normal = _removed_point(sh, rng, k)
            o = _outside_origin(sh, rng, target, normal)
            tmax = INF
            if sh.kind == "sphere" and k % 2 == 1:      # TMax between the roots: the far root, kept or not, is out
                tmax = 0.5 * (1 + _far_root(sh, o, target - o))
            rows.append(A.world(sh, o, target - o, tmax))
    return A._rows(rows), index


def aimed(scene):
    """Per primitive AIMED_KEPT rays from 2 to 6 radii away towards random points of its kept surface (a quarter of
    a sphere's from inside it: the far root; a quarter with TMax between the roots) and, where a part is removed,
    AIMED_REMOVED rays towards points of that part (half of a sphere's with TMax between the roots)."""
    return _aimed(scene)[0]


def aimed_index(scene):
    return _aimed(scene)[1]


def _offsets(scene):
    """adversarial_rays._sweeps' constructions, the parameter at p0 (1 + s) for s in OFFSETS. One placement differs:
    the radius sweeps of a disk sector run at azimuth phi_max / 12, not along the seam phi = 0."""
    rows, index = [], []

    def add(name, sh, p0, ray):
        index.append(Sweep(name, sh.prim, len(rows)))
        for s in OFFSETS:
            rows.append(ray(p0 * (1 + s)))

    for sh in A.shapes(scene):
        r = sh.radius
        hp = A.surface_point(sh)
        if sh.kind == "sphere":
            phi = sh.phi_max / 12 if A.partial(sh) else 0.0
            zt = 0.5 * (sh.z_min + sh.z_max) if A.partial(sh) else 0.0
            c, s = np.cos(phi), np.sin(phi)
            rho = np.sqrt(r * r - zt * zt)
            h0 = np.array([rho * c, rho * s, zt]) if A.partial(sh) else np.array([r, 0.0, 0.0])
            add("tangent", sh, r, lambda p: A.world(sh, (p * c, p * s, -2 * r), (0.0, 0.0, 1.0), 4 * r))
            add("tmax_t0", sh, 1.0, lambda p: A.world(sh, 2 * h0, -h0, p))
            add("tmax_t1", sh, 1.0, lambda p: A.world(sh, (0.0, 0.0, 0.0), h0, p))
            add("cross", sh, 1.0, lambda p: A.world(sh, p * h0, -h0, 1.0))
            for name, z in (("z_min", sh.z_min), ("z_max", sh.z_max)):
                if abs(z) < r:
                    add(name, sh, z, lambda p: A.world(sh, (2 * r * c, 2 * r * s, p), (-r * c, -r * s, 0.0), 2.0))
            if sh.phi_max < TWO_PI:
                def at_phi(p):
                    h = np.array([rho * np.cos(p), rho * np.sin(p), zt])
                    return A.world(sh, 2 * h, -h, 2.0)
                add("phi_max", sh, sh.phi_max, at_phi)
                add("phi_seam", sh, TWO_PI, at_phi)
        else:
            down = (0.0, 0.0, -1.0)
            h = sh.height
            a = sh.phi_max / 12 if sh.phi_max < TWO_PI else 0.0
            ca, sa = np.cos(a), np.sin(a)
            add("tmax_t0", sh, 2.0, lambda p: A.world(sh, hp + (0, 0, 2), down, p))
            add("cross", sh, 1.0, lambda p: A.world(sh, hp + (0, 0, p - 1.0), down, 1.0))
            add("radius", sh, r, lambda p: A.world(sh, (p * ca, p * sa, h + 2), down, 3.0))
            if sh.inner > 0:
                add("inner_radius", sh, sh.inner, lambda p: A.world(sh, (p * ca, p * sa, h + 2), down, 3.0))
            if sh.phi_max < TWO_PI:
                mid = 0.5 * (sh.inner + r)

                def at_phi(p):
                    return A.world(sh, (mid * np.cos(p), mid * np.sin(p), h + 2), down, 3.0)
                add("phi_max", sh, sh.phi_max, at_phi)
                add("phi_seam", sh, TWO_PI, at_phi)
    return A._rows(rows), index


def offsets(scene):
    """Every sweep of adversarial_rays with its parameter 1e-6, 1e-4 and 1e-2 (relative) on either side of the
    boundary in place of ulps: len(OFFSETS) rays per sweep, decided on both sides."""
    return _offsets(scene)[0]


def offsets_index(scene):
    return _offsets(scene)[1]


def shadowing(scene):
    """Rays through two or more primitives. Along the row of small spheres, both ways, from before the row and from
    between two of its spheres, TMax infinite, short of the first sphere ahead and between the first and the second.
    And along z through the zones of the nested disks (disk, gap, ring, gap, annulus, its missing sector, outside),
    which have a small sphere of the row above them at one azimuth and the full sphere below: both ways, TMax
    infinite and between each two planes crossed."""
    sh = A.shapes(scene)
    row = sorted((s for s in sh if s.kind == "sphere" and s.radius == 0.3), key=lambda s: s.centre[0])
    rows = []
    r = row[0].radius
    xs = [s.centre[0] for s in row]
    y0, z0 = row[0].centre[1], row[0].centre[2]
    starts = [xs[0] - 1.5] + [0.5 * (a + b) for a, b in zip(xs, xs[1:])] + [xs[-1] + 1.5]
    for dy, dz in ((0.0, 0.0), (0.1, 0.05), (-0.15, 0.12), (0.07, -0.2)):
        for x in starts:
            for sx in (1.0, -1.0):
                ahead = sorted(abs(c - x) for c in xs if (c - x) * sx > 0)
                tm = [INF]
                if ahead:
                    tm.append(ahead[0] - 2 * r)                       # short of the first sphere
                    tm.append(ahead[0] + 1.5)                         # between the first and the second
                for tmax in tm:
                    rows.append(np.array([x, y0 + dy, z0 + dz, sx, 0.0, 0.0, tmax]))
        for sx in (1.0, -1.0):   # oblique: through a part of the row only
            rows.append(np.array([xs[0] - 1.5 * sx, y0 + dy, z0 + dz - 0.35, sx, 0.0, 0.05, INF]))
    annulus = next(s for s in sh if s.kind == "disk" and s.inner > 0 and s.phi_max < TWO_PI)
    cx, cy, cz = annulus.centre
    below = next(s for s in sh if s.kind == "sphere" and abs(s.centre[0] - cx) < 1e-9 and s.centre[2] < cz)
    zones = [(0.25, 1.0), (0.53, 2.0), (0.625, 3.0), (0.72, 4.0), (1.2, 0.7), (1.2, 5.0), (1.6, 5.6), (2.3, 1.5)]
    zones.append((float(np.hypot(xs[0] - cx, 0.1)), float(np.arctan2(0.1, xs[0] - cx))))   # under the row's first sphere
    top, bottom = z0 + 5.0, below.centre[2] - 5.0
    for rho, phi in zones:
        x, y = cx + rho * np.cos(phi), cy + rho * np.sin(phi)
        for o_z, s_z in ((top, -1.0), (bottom, 1.0)):
            planes = sorted(abs(z - o_z) for z in (z0, cz, below.centre[2]))
            for tmax in (INF, 0.5 * (planes[0] + planes[1]), 0.5 * (planes[1] + planes[2]), planes[0] - 1.0):
                rows.append(np.array([x, y, o_z, 0.0, 0.0, s_z, tmax]))
    return A._rows(rows)


FAMILIES = {"aimed": aimed, "offsets": offsets, "shadowing": shadowing}
COMPARED = ("aimed", "offsets", "shadowing", "inside", "random", "axis")   # with adversarial_rays' own


@functools.lru_cache(maxsize=None)
def rays(scene_key, family):
    """The family's rays on the scene, this module's or adversarial_rays': computed once, read-only."""
    if family in FAMILIES:
        return FAMILIES[family](A.SCENES[scene_key]())
    return A.rays(scene_key, family)


@functools.lru_cache(maxsize=None)
def reference(scene_key, family):
    """intersect() on rays(scene_key, family): computed once, read-only."""
    ref = intersect(A.SCENES[scene_key](), rays(scene_key, family))
    for a in ref:
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def oracle(scene_key, family):
    """(closest rows, any-hit flags) of the oracle on rays(scene_key, family): computed once, read-only."""
    if family not in FAMILIES:
        return A.oracle(scene_key, family)
    import oracle_lib as O
    desc = A.SCENES[scene_key]().desc
    want = O.intersect(desc, rays(scene_key, family), closest=True)
    wocc = O.intersect(desc, rays(scene_key, family), closest=False)
    want.setflags(write=False)
    wocc.setflags(write=False)
    return want, wocc

"""Triangle meshes that are not a height field, shared by tests/test_mesh_zoo.py
(CPU: pins the oracle against brute force) and tests/test_gpu_mesh_zoo.py (the
device LBVH and walk against that oracle). Host-side pbrt_sb_* builder only,
deterministic seeds.

A family is a function returning a Case or a dict of Cases. A Case holds its
meshes (p float32 [nv, 3], indices int32 [nt, 3], material name, reverse), its
rays (n, 7) and builds its scenes on demand; it keeps every Scene it built, so
a `desc` stays valid for as long as the Case is alive (the functions cache
their Cases for the life of the process).

What each family is for:
  grid_ties   exact ties: up to six coplanar triangles at one t
  duplicates  the same triangle several times: the smallest global index wins
  degenerates zero-area triangles, dropped from the tree while gid counts them
  tiny        1, 2, 3 and 5 triangles (no Karras launch, the root a leaf, ...)
  multi       five meshes, four materials, mixed reverse flags, over a floor
  soup        random intersecting triangles, rays aimed at vertices, centroids,
              along axes, and from inside triangle planes
  tmax_edge   TMax exactly at, and one ulp above, the closest hit
  cluster     one Morton code for many triangles; one centroid for all (ext 0)
  scaled      the soup times 2^+-40, 2^+-100
  subnormal   the soup so small that float32 vertices are subnormal
  mixed_tie   a disk coplanar with the grid: analytic primitive against mesh
"""
import functools
import math

import numpy as np

import pbrtgpu as G

INF = math.inf


def kept_mask(tris_in):
    """The library's rule (mesh_bvh_build, orc_mesh_get): a triangle (row of
    nine float32) is in the tree iff |e1 x e2|^2 > 0 in float64."""
    t = np.asarray(tris_in).reshape(-1, 9).astype(np.float64)
    c = np.cross(t[:, 3:6] - t[:, 0:3], t[:, 6:9] - t[:, 0:3])
    return (c * c).sum(axis=1) > 0


# ------------------------------------------------------------------ the Case
class Case:
    def __init__(self, name, meshes, rays, spheres=(), view=None, builder=None):
        self.name = name
        self.meshes = [(np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(i, dtype=np.int32), m, bool(r))
                       for p, i, m, r in meshes]
        self.rays = np.ascontiguousarray(rays, dtype=np.float64)
        self.rays.setflags(write=False)
        self.spheres = tuple(spheres)   # ((x, y, z), radius) of the mixed variant
        self.view = view                # (eye, look, up, fov) of the renders
        self.builder = builder          # a scene with more than meshes and spheres (multi, mixed_tie)
        self._scenes = {}

    # the triangles in global index order, as the library gathers them
    @property
    def tris_in(self):
        """(nt, 9) float32: every input triangle, zero-area ones included."""
        return np.concatenate([p[i].reshape(-1, 9) for p, i, _, _ in self.meshes])

    @property
    def kept(self):
        return kept_mask(self.tris_in)

    @property
    def mesh_first(self):
        return np.concatenate([[0], np.cumsum([i.shape[0] for _, i, _, _ in self.meshes])])

    def scene(self, mixed=False, size=(32, 24), meshes=None):
        """The built Scene: the meshes alone (n_prims == 0: the kMeshOnly
        kernels) or, mixed, with the Case's analytic primitives. meshes: other
        meshes in the same surroundings (a variant; the caller keeps that Scene)."""
        if meshes is not None:
            return build_scene(meshes, self.spheres if mixed else (), size, self.view, self.builder if mixed else None)
        key = (bool(mixed), size)
        if key not in self._scenes:
            self._scenes[key] = self.scene(mixed, size, self.meshes)
        return self._scenes[key]

    @property
    def has_mixed(self):
        return bool(self.spheres) or self.builder is not None

    def with_copies(self):
        """The meshes followed by an exact copy of each, with another material
        and the opposite flag: every copy loses every tie to its original."""
        other = {"matte": "glass", "matte2": "mirror", "glass": "matte", "mirror": "oren", "oren": "matte2"}
        return self.meshes + [(p, i, other[m], not r) for p, i, m, r in self.meshes]


def build_scene(meshes, spheres=(), size=(32, 24), view=None, builder=None):
    s = G.Scene()
    mats = {"matte": s.add_matte((0.5, 0.5, 0.5)), "matte2": s.add_matte((0.6, 0.1, 0.1)), "glass": s.add_glass(),
            "mirror": s.add_mirror(), "oren": s.add_matte((0.5, 0.6, 0.4), sigma=30.0)}
    if builder is not None:
        builder(s, mats)
    for c, rad in spheres:
        s.add_primitive(s.add_sphere(G.translate(0, 0, 0), rad), mats["matte2"], G.translate(*c))
    for p, idx, m, rev in meshes:
        s.add_mesh(p, idx, mats[m], rev)
    eye, look, up, fov = view or ((3.0, 3.0, 30.0), (3.0, 3.0, 0.0), (0.0, 1.0, 0.0), 40.0)
    if builder is None:
        s.add_point_light(G.translate(eye[0] + 1.5, eye[1] + 2.5, eye[2]), (400, 400, 400))
    s.set_film(*size)
    s.set_camera(G.look_at(eye, look, up), fov=fov)
    return s.build(max_prims_in_node=1)


def rays_of(o, d, tmax=INF):
    o, d = np.atleast_2d(np.asarray(o, dtype=np.float64)), np.atleast_2d(np.asarray(d, dtype=np.float64))
    n = max(o.shape[0], d.shape[0])
    out = np.empty((n, 7))
    out[:, 0:3], out[:, 3:6], out[:, 6] = o, d, tmax
    return out


# ----------------------------------------------------------------- the grid
def grid(n, z=0.0, x0=0.0, y0=0.0):
    """An n x n quad grid with integer coordinates in the plane z, every quad
    cut along the same diagonal: six triangles meet at an inner vertex."""
    p = np.array([(x0 + i, y0 + j, z) for j in range(n + 1) for i in range(n + 1)], dtype=np.float32)
    idx = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i, (j + 1) * (n + 1) + i + 1
            idx += [(a, b, d), (a, d, c)]
    return p, np.array(idx, dtype=np.int32)


def grid_targets(n):
    """Every vertex, the midpoint of every axis-parallel edge and every cell
    centre (the midpoint of the cell's diagonal edge)."""
    v = [(i, j) for j in range(n + 1) for i in range(n + 1)]
    e = [(i + 0.5, j) for j in range(n + 1) for i in range(n)] + [(i, j + 0.5) for j in range(n) for i in range(n + 1)]
    c = [(i + 0.5, j + 0.5) for j in range(n) for i in range(n)]
    return np.array(v + e + c, dtype=np.float64)


# directions with exactly representable components; o = target - 4 d, so t == 4 exactly
GRID_DIRS = ((0.0, 0.0, -1.0), (0.5, 0.25, -1.0), (-0.25, 0.5, -1.0), (0.0, 0.0, 1.0))


def grid_rays(n, dirs=GRID_DIRS, targets=None):
    tg = grid_targets(n) if targets is None else targets
    out = []
    for d in dirs:
        d = np.array(d)
        o = np.concatenate([tg, np.zeros((tg.shape[0], 1))], axis=1) - 4.0 * d
        out.append(rays_of(o, d))
    return np.concatenate(out)


def grid_spheres(n):
    return (((n / 2 + 0.25, n / 2, 1.0), 0.75), ((1.0, 1.0, -1.25), 0.5))


TOP_VIEW = ((3.0, 3.0, 9.0), (3.0, 3.0, 0.0), (0.0, 1.0, 0.0), 50.0)   # straight down the z axis onto grid(6)


@functools.lru_cache(maxsize=None)
def grid_ties():
    """{6, 24}: the small grid, and one whose tied triangles lie in leaves far
    apart in every threaded order (1152 triangles)."""
    out = {}
    for n in (6, 24):
        p, idx = grid(n)
        out[n] = Case(f"grid_ties[{n}]", [(p, idx, "matte", False)], grid_rays(n), grid_spheres(n),
                      view=TOP_VIEW if n == 6 else None)
    return out


@functools.lru_cache(maxsize=None)
def duplicates():
    p, idx = grid(6)
    out = {"two_meshes": Case("duplicates[two_meshes]", [(p, idx, "matte", False), (p, idx, "mirror", True)],
                              grid_rays(6), grid_spheres(6), view=TOP_VIEW)}
    perm = np.random.default_rng(21).permutation(idx.shape[0])
    out["shuffled"] = Case("duplicates[shuffled]", [(p, np.concatenate([idx[perm], idx]), "matte", False)],
                           grid_rays(6), grid_spheres(6))
    # ties at a t that no float32 holds, between triangles in general position
    sp, sidx = soup_mesh(200, 53)
    perm = np.random.default_rng(22).permutation(sidx.shape[0])
    out["soup"] = Case("duplicates[soup]", [(sp, np.concatenate([sidx[perm], sidx]), "matte", False)],
                       soup_rays(sp, sidx, 54), SOUP_SPHERES)
    tp = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0)], dtype=np.float32)
    tg = np.array([(x / 2, y / 2) for y in range(-1, 10) for x in range(-1, 10)])   # inside, on edges, at vertices, outside
    for k in (2, 9, 65):
        out[f"x{k}"] = Case(f"duplicates[x{k}]", [(tp, np.tile([[0, 1, 2]], (k, 1)), "matte", False)],
                            grid_rays(0, targets=tg), (((1.0, 1.0, 1.0), 0.5),))
    return out


def degenerate_triangles(p, n, count, seed):
    """count zero-area triangles over grid(n)'s vertices p, of three kinds in
    turn: a repeated index, two coincident vertices (a second vertex at the same
    position), three collinear vertices. Returns (p with the twins appended, idx)."""
    rng = np.random.default_rng(seed)
    nv = p.shape[0]
    p2 = np.concatenate([p, p])   # vertex nv + i is the twin of vertex i
    idx = []
    for k in range(count):
        a, b = rng.choice(nv, 2, replace=False)
        if k % 3 == 0:
            idx.append((a, a, b))
        elif k % 3 == 1:
            idx.append((a, nv + a, b))
        else:
            i, j = rng.integers(0, n - 1), rng.integers(0, n + 1)
            r = j * (n + 1) + i
            idx.append((r, r + 1, r + 2))   # three in a row
    return p2, np.array(idx, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def degenerates():
    p, idx = grid(6)
    p2, deg = degenerate_triangles(p, 6, idx.shape[0], 31)
    inter = np.empty((2 * idx.shape[0], 3), dtype=np.int32)
    inter[0::2], inter[1::2] = deg, idx   # a zero-area triangle before every valid one
    out = {"interleaved": Case("degenerates[interleaved]", [(p2, inter, "matte", False)], grid_rays(6),
                               grid_spheres(6), view=TOP_VIEW)}
    out["all"] = Case("degenerates[all]", [(p2, deg[:10], "matte", False)], grid_rays(6), grid_spheres(6))
    pa, ia = grid(3)
    pc, ic = grid(4, z=-1.0, x0=2.0, y0=2.0)
    # collinear triangles in general position: v, v + e, v + 2e with few mantissa
    # bits, so the area is exactly zero, while a ray aimed at the segment from
    # anywhere sees rounded edge functions that can all come out with one sign:
    # the bare triangle test can report a hit, only the dropping rule says no
    rng = np.random.default_rng(32)
    v = rng.integers(-512, 513, size=(60, 3)) / 128.0
    e = rng.integers(-128, 129, size=(60, 3)) / 128.0
    e[(e == 0).all(axis=1)] = 0.5
    col = np.stack([v, v + e, v + 2 * e], axis=1)
    val, _ = soup_mesh(60, 33, lo=0.3, hi=2.0)
    ps = np.empty((120, 3, 3))
    ps[0::2], ps[1::2] = col, val.reshape(60, 3, 3)
    k = np.repeat(np.arange(60), 25)
    tg = v[k] + e[k] * rng.uniform(0, 2, size=(k.size, 1))
    o = rng.normal(size=(k.size, 3))
    o *= 9.0 / np.linalg.norm(o, axis=1, keepdims=True)
    out["collinear"] = Case("degenerates[collinear]",
                            [(ps.reshape(-1, 3), np.arange(360, dtype=np.int32).reshape(-1, 3), "matte", False)],
                            rays_of(o, tg - o), (((0.0, 0.0, 0.0), 1.0),))
    out["between"] = Case("degenerates[between]", [(pa, ia, "matte", False), (p2, deg[:10], "glass", False),
                                                   (pc, ic, "mirror", True)], grid_rays(6), grid_spheres(6))
    return out


@functools.lru_cache(maxsize=None)
def tiny():
    p, idx = grid(6)
    return {k: Case(f"tiny[{k}]", [(p, idx[:k], "matte", False)], grid_rays(6), (((1.0, 0.25, 1.0), 0.5),))
            for k in (1, 2, 3, 5)}


# -------------------------------------------------------------------- multi
def patch(nx, nz, f):
    """An nx x nz quad patch, vertex (i, j) at f(i / nx, j / nz)."""
    p = np.array([f(i / nx, j / nz) for j in range(nz + 1) for i in range(nx + 1)], dtype=np.float32)
    idx = []
    for j in range(nz):
        for i in range(nx):
            a, b, c, d = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i, (j + 1) * (nx + 1) + i + 1
            idx += [(a, b, d), (a, d, c)]
    return p, np.array(idx, dtype=np.int32)


def multi_floor(s, mats):
    """scenes.mesh_material_scene's floor, sphere and lights."""
    chk = s.add_checker((0.2, 0, 0), (0, 0, 0.2), 0, 0, (1, 1, 1), (0.18, 0.18, 0.18))
    s.add_primitive(s.add_disk(G.rotate(0, 90), 0.0, 100.0), chk)
    s.add_primitive(s.add_sphere(G.translate(0, 0, 0), 1.5), mats["matte2"], G.translate(0, 1.5, -4))
    s.add_point_light(G.translate(-6, 10, 8), (60, 60, 60))
    s.add_area_light((6, 6, 6), s.add_sphere(G.translate(0, 9, 2), 0.75))


MULTI_VIEW = ((0.0, 7.0, 12.0), (0.0, 1.5, 0.0), (0.0, 1.0, 0.0), 55.0)


@functools.lru_cache(maxsize=None)
def multi():
    """Five meshes of 32, 1, 18, 8 and 2 triangles over the checker floor."""
    meshes = [
        patch(4, 4, lambda u, v: (-5 + 4 * u, 1.0 + 1.6 * u + 0.9 * v, -2 + 4 * v)) + ("glass", False),
        (np.array([(1, 0.5, -1), (4, 0.5, -1), (2.5, 3.5, -2)], dtype=np.float32), np.array([[0, 1, 2]]), "mirror", True),
        patch(3, 3, lambda u, v: (0.5 + 3 * u, 0.8 + 0.3 * u, 0.5 + 3 * v)) + ("oren", True),
        patch(2, 2, lambda u, v: (-1 + 2 * u, 0.2 + 2 * v, -1.5)) + ("matte", False),
        patch(1, 1, lambda u, v: (-0.8 + 1.6 * u, 0.6 + 1.2 * v, 3.0 + 0.5 * v)) + ("glass", True),
    ]
    rng = np.random.default_rng(41)
    n = 1500
    o = np.array(MULTI_VIEW[0]) + rng.normal(size=(n, 3)) * 0.5
    tg = np.stack([rng.uniform(-5.5, 4.5, n), rng.uniform(0, 3.5, n), rng.uniform(-3, 4, n)], axis=1)
    rays = rays_of(o, tg - o)
    c = Case("multi", meshes, rays, view=MULTI_VIEW, builder=multi_floor)
    return c


# --------------------------------------------------------------------- soup
def soup_mesh(n, seed, lo=1e-3, hi=3.0, spread=4.0):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-spread, spread, size=(n, 1, 3))
    size = np.exp(rng.uniform(np.log(lo), np.log(hi), size=(n, 1, 1)))
    p = (centre + size * rng.normal(size=(n, 3, 3))).reshape(-1, 3).astype(np.float32)
    return p, np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


def soup_rays(p, idx, seed):
    """Random rays; rays aimed at vertices and at centroids; axis-parallel rays
    (one and two zero direction components) through centroids; rays whose
    origin lies in a triangle's plane, or on one of its vertices."""
    rng = np.random.default_rng(seed)
    t = p[idx].astype(np.float64)   # (n, 3, 3)
    n = t.shape[0]
    cen = t.mean(axis=1)
    parts = []
    m = 1500
    parts.append(rays_of(rng.uniform(-8, 8, (m, 3)), rng.normal(size=(m, 3))))
    for tg in (t[rng.integers(0, n, m), rng.integers(0, 3, m)], cen[rng.integers(0, n, m)]):
        o = rng.normal(size=(m, 3))
        o *= 10.0 / np.linalg.norm(o, axis=1, keepdims=True)
        parts.append(rays_of(o, tg - o))
    k = rng.integers(0, n, 600)   # two zero components: along an axis through a centroid
    ax = rng.integers(0, 3, 600)
    sg = rng.choice([-1.0, 1.0], 600)
    d = np.zeros((600, 3))
    d[np.arange(600), ax] = sg
    parts.append(rays_of(cen[k] - 10.0 * d, d))
    k = rng.integers(0, n, 600)   # one zero component
    d = rng.normal(size=(600, 3))
    d[np.arange(600), rng.integers(0, 3, 600)] = 0.0
    parts.append(rays_of(cen[k] - 6.0 * d, d))
    k = rng.integers(0, n, 300)   # the origin in the plane of triangle k
    b = rng.uniform(-0.5, 1.5, (300, 3))
    b /= b.sum(axis=1, keepdims=True)
    parts.append(rays_of((t[k] * b[:, :, None]).sum(axis=1), rng.normal(size=(300, 3))))
    k = rng.integers(0, n, 300)   # the origin on a vertex, exactly
    parts.append(rays_of(t[k, rng.integers(0, 3, 300)], rng.normal(size=(300, 3))))
    rays = np.concatenate(parts)
    finite = rng.uniform(size=rays.shape[0]) < 0.2
    rays[finite, 6] = rng.uniform(1, 15, int(finite.sum()))
    return rays


SOUP_SPHERES = (((0.5, -0.5, 1.0), 1.25), ((-3.0, 2.0, -2.0), 0.75), ((2.5, 3.0, -1.0), 0.4))


@functools.lru_cache(maxsize=None)
def soup():
    p, idx = soup_mesh(600, 51)
    return Case("soup", [(p, idx, "matte", False)], soup_rays(p, idx, 52), SOUP_SPHERES)


@functools.lru_cache(maxsize=None)
def tmax_edge():
    """The soup's rays with TMax exactly at the oracle's closest t (exclusive:
    a miss) and at the next double above it (that hit again). Built from the
    oracle's hits on the mesh-only scene; rows 0..m-1 are the first kind,
    m..2m-1 the second, of the same m rays."""
    import oracle_lib as O
    s = soup()
    want = O.intersect(s.scene().desc, s.rays, closest=True)
    take = np.flatnonzero(want[:, 0] == 1)[:1500]
    at, above = s.rays[take].copy(), s.rays[take].copy()
    at[:, 6] = want[take, 1]
    above[:, 6] = np.nextafter(want[take, 1], INF)
    return Case("tmax_edge", s.meshes, np.concatenate([at, above]), SOUP_SPHERES)


def scaled_case(name, k):
    """The soup, its ray origins and its finite TMax values times 2^k."""
    s = soup()
    f = np.ldexp(1.0, k)
    p, idx, m, r = s.meshes[0]
    rays = s.rays.copy()
    rays[:, 0:3] *= f
    rays[:, 6] *= f   # Inf stays Inf
    p32 = (p.astype(np.float64) * f).astype(np.float32)
    return Case(name, [(p32, idx, m, r)], rays)


@functools.lru_cache(maxsize=None)
def scaled():
    out = {k: scaled_case(f"scaled[2^{k}]", k) for k in (40, -40, 100, -100)}
    for k, c in out.items():   # powers of two this size lose no vertex bit
        assert np.array_equal(c.meshes[0][0].astype(np.float64) * np.ldexp(1.0, -k), soup().meshes[0][0])
    return out


SUBNORMAL_EXP = -122   # the soup's coordinates below 2^-4 become subnormal float32


@functools.lru_cache(maxsize=None)
def subnormal():
    return scaled_case("subnormal", SUBNORMAL_EXP)


# ------------------------------------------------------------------ cluster
@functools.lru_cache(maxsize=None)
def cluster():
    """'outlier': 300 triangles in a 1e-3 box and one triangle 1e4 away, so the
    300 share one 30-bit Morton code and the tree under them splits on index
    bits only. 'star': 24 triangles of different sizes and planes whose float32
    centroids are all exactly (0, 0, 0): ext == 0 with n > 1."""
    rng = np.random.default_rng(61)
    n = 300
    centre = rng.uniform(2e-4, 8e-4, size=(n, 1, 3))
    size = rng.uniform(1e-4, 3e-4, size=(n, 1, 1))
    p = (centre + size * rng.normal(size=(n, 3, 3))).reshape(-1, 3)
    far = np.array([(1e4, 1e4, 1e4), (1e4 + 2, 1e4, 1e4 - 1), (1e4, 1e4 + 2, 1e4 - 1)])
    p = np.concatenate([p, far]).astype(np.float32)
    idx = np.arange(3 * (n + 1), dtype=np.int32).reshape(-1, 3)
    m = 900
    o = rng.normal(size=(m, 3))
    o = 5e-4 + o * (5e-3 / np.linalg.norm(o, axis=1, keepdims=True))
    tg = rng.uniform(2e-4, 8e-4, size=(m, 3))
    near = rays_of(o, tg - o)
    b = rng.dirichlet((1, 1, 1), 100)
    tg = (far[None] * b[:, :, None]).sum(axis=1) + rng.normal(size=(100, 3)) * 0.3   # around the outlier
    o = rng.uniform(0, 1e-3, size=(100, 3))
    out = {"outlier": Case("cluster[outlier]", [(p, idx, "matte", False)],
                           np.concatenate([near, rays_of(o, tg - o)]), (((5e-4, 5e-4, 2.5e-3), 2e-4),))}
    # the star: v2 = -(v0 + v1) in float32, so (v0 + v1 + v2) / 3 is exactly 0 in float32 too
    v0 = rng.integers(-8, 9, size=(24, 3)).astype(np.float32)
    v1 = rng.integers(-8, 9, size=(24, 3)).astype(np.float32)
    sz = np.ldexp(np.float32(1), -rng.integers(0, 6, size=(24, 1))).astype(np.float32)
    v0, v1 = v0 * sz, v1 * sz
    v2 = -(v0 + v1)
    ps = np.stack([v0, v1, v2], axis=1).reshape(-1, 3)
    ms = 400
    o = rng.normal(size=(ms, 3))
    o *= 20.0 / np.linalg.norm(o, axis=1, keepdims=True)
    tg = rng.normal(size=(ms, 3)) * 1.5
    tg[:100] = 0.0   # through the common centroid: every triangle at one point
    o[:50] = np.round(o[:50])
    out["star"] = Case("cluster[star]", [(ps, np.arange(72, dtype=np.int32).reshape(-1, 3), "matte", False)],
                       rays_of(o, tg - o), (((0.0, 0.0, 6.0), 1.0),))
    return out


# ---------------------------------------------------------------- mixed_tie
def tie_disk(s, mats):
    """A disk of radius 3.5 with identity orientation: in the plane z = 0 about the origin."""
    s.add_primitive(s.add_disk(G.translate(0, 0, 0), 0.0, 3.5), mats["matte2"])
    s.add_point_light(G.translate(3, 3, 12), (400, 400, 400))


@functools.lru_cache(maxsize=None)
def mixed_tie():
    """grid(6) and a coplanar disk; rays straight down onto the grid's targets
    and onto the same targets moved by (-3, -3): disk and grid, grid alone,
    disk alone, neither."""
    p, idx = grid(6)
    tg = np.concatenate([grid_targets(6), grid_targets(6) - 3.0])
    tg = tg[(tg != 0).any(axis=1)]   # not the disk's centre: the reference's normal there is NaN (dpdu == 0)
    return Case("mixed_tie", [(p, idx, "matte", False)], grid_rays(6, dirs=GRID_DIRS[:1], targets=tg),
                builder=tie_disk)


def query_cases():
    """Every Case with rays, by name."""
    out = {}
    for fam in (grid_ties, duplicates, degenerates, tiny, cluster, scaled):
        out.update({c.name: c for c in fam().values()})
    for fam in (multi, soup, tmax_edge, subnormal, mixed_tie):
        c = fam()
        out[c.name] = c
    return out

"""Caller-owned rays and path states for the Li queries (pbrt_gpu_li_device, pbrt_gpu_direct_li_device,
pbrt_gpu_path_begin_device / pbrt_gpu_path_step_device): rays that no camera produces. Host-side
builder and numpy only; the oracle is loaded where a family needs its answers.

Read by tests/test_li_rays_host.py (the families on the oracle alone: what each must contain is
asserted and the counts are pinned) and by tests/test_gpu_li_rays.py (device against oracle).

Scenes: tests/adversarial_rays.py's edge_small(1) (31 nodes, LDS-staged) and edge_large() (113
nodes, the [64]-stack walk), both Matte, and the same shapes at the same places with the materials
taken in turn from Matte, Mirror, smooth Glass and OrenNayar and a diffuse area light on a sphere
next to the point light. A light is no primitive: the trees are the Matte scenes' own.

Families: adversarial_rays.FAMILIES (the first-hit decisions at the boundaries now feed shading;
the disk_plane rays through a disk's exact centre, whose radiance is NaN, are counted with
`degenerate`), and
  scaled     rays that hit, with d times 2^-30, 0.5, 3, 2^30 (a finite TMax divided alike): the
             reference takes wo := ray.Direction unnormalised into the BSDF (SURVEY #8);
  tmax       for rays that hit at t: TMax from sweep_values(t), and 0, 5e-324, -1, NaN;
  secondary  origins on surfaces (the un-offset hit points of oracle_intersect), at sphere
             centres, inside spheres and in a disk's plane: where a path's later rays start;
  state      (path_step only) mid-path states of the oracle, permuted and edited as a caller may.
A batch is a family's rays with a PCG32 stream per ray (and, for `state`, the start state).
"""
import functools
from collections import namedtuple

import numpy as np

import adversarial_rays as A
import pbrtgpu as G
from pbrtgpu import abi

INF = float("inf")
MAX_DEPTH = 5
DEEP = 12          # one case per kernel on `secondary`: Russian roulette starts at the fifth iteration
SCALES = (2.0 ** -30, 0.5, 3.0, 2.0 ** 30)
TMAX_EXTRA = (0.0, A.DENORM, -1.0, A.NAN)
MATTE, MIRROR, GLASS, OREN = "matte", "mirror", "glass", "oren_nayar"
AREA_LIGHT_AT, AREA_LIGHT_RADIUS, AREA_LIGHT_L = (3.0, 20.0, 8.0), 1.0, (80.0, 80.0, 80.0)


# ----------------------------------------------------------------------- scenes
class _InTurn:
    """A scene builder whose primitives take their materials in turn from `mats`, whatever the
    caller names: adversarial_rays._edge_shapes with four materials instead of one."""

    def __init__(self, s, mats):
        self._s, self._mats, self._n = s, mats, 0

    def __getattr__(self, name):
        return getattr(self._s, name)

    def add_primitive(self, shape, _material, *args):
        m = self._mats[self._n % len(self._mats)]
        self._n += 1
        return self._s.add_primitive(shape, m, *args)


def _kx_scene(large):
    s = G.Scene()
    t = _InTurn(s, [s.add_matte((0.5, 0.5, 0.5)), s.add_mirror(), s.add_glass(), s.add_matte((0.6, 0.5, 0.4), sigma=20.0)])
    A._edge_shapes(t, None, nested=large)
    if large:   # edge_large's fillers
        rng = np.random.default_rng(11)
        for j in range(5):
            for i in range(8):
                c = np.array([-10.5 + 3.0 * i, 0.0, 28.0 + 3.0 * j]) + rng.uniform(-0.4, 0.4, 3)
                t.add_primitive(s.add_sphere(G.translate(*c), rng.uniform(0.25, 0.45)), None)
    s.add_point_light(G.translate(0, 20, 8), (100, 100, 100))
    s.add_area_light(AREA_LIGHT_L, s.add_sphere(G.translate(*AREA_LIGHT_AT), AREA_LIGHT_RADIUS))
    s.set_film(32, 32)
    s.set_camera(G.look_at((0, 40, 55), (0, 0, 16), (0, 1, 0)), fov=50)
    return s.build(max_prims_in_node=1)


@functools.lru_cache(maxsize=None)
def small_kx():
    return _kx_scene(False)


@functools.lru_cache(maxsize=None)
def large_kx():
    return _kx_scene(True)


SCENES = {"small": lambda: A.edge_small(1), "large": A.edge_large, "small_kx": small_kx, "large_kx": large_kx}
MATTE_TWIN = {"small": "small", "large": "large", "small_kx": "small", "large_kx": "large"}   # the scene of the same tree
# the instantiation <kX, kDepth> of k_li, k_path_step and k_li_direct a scene selects
KX = {"small": False, "large": False, "small_kx": True, "large_kx": True}
DEPTH = {"small": 0, "large": 64, "small_kx": 0, "large_kx": 64}


def kernel(key, base):
    return f"{base}<{'true' if KX[key] else 'false'}, {DEPTH[key]}>"


def material_kinds(scene):
    """The material of each primitive of the descriptor, in its (BVH) order."""
    d = scene.desc
    out = []
    for i in range(d.n_prims):
        m = d.materials[d.prims[i].material]
        out.append({abi.PBRT_MAT_MIRROR: MIRROR, abi.PBRT_MAT_GLASS: GLASS}.get(m.type, OREN if m.sigma != 0 else MATTE))
    return out


# --------------------------------------------------------------------- families
def _rows(rows):
    a = np.array(rows, dtype=np.float64).reshape(-1, 7)
    a.setflags(write=False)
    return a


def _first_hits(scene, rays):
    import oracle_lib as O
    return O.intersect(scene.desc, rays, closest=True)


Hitting = namedtuple("Hitting", "rays t kinds state inc")


@functools.lru_cache(maxsize=None)
def _hitting(scene, per_material=12, seed=5, lit_only=False):
    """Rays of axis, poles, inside and random that hit (oracle_intersect) and on which the oracle's
    Path.Li does not panic, each with the PCG32 stream it was tried with: per_material of them for
    each material of the scene (a Matte scene: 4 * per_material), those whose radiance is not black
    first (lit_only: no others), in a fixed order. t is the first hit's distance, kinds its material."""
    import oracle_lib as O
    rays = np.concatenate([A.axis(scene), A.poles(scene), A.inside(scene), A.random(scene)])
    rays = rays[(np.abs(rays[:, 3:6]).max(axis=1) > 0)]
    w = _first_hits(scene, rays)
    st, inc = streams(rays.shape[0], seed)
    li = O.path_li(scene.desc, rays, st, inc, max_depth=MAX_DEPTH)
    ok = np.flatnonzero((w[:, 0] == 1) & (li.status == O.ENDED) & ~np.isnan(li.L).any(axis=1))
    kinds = np.array(material_kinds(scene))[w[ok, 2].astype(int)]
    lit = li.L[ok].max(axis=1) > 0
    rng = np.random.default_rng(seed)
    pick = []
    names = sorted(set(kinds))
    for k in names:
        order = rng.permutation(np.flatnonzero(kinds == k))
        order = np.concatenate([order[lit[order]], order[~lit[order]][:0 if lit_only else None]])
        pick += list(ok[order[:per_material * 4 // len(names)]])
    pick = np.array(sorted(pick))
    return Hitting(rays[pick], w[pick, 1], np.array(material_kinds(scene))[w[pick, 2].astype(int)], st[pick], inc[pick])


N_SCALED = 1 + len(SCALES)   # a ray, then its copies, in SCALES' order


def scaled(scene):
    rows = []
    for r in _hitting(scene).rays:
        rows.append(r)
        for f in SCALES:
            c = r.copy()
            c[3:6] = r[3:6] * f
            if np.isfinite(r[6]):
                c[6] = r[6] / f
            rows.append(c)
    return _rows(rows)


def scaled_kinds(scene):
    """The material each group of N_SCALED rows first hits."""
    return _hitting(scene).kinds


N_TMAX = A.SWEEP_N + len(TMAX_EXTRA)   # a sweep, then the four extra values


def tmax(scene):
    h = _hitting(scene, per_material=3, seed=6, lit_only=True)   # lit: L differs between a hit and a miss
    rows = []
    for r, t0 in zip(h.rays, h.t):
        for v in list(A.sweep_values(float(t0))) + list(TMAX_EXTRA):
            c = r.copy()
            c[6] = v
            rows.append(c)
    return _rows(rows)


@functools.lru_cache(maxsize=None)
def _secondary(scene, seed=8):
    """(rows, per row: where the origin lies (ON_SURFACE, AT_CENTRE, INSIDE, IN_DISK_PLANE) and the
    primitive it lies on or in)."""
    rng = np.random.default_rng(seed)
    rows, where, prim = [], [], []

    def add(row, wh, pr):
        rows.append(row)
        where.append(wh)
        prim.append(pr)

    # on a surface: the un-offset p of camera and random first hits
    src = np.concatenate([camera_rays(scene)[::5], A.random(scene)])
    w = _first_hits(scene, src)
    hit = np.flatnonzero((w[:, 0] == 1) & ~np.isnan(w).any(axis=1))
    for i in rng.permutation(hit)[:40]:
        p, n = w[i, 3:6], w[i, 6:9]
        v = rng.normal(size=3)
        u = v / np.linalg.norm(v)
        if u @ n < 0:
            u = -u   # u leaves on the normal's side, -u on the other
        z0, z1 = u.copy(), -u
        z0[int(np.argmin(np.abs(u)))] = 0.0
        z1[int(np.argmin(np.abs(u)))] = -0.0
        for d in (u, -u, 2.5 * u, -0.3 * u, z0, z1):   # unit and not, zero components of both signs
            add(np.concatenate([p, d, [INF]]), ON_SURFACE, int(w[i, 2]))
    kinds = material_kinds(scene)
    for s in A.edge_shapes(scene):
        if s.kind == "sphere":
            for _ in range(2):
                add(np.concatenate([s.centre, rng.normal(size=3), [INF]]), AT_CENTRE, s.prim)
            # inside, towards the surface at every angle: beyond the critical angle a Glass sphere reflects
            n_in = 10 if kinds[s.prim] == GLASS else 2
            for j in range(n_in):
                v = rng.normal(size=3)
                o = s.centre + v / np.linalg.norm(v) * s.radius * (0.2 + 0.75 * j / 10)
                add(np.concatenate([o, rng.normal(size=3) * (1.0 if j % 2 else 0.25), [INF]]), INSIDE, s.prim)
        else:   # in the disk's plane: along it (both zero signs) and leaving it
            hp = A.surface_point(s)
            for d in ((1.0, 0.0, 0.0), (0.0, 1.0, -0.0), (0.3, 0.4, 1.0), (0.3, -0.4, -2.0)):
                add(A.world(s, hp, d), IN_DISK_PLANE, s.prim)
    return _rows(rows), np.array(where), np.array(prim)


ON_SURFACE, AT_CENTRE, INSIDE, IN_DISK_PLANE = range(4)


def secondary(scene):
    return _secondary(scene)[0]


def camera_rays(scene):
    """The scene's camera rays at the pixel corners, from the oracle's exports."""
    from test_gpu_query import full_window, oracle_camera_rays
    return oracle_camera_rays(scene.desc, full_window(scene), (0.0, 0.0))


def _nan_first_hit(scene, rays):
    """Rays whose first hit has a NaN element under oracle_intersect (a disk met at its exact centre)."""
    w = _first_hits(scene, rays)
    return (w[:, 0] == 1) & np.isnan(w).any(axis=1)


def disk_plane(scene):
    """adversarial_rays.disk_plane without the rays that meet a disk at its exact centre, where the
    reference's normal is NaN and so is every radiance behind it: those are in `degenerate`."""
    rays = A.disk_plane(scene)
    return _rows(rays[~_nan_first_hit(scene, rays)])


def degenerate(scene):
    rays = A.disk_plane(scene)
    return _rows(np.concatenate([A.degenerate(scene), rays[_nan_first_hit(scene, rays)]]))


FAMILIES = {**A.FAMILIES, "disk_plane": disk_plane, "degenerate": degenerate, "scaled": scaled, "tmax": tmax,
            "secondary": secondary}
STATE = "state"
ALL = list(FAMILIES) + [STATE]

Batch = namedtuple("Batch", "rays state inc start")


def streams(n, seed):
    rng = np.random.default_rng(seed)
    st = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    inc = rng.integers(0, 2**63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    return st, inc


# the `state` family's edits, applied in turn; each (name, function of the row's PathStart fields)
def _edit(kind, f, max_depth):
    if kind == "beta_channels":
        f["beta"] = f["beta"] * np.array([0.0, 1e-3, 7.5])
    elif kind == "eta_quarter":
        f["eta_scale"] = 0.25
    elif kind == "eta_four":
        f["eta_scale"] = 4.0
    elif kind == "L_preloaded":
        f["L"] = f["L"] + np.array([0.25, 1e-3, 3.0])
    elif kind == "rr_early":        # the next iteration is the fourth: Russian roulette applies
        f["bounces"] = 3
    elif kind == "rr_early_eta_quarter":
        f["bounces"], f["eta_scale"] = 3, 0.25
    elif kind == "rr_early_eta_four":
        f["bounces"], f["eta_scale"], f["beta"] = 3, 4.0, f["beta"] * 0.2
    elif kind == "at_max_depth":
        f["bounces"] = max_depth
    elif kind == "beyond_max_depth":
        f["bounces"] = max_depth + 3
    else:
        assert kind == "as_is"


EDITS = ("as_is", "beta_channels", "eta_quarter", "eta_four", "L_preloaded", "rr_early", "rr_early_eta_quarter",
         "rr_early_eta_four", "at_max_depth", "beyond_max_depth")


def state_batch(key, n=250, seed=9):
    """Mid-path states: the oracle's paths on camera, inside and random rays that are alive after 1,
    2 and 3 iterations, permuted, the first n, row i edited by EDITS[i % len(EDITS)]."""
    import oracle_lib as O
    scene = SCENES[key]()
    src = np.concatenate([camera_rays(scene)[::3], A.inside(scene), A.random(scene)])
    st, inc = streams(src.shape[0], seed)
    parts = []
    for k in (1, 2, 3):
        got = O.path_li(scene.desc, src, st, inc, max_depth=MAX_DEPTH, k=k)
        alive = np.flatnonzero((got.status == O.ALIVE) & ~np.isnan(got.ray).any(axis=1))
        parts.append((got, alive))
    rng = np.random.default_rng(seed + 1)
    order = rng.permutation(sum(len(a) for _, a in parts))[:n]
    owner = np.concatenate([np.full(len(a), j) for j, (_, a) in enumerate(parts)])
    index = np.concatenate([a for _, a in parts])
    rays, state, incs, rows = [], [], [], []
    for i, o in enumerate(order):
        got, src_i = parts[owner[o]][0], index[o]
        f = {name: np.array(getattr(got, name)[src_i]) for name in O.PathStart._fields}
        _edit(EDITS[i % len(EDITS)], f, MAX_DEPTH)
        rays.append(got.ray[src_i])
        state.append(got.state[src_i])
        incs.append(inc[src_i])
        rows.append(f)
    start = O.PathStart(*[np.array([r[name] for r in rows]) for name in O.PathStart._fields])
    return Batch(_rows(rays), np.array(state, dtype=np.uint64), np.array(incs, dtype=np.uint64), start)


@functools.lru_cache(maxsize=None)
def batch(key, family):
    """The family's rays on SCENES[key], a PCG32 stream per ray, and the start state (None: fresh).
    Computed once, read-only."""
    if family == STATE:
        b = state_batch(key)
    else:
        rays = FAMILIES[family](SCENES[key]())
        st, inc = streams(rays.shape[0], 100 + ALL.index(family))
        if family == "scaled":   # a ray and its copies share the stream the ray was chosen with
            h = _hitting(SCENES[key]())
            st, inc = np.repeat(h.state, N_SCALED), np.repeat(h.inc, N_SCALED)
        elif family == "tmax":
            h = _hitting(SCENES[key](), per_material=3, seed=6, lit_only=True)
            st, inc = np.repeat(h.state, N_TMAX), np.repeat(h.inc, N_TMAX)
        b = Batch(rays, st, inc, None)
    for a in (b.rays, b.state, b.inc) + (tuple(b.start) if b.start is not None else ()):
        a.setflags(write=False)
    return b


# ----------------------------------------------------------------- the oracle
@functools.lru_cache(maxsize=None)
def oracle_steps(key, family, max_depth=MAX_DEPTH):
    """[the PathLi after k iterations for k = 1 .. max_depth]; the last is the run to the end."""
    import oracle_lib as O
    b = batch(key, family)
    desc = SCENES[key]().desc
    out = [O.path_li(desc, b.rays, b.state, b.inc, max_depth=max_depth, k=k, start=b.start) for k in range(1, max_depth + 1)]
    end = O.path_li(desc, b.rays, b.state, b.inc, max_depth=max_depth, start=b.start)
    for f in O.PathLi._fields:   # max_depth iterations end every path
        assert getattr(end, f).tobytes() == getattr(out[-1], f).tobytes(), f
    return out


def oracle_li(key, family, max_depth=MAX_DEPTH):
    return oracle_steps(key, family, max_depth)[-1]


def late_panics(key, family, max_depth=MAX_DEPTH):
    """Rows whose panic comes after draws of its own iteration: the light sample's visibility ray, or
    UniformSampleOneLight's Ld > 10 (a panic of the closest-hit walk comes before any draw)."""
    import oracle_lib as O
    b = batch(key, family)
    draws = np.zeros(b.rays.shape[0], dtype=np.uint32) if b.start is None else b.start.draws.astype(np.uint32)
    late = np.zeros(b.rays.shape[0], dtype=bool)
    seen = np.zeros(b.rays.shape[0], dtype=bool)
    for s in oracle_steps(key, family, max_depth):
        new = (s.status == O.PANICKED) & ~seen
        late |= new & (s.draws != draws)
        seen |= new
        draws = s.draws
    return late


@functools.lru_cache(maxsize=None)
def oracle_direct(key, family, dl_strategy, max_depth=MAX_DEPTH):
    import oracle_lib as O
    b = batch(key, family)
    return O.direct_li(SCENES[key]().desc, b.rays, b.state, b.inc, max_depth=max_depth, dl_strategy=dl_strategy)

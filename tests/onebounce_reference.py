"""The film of a one-bounce render in closed form, written in numpy from the reference's
Go sources (camera.go, transform.go, film.go, path.go, integrator.go, lights/point.go,
reflection.go, interaction.go, spectrum.go, materials/matte.go) and independent of the
oracle: camera -> hit -> BSDF -> light -> visibility -> film. Hits and occlusion come
from tests/analytic_reference.py. numpy and the host-side scene builder only: no GPU.

Why a closed form exists. With maxDepth = 2, Path.Li adds the direct light of the first
hit and stops: bounces is 1 at the first hit, UniformSampleOneLight adds its light, and the
second pass of the loop ends on bounces >= maxDepth before anything else is added
(path.go:41, :66, :85). With one point light and the stratified sampler nothing in that sum
is random: every 2D sample is (0, 0), a point light ignores uLight, and of one light that
one is always chosen. So every traced sample of a pixel carries the same radiance

    L = Kd / pi * |wi . n| * I / |pLight - p|^2      where wi and wo lie on the same side of
                                                     the surface and the light is unoccluded,
    L = 0                                            otherwise, and on a miss.

The quirks of SURVEY section 9 that bear on the film are named where they enter (film()).

Left out. A pixel is left out if a corner ray that contributes to it is undecided: the
camera ray or its shadow ray within analytic_reference.EPS of a decision boundary (a
silhouette through the corner is a tangent camera ray), or wi within EPS of the tangent
plane.
"""
import functools
from collections import namedtuple

import numpy as np

import analytic_reference as R
import pbrtgpu as G

# ------------------------------------------------------------------- the scene
RES = (16, 12)
SPP = (2, 2)
FOV = 60.0
SCREEN = (0.0, 0.0, 1.0, 1.0)             # min x, min y, max x, max y: server.go's crop window [0, 1]^2
FILTER_RADIUS = (0.5, 0.5)
POS, LOOK, UP = (7.0, -9.0, 9.0), (2.0, 8.0, 3.0), (0.0, 0.0, 1.0)
LIGHT, INTENSITY = (1.0, -2.0, 7.0), (40.0, 36.0, 30.0)
KD = {"floor": (0.6, 0.55, 0.5), "reversed": (0.7, 0.2, 0.2), "plain": (0.2, 0.3, 0.7), "occluder": (0.3, 0.6, 0.3)}
FLOOR_RADIUS = 5.0
SPHERES = {"reversed": ((-1.8, 0.5, 1.0), 1.0, True), "plain": ((1.6, 2.0, 1.2), 1.2, False),
           "occluder": ((0.7, -1.5, 3.2), 0.6, False)}
MAX_DEPTH = 2
SHADOW_EPSILON = 0.0001


@functools.lru_cache(maxsize=None)
def scene():
    """A floor disk (z = 0), a reversed and a plain sphere on it, a small occluder sphere between the light and
    the floor, one point light."""
    s = G.Scene()
    s.add_primitive(s.add_disk(G.translate(0, 0, 0), 0.0, FLOOR_RADIUS), s.add_matte(KD["floor"]))
    for name, (c, r, rev) in SPHERES.items():
        s.add_primitive(s.add_sphere(G.translate(*c), r, reverse=rev), s.add_matte(KD[name]))
    s.add_point_light(G.translate(*LIGHT), INTENSITY)
    s.set_film(RES[0], RES[1], filter_radius=FILTER_RADIUS)
    s.set_camera(G.look_at(POS, LOOK, UP), screen=SCREEN, fov=FOV)
    return s.build(max_prims_in_node=1)


def render_desc(**kw):
    return G.render_desc(SPP[0], SPP[1], max_depth=MAX_DEPTH, **kw)


# ------------------------------------------------------------------ the camera
Xf = namedtuple("Xf", "m inv")


def _matmul(a, b):
    """Matrix4x4.Mul (transform.go:62-70, #18): the last term is m[i][3] * m[3][j], of the left operand alone."""
    return a[:, :3] @ b[:3, :] + np.outer(a[:, 3], a[3, :])


def _mul(a, b):
    """Transform.Mul (transform.go:179-184, #18): the inverses are multiplied in the operands' order."""
    return Xf(_matmul(a.m, b.m), _matmul(a.inv, b.inv))


def _scale(x, y, z):
    return Xf(np.diag([x, y, z, 1.0]), np.diag([1 / x, 1 / y, 1 / z, 1.0]))


def _translate(x, y, z):
    m, inv = np.eye(4), np.eye(4)
    m[:3, 3] = (x, y, z)
    inv[:3, 3] = (-x, -y, -z)
    return Xf(m, inv)


def _inverse(a):
    return Xf(a.inv, a.m)


def raster_to_camera():
    """camera.go:106-113 and transform.go:492-502, with the products as the reference forms them."""
    n, f = 1e-2, 1000.0
    persp = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, f / (f - n), -f * n / (f - n)], [0, 0, 1, 0]], dtype=np.float64)
    inv_tan = 1.0 / np.tan(np.radians(FOV) / 2)
    camera_to_screen = _mul(_scale(inv_tan, inv_tan, 1), Xf(persp, np.linalg.inv(persp)))
    x0, y0, x1, y1 = SCREEN
    s2r = _mul(_mul(_scale(RES[0], RES[1], 1.0), _scale(1 / (x1 - x0), 1 / (y0 - y1), 1.0)), _translate(-x0, -y1, 0))
    return _mul(_inverse(camera_to_screen), _inverse(s2r)).m


def camera_to_world():
    """LookAt (transform.go:453-486): the columns right, up, dir, pos."""
    pos, look, up = (np.array(v, dtype=np.float64) for v in (POS, LOOK, UP))
    d = (look - pos) / np.linalg.norm(look - pos)
    right = np.cross(up / np.linalg.norm(up), d)
    right /= np.linalg.norm(right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, np.cross(d, right), d, pos
    return m


def camera_rays():
    """One ray per pixel, row-major (RES[1] x RES[0], 7): #3, every stratified 2D sample is (0, 0), so pFilm is the
    pixel's integer corner and the lens sample is unused (a pinhole); camera.go:192-241."""
    r2c, c2w = raster_to_camera(), camera_to_world()
    ys, xs = np.mgrid[0:RES[1], 0:RES[0]]
    praster = np.stack([xs.ravel(), ys.ravel(), np.zeros(xs.size), np.ones(xs.size)], axis=1).astype(np.float64)
    pc = praster @ r2c.T
    pc = pc[:, :3] / pc[:, 3:4]                      # TransformPoint divides by w where it is not 1
    d = pc / np.linalg.norm(pc, axis=1)[:, None]
    out = np.empty((xs.size, 7))
    out[:, :3] = c2w[:3, 3]
    out[:, 3:6] = d @ c2w[:3, :3].T
    out[:, 6] = np.inf
    return out


# -------------------------------------------------------------------- the film
Film = namedtuple("Film", "xyz compared labels corner_labels L")


def rgb_to_xyz(rgb):
    """spectrum.go:35-41."""
    m = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    return rgb @ m.T


@functools.lru_cache(maxsize=None)
def film():
    """Film of xyz (RES[1], RES[0], 3), compared (bool per pixel), labels (per pixel the set of its corners'
    labels), corner_labels and L (per corner ray)."""
    sc = scene()
    prims = R.primitives(sc)
    names = {}
    for pr in prims:
        centre = tuple(float(v) for v in pr.M[:3, 3])
        names[pr.index] = "floor" if pr.kind == "disk" else next(k for k, v in SPHERES.items() if v[0] == centre)
    rays = camera_rays()
    n = rays.shape[0]
    hit = R.intersect(sc, rays)
    light, intensity = np.array(LIGHT), np.array(INTENSITY)
    to_light = light - hit.p
    dist2 = (to_light * to_light).sum(axis=1)
    wi = to_light / np.sqrt(dist2)[:, None]              # point.go:45
    # the BSDF reads isect.Wo (integrator.go:95), which the shapes set to -ray.Direction; #8 (`wo := ray.Direction`,
    # path.go:91) feeds only BSDF.SampleF, whose ray ends on bounces >= maxDepth before it adds anything
    wo = -rays[:, 3:6]
    # #22: a reversed sphere's normal points inwards, which changes neither |wi . n| nor the test below
    cos_i, cos_o = (wi * hit.n).sum(axis=1), (wo * hit.n).sum(axis=1)
    reflect = cos_i * cos_o > 0                         # reflection.go:175: Lambertian is a reflection lobe
    grazing = np.abs(cos_i) <= R.EPS
    # #14: the shadow ray starts at the un-offset hit point (its direction comes from the offset origin, which
    # MachineEpsilon's denormal value (#16) leaves within an ulp of it); #30: the light's interaction has a zero
    # normal, so its end is the light's position itself; TMax = 1 - ShadowEpsilon (interaction.go:91-102)
    shadow = np.concatenate([hit.p, to_light, np.full((n, 1), 1 - SHADOW_EPSILON)], axis=1)
    tested = hit.hit & reflect                          # integrator.go:108: the visibility is tested where f is not black
    occ = R.intersect(sc, shadow[tested], start_on=hit.prim[tested])
    blocked, shadow_decided = np.zeros(n, dtype=bool), np.ones(n, dtype=bool)
    blocked[tested], shadow_decided[tested] = occ.hit, occ.decided
    kd = np.array([KD[names[p]] if p >= 0 else (0, 0, 0) for p in hit.prim], dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        # #10: UniformSampleOneLight drops its division by lightPdf; the point light's own pdf is 1
        L = kd / np.pi * np.abs(cos_i)[:, None] * (intensity / dist2[:, None])
    L = np.where((tested & ~blocked)[:, None], L, 0.0)
    assert L.max() <= 10                                # (integrator.go:73 panics above 10)
    decided = hit.decided & shadow_decided & ~(hit.hit & grazing)
    corner_labels = np.array(["background" if p < 0 else names[p] for p in hit.prim], dtype=object)
    on_floor = corner_labels == "floor"
    corner_labels[on_floor & tested & ~blocked] = "lit floor"
    corner_labels[on_floor & tested & blocked] = "shadowed floor"
    # #2: StartNextSample pre-increments, so spp - 1 samples are traced, all with the same camera ray
    samples = SPP[0] * SPP[1] - 1
    # #6: a box filter of radius 0.5 spreads the corner sample (x, y) over the pixels x - 1, x and y - 1, y that exist
    # (film.go:217-221, weight 1), the tile sums L and the film adds RGBToXYZ of the sum: no division by the weight
    W, H = RES
    rgb = np.zeros((H, W, 3))
    compared = np.ones((H, W), dtype=bool)
    labels = [[set() for _ in range(W)] for _ in range(H)]
    for y in range(H):
        for x in range(W):
            i = y * W + x
            for py in (y - 1, y):
                for px in (x - 1, x):
                    if px >= 0 and py >= 0:
                        for _ in range(samples):
                            rgb[py, px] += L[i]
                        compared[py, px] &= decided[i]
                        labels[py][px].add(corner_labels[i])
    return Film(rgb_to_xyz(rgb), compared, labels, corner_labels.reshape(H, W), L.reshape(H, W, 3))


def gap(got, want):
    """Per channel, relative to the channel's value (a zero channel has to be zero): the largest over the compared pixels."""
    f = film()
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(want != 0, np.abs(got - want) / np.abs(want), np.where(got == want, 0.0, np.inf))
    return float(rel[f.compared].max())

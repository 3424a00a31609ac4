"""pbrtgpu — Python host wrapper over the C ABI of the MI355X hot path.

The product is the C-ABI library lib/libpbrt_gpu.so (include/pbrt_gpu.h,
include/pbrt_scene.h). This module only loads it with ctypes and mirrors the
reference's driver-side vocabulary so tests and bench read like go-pbrt:

    scene = Scene.readme(1920, 1080)            # internal/render/server.go:29-164
    with Renderer(scene) as r:                  # pbrt_gpu_create
        film, stats = r.render(render_desc())   # pbrt.Render -> fp64 XYZ film

There is deliberately no CPU fallback: if the HIP library is missing or no
GPU is visible, construction raises.
"""
import ctypes as C
import os
import struct
import zlib

import numpy as np

from . import abi
from .abi import *  # noqa: F401,F403  (re-export the ABI constants/structs)

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("PBRT_GPU_LIB") or os.path.join(PKG_DIR, "lib", "libpbrt_gpu.so")

_lib = None


class PbrtError(RuntimeError):
    def __init__(self, code, msg, stats=None):
        super().__init__(f"pbrt status {code}: {msg}")
        self.code = code
        self.stats = stats


def lib():
    """Load lib/libpbrt_gpu.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} missing: run `make -C go-pbrt_amd` (or __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    L.pbrt_gpu_build_id.restype = C.c_char_p
    L.pbrt_gpu_build_id.argtypes = []
    P, d, i64 = C.POINTER, C.c_double, C.c_int64
    T = P(abi.Transform)
    L.pbrt_gpu_create.argtypes = [P(abi.SceneDesc), P(abi.GpuOpts), P(C.c_void_p)]
    L.pbrt_gpu_render.argtypes = [C.c_void_p, P(abi.RenderDesc), P(d), P(abi.GpuStats)]
    L.pbrt_gpu_render_async.argtypes = [C.c_void_p, P(abi.RenderDesc)]
    L.pbrt_gpu_render_async_into.argtypes = [C.c_void_p, P(abi.RenderDesc), C.c_void_p]
    L.pbrt_gpu_synchronize.argtypes = [C.c_void_p, P(abi.GpuStats)]
    L.pbrt_gpu_film_device.argtypes = [C.c_void_p]
    L.pbrt_gpu_film_device.restype = C.c_void_p
    L.pbrt_gpu_film_download.argtypes = [C.c_void_p, P(d)]
    L.pbrt_gpu_stream.argtypes = [C.c_void_p]
    L.pbrt_gpu_stream.restype = C.c_void_p
    L.pbrt_gpu_intersect.argtypes = [C.c_void_p, P(abi.RaySoA), C.c_size_t, P(abi.HitSoA)]
    L.pbrt_gpu_intersect_p.argtypes = [C.c_void_p, P(abi.RaySoA), C.c_size_t, P(C.c_uint8)]
    L.pbrt_gpu_cancel.argtypes = [C.c_void_p]
    L.pbrt_gpu_cancel.restype = None
    L.pbrt_gpu_last_error.argtypes = [C.c_void_p]
    L.pbrt_gpu_last_error.restype = C.c_char_p
    L.pbrt_gpu_destroy.argtypes = [C.c_void_p]
    L.pbrt_gpu_destroy.restype = None
    abi.declare_group(L)
    abi.declare_query(L)
    if hasattr(L, "pbrt_gpu_li_device"):   # (a library of an earlier build, PBRT_GPU_LIB, has no such entry)
        abi.declare_li(L)
    if hasattr(L, "pbrt_gpu_direct_li_device"):
        abi.declare_direct_li(L)
    if hasattr(L, "pbrt_gpu_film_add_device"):
        abi.declare_frame(L)
    if hasattr(L, "pbrt_gpu_path_step_device"):
        abi.declare_path(L)
    if hasattr(L, "pbrt_gpu_li_stratified_device"):
        abi.declare_strat(L)
    abi.declare_launch_log(L)
    abi.declare_probe(L)
    L.pbrt_film_to_rgba8.argtypes = [P(d), i64, i64, P(C.c_uint8)]
    L.pbrt_gpu_tile_ticks.argtypes = [C.c_void_p, P(C.c_uint32), i64, P(i64)]
    L.pbrt_gpu_tile_ticks.restype = i64
    L.pbrt_gpu_tile_costs.argtypes = [C.c_void_p, P(C.c_float), i64]
    L.pbrt_gpu_tile_costs.restype = i64
    L.pbrt_gpu_counters.argtypes = [C.c_void_p, P(C.c_uint64), C.c_int]
    L.pbrt_gpu_schedule_source.argtypes = [C.c_void_p]
    L.pbrt_gpu_schedule_cache_clear.argtypes = []
    L.pbrt_gpu_overlap_slots.argtypes = [C.c_void_p]
    L.pbrt_gpu_overlap_slots.restype = C.c_int64
    L.pbrt_gpu_schedule_cache_clear.restype = None
    for name in ("pbrt_translate", "pbrt_scale"):
        getattr(L, name).argtypes = [d, d, d, T]
        getattr(L, name).restype = None
    for name in ("pbrt_rotate_x", "pbrt_rotate_y", "pbrt_rotate_z"):
        getattr(L, name).argtypes = [d, T]
        getattr(L, name).restype = None
    L.pbrt_transform_mul.argtypes = [T, T, T]
    L.pbrt_transform_mul.restype = None
    L.pbrt_transform_inverse.argtypes = [T, T]
    L.pbrt_transform_inverse.restype = None
    L.pbrt_matrix_inverse.argtypes = [P(abi.Matrix4x4), P(abi.Matrix4x4)]
    L.pbrt_new_transform.argtypes = [P(abi.Matrix4x4), T]
    L.pbrt_look_at.argtypes = [P(d), P(d), P(d), T]
    L.pbrt_perspective.argtypes = [d, d, d, T]
    L.pbrt_perspective.restype = None
    L.pbrt_transform_point.argtypes = [T, P(d), P(d), P(d), P(d)]
    L.pbrt_transform_point.restype = None
    L.pbrt_transform_ray.argtypes = [T, P(d), P(d), P(d), P(d)]
    L.pbrt_transform_ray.restype = None
    L.pbrt_make_sphere.argtypes = [T, C.c_int, d, d, d, d, P(abi.ShapeDesc)]
    L.pbrt_make_sphere.restype = None
    L.pbrt_make_disk.argtypes = [T, d, d, d, d, P(abi.ShapeDesc)]
    L.pbrt_make_disk.restype = None
    L.pbrt_make_matte_constant.argtypes = [d, d, d, d, P(abi.MaterialDesc)]
    L.pbrt_make_matte_constant.restype = None
    L.pbrt_make_matte_checkerboard.argtypes = [P(d), P(d), d, d, P(d), P(d), d, P(abi.MaterialDesc)]
    L.pbrt_make_matte_checkerboard.restype = None
    L.pbrt_random_sampler.argtypes = [C.c_int32, P(abi.RenderDesc)]
    L.pbrt_random_sampler.restype = None
    L.pbrt_make_mirror.argtypes = [P(d), P(abi.MaterialDesc)]
    L.pbrt_make_mirror.restype = None
    L.pbrt_make_glass.argtypes = [P(d), P(d), d, d, d, P(abi.MaterialDesc)]
    L.pbrt_make_glass.restype = None
    L.pbrt_make_point_light.argtypes = [T, P(d), P(abi.LightDesc)]
    L.pbrt_make_point_light.restype = None
    L.pbrt_make_distant_light.argtypes = [T, P(d), P(d), P(abi.LightDesc)]
    L.pbrt_make_distant_light.restype = None
    L.pbrt_make_diffuse_area_light.argtypes = [P(d), C.c_int, C.c_int, P(abi.LightDesc)]
    L.pbrt_make_diffuse_area_light.restype = None
    L.pbrt_sb_create.restype = C.c_void_p
    L.pbrt_sb_destroy.argtypes = [C.c_void_p]
    L.pbrt_sb_destroy.restype = None
    L.pbrt_sb_add_shape.argtypes = [C.c_void_p, P(abi.ShapeDesc)]
    L.pbrt_sb_add_material.argtypes = [C.c_void_p, P(abi.MaterialDesc)]
    L.pbrt_sb_add_primitive.argtypes = [C.c_void_p, P(abi.PrimitiveDesc)]
    L.pbrt_sb_add_light.argtypes = [C.c_void_p, P(abi.LightDesc)]
    L.pbrt_sb_set_film.argtypes = [C.c_void_p, i64, i64, P(d), d, d, d]
    L.pbrt_sb_set_perspective_camera.argtypes = [C.c_void_p, T, P(d), d, d, d, d, d]
    L.pbrt_sb_build.argtypes = [C.c_void_p, C.c_int, P(P(abi.SceneDesc))]
    L.pbrt_sb_prim_order.argtypes = [C.c_void_p, P(C.c_int32), C.c_int]
    L.pbrt_scene_light_distribution.argtypes = [P(abi.SceneDesc), C.c_int, P(abi.DistributionDesc)]
    L.pbrt_scene_readme.argtypes = [i64, i64, P(C.c_void_p)]
    L.pbrt_scene_cornell.argtypes = [i64, i64, P(C.c_void_p)]
    L.pbrt_scene_heightfield.argtypes = [i64, i64, C.c_int32, C.c_uint64, C.c_int32, P(C.c_void_p)]
    L.pbrt_sb_add_mesh.argtypes = [C.c_void_p, C.c_int32, P(C.c_float), C.c_int32, P(C.c_int32), C.c_int32,
                                   C.c_int32]
    L.pbrt_gpu_mesh_info.argtypes = [C.c_void_p, P(d), C.c_int]
    L.pbrt_gpu_mesh_download.argtypes = [C.c_void_p, C.c_void_p, P(C.c_int32), P(C.c_float)]
    _lib = L
    return L


def hip_runtimes():
    """Paths of the distinct HIP runtime libraries (libamdhip64) mapped into this
    process. One is normal. Two means that a torch wheel's own copy and the one
    libpbrt_gpu.so links were both loaded, which happens when the library is
    loaded before torch is imported; the copy that
    initialises second then finds no GPU."""
    found = []
    try:
        with open("/proc/self/maps") as maps:
            for line in maps:
                part = line.split(None, 5)
                if len(part) == 6 and "libamdhip64" in os.path.basename(part[5].strip()):
                    path = part[5].strip()
                    if path not in found:
                        found.append(path)
    except OSError:   # no procfs: nothing to report
        pass
    return found


def _create_failed(what):
    """The message of a failed pbrt_gpu[_group]_create."""
    rts = hip_runtimes()
    if len(rts) > 1:
        return (f"{what} failed: this process holds {len(rts)} HIP runtimes ({', '.join(rts)}) and only the "
                "first to initialise sees the GPU; import torch before pbrtgpu loads libpbrt_gpu.so "
                "(pbrtgpu.lib(), a Scene or a Renderer) so that both share one")
    return f"{what} failed (no GPU visible?)"


def build_id():
    """Content hash of the sources the loaded library was built from."""
    return lib().pbrt_gpu_build_id().decode()


def kernel_names():
    """Every kernel name the launch log can produce (pbrt_gpu_kernel_names; needs no GPU)."""
    n = lib().pbrt_gpu_kernel_names(None, 0)
    out = (C.c_char_p * n)()
    lib().pbrt_gpu_kernel_names(out, n)
    return [s.decode() for s in out]


def kernel_choice(family, *args):
    """The kernel the selector (kernel_select.hip) of `family` gives for these template arguments, by its
    launch-log name, or None if it is not compiled (pbrt_diag_kernel_choice; needs no GPU)."""
    abi.declare_kernel_choice(lib())
    a = (C.c_int * max(len(args), 1))(*[int(x) for x in args])
    name = lib().pbrt_diag_kernel_choice(family.encode(), a, len(args))
    return name.decode() if name is not None else None


class Launch(tuple):
    """One record of the launch log: (name, grid, block, lds, stream); grid and block
    are 3-tuples, lds the dynamic LDS bytes, stream 0 (the context's main stream), 2
    or 3. lds_static holds the kernel's static LDS bytes."""
    name = property(lambda s: s[0])
    grid = property(lambda s: s[1])
    block = property(lambda s: s[2])
    lds = property(lambda s: s[3])
    stream = property(lambda s: s[4])
    lds_static = 0


def _launch_log(ctx, outside):
    which = abi.PBRT_LAUNCHES_OUTSIDE if outside else abi.PBRT_LAUNCHES_FRAME
    n = lib().pbrt_gpu_launch_log(ctx, which, None, 0, None)
    if n < 0:
        raise PbrtError(-n, "pbrt_gpu_launch_log failed")
    recs = (abi.LaunchRec * max(n, 1))()
    over = C.c_uint64(0)
    n = lib().pbrt_gpu_launch_log(ctx, which, recs, n, C.byref(over))
    if n < 0:
        raise PbrtError(-n, "pbrt_gpu_launch_log failed")
    out = []
    for r in recs[:n]:
        rec = Launch((r.name.decode(), tuple(r.grid), tuple(r.block), int(r.lds_dynamic), int(r.stream)))
        rec.lds_static = int(r.lds_static)
        out.append(rec)
    return out, int(over.value)


def _d3(v):
    return (C.c_double * 3)(*v)


# ------------------------------------------------------------------ transforms
def translate(x, y, z):
    t = abi.Transform()
    lib().pbrt_translate(x, y, z, C.byref(t))
    return t


def scale(x, y, z):
    t = abi.Transform()
    lib().pbrt_scale(x, y, z, C.byref(t))
    return t


def rotate(axis, degrees):
    t = abi.Transform()
    getattr(lib(), "pbrt_rotate_" + "xyz"[axis])(degrees, C.byref(t))
    return t


def mul(a, b):
    t = abi.Transform()
    lib().pbrt_transform_mul(C.byref(a), C.byref(b), C.byref(t))
    return t


def look_at(pos, look, up):
    t = abi.Transform()
    rc = lib().pbrt_look_at(_d3(pos), _d3(look), _d3(up), C.byref(t))
    if rc:
        raise PbrtError(rc, "LookAt: up parallel to view direction")
    return t


def transform_ray(t, o, d):
    oo, od = (C.c_double * 3)(), (C.c_double * 3)()
    lib().pbrt_transform_ray(C.byref(t), _d3(o), _d3(d), oo, od)
    return list(oo), list(od)


# ------------------------------------------------------------------------ scene
class Scene:
    """A pbrt_scene_builder plus its built pbrt_scene_desc."""

    def __init__(self, handle=None):
        self.h = handle if handle is not None else lib().pbrt_sb_create()
        self.desc_ptr = None

    @classmethod
    def readme(cls, w, h):
        hb = C.c_void_p()
        rc = lib().pbrt_scene_readme(w, h, C.byref(hb))
        if rc:
            raise PbrtError(rc, "pbrt_scene_readme")
        s = cls(hb.value)
        s._fetch()
        return s

    @classmethod
    def cornell(cls, w, h):
        hb = C.c_void_p()
        rc = lib().pbrt_scene_cornell(w, h, C.byref(hb))
        if rc:
            raise PbrtError(rc, "pbrt_scene_cornell")
        s = cls(hb.value)
        s._fetch()
        return s

    @classmethod
    def readme_glass(cls, w, h, special="glass", mirror=True):
        """internal/render/server.go:67-91 (commented out): the README scene plus
        a sphere of radius 5 at (50, 2.5, 50) of NewGlass(Kr = Kt = 0.5, index
        1.5) -- the commented code attaches the checkerboard `m`, the glass it
        defines is what image.png shows. special = "black": that sphere a black
        Matte instead. mirror: a Mirror (Kr 0.9) sphere beside it at (35, 5, 45).
        Built (BVH, 2 primitives per node as server.go:162)."""
        s = cls.readme(w, h)
        m = s.add_glass() if special == "glass" else s.add_matte((0.0, 0.0, 0.0))
        spheres = [((50, 2.5, 50), m)]
        if mirror:
            spheres.append(((35, 5.0, 45), s.add_mirror()))
        for (pos, mat) in spheres:
            sph = s.add_sphere(translate(0, 0, 0), 5.0)
            s.add_primitive(sph, mat, translate(*pos))
        s.build(2)
        return s

    @classmethod
    def heightfield(cls, w, h, quads=707, seed=1, spheres=False):
        """BASELINE config D (quads 707: 999 698 triangles) / E (2236): the
        height-field extension scene (include/pbrt_scene.h)."""
        hb = C.c_void_p()
        rc = lib().pbrt_scene_heightfield(w, h, quads, seed, 1 if spheres else 0, C.byref(hb))
        if rc:
            raise PbrtError(rc, "pbrt_scene_heightfield")
        s = cls(hb.value)
        s._fetch()
        return s

    # builder API (pbrt_sb_*) -------------------------------------------------
    def add_mesh(self, p, indices, material, reverse=False):
        """p: (nv, 3) float32 world positions; indices: (nt, 3) int32."""
        p = np.ascontiguousarray(p, dtype=np.float32)
        idx = np.ascontiguousarray(indices, dtype=np.int32)
        r = lib().pbrt_sb_add_mesh(self.h, p.shape[0], p.ctypes.data_as(C.POINTER(C.c_float)), idx.shape[0],
                                   idx.ctypes.data_as(C.POINTER(C.c_int32)), material, int(reverse))
        if r < 0:
            raise PbrtError(-r, "pbrt_sb_add_mesh")
        return r

    def add_sphere(self, o2w, radius, reverse=False, z_min=None, z_max=None, phi_max=360.0):
        sd = abi.ShapeDesc()
        lib().pbrt_make_sphere(C.byref(o2w), int(reverse), radius, -radius if z_min is None else z_min,
                               radius if z_max is None else z_max, phi_max, C.byref(sd))
        return lib().pbrt_sb_add_shape(self.h, C.byref(sd))

    def add_disk(self, o2w, height, radius, inner=0.0, phi_max=360.0):
        sd = abi.ShapeDesc()
        lib().pbrt_make_disk(C.byref(o2w), height, radius, inner, phi_max, C.byref(sd))
        return lib().pbrt_sb_add_shape(self.h, C.byref(sd))

    def add_matte(self, rgb, sigma=0.0):
        m = abi.MaterialDesc()
        lib().pbrt_make_matte_constant(rgb[0], rgb[1], rgb[2], sigma, C.byref(m))
        return lib().pbrt_sb_add_material(self.h, C.byref(m))

    def add_checker(self, vs, vt, ds, dt, tex1, tex2, sigma=0.0):
        m = abi.MaterialDesc()
        lib().pbrt_make_matte_checkerboard(_d3(vs), _d3(vt), ds, dt, _d3(tex1), _d3(tex2), sigma, C.byref(m))
        return lib().pbrt_sb_add_material(self.h, C.byref(m))

    def add_mirror(self, kr=(0.9, 0.9, 0.9)):
        """materials.NewMirror (mirror.go:9-14; Kr 0.9 by default)."""
        m = abi.MaterialDesc()
        lib().pbrt_make_mirror(_d3(kr), C.byref(m))
        return lib().pbrt_sb_add_material(self.h, C.byref(m))

    def add_glass(self, kr=(0.5, 0.5, 0.5), kt=(0.5, 0.5, 0.5), u_roughness=0.0, v_roughness=0.0, eta=1.5):
        """materials.NewGlass (glass.go:15-26); defaults are server.go:80-87's glass."""
        m = abi.MaterialDesc()
        lib().pbrt_make_glass(_d3(kr), _d3(kt), u_roughness, v_roughness, eta, C.byref(m))
        return lib().pbrt_sb_add_material(self.h, C.byref(m))

    def add_primitive(self, shape, material, prim_to_world=None):
        p = abi.PrimitiveDesc()
        p.shape, p.material = shape, material
        if prim_to_world is None:
            p.kind = abi.PBRT_PRIM_GEOMETRIC
        else:
            p.kind = abi.PBRT_PRIM_TRANSFORMED
            p.prim_to_world = prim_to_world
        return lib().pbrt_sb_add_primitive(self.h, C.byref(p))

    def add_point_light(self, l2w, I):
        ld = abi.LightDesc()
        lib().pbrt_make_point_light(C.byref(l2w), _d3(I), C.byref(ld))
        return lib().pbrt_sb_add_light(self.h, C.byref(ld))

    def add_distant_light(self, l2w, L, w):
        ld = abi.LightDesc()
        lib().pbrt_make_distant_light(C.byref(l2w), _d3(L), _d3(w), C.byref(ld))
        return lib().pbrt_sb_add_light(self.h, C.byref(ld))

    def add_area_light(self, Lemit, shape, two_sided=False):
        ld = abi.LightDesc()
        lib().pbrt_make_diffuse_area_light(_d3(Lemit), shape, int(two_sided), C.byref(ld))
        return lib().pbrt_sb_add_light(self.h, C.byref(ld))

    def set_film(self, w, h, crop=(0, 0, 1, 1), filter_radius=(1.0, 1.0), max_lum=1.0):
        rc = lib().pbrt_sb_set_film(self.h, w, h, (C.c_double * 4)(*crop), filter_radius[0], filter_radius[1], max_lum)
        if rc:
            raise PbrtError(rc, "set_film")

    def set_camera(self, cam2world, screen=(0, 0, 1, 1), shutter=(0.0, 1.0), lens=0.0, focal=20.0, fov=100.0):
        rc = lib().pbrt_sb_set_perspective_camera(self.h, C.byref(cam2world), (C.c_double * 4)(*screen),
                                                  shutter[0], shutter[1], lens, focal, fov)
        if rc:
            raise PbrtError(rc, "set_camera")

    def build(self, max_prims_in_node=2):
        """accelerator.NewBVH(prims, maxPrimsInNode, SplitSAH) + pbrt.NewScene."""
        ptr = C.POINTER(abi.SceneDesc)()
        rc = lib().pbrt_sb_build(self.h, max_prims_in_node, C.byref(ptr))
        if rc:
            raise PbrtError(rc, "pbrt_sb_build")
        self.desc_ptr = ptr
        return self

    def _fetch(self):
        # fixtures are already built (maxPrimsInNode 2); rebuilding is idempotent
        self.build(2)

    @property
    def desc(self):
        return self.desc_ptr.contents

    def prim_order(self):
        n = self.desc.n_prims
        out = (C.c_int32 * max(n, 1))()
        lib().pbrt_sb_prim_order(self.h, out, n)
        return list(out)[:n]

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.pbrt_sb_destroy(self.h)
            self.h = None


# --------------------------------------------------------------- device buffers
class ContextToken:
    """Whether a Renderer's context is alive. The Renderer and every DeviceBuffer
    it made share one token, and Renderer.close() clears it before the context
    is destroyed: from then on no buffer touches the library again, in whatever
    order the objects are finalised (interpreter teardown included)."""
    __slots__ = ("alive",)

    def __init__(self):
        self.alive = True


BUFFER_DTYPES = (np.dtype(np.float64), np.dtype(np.int32), np.dtype(np.uint8), np.dtype(np.uint64),
                 np.dtype(np.uint32))
RAY_KEYS = ("ox", "oy", "oz", "dx", "dy", "dz")
HIT_DTYPES = {"hit": np.uint8, "t_max": np.float64, "prim": np.int32, "px": np.float64, "py": np.float64,
              "pz": np.float64, "nx": np.float64, "ny": np.float64, "nz": np.float64}
RNG_KEYS = ("state", "inc")
LI_DTYPES = {"r": np.float64, "g": np.float64, "b": np.float64, "state": np.uint64, "draws": np.uint32,
             "rays": np.uint32}
# pbrt_path_soa's arrays (tmax optional): 141 bytes a path, 133 without tmax
PATH_DTYPES = {**{k: np.float64 for k in RAY_KEYS + ("tmax", "lr", "lg", "lb", "br", "bg", "bb", "eta_scale")},
               "state": np.uint64, "inc": np.uint64, "draws": np.uint32, "rays": np.uint32, "bounces": np.int32,
               "status": np.uint8}
PATH_BYTES = sum(np.dtype(dt).itemsize for dt in PATH_DTYPES.values())
# pbrt_path_step_soa's arrays (all optional): the hit's, material, and the term added to L
STEP_DTYPES = {**HIT_DTYPES, "material": np.int32, "ar": np.float64, "ag": np.float64, "ab": np.float64}
# frame_samples' outputs (tmax, px, py optional) and film_add's inputs
SAMPLE_DTYPES = {**{k: np.float64 for k in RAY_KEYS + ("tmax", "pfilm_x", "pfilm_y")}, "state": np.uint64,
                 "inc": np.uint64, "px": np.int32, "py": np.int32}
SAMPLE_REQUIRED = RAY_KEYS + ("pfilm_x", "pfilm_y", "state", "inc")
FILM_KEYS = ("pfilm_x", "pfilm_y", "r", "g", "b")
FRAME_BYTES_PER_SAMPLE = 8 * (len(SAMPLE_REQUIRED) + 3)   # a composed frame's arrays: 104 B (render_samples)
STRAT_SAMPLE_KEYS = ("k", "table")   # int32 per sample; "s1d": float64, n_dims * spp per pixel of the range
STRAT_BYTES_PER_SAMPLE = FRAME_BYTES_PER_SAMPLE + 8   # with k and table: 112 B (render_samples_stratified)


class DeviceBuffer:
    """pbrt_gpu_buffer: n elements of float64, int32, uint8, uint64 or uint32 in device memory
    that the Renderer's context owns. Made by Renderer.buffer / Renderer.upload.
    It keeps its Renderer alive; once that Renderer is closed the buffer is
    closed too (its memory went with the context): close() and deletion then do
    nothing and every other use raises PbrtError."""

    def __init__(self, renderer, handle, ptr, n, dtype):
        self.renderer = renderer
        self._token = renderer._token
        self._h = handle
        self._ptr = ptr
        self.n = int(n)
        self.dtype = np.dtype(dtype)

    @property
    def closed(self):
        return self._h is None or not self._token.alive

    def _live(self):
        if self.closed:
            raise PbrtError(abi.PBRT_E_INVALID, "the device buffer (or its Renderer) is closed")

    @property
    def ptr(self):
        self._live()
        return self._ptr

    @property
    def nbytes(self):
        return self.n * self.dtype.itemsize

    def upload(self, array, offset=0):
        """Copies a host array to elements [offset, offset + len(array))."""
        self._live()
        a = np.ascontiguousarray(array)
        if a.dtype != self.dtype:
            raise PbrtError(abi.PBRT_E_INVALID, f"upload of {a.dtype} into a {self.dtype} buffer")
        if offset < 0 or offset + a.size > self.n:
            raise PbrtError(abi.PBRT_E_INVALID, f"elements [{offset}, {offset + a.size}) outside a buffer of {self.n}")
        rc = lib().pbrt_gpu_buffer_upload(self._h, offset * self.dtype.itemsize, a.ctypes.data, a.nbytes)
        self.renderer._check(rc)
        return self

    def download(self):
        """The buffer's n elements as a host array (synchronises the context's stream)."""
        self._live()
        out = np.empty(self.n, dtype=self.dtype)
        self.renderer._check(lib().pbrt_gpu_buffer_download(self._h, 0, out.ctypes.data, out.nbytes))
        return out

    def close(self):
        h, self._h = self._h, None
        if h is not None and self._token.alive and _lib is not None:
            _lib.pbrt_gpu_buffer_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter teardown: module globals may already be gone
            pass


def check_buffers(renderer, n, bufs):
    """The bounds protection of the device-query calls: every (name, buffer,
    dtype) of bufs must be an open DeviceBuffer of this renderer, of that dtype
    and of at least n elements. Raises PbrtError(PBRT_E_INVALID) before anything
    reaches the library; needs no context."""
    if not isinstance(n, (int, np.integer)) or n < 0 or n > 2**31 - 1:
        raise PbrtError(abi.PBRT_E_INVALID, f"ray count {n!r} outside 0 .. 2^31 - 1")
    for name, b, dtype in bufs:
        if not isinstance(b, DeviceBuffer):
            raise PbrtError(abi.PBRT_E_INVALID, f"{name}: not a DeviceBuffer")
        if b.closed:
            raise PbrtError(abi.PBRT_E_INVALID, f"{name}: the buffer is closed")
        if b.renderer is not renderer:
            raise PbrtError(abi.PBRT_E_INVALID, f"{name}: the buffer belongs to another Renderer")
        if b.dtype != np.dtype(dtype):
            raise PbrtError(abi.PBRT_E_INVALID, f"{name}: {b.dtype} buffer where {np.dtype(dtype)} is needed")
        if b.n < n:
            raise PbrtError(abi.PBRT_E_INVALID, f"{name}: {b.n} elements for {n} rays")


def _ray_bufs(rays):
    """rays as [(name, buffer, dtype)]: a dict with ox..dz and an optional tmax,
    or a tuple of 6 or 7 buffers in that order."""
    if not isinstance(rays, dict):
        rays = tuple(rays)
        if len(rays) not in (6, 7):
            raise PbrtError(abi.PBRT_E_INVALID, "rays: 6 buffers (ox..dz) or 7 (with tmax)")
        rays = dict(zip(RAY_KEYS + ("tmax",), rays))
    unknown = set(rays) - set(RAY_KEYS) - {"tmax"}
    missing = [k for k in RAY_KEYS if rays.get(k) is None]
    if unknown or missing:
        raise PbrtError(abi.PBRT_E_INVALID, f"rays: unknown {sorted(unknown)}, missing {missing}")
    return [(k, rays[k], np.float64) for k in RAY_KEYS + ("tmax",) if rays.get(k) is not None]


def _soa(struct, bufs):
    """A ctypes SoA struct whose fields point at the (checked) buffers."""
    s = struct()
    for name, b, _ in bufs:
        setattr(s, name, C.cast(C.c_void_p(b.ptr), dict(struct._fields_)[name]))
    return s


def _li_soas(renderer, what, rays, rng, n, out):
    """The checked (RaySoA, RngSoA, RadianceSoA) of a Li query (li_device, direct_li_device):
    rng a dict or a (state, inc) pair; out holds r, g, b and any of state, draws, rays."""
    if not isinstance(rng, dict):
        rng = dict(zip(RNG_KEYS, tuple(rng)))
    unknown = (set(out) - set(LI_DTYPES)) | (set(rng) - set(RNG_KEYS))
    missing = [k for k in ("r", "g", "b") if out.get(k) is None] + [k for k in RNG_KEYS if rng.get(k) is None]
    if unknown or missing:
        raise PbrtError(abi.PBRT_E_INVALID, f"{what}: unknown {sorted(unknown)}, missing {missing}")
    rb = _ray_bufs(rays)
    gb = [(k, rng[k], np.uint64) for k in RNG_KEYS]
    ob = [(k, out[k], dt) for k, dt in LI_DTYPES.items() if out.get(k) is not None]
    check_buffers(renderer, n, rb + gb + ob)
    return _soa(abi.RaySoA, rb), _soa(abi.RngSoA, gb), _soa(abi.RadianceSoA, ob)


# --------------------------------------------------------------------- renderer
class Renderer:
    """pbrt_gpu_ctx: the scene resident on one GPU."""

    KERNELS = {"auto": abi.PBRT_KERNEL_AUTO, "serial": abi.PBRT_KERNEL_SERIAL, "wave": abi.PBRT_KERNEL_WAVE,
               "wavefront": abi.PBRT_KERNEL_WAVEFRONT, "wave_ci": abi.PBRT_KERNEL_WAVE_CI,
               "wave_dl": abi.PBRT_KERNEL_WAVE_DL, "wave_cam": abi.PBRT_KERNEL_WAVE_CAM}

    def __init__(self, scene, device=-1, lanes_per_wave=0, occupancy=0, kernel="auto"):
        desc = scene.desc if isinstance(scene, Scene) else scene
        self._scene = scene  # keep the descriptor alive
        self._token = ContextToken()   # shared with every DeviceBuffer of this context
        self._primary = {}             # primary_hits: (w, h) -> its buffers
        self.res = (int(desc.film.res_x), int(desc.film.res_y))
        opts = abi.GpuOpts()
        opts.device, opts.lanes_per_wave = device, lanes_per_wave
        opts.occupancy, opts.kernel = occupancy, self.KERNELS[kernel]
        h = C.c_void_p()
        rc = lib().pbrt_gpu_create(C.byref(desc), C.byref(opts), C.byref(h))
        if rc:
            raise PbrtError(rc, _create_failed("pbrt_gpu_create") if rc == abi.PBRT_E_HIP
                            else "pbrt_gpu_create failed (bad scene descriptor or options)")
        self.h = h.value
        self.w = desc.film.crop_max_x - desc.film.crop_min_x
        self.hgt = desc.film.crop_max_y - desc.film.crop_min_y

    def _check(self, rc, stats=None):
        if rc:
            raise PbrtError(rc, lib().pbrt_gpu_last_error(self.h).decode(), stats)

    def render(self, rd):
        film = np.zeros((self.hgt, self.w, 3), dtype=np.float64)
        st = abi.GpuStats()
        rc = lib().pbrt_gpu_render(self.h, C.byref(rd), film.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st))
        self._check(rc, st)
        return film, st

    def render_async(self, rd, film_device_ptr=None):
        """Enqueue a frame; film_device_ptr = caller device buffer (e.g. tensor.data_ptr())."""
        if film_device_ptr is None:
            self._check(lib().pbrt_gpu_render_async(self.h, C.byref(rd)))
        else:
            self._check(lib().pbrt_gpu_render_async_into(self.h, C.byref(rd), C.c_void_p(film_device_ptr)))

    def synchronize(self):
        st = abi.GpuStats()
        self._check(lib().pbrt_gpu_synchronize(self.h, C.byref(st)), st)
        return st

    def film(self):
        film = np.zeros((self.hgt, self.w, 3), dtype=np.float64)
        self._check(lib().pbrt_gpu_film_download(self.h, film.ctypes.data_as(C.POINTER(C.c_double))))
        return film

    def film_device_ptr(self):
        return lib().pbrt_gpu_film_device(self.h)

    def stream(self):
        return lib().pbrt_gpu_stream(self.h)

    def mesh_info(self):
        """{tris, nodes, depth, build_ms, meshes, wide} of the context's device LBVH
        (wide: the 4-ary layout, MeshNode4; else eight threaded binary orderings)."""
        out = (C.c_double * 8)()
        lib().pbrt_gpu_mesh_info(self.h, out, 8)
        return {"tris": int(out[0]), "nodes": int(out[1]), "depth": int(out[2]), "build_ms": out[3],
                "meshes": int(out[4]), "wide": bool(out[5])}

    def mesh_download(self):
        """(nodes, gid [tris], tris [tris, 9]) of the device LBVH; nodes is a [n]
        MeshNode4 structured array for the wide layout, else [8, n] MeshNode."""
        info = self.mesh_info()
        if info["wide"]:
            dt = np.dtype([("lo", np.float32, (3, 4)), ("hi", np.float32, (3, 4)), ("child", np.uint32, 4),
                           ("parent", np.uint32), ("axis", np.uint32), ("count", np.uint32), ("pad", np.uint32)])
            nodes = np.zeros(info["nodes"], dtype=dt)
        else:
            dt = np.dtype([("bmin", np.float32, 3), ("escape", np.uint32), ("bmax", np.float32, 3),
                           ("leaf", np.uint32)])
            nodes = np.zeros(8 * info["nodes"], dtype=dt)
        gid = np.zeros(info["tris"], dtype=np.int32)
        tris = np.zeros((info["tris"], 9), dtype=np.float32)
        rc = lib().pbrt_gpu_mesh_download(self.h, nodes.ctypes.data_as(C.c_void_p),
                                          gid.ctypes.data_as(C.POINTER(C.c_int32)),
                                          tris.ctypes.data_as(C.POINTER(C.c_float)))
        self._check(rc)
        return (nodes if info["wide"] else nodes.reshape(8, info["nodes"])), gid, tris

    def tile_ticks(self):
        """(per-slot chain ticks of the last EXACT frame at 100 MHz, heavy slots of its split)."""
        heavy = C.c_int64(0)
        n = lib().pbrt_gpu_tile_ticks(self.h, None, 0, C.byref(heavy))
        out = np.zeros(max(n, 0), dtype=np.uint32)
        if n > 0:
            lib().pbrt_gpu_tile_ticks(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32)), n, C.byref(heavy))
        return out, int(heavy.value)

    def tile_costs(self):
        """(n_slots, 4) cold-frame cost features of the last EXACT frame's probe
        (chain work, hit pixels, pixels, cost); empty if that frame had a learned order."""
        n = lib().pbrt_gpu_tile_costs(self.h, None, 0)
        out = np.zeros((max(n, 0), 4), dtype=np.float32)
        if n > 0:
            rc = lib().pbrt_gpu_tile_costs(self.h, out.ctypes.data_as(C.POINTER(C.c_float)), n)
            if rc < 0:
                self._check(-rc)
        return out

    SCHEDULE_SOURCES = {0: "launch order", 1: "probe", 2: "learned", 3: "cached"}

    def schedule_source(self):
        """Where the last EXACT frame's tile schedule came from: 'launch order', 'probe'
        (cold-frame estimate), 'learned' (this context's previous frame) or 'cached'
        (the process-wide cache: another context's frame of the same scene and configuration)."""
        return self.SCHEDULE_SOURCES[lib().pbrt_gpu_schedule_source(self.h)]

    def overlap_slots(self):
        """Slots of the last EXACT frame whose path stage ran completion-driven
        (pbrt_gpu_overlap_slots; 0: after the chain stage)."""
        return lib().pbrt_gpu_overlap_slots(self.h)

    def launches(self, outside=False):
        """The kernel launches of the last frame, in launch order, as (name, grid, block,
        lds, stream) records (Launch); outside=True: those outside a frame since the
        context was created (mesh LBVH build, ray queries). This is how to confirm that
        an environment knob or an option reached the kernel it names."""
        recs, self.launch_overflow = _launch_log(self.h, outside)
        return recs

    def lds_per_block(self):
        """The device's LDS limit per workgroup (bytes)."""
        return lib().pbrt_gpu_lds_per_block(self.h)

    def counters(self):
        """pbrt_gpu_counters of the last render (include/pbrt_diag.h order)."""
        out = np.zeros(128, dtype=np.uint64)
        n = lib().pbrt_gpu_counters(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), 128)
        return out[:max(n, 0)]

    def intersect(self, rays):
        """rays: (n,7) [ox,oy,oz,dx,dy,dz,tmax] -> (n,9) like the oracle."""
        rays = np.ascontiguousarray(rays, dtype=np.float64)
        n = rays.shape[0]
        cols = [np.ascontiguousarray(rays[:, k]) for k in range(7)]
        soa = abi.RaySoA(*[c.ctypes.data_as(C.POINTER(C.c_double)) for c in cols])
        hit = np.zeros(n, np.uint8)
        tmax = np.zeros(n)
        prim = np.zeros(n, np.int32)
        p = [np.zeros(n) for _ in range(6)]
        hs = abi.HitSoA(hit.ctypes.data_as(C.POINTER(C.c_uint8)), tmax.ctypes.data_as(C.POINTER(C.c_double)),
                        prim.ctypes.data_as(C.POINTER(C.c_int32)),
                        *[a.ctypes.data_as(C.POINTER(C.c_double)) for a in p])
        rc = lib().pbrt_gpu_intersect(self.h, C.byref(soa), n, C.byref(hs))
        out = np.stack([hit.astype(np.float64), tmax, prim.astype(np.float64)] + p, axis=1)
        return rc, out

    def intersect_p(self, rays):
        rays = np.ascontiguousarray(rays, dtype=np.float64)
        n = rays.shape[0]
        cols = [np.ascontiguousarray(rays[:, k]) for k in range(7)]
        soa = abi.RaySoA(*[c.ctypes.data_as(C.POINTER(C.c_double)) for c in cols])
        occ = np.zeros(n, np.uint8)
        rc = lib().pbrt_gpu_intersect_p(self.h, C.byref(soa), n, occ.ctypes.data_as(C.POINTER(C.c_uint8)))
        return rc, occ

    # ---- device-resident queries: numpy and ctypes only; the device memory is
    # the context's own (DeviceBuffer), so nothing here can outlive the context
    def buffer(self, n, dtype=np.float64):
        """A DeviceBuffer of n elements (float64, int32, uint8, uint64 or uint32), uninitialised."""
        dtype = np.dtype(dtype)
        if dtype not in BUFFER_DTYPES or n <= 0:
            raise PbrtError(abi.PBRT_E_INVALID,
                            f"buffer of {n} x {dtype}: float64, int32, uint8, uint64 or uint32, n > 0")
        if not getattr(self, "h", None):
            raise PbrtError(abi.PBRT_E_INVALID, "the Renderer is closed")
        h = C.c_void_p()
        self._check(lib().pbrt_gpu_buffer_create(self.h, int(n) * dtype.itemsize, C.byref(h)))
        return DeviceBuffer(self, h.value, lib().pbrt_gpu_buffer_ptr(h.value), n, dtype)

    def upload(self, array):
        """A DeviceBuffer holding a copy of a 1-D host array."""
        a = np.ascontiguousarray(array).reshape(-1)
        return self.buffer(a.size, a.dtype).upload(a)

    def intersect_device(self, rays, n, hits, staged=False):
        """pbrt_gpu_intersect_device: closest hits of rays[0:n] into the buffers of
        hits ({"hit": uint8, and any of t_max, prim (int32), px..nz}). Enqueue only:
        read the results with DeviceBuffer.download() or after query_status().
        Returns the status (PBRT_E_INVALID while a render is in flight).
        staged: the diagnostic pbrt_diag_intersect_staged_device, the same query
        on the LDS-staged walk of the render kernels (a tree of at most 64 nodes,
        no mesh; PBRT_E_INVALID otherwise)."""
        unknown = set(hits) - set(HIT_DTYPES)
        if unknown or hits.get("hit") is None:
            raise PbrtError(abi.PBRT_E_INVALID, f"hits: 'hit' is required; unknown {sorted(unknown)}")
        rb = _ray_bufs(rays)
        hb = [(k, hits[k], HIT_DTYPES[k]) for k in HIT_DTYPES if hits.get(k) is not None]
        check_buffers(self, n, rb + hb)
        rs, hs = _soa(abi.RaySoA, rb), _soa(abi.HitSoA, hb)
        entry = lib().pbrt_diag_intersect_staged_device if staged else lib().pbrt_gpu_intersect_device
        return entry(self.h, C.byref(rs), n, C.byref(hs))

    def intersect_p_device(self, rays, n, occluded, staged=False):
        """pbrt_gpu_intersect_p_device: any-hit flags (uint8 buffer) of rays[0:n].
        staged: pbrt_diag_intersect_p_staged_device (see intersect_device)."""
        rb = _ray_bufs(rays)
        check_buffers(self, n, rb + [("occluded", occluded, np.uint8)])
        rs = _soa(abi.RaySoA, rb)
        entry = lib().pbrt_diag_intersect_p_staged_device if staged else lib().pbrt_gpu_intersect_p_device
        return entry(self.h, C.byref(rs), n, C.c_void_p(occluded.ptr))

    def cull_groups(self):
        """Leaf culling groups of the context's LDS-staged tree (pbrt_gpu_cull_groups; 0: none)."""
        return lib().pbrt_gpu_cull_groups(self.h)

    def camera_rays(self, window=None, film_offset=(0.5, 0.5), lens=(0.5, 0.5), time_u=0.0, out=None):
        """pbrt_gpu_camera_rays_device: the camera rays of the pixel window (x0, y0,
        x1, y1) (None: the whole film resolution) in raster order, pFilm = pixel +
        film_offset. out: ray buffers as intersect_device takes them (tmax
        optional); None allocates seven. Returns them as a dict."""
        x0, y0, x1, y1 = (0, 0) + self.res if window is None else (int(v) for v in window)
        if not (0 <= x0 < x1 <= self.res[0] and 0 <= y0 < y1 <= self.res[1]):
            raise PbrtError(abi.PBRT_E_INVALID, f"window {(x0, y0, x1, y1)} outside the film {self.res}")
        n = (x1 - x0) * (y1 - y0)
        if out is None:
            out = {k: self.buffer(n) for k in RAY_KEYS + ("tmax",)}
        rb = _ray_bufs(out)
        check_buffers(self, n, rb)
        d = abi.CameraRaysDesc(x0, y0, x1, y1, film_offset[0], film_offset[1], lens[0], lens[1], time_u)
        rs = _soa(abi.RaySoAOut, rb)
        self._check(lib().pbrt_gpu_camera_rays_device(self.h, C.byref(d), C.byref(rs)))
        return {k: b for k, b, _ in rb}

    def li_device(self, rays, rng, n, out, max_depth=10, light_strategy=abi.PBRT_LIGHT_STRATEGY_UNIFORM,
                  rr_threshold=1.0, integrator=abi.PBRT_INTEGRATOR_PATH):
        """pbrt_gpu_li_device: Path.Li of rays[0:n], ray i on the PCG32 stream (rng["state"][i],
        rng["inc"][i]) (uint64 buffers; a dict or a pair), into the buffers of out: r, g, b
        (float64, required) and any of state (uint64: the stream after the path), draws (uint32:
        its PCG32 draws) and rays (uint32: closest | shadow << 16). Enqueue only, like
        intersect_device; a ray on which the reference panics has L = 0 and is counted in
        query_status(). Returns the status (PBRT_E_UNSUPPORTED: last_error() says why)."""
        rs, gs, os_ = _li_soas(self, "li_device", rays, rng, n, out)
        d = abi.li_desc(max_depth, light_strategy, rr_threshold, integrator)
        return lib().pbrt_gpu_li_device(self.h, C.byref(d), C.byref(rs), C.byref(gs), n, C.byref(os_))

    def direct_li_device(self, rays, rng, n, out, max_depth=5, dl_strategy=abi.PBRT_DL_UNIFORM_SAMPLE_ALL):
        """pbrt_gpu_direct_li_device: DirectLighting.Li of rays[0:n], with li_device's buffers,
        outputs and buffer checks: ray i on the PCG32 stream (rng["state"][i], rng["inc"][i]), into
        r, g, b (required) and any of state, draws and rays (closest | shadow << 16). Enqueue
        only; a ray on which the reference panics has L = 0 and is counted in query_status().
        Returns the status (PBRT_E_UNSUPPORTED: last_error() says why)."""
        rs, gs, os_ = _li_soas(self, "direct_li_device", rays, rng, n, out)
        d = abi.direct_li_desc(max_depth, dl_strategy)
        return lib().pbrt_gpu_direct_li_device(self.h, C.byref(d), C.byref(rs), C.byref(gs), n, C.byref(os_))

    # ---- Path.Li one bounce at a time (pbrt_gpu_path_begin_device, pbrt_gpu_path_step_device)
    def path_buffers(self, n, tmax=False):
        """The arrays of pbrt_path_soa for n paths as a dict of DeviceBuffers (PATH_DTYPES; tmax only
        when asked: without it a step's ray has TMax +Inf), uninitialised: path_begin fills them."""
        return {k: self.buffer(n, dt) for k, dt in PATH_DTYPES.items() if tmax or k != "tmax"}

    def path_queue(self, n):
        """A pbrt_path_queue for up to n paths: {"index": int32 x n, "count": uint32 x 1}."""
        return {"index": self.buffer(n, np.int32), "count": self.buffer(1, np.uint32)}

    def _path_soa(self, what, paths, n):
        unknown = set(paths) - set(PATH_DTYPES)
        missing = [k for k in PATH_DTYPES if k != "tmax" and paths.get(k) is None]
        if unknown or missing:
            raise PbrtError(abi.PBRT_E_INVALID, f"{what}: paths: unknown {sorted(unknown)}, missing {missing}")
        pb = [(k, paths[k], dt) for k, dt in PATH_DTYPES.items() if paths.get(k) is not None]
        check_buffers(self, n, pb)
        return _soa(abi.PathSoA, pb)

    def _path_queue(self, what, q, n):
        if q is None:
            return None
        if set(q) != {"index", "count"} or q["index"] is None or q["count"] is None:
            raise PbrtError(abi.PBRT_E_INVALID, f"{what}: a queue is {{'index': int32 x n, 'count': uint32 x 1}}")
        check_buffers(self, n, [(what + ".index", q["index"], np.int32)])
        check_buffers(self, 1, [(what + ".count", q["count"], np.uint32)])
        return _soa(abi.PathQueue, [("index", q["index"], np.int32), ("count", q["count"], np.uint32)])

    def path_begin(self, rays, rng, n, paths):
        """pbrt_gpu_path_begin_device: the fresh state of n paths (L 0, beta 1, eta_scale 1, no
        bounce, draw or ray, ALIVE) from li_device's rays and rng, into the buffers of paths
        (path_buffers). Enqueue only. Returns the status."""
        if not isinstance(rng, dict):
            rng = dict(zip(RNG_KEYS, tuple(rng)))
        if set(rng) != set(RNG_KEYS):
            raise PbrtError(abi.PBRT_E_INVALID, f"path_begin: rng is {RNG_KEYS}")
        rb = _ray_bufs(rays)
        gb = [(k, rng[k], np.uint64) for k in RNG_KEYS]
        check_buffers(self, n, rb + gb)
        ps = self._path_soa("path_begin", paths, n)
        rs, gs = _soa(abi.RaySoA, rb), _soa(abi.RngSoA, gb)
        return lib().pbrt_gpu_path_begin_device(self.h, C.byref(rs), C.byref(gs), n, C.byref(ps))

    def path_step(self, paths, n, in_queue=None, out_queue=None, step=None, max_depth=10,
                  light_strategy=abi.PBRT_LIGHT_STRATEGY_UNIFORM, rr_threshold=1.0, integrator=abi.PBRT_INTEGRATOR_PATH):
        """pbrt_gpu_path_step_device: one iteration of Path.Li for every ALIVE path the call covers:
        paths 0 .. n-1, or those in_queue names (path_queue; its count is read on the device). The
        paths that are ALIVE afterwards are appended to out_queue (its count is zeroed first). step:
        a dict of any of STEP_DTYPES' buffers (the hit's arrays, material, ar/ag/ab), written at the
        indices of the paths advanced. The desc is li_device's. Enqueue only; a path on which the
        reference panics is PANICKED with L = 0 and counted in query_status(). Returns the status
        (PBRT_E_UNSUPPORTED: last_error() says why)."""
        ps = self._path_soa("path_step", paths, n)
        qi, qo = self._path_queue("in_queue", in_queue, n), self._path_queue("out_queue", out_queue, n)
        if qi is not None and qo is not None and (in_queue["index"] is out_queue["index"] or
                                                  in_queue["count"] is out_queue["count"]):
            raise PbrtError(abi.PBRT_E_INVALID, "path_step: the in and out queues alias")
        ss = None
        if step is not None:
            unknown = set(step) - set(STEP_DTYPES)
            if unknown:
                raise PbrtError(abi.PBRT_E_INVALID, f"path_step: step: unknown {sorted(unknown)}")
            sb = [(k, step[k], dt) for k, dt in STEP_DTYPES.items() if step.get(k) is not None]
            check_buffers(self, n, sb)
            ss = abi.PathStepSoA()
            ss.hit = _soa(abi.HitSoA, [t for t in sb if t[0] in HIT_DTYPES])
            for k, b, _ in sb:
                if k not in HIT_DTYPES:
                    setattr(ss, k, C.cast(C.c_void_p(b.ptr), dict(abi.PathStepSoA._fields_)[k]))
        d = abi.li_desc(max_depth, light_strategy, rr_threshold, integrator)
        ref = lambda s: C.byref(s) if s is not None else None   # noqa: E731
        return lib().pbrt_gpu_path_step_device(self.h, C.byref(d), C.byref(ps), ref(qi), ref(qo), n, ref(ss))

    def radiance_stepwise(self, rays, state, inc, max_depth=10, **desc):
        """radiance() composed of path_begin and max_depth path_steps over ping-pong queues: the
        same arguments (desc: light_strategy, rr_threshold), the same return value (L (n, 3), state,
        draws, rays), the same bits."""
        return self._stepwise("radiance_stepwise", rays, state, inc, max_depth, desc, False)[:4]

    def radiance_by_bounce(self, rays, state, inc, max_depth=10, **desc):
        """radiance_stepwise that also returns the (max_depth, n, 3) array of the terms each step
        added to L (0 where a path was not advanced): (L, state, draws, rays, added). Their sum in
        step order, as float64 additions from 0, is L."""
        return self._stepwise("radiance_by_bounce", rays, state, inc, max_depth, desc, True)

    def _stepwise(self, what, rays, state, inc, max_depth, desc, by_bounce):
        rays = np.ascontiguousarray(rays, dtype=np.float64)
        n = rays.shape[0]
        if rays.ndim != 2 or rays.shape[1] not in (6, 7) or len(state) != n or len(inc) != n:
            raise PbrtError(abi.PBRT_E_INVALID, f"{what}: rays (n, 6) or (n, 7), state and inc of n elements")
        added = np.zeros((max(int(max_depth), 0), n, 3))
        if n == 0:
            return np.zeros((0, 3)), np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32), added
        bufs = []
        try:
            rb = [self.upload(rays[:, k]) for k in range(rays.shape[1])]
            gb = [self.upload(np.asarray(a, dtype=np.uint64)) for a in (state, inc)]
            pb = self.path_buffers(n, tmax=rays.shape[1] == 7)
            qs = [self.path_queue(n), self.path_queue(n)]
            bufs = rb + gb + list(pb.values()) + [b for q in qs for b in q.values()]
            sb = None
            if by_bounce:
                sb = {k: self.buffer(n) for k in ("ar", "ag", "ab")}
                bufs += list(sb.values())
            self._check(self.path_begin(tuple(rb), tuple(gb), n, pb))
            for k in range(int(max_depth)):
                if by_bounce:
                    for b in sb.values():
                        b.upload(np.zeros(n))
                self._check(self.path_step(pb, n, None if k == 0 else qs[k % 2], qs[(k + 1) % 2], sb,
                                           max_depth=max_depth, **desc))
                if by_bounce:
                    added[k] = np.stack([sb[c].download() for c in ("ar", "ag", "ab")], axis=1)
            if int(max_depth) < 1:   # (the library's refusal, with nothing stepped)
                self._check(self.path_step(pb, n, max_depth=max_depth, **desc))
            rc, rec = self.query_status()
            if rc:
                raise PbrtError(rc, self.last_error(), rec)
            got = {k: pb[k].download() for k in ("lr", "lg", "lb", "state", "draws", "rays")}
        finally:
            for b in bufs:
                b.close()
        return np.stack([got["lr"], got["lg"], got["lb"]], axis=1), got["state"], got["draws"], got["rays"], added

    def direct_li_scratch_bytes(self):
        """pbrt_gpu_direct_li_scratch_bytes: the size of direct_li_device's level-record buffer (it
        changes only when a call allocates; 0 on a Matte-only scene)."""
        return lib().pbrt_gpu_direct_li_scratch_bytes(self.h)

    def last_error(self):
        """pbrt_gpu_last_error: the reason of the context's last refusal."""
        return lib().pbrt_gpu_last_error(self.h).decode()

    # ---- a frame from public pieces: samples, li_device, film_add, film_rgba8
    def num_tiles(self, tile_size=16):
        """Tiles of the film's cropped bounds at tile_size (integrator.go:316-325)."""
        return ((self.w + tile_size - 1) // tile_size) * ((self.hgt + tile_size - 1) // tile_size)

    def _frame_desc(self, what, ns, tile_begin, tile_end, tile_size, flags=0):
        """(desc, element count) of a tile range; raises where pbrt_gpu_frame_count refuses the desc.
        (A tile size or ns beyond what the kernels handle counts 0 here: the call itself then
        returns PBRT_E_UNSUPPORTED with the reason.)"""
        if tile_end is None:
            tile_end = self.num_tiles(tile_size) if tile_size >= 1 else 0
        d = abi.frame_desc(tile_size, ns, tile_begin, tile_end, flags)
        n = lib().pbrt_gpu_frame_count(self.h, C.byref(d))
        if n < 0:
            raise PbrtError(-n, f"{what}: tile_size {tile_size}, ns {ns}, tiles [{tile_begin}, {tile_end}): "
                                "outside the film's tiles, or more than 2^31 - 1 samples")
        return d, n

    def frame_count(self, ns, tile_begin=0, tile_end=None, tile_size=16):
        """pbrt_gpu_frame_count: the elements of the tile range [tile_begin, tile_end) (None: to the
        last tile) in the frame layout, ns samples per pixel."""
        return self._frame_desc("frame_count", ns, tile_begin, tile_end, tile_size)[1]

    def frame_samples(self, out, ns, tile_begin=0, tile_end=None, tile_size=16):
        """pbrt_gpu_frame_samples_device: the traced samples (k = 1 .. ns, spp = ns + 1) of a
        THROUGHPUT render with n_dims = 0 over a tile range, in the frame layout, into the
        buffers of out: ox..dz, pfilm_x, pfilm_y (float64), state, inc (uint64), and optionally
        tmax (float64), px, py (int32). Enqueue only. Returns the status."""
        unknown = set(out) - set(SAMPLE_DTYPES)
        missing = [k for k in SAMPLE_REQUIRED if out.get(k) is None]
        if unknown or missing:
            raise PbrtError(abi.PBRT_E_INVALID, f"frame_samples: unknown {sorted(unknown)}, missing {missing}")
        d, n = self._frame_desc("frame_samples", ns, tile_begin, tile_end, tile_size)
        ob = [(k, out[k], dt) for k, dt in SAMPLE_DTYPES.items() if out.get(k) is not None]
        check_buffers(self, n, ob)
        os_ = _soa(abi.FrameSamplesSoA, ob)
        return lib().pbrt_gpu_frame_samples_device(self.h, C.byref(d), C.byref(os_))

    def _film_ptr(self, what, film, elements, dtype):
        """The device address of a film argument: a DeviceBuffer of this context (checked against
        the elements the call touches) or an address (a tensor's data_ptr(), film_device_ptr())."""
        if isinstance(film, DeviceBuffer):
            check_buffers(self, elements, [(what, film, dtype)])
            return film.ptr
        if not isinstance(film, (int, np.integer)) or not film:
            raise PbrtError(abi.PBRT_E_INVALID, f"{what}: a DeviceBuffer or a device address")
        return int(film)

    def film_add(self, samples, ns, film, tile_begin=0, tile_end=None, tile_size=16, clear=False):
        """pbrt_gpu_film_add_device: adds the film of the samples of a tile range (pfilm_x,
        pfilm_y, r, g, b: float64 buffers in the frame layout, ns per pixel) to film, the (H, W,
        3) XYZ film on the device (a float64 DeviceBuffer or a device address); clear zeroes it
        first. Ascending ranges over several calls give the bits of one call. Enqueue only.
        Returns the status (PBRT_E_UNSUPPORTED: last_error() says why)."""
        unknown = set(samples) - set(FILM_KEYS)
        missing = [k for k in FILM_KEYS if samples.get(k) is None]
        if unknown or missing:
            raise PbrtError(abi.PBRT_E_INVALID, f"film_add: unknown {sorted(unknown)}, missing {missing}")
        d, n = self._frame_desc("film_add", ns, tile_begin, tile_end, tile_size,
                                abi.PBRT_FILM_ADD_CLEAR if clear else 0)
        sb = [(k, samples[k], np.float64) for k in FILM_KEYS]
        check_buffers(self, n, sb)
        ptr = self._film_ptr("film", film, self.hgt * self.w * 3, np.float64)
        ss = _soa(abi.FilmSamplesSoA, sb)
        return lib().pbrt_gpu_film_add_device(self.h, C.byref(d), C.byref(ss), C.c_void_p(ptr))

    def film_rgba8(self, film, rgba=None, w=None, h=None):
        """pbrt_gpu_film_rgba8_device: film_to_rgba8's bytes of a device film of w x h pixels (None:
        the context's film size) into rgba, a uint8 DeviceBuffer of w * h * 4 (None: a new one) or a
        4-byte aligned device address. Enqueue only. Returns rgba."""
        w, h = self.w if w is None else int(w), self.hgt if h is None else int(h)
        if w <= 0 or h <= 0 or w * h > 2**31 - 1:
            raise PbrtError(abi.PBRT_E_INVALID, f"film_rgba8: {w} x {h} pixels")
        if rgba is None:
            rgba = self.buffer(w * h * 4, np.uint8)
        fptr = self._film_ptr("film", film, w * h * 3, np.float64)
        rptr = self._film_ptr("rgba", rgba, w * h * 4, np.uint8)
        self._check(lib().pbrt_gpu_film_rgba8_device(self.h, C.c_void_p(fptr), w, h, C.c_void_p(rptr)))
        return rgba

    def film_scratch_bytes(self):
        """pbrt_gpu_film_scratch_bytes: the size of film_add's scratch buffer (it changes only when
        a call allocates)."""
        return lib().pbrt_gpu_film_scratch_bytes(self.h)

    def frame_ranges(self, ns, tile_size=16, budget_bytes=1 << 30):
        """Ascending tile ranges [(begin, end, elements)] over the whole film whose sample arrays
        (FRAME_BYTES_PER_SAMPLE bytes a sample) fit budget_bytes, at least one tile each."""
        nt = self.num_tiles(tile_size)
        per = max(1, int(budget_bytes) // (FRAME_BYTES_PER_SAMPLE * ns * tile_size * tile_size))
        return [(b, min(b + per, nt), self.frame_count(ns, b, min(b + per, nt), tile_size)) for b in range(0, nt, per)]

    def render_samples(self, spp, max_depth=10, light_strategy=abi.PBRT_LIGHT_STRATEGY_UNIFORM, rr_threshold=1.0,
                       tile_size=16, budget_bytes=1 << 30, film=None, count_rays=False,
                       integrator=abi.PBRT_INTEGRATOR_PATH, dl_strategy=abi.PBRT_DL_UNIFORM_SAMPLE_ALL):
        """A THROUGHPUT frame with n_dims = 0 composed of the public stages: per ascending tile
        range sized to budget_bytes, frame_samples, li_device and film_add, all on the device; the
        film is pbrt_gpu_render's, bit for bit. film: a float64 DeviceBuffer of H * W * 3 to
        compose into (None: one of the call's own). integrator: PBRT_INTEGRATOR_PATH, or
        PBRT_INTEGRATOR_DIRECT_LIGHTING, whose Li stage is direct_li_device with dl_strategy
        (light_strategy and rr_threshold are Path's alone). Returns (the (H, W, 3) film, info):
        info has the ranges, the samples and, with count_rays, the reference's closest and shadow
        ray counts (which downloads 4 bytes per sample). Raises PbrtError on a refusal and
        PBRT_E_REF_PANIC when the reference panics on a path."""
        ns = int(spp) - 1
        if ns < 1:
            raise PbrtError(abi.PBRT_E_INVALID, "render_samples: spp >= 2 (sample 0 of a pixel is never traced)")
        if integrator not in (abi.PBRT_INTEGRATOR_PATH, abi.PBRT_INTEGRATOR_DIRECT_LIGHTING):
            raise PbrtError(abi.PBRT_E_INVALID, f"render_samples: integrator {integrator}")
        direct = integrator == abi.PBRT_INTEGRATOR_DIRECT_LIGHTING
        ranges = self.frame_ranges(ns, tile_size, budget_bytes)
        cap = max(n for _, _, n in ranges)
        own = []
        try:
            if film is None:
                film = self.buffer(self.hgt * self.w * 3)
                own.append(film)
            sb = {k: self.buffer(cap, SAMPLE_DTYPES[k]) for k in SAMPLE_REQUIRED}
            ob = {k: self.buffer(cap) for k in ("r", "g", "b")}
            if count_rays:
                ob["rays"] = self.buffer(cap, np.uint32)
            own += list(sb.values()) + list(ob.values())
            rays = {k: sb[k] for k in RAY_KEYS}
            rng = {k: sb[k] for k in RNG_KEYS}
            fs = dict(pfilm_x=sb["pfilm_x"], pfilm_y=sb["pfilm_y"], r=ob["r"], g=ob["g"], b=ob["b"])
            closest = shadow = 0
            for i, (b, e, n) in enumerate(ranges):
                self._check(self.frame_samples(sb, ns, b, e, tile_size))
                if direct:
                    self._check(self.direct_li_device(rays, rng, n, ob, max_depth, dl_strategy))
                else:
                    self._check(self.li_device(rays, rng, n, ob, max_depth, light_strategy, rr_threshold))
                self._check(self.film_add(fs, ns, film, b, e, tile_size, clear=i == 0))
                if count_rays:
                    v = ob["rays"].download()[:n]
                    closest += int((v & 0xFFFF).sum())
                    shadow += int((v >> 16).sum())
            rc, rec = self.query_status()
            if rc:
                raise PbrtError(rc, self.last_error(), rec)
            out = film.download()[:self.hgt * self.w * 3].reshape(self.hgt, self.w, 3)
        finally:
            for b in own:
                b.close()
        info = {"ranges": len(ranges), "samples": sum(n for _, _, n in ranges)}
        if count_rays:
            info.update(closest_rays=closest, shadow_rays=shadow)
        return out, info

    # ---- the same pieces under sampler.Stratified
    def frame_samples_stratified(self, out, strat, sampler_x, sampler_y, n_dims, jitter=False, tile_begin=0,
                                 tile_end=None, tile_size=16):
        """pbrt_gpu_frame_samples_stratified_device: the traced samples (k = 1 .. spp - 1) of a
        THROUGHPUT render under Stratified(sampler_x, sampler_y, jitter, n_dims), n_dims >= 1, over a
        tile range. out: frame_samples' buffers; strat: k and table (int32 per sample) and s1d
        (float64, n_dims * spp per pixel of the range: the pixels' tables). Enqueue only. Returns
        the status (PBRT_E_UNSUPPORTED: last_error() says why)."""
        unknown = (set(out) - set(SAMPLE_DTYPES)) | (set(strat) - set(STRAT_SAMPLE_KEYS) - {"s1d"})
        missing = [k for k in SAMPLE_REQUIRED if out.get(k) is None] + \
                  [k for k in STRAT_SAMPLE_KEYS + ("s1d",) if strat.get(k) is None]
        if unknown or missing:
            raise PbrtError(abi.PBRT_E_INVALID, f"frame_samples_stratified: unknown {sorted(unknown)}, missing {missing}")
        spp = int(sampler_x) * int(sampler_y)
        d, n = self._frame_desc("frame_samples_stratified", spp - 1, tile_begin, tile_end, tile_size)
        npx = n // (spp - 1) if spp > 1 else 0
        ob = [(k, out[k], dt) for k, dt in SAMPLE_DTYPES.items() if out.get(k) is not None]
        kb = [(k, strat[k], np.int32) for k in STRAT_SAMPLE_KEYS]
        check_buffers(self, n, ob + kb)
        check_buffers(self, npx * max(int(n_dims), 0) * spp, [("s1d", strat["s1d"], np.float64)])
        s = abi.strat_sampler_desc(sampler_x, sampler_y, n_dims, jitter)
        os_, ss = _soa(abi.FrameSamplesSoA, ob), _soa(abi.StratSamplesSoA, kb + [("s1d", strat["s1d"], np.float64)])
        return lib().pbrt_gpu_frame_samples_stratified_device(self.h, C.byref(d), C.byref(s), C.byref(os_), C.byref(ss))

    def li_stratified_device(self, rays, rng, n, out, strat, n_tables, spp, n_dims, first_1d, first_2d, max_depth=10,
                             light_strategy=abi.PBRT_LIGHT_STRATEGY_UNIFORM, rr_threshold=1.0,
                             integrator=abi.PBRT_INTEGRATOR_PATH):
        """pbrt_gpu_li_stratified_device: li_device under the stratified sampler. strat: s1d (float64,
        n_tables tables of n_dims * spp), table and k (int32 per ray); first_1d, first_2d: the
        dimensions the rays' first Get1D / Get2D read. With n_dims = 0 strat may be empty. The other
        arguments, the outputs and the buffer checks are li_device's. Returns the status."""
        rs, gs, os_ = _li_soas(self, "li_stratified_device", rays, rng, n, out)
        unknown = set(strat) - set(STRAT_SAMPLE_KEYS) - {"s1d"}
        if unknown:
            raise PbrtError(abi.PBRT_E_INVALID, f"li_stratified_device: unknown {sorted(unknown)}")
        kb = [(k, strat[k], np.int32) for k in STRAT_SAMPLE_KEYS if strat.get(k) is not None]
        check_buffers(self, n, kb)
        tb = [("s1d", strat["s1d"], np.float64)] if strat.get("s1d") is not None else []
        if min(int(n_tables), int(spp), int(n_dims)) > 0:
            check_buffers(self, int(n_tables) * int(n_dims) * int(spp), tb)
        ss = _soa(abi.StratSoA, kb + tb)
        ss.n_tables, ss.spp, ss.n_dims, ss.first_1d, ss.first_2d = n_tables, spp, n_dims, first_1d, first_2d
        d = abi.li_desc(max_depth, light_strategy, rr_threshold, integrator)
        return lib().pbrt_gpu_li_stratified_device(self.h, C.byref(d), C.byref(rs), C.byref(gs), n, C.byref(os_),
                                                   C.byref(ss))

    def frame_ranges_stratified(self, spp, n_dims, tile_size=16, budget_bytes=1 << 30):
        """frame_ranges for a stratified frame: a pixel takes its spp - 1 samples of
        STRAT_BYTES_PER_SAMPLE bytes and its table of n_dims * spp doubles."""
        nt, ns = self.num_tiles(tile_size), spp - 1
        per_px = STRAT_BYTES_PER_SAMPLE * ns + 8 * n_dims * spp
        per = max(1, int(budget_bytes) // (per_px * tile_size * tile_size))
        return [(b, min(b + per, nt), self.frame_count(ns, b, min(b + per, nt), tile_size)) for b in range(0, nt, per)]

    def render_samples_stratified(self, sampler_x, sampler_y, n_dims, jitter=False, max_depth=10,
                                  light_strategy=abi.PBRT_LIGHT_STRATEGY_UNIFORM, rr_threshold=1.0, tile_size=16,
                                  budget_bytes=1 << 30, film=None, count_rays=False):
        """A THROUGHPUT Path frame under Stratified(sampler_x, sampler_y, jitter, n_dims), n_dims >= 1,
        composed of the public stages: per ascending tile range sized to budget_bytes,
        frame_samples_stratified, li_stratified_device with the cursors after the camera sample, and
        film_add, all on the device; the film is pbrt_gpu_render's, bit for bit. Arguments and the
        returned (film, info) are render_samples'."""
        spp = int(sampler_x) * int(sampler_y)
        ns = spp - 1
        if ns < 1 or n_dims < 1:
            raise PbrtError(abi.PBRT_E_INVALID, "render_samples_stratified: spp >= 2 (sample 0 of a pixel is never "
                                                "traced) and n_dims >= 1 (n_dims = 0 is render_samples)")
        ranges = self.frame_ranges_stratified(spp, n_dims, tile_size, budget_bytes)
        cap = max(n for _, _, n in ranges)
        c1, c2 = abi.camera_cursors(n_dims)
        own = []
        try:
            if film is None:
                film = self.buffer(self.hgt * self.w * 3)
                own.append(film)
            sb = {k: self.buffer(cap, SAMPLE_DTYPES[k]) for k in SAMPLE_REQUIRED}
            ob = {k: self.buffer(cap) for k in ("r", "g", "b")}
            if count_rays:
                ob["rays"] = self.buffer(cap, np.uint32)
            kb = {k: self.buffer(cap, np.int32) for k in STRAT_SAMPLE_KEYS}
            kb["s1d"] = self.buffer((cap // ns) * n_dims * spp)
            own += list(sb.values()) + list(ob.values()) + list(kb.values())
            rays = {k: sb[k] for k in RAY_KEYS}
            rng = {k: sb[k] for k in RNG_KEYS}
            fs = dict(pfilm_x=sb["pfilm_x"], pfilm_y=sb["pfilm_y"], r=ob["r"], g=ob["g"], b=ob["b"])
            closest = shadow = 0
            for i, (b, e, n) in enumerate(ranges):
                self._check(self.frame_samples_stratified(sb, kb, sampler_x, sampler_y, n_dims, jitter, b, e, tile_size))
                self._check(self.li_stratified_device(rays, rng, n, ob, kb, n // ns, spp, n_dims, c1, c2, max_depth,
                                                      light_strategy, rr_threshold))
                self._check(self.film_add(fs, ns, film, b, e, tile_size, clear=i == 0))
                if count_rays:
                    v = ob["rays"].download()[:n]
                    closest += int((v & 0xFFFF).sum())
                    shadow += int((v >> 16).sum())
            rc, rec = self.query_status()
            if rc:
                raise PbrtError(rc, self.last_error(), rec)
            out = film.download()[:self.hgt * self.w * 3].reshape(self.hgt, self.w, 3)
        finally:
            for b in own:
                b.close()
        info = {"ranges": len(ranges), "samples": sum(n for _, _, n in ranges)}
        if count_rays:
            info.update(closest_rays=closest, shadow_rays=shadow)
        return out, info

    def radiance_stratified(self, rays, state, inc, s1d, table, k, first_1d, first_2d, **desc):
        """Path.Li of host rays under the stratified sampler, in the shape of radiance: s1d is
        (n_tables, n_dims, spp) float64, table and k the table and sample index of each ray (int32),
        first_1d / first_2d the starting cursors; desc is li_device's. Returns (L (n, 3), state,
        draws, rays)."""
        s1d = np.ascontiguousarray(s1d, dtype=np.float64)
        if s1d.ndim != 3 or len(table) != len(state) or len(k) != len(state):
            raise PbrtError(abi.PBRT_E_INVALID, "radiance_stratified: s1d (n_tables, n_dims, spp), table and k of n elements")
        n_tables, n_dims, spp = s1d.shape
        bufs = []

        def query(rb, gb, n, ob, **dd):
            st = {}
            if s1d.size:
                st = dict(s1d=self.upload(s1d.reshape(-1)), table=self.upload(np.asarray(table, dtype=np.int32)),
                          k=self.upload(np.asarray(k, dtype=np.int32)))
                bufs.extend(st.values())
            return self.li_stratified_device(rb, gb, n, ob, st, n_tables, spp, n_dims, first_1d, first_2d, **dd)
        try:
            return self._host_radiance("radiance_stratified", query, rays, state, inc, desc)
        finally:
            for b in bufs:
                b.close()

    def radiance(self, rays, state, inc, **desc):
        """Path.Li of host rays: rays is (n, 6) [ox, oy, oz, dx, dy, dz] or (n, 7) with tmax,
        state and inc the PCG32 stream of each ray (uint64). Uploads, queries and downloads;
        desc is li_device's (max_depth, light_strategy, rr_threshold). Returns (L (n, 3),
        state, draws, rays); raises PbrtError on a refusal and PBRT_E_REF_PANIC when the
        reference panics on a ray (its stats field is the QueryRecord)."""
        return self._host_radiance("radiance", self.li_device, rays, state, inc, desc)

    def direct_radiance(self, rays, state, inc, **desc):
        """DirectLighting.Li of host rays, in the shape of radiance: desc is direct_li_device's
        (max_depth, dl_strategy). Returns (L (n, 3), state, draws, rays)."""
        return self._host_radiance("direct_radiance", self.direct_li_device, rays, state, inc, desc)

    def _host_radiance(self, what, query, rays, state, inc, desc):
        rays = np.ascontiguousarray(rays, dtype=np.float64)
        n = rays.shape[0]
        if rays.ndim != 2 or rays.shape[1] not in (6, 7) or len(state) != n or len(inc) != n:
            raise PbrtError(abi.PBRT_E_INVALID, f"{what}: rays (n, 6) or (n, 7), state and inc of n elements")
        if n == 0:
            return np.zeros((0, 3)), np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        bufs = []
        try:
            rb = [self.upload(rays[:, k]) for k in range(rays.shape[1])]
            gb = [self.upload(np.asarray(a, dtype=np.uint64)) for a in (state, inc)]
            ob = {k: self.buffer(n, dt) for k, dt in LI_DTYPES.items()}
            bufs = rb + gb + list(ob.values())
            self._check(query(tuple(rb), tuple(gb), n, ob, **desc))
            rc, rec = self.query_status()
            if rc:
                raise PbrtError(rc, self.last_error(), rec)
            got = {k: b.download() for k, b in ob.items()}
        finally:
            for b in bufs:
                b.close()
        return np.stack([got["r"], got["g"], got["b"]], axis=1), got["state"], got["draws"], got["rays"]

    def query_status(self):
        """(status, QueryRecord) of the queries since the last call: synchronises
        the stream; PBRT_E_REF_PANIC when the reference panics on some ray."""
        rec = abi.QueryRecord()
        rc = lib().pbrt_gpu_query_status(self.h, C.byref(rec))
        return rc, rec

    def primary_hits(self, window=None, **offsets):
        """Primary visibility of a pixel window: camera rays chained into a
        closest-hit query on the context's stream, with no host step or copy.
        Returns {"n", "rays": {...}, "hits": {...}} of DeviceBuffers, allocated
        once per window size and reused (so valid until the next call of that
        size); offsets are camera_rays' film_offset, lens and time_u."""
        x0, y0, x1, y1 = (0, 0) + self.res if window is None else (int(v) for v in window)
        n = (x1 - x0) * (y1 - y0)
        bufs = self._primary.get((x1 - x0, y1 - y0))
        if bufs is None or any(b.closed for part in bufs for b in part.values()):
            if n <= 0:
                raise PbrtError(abi.PBRT_E_INVALID, f"empty window {(x0, y0, x1, y1)}")
            bufs = ({k: self.buffer(n) for k in RAY_KEYS + ("tmax",)},
                    {k: self.buffer(n, dt) for k, dt in HIT_DTYPES.items()})
            self._primary[(x1 - x0, y1 - y0)] = bufs
        rays, hits = bufs
        self.camera_rays((x0, y0, x1, y1), out=rays, **offsets)
        self._check(self.intersect_device(rays, n, hits))
        return {"n": n, "rays": dict(rays), "hits": dict(hits)}

    def close(self):
        if getattr(self, "_token", None) is not None:
            self._token.alive = False   # every DeviceBuffer of this context is closed from here on
            self._primary = {}
        if getattr(self, "h", None):
            lib().pbrt_gpu_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        self.close()


class RendererGroup:
    """pbrt_gpu_group: the scene resident on several GPUs, rendered as one frame.

    devices: 1..8 HIP ordinals (one member each; an ordinal may repeat, which
    runs the whole mechanism on one GPU). The film is merged on devices[0] in
    tile-index order and is bit-identical to a single Renderer's."""

    def __init__(self, scene, devices, lanes_per_wave=0, occupancy=0, kernel="auto"):
        desc = scene.desc if isinstance(scene, Scene) else scene
        self._scene = scene  # keep the descriptor alive
        opts = abi.GpuOpts()
        opts.device, opts.lanes_per_wave = -1, lanes_per_wave
        opts.occupancy, opts.kernel = occupancy, Renderer.KERNELS[kernel]
        devices = list(devices)
        devs = (C.c_int32 * max(len(devices), 1))(*devices)
        h = C.c_void_p()
        rc = lib().pbrt_gpu_group_create(C.byref(desc), C.byref(opts), devs, len(devices), C.byref(h))
        if rc:
            raise PbrtError(rc, _create_failed("pbrt_gpu_group_create") if rc == abi.PBRT_E_HIP
                            else "pbrt_gpu_group_create failed (bad device list, scene descriptor or options)")
        self.h = h.value
        self.devices = devices
        self.w = desc.film.crop_max_x - desc.film.crop_min_x
        self.hgt = desc.film.crop_max_y - desc.film.crop_min_y

    def _check(self, rc, stats=None):
        if rc:
            raise PbrtError(rc, lib().pbrt_gpu_group_last_error(self.h).decode(), stats)

    def __len__(self):
        return lib().pbrt_gpu_group_size(self.h)

    def render(self, rd):
        film = np.zeros((self.hgt, self.w, 3), dtype=np.float64)
        st = abi.GpuStats()
        rc = lib().pbrt_gpu_group_render(self.h, C.byref(rd), film.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st))
        self._check(rc, st)
        return film, st

    def render_async(self, rd, film_device_ptr=None):
        """Start a frame; film_device_ptr = caller buffer on devices[0] (e.g. tensor.data_ptr())."""
        self._check(lib().pbrt_gpu_group_render_async(self.h, C.byref(rd),
                                                      C.c_void_p(film_device_ptr) if film_device_ptr else None))

    def synchronize(self):
        st = abi.GpuStats()
        self._check(lib().pbrt_gpu_group_synchronize(self.h, C.byref(st)), st)
        return st

    def film(self):
        film = np.zeros((self.hgt, self.w, 3), dtype=np.float64)
        self._check(lib().pbrt_gpu_group_film_download(self.h, film.ctypes.data_as(C.POINTER(C.c_double))))
        return film

    def film_device_ptr(self):
        return lib().pbrt_gpu_group_film_device(self.h)

    def member_stats(self, i):
        st = abi.GpuStats()
        self._check(lib().pbrt_gpu_group_member_stats(self.h, i, C.byref(st)))
        return st

    def member_schedule_source(self, i):
        """PBRT_SCHED_* of member i's last EXACT frame (pbrt_gpu_schedule_source)."""
        return lib().pbrt_gpu_schedule_source(lib().pbrt_gpu_group_member(self.h, i))

    def member_launches(self, i, outside=False):
        """Member i's launch log (Renderer.launches). The group's own k_merge_film_group
        launch belongs to no member context and is not in it."""
        return _launch_log(lib().pbrt_gpu_group_member(self.h, i), outside)[0]

    def cancel(self):
        """Cancel the frame in flight on every member (thread-safe)."""
        lib().pbrt_gpu_group_cancel(self.h)

    def close(self):
        if getattr(self, "h", None):
            lib().pbrt_gpu_group_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        self.close()


def schedule_cache_clear():
    """Empty the process-wide schedule cache (pbrt_gpu_schedule_cache_clear)."""
    lib().pbrt_gpu_schedule_cache_clear()


def film_to_rgba8(film):
    """film.go:142-179 WriteImage pixel conversion (no XYZ->RGB, no gamma)."""
    film = np.ascontiguousarray(film, dtype=np.float64)
    h, w, _ = film.shape
    out = np.zeros((h, w, 4), np.uint8)
    rc = lib().pbrt_film_to_rgba8(film.ctypes.data_as(C.POINTER(C.c_double)), w, h,
                                  out.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc:
        raise PbrtError(rc, "film_to_rgba8")
    return out


def write_png(path, film):
    """Film.WriteImage (film.go:142-179): the fp64 XYZ film as an 8-bit PNG.

    Pixels are pbrt_film_to_rgba8's (uint8(Clamp(v, 0, 1) * 255) per channel,
    no XYZ->RGB, no gamma, alpha 255). Every pixel is opaque, so the image is
    written as 8-bit truecolour without alpha, the colour type Go's png.Encode
    picks for an opaque NRGBA image; scanlines use filter 0 (Go picks filters
    adaptively, so the file bytes differ while the decoded pixels are the same)."""
    rgba = film_to_rgba8(film)
    h, w, _ = rgba.shape
    raw = np.zeros((h, 1 + 3 * w), np.uint8)
    raw[:, 1:] = rgba[:, :, :3].reshape(h, 3 * w)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
           + chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(png)
    return rgba


def read_png_rgb(path):
    """Decode an 8-bit truecolour PNG with filter-0 scanlines (write_png's) -> (h, w, 3) uint8."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            w, h = struct.unpack(">II", body[:8])
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3)

"""ctypes mirrors of include/pbrt_gpu.h (the C ABI of the device path).

These structures are plain data layouts; they carry no behaviour. Field order
and types must match include/pbrt_gpu.h exactly (checked by
tests/test_abi.py against the sizes the library reports).
"""
import ctypes as C

PBRT_OK = 0
PBRT_E_INVALID = 1
PBRT_E_HIP = 2
PBRT_E_RCCL = 3
PBRT_E_CANCELLED = 4
PBRT_E_REF_PANIC = 5
PBRT_E_UNSUPPORTED = 6

PBRT_SHAPE_SPHERE = 1
PBRT_SHAPE_DISK = 2
PBRT_TEX_CONSTANT = 1
PBRT_TEX_CHECKERBOARD2D = 2
PBRT_MAT_MATTE, PBRT_MAT_MIRROR, PBRT_MAT_GLASS = 0, 1, 2
PBRT_PRIM_GEOMETRIC = 1
PBRT_PRIM_TRANSFORMED = 2
PBRT_LIGHT_POINT = 1
PBRT_LIGHT_DISTANT = 2
PBRT_LIGHT_DIFFUSE_AREA = 3
PBRT_INTEGRATOR_PATH = 1
PBRT_INTEGRATOR_DIRECT_LIGHTING = 2
PBRT_LIGHT_STRATEGY_UNIFORM = 1
PBRT_LIGHT_STRATEGY_POWER = 2
PBRT_DL_UNIFORM_SAMPLE_ALL = 1
PBRT_DL_UNIFORM_SAMPLE_ONE = 2
PBRT_MODE_EXACT = 0
PBRT_MODE_THROUGHPUT = 1
PBRT_KERNEL_AUTO = 0
PBRT_KERNEL_SERIAL = 1
PBRT_KERNEL_WAVE = 2
PBRT_KERNEL_WAVEFRONT = 3
PBRT_KERNEL_WAVE_CI = 4
PBRT_KERNEL_WAVE_DL = 5
PBRT_KERNEL_WAVE_CAM = 6
PBRT_FLAG_SERIAL_START_PIXEL = 1
PBRT_FLAG_PANIC_FIDELITY = 2

PBRT_PANIC_NONE = 0
PBRT_PANIC_LD_GT_10 = 1
PBRT_PANIC_EFLOAT = 2
PBRT_PANIC_BVH_STACK = 3
PBRT_PANIC_NIL_DEREF = 4

PBRT_MAX_DIST = 64


class Matrix4x4(C.Structure):
    _fields_ = [("m", (C.c_double * 4) * 4)]


class Transform(C.Structure):
    _fields_ = [("m", Matrix4x4), ("m_inv", Matrix4x4)]


class ShapeDesc(C.Structure):
    _fields_ = [
        ("type", C.c_int32),
        ("reverse_orientation", C.c_int32),
        ("transform_swaps_handedness", C.c_int32),
        ("pad0", C.c_int32),
        ("object_to_world", Transform),
        ("radius", C.c_double),
        ("z_min", C.c_double),
        ("z_max", C.c_double),
        ("theta_min", C.c_double),
        ("theta_max", C.c_double),
        ("phi_max", C.c_double),
        ("height", C.c_double),
        ("inner_radius", C.c_double),
    ]


class MaterialDesc(C.Structure):
    _fields_ = [
        ("kd_type", C.c_int32),
        ("type", C.c_int32),
        ("kd", C.c_double * 3),
        ("vs", C.c_double * 3),
        ("vt", C.c_double * 3),
        ("ds", C.c_double),
        ("dt", C.c_double),
        ("tex1", C.c_double * 3),
        ("tex2", C.c_double * 3),
        ("sigma", C.c_double),
        ("kr", C.c_double * 3),
        ("kt", C.c_double * 3),
        ("eta", C.c_double),
        ("u_roughness", C.c_double),
        ("v_roughness", C.c_double),
    ]


class PrimitiveDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("shape", C.c_int32),
        ("material", C.c_int32),
        ("pad0", C.c_int32),
        ("prim_to_world", Transform),
    ]


class BVHNode(C.Structure):
    _fields_ = [
        ("bmin", C.c_double * 3),
        ("bmax", C.c_double * 3),
        ("offset", C.c_uint32),
        ("n_prims", C.c_uint16),
        ("axis", C.c_uint8),
        ("pad0", C.c_uint8),
    ]


class LightDesc(C.Structure):
    _fields_ = [
        ("type", C.c_int32),
        ("shape", C.c_int32),
        ("two_sided", C.c_int32),
        ("pad0", C.c_int32),
        ("spectrum", C.c_double * 3),
        ("p_light", C.c_double * 3),
        ("w_light", C.c_double * 3),
        ("world_radius", C.c_double),
    ]


class CameraDesc(C.Structure):
    _fields_ = [
        ("camera_to_world", Transform),
        ("raster_to_camera", Transform),
        ("lens_radius", C.c_double),
        ("focal_distance", C.c_double),
        ("shutter_open", C.c_double),
        ("shutter_close", C.c_double),
    ]


class FilmDesc(C.Structure):
    _fields_ = [
        ("res_x", C.c_int64),
        ("res_y", C.c_int64),
        ("crop_min_x", C.c_int64),
        ("crop_min_y", C.c_int64),
        ("crop_max_x", C.c_int64),
        ("crop_max_y", C.c_int64),
        ("filter_radius_x", C.c_double),
        ("filter_radius_y", C.c_double),
        ("max_sample_luminance", C.c_double),
        ("filter_table", C.c_double * 256),
    ]


class DistributionDesc(C.Structure):
    _fields_ = [
        ("count", C.c_int32),
        ("pad0", C.c_int32),
        ("func_int", C.c_double),
        ("func", C.c_double * PBRT_MAX_DIST),
        ("cdf", C.c_double * (PBRT_MAX_DIST + 1)),
    ]


class MeshDesc(C.Structure):
    """pbrt_mesh_desc: extension (configs D/E), include/pbrt_gpu.h."""
    _fields_ = [
        ("n_vertices", C.c_int32),
        ("n_triangles", C.c_int32),
        ("material", C.c_int32),
        ("reverse_orientation", C.c_int32),
        ("p", C.POINTER(C.c_float)),
        ("indices", C.POINTER(C.c_int32)),
    ]


class SceneDesc(C.Structure):
    _fields_ = [
        ("n_shapes", C.c_int32),
        ("n_materials", C.c_int32),
        ("n_prims", C.c_int32),
        ("n_nodes", C.c_int32),
        ("n_lights", C.c_int32),
        ("pad0", C.c_int32),
        ("shapes", C.POINTER(ShapeDesc)),
        ("materials", C.POINTER(MaterialDesc)),
        ("prims", C.POINTER(PrimitiveDesc)),
        ("nodes", C.POINTER(BVHNode)),
        ("lights", C.POINTER(LightDesc)),
        ("camera", CameraDesc),
        ("film", FilmDesc),
        ("world_min", C.c_double * 3),
        ("world_max", C.c_double * 3),
        ("n_meshes", C.c_int32),
        ("pad1", C.c_int32),
        ("meshes", C.POINTER(MeshDesc)),
    ]


class RenderDesc(C.Structure):
    _fields_ = [
        ("sampler_x", C.c_int32),
        ("sampler_y", C.c_int32),
        ("jitter", C.c_int32),
        ("n_dims", C.c_int32),
        ("integrator", C.c_int32),
        ("max_depth", C.c_int32),
        ("light_strategy", C.c_int32),
        ("dl_strategy", C.c_int32),
        ("rr_threshold", C.c_double),
        ("tile_size", C.c_int64),
        ("tile_begin", C.c_int64),
        ("tile_end", C.c_int64),
        ("tile_stride", C.c_int64),
        ("mode", C.c_int32),
        ("flags", C.c_int32),
    ]


class GpuStats(C.Structure):
    _fields_ = [
        ("tiles_rendered", C.c_uint64),
        ("camera_samples", C.c_uint64),
        ("paths_traced", C.c_uint64),
        ("kernel_ms", C.c_double),
        ("merge_ms", C.c_double),
        ("total_ms", C.c_double),
        ("panic_kind", C.c_int32),
        ("panic_tile", C.c_int32),
        ("panic_pixel_x", C.c_int64),
        ("panic_pixel_y", C.c_int64),
        ("panic_sample", C.c_int32),
        ("panic_bounce", C.c_int32),
        ("kernel", C.c_int32),
        ("batches", C.c_int32),
        ("chain_ms", C.c_double),
        ("paths_ms", C.c_double),
        ("rays_closest", C.c_uint64),
        ("rays_shadow", C.c_uint64),
    ]


class RaySoA(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_double)) for n in ("ox", "oy", "oz", "dx", "dy", "dz", "tmax")]


class HitSoA(C.Structure):
    _fields_ = [
        ("hit", C.POINTER(C.c_uint8)),
        ("t_max", C.POINTER(C.c_double)),
        ("prim", C.POINTER(C.c_int32)),
        ("px", C.POINTER(C.c_double)),
        ("py", C.POINTER(C.c_double)),
        ("pz", C.POINTER(C.c_double)),
        ("nx", C.POINTER(C.c_double)),
        ("ny", C.POINTER(C.c_double)),
        ("nz", C.POINTER(C.c_double)),
    ]


class GpuOpts(C.Structure):
    _fields_ = [("device", C.c_int32), ("lanes_per_wave", C.c_int32), ("occupancy", C.c_int32),
                ("kernel", C.c_int32), ("reserved", C.c_int32 * 4)]


def render_desc(spp_x=8, spp_y=8, jitter=False, n_dims=4, integrator=PBRT_INTEGRATOR_PATH,
                max_depth=10, rr_threshold=1.0, light_strategy=PBRT_LIGHT_STRATEGY_UNIFORM,
                dl_strategy=PBRT_DL_UNIFORM_SAMPLE_ALL, tile_size=16, tile_begin=0, tile_end=0,
                tile_stride=1, mode=PBRT_MODE_EXACT, flags=0):
    """RenderDesc with the defaults of internal/render/server.go:142,162,164."""
    rd = RenderDesc()
    rd.sampler_x, rd.sampler_y, rd.jitter, rd.n_dims = spp_x, spp_y, int(bool(jitter)), n_dims
    rd.integrator, rd.max_depth = integrator, max_depth
    rd.light_strategy, rd.dl_strategy = light_strategy, dl_strategy
    rd.rr_threshold = rr_threshold
    rd.tile_size, rd.tile_begin, rd.tile_end, rd.tile_stride = tile_size, tile_begin, tile_end, tile_stride
    rd.mode, rd.flags = mode, flags
    return rd


PBRT_LAUNCHES_FRAME, PBRT_LAUNCHES_OUTSIDE = 0, 1


class LaunchRec(C.Structure):
    """pbrt_launch_rec (include/pbrt_diag.h): one kernel launch of a context."""
    _fields_ = [
        ("name", C.c_char_p),
        ("fn", C.c_void_p),
        ("grid", C.c_uint32 * 3),
        ("block", C.c_uint32 * 3),
        ("lds_dynamic", C.c_uint32),
        ("lds_static", C.c_uint32),
        ("stream", C.c_int32),
        ("pad0", C.c_int32),
    ]


def declare_launch_log(L):
    """ctypes prototypes of the launch log (include/pbrt_diag.h)."""
    L.pbrt_gpu_launch_log.argtypes = [C.c_void_p, C.c_int, C.POINTER(LaunchRec), C.c_int64, C.POINTER(C.c_uint64)]
    L.pbrt_gpu_launch_log.restype = C.c_int64
    L.pbrt_gpu_kernel_names.argtypes = [C.POINTER(C.c_char_p), C.c_int]
    L.pbrt_gpu_lds_per_block.argtypes = [C.c_void_p]
    L.pbrt_gpu_lds_per_block.restype = C.c_int64


def declare_kernel_choice(L):
    """ctypes prototype of pbrt_diag_kernel_choice (include/pbrt_diag.h). Apart from the other
    prototypes: a library of an earlier build (PBRT_GPU_LIB) loads without this entry."""
    L.pbrt_diag_kernel_choice.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_int]
    L.pbrt_diag_kernel_choice.restype = C.c_char_p


PBRT_GROUP_MAX = 8


def declare_group(L):
    """ctypes prototypes of the device-group entry points (pbrt_gpu_group_*)."""
    P, vp = C.POINTER, C.c_void_p
    L.pbrt_gpu_group_create.argtypes = [P(SceneDesc), P(GpuOpts), P(C.c_int32), C.c_int32, P(vp)]
    L.pbrt_gpu_group_render.argtypes = [vp, P(RenderDesc), P(C.c_double), P(GpuStats)]
    L.pbrt_gpu_group_render_async.argtypes = [vp, P(RenderDesc), vp]
    L.pbrt_gpu_group_synchronize.argtypes = [vp, P(GpuStats)]
    L.pbrt_gpu_group_film_device.argtypes = [vp]
    L.pbrt_gpu_group_film_device.restype = vp
    L.pbrt_gpu_group_film_download.argtypes = [vp, P(C.c_double)]
    L.pbrt_gpu_group_size.argtypes = [vp]
    L.pbrt_gpu_group_member.argtypes = [vp, C.c_int]
    L.pbrt_gpu_group_member.restype = vp
    L.pbrt_gpu_group_member_stats.argtypes = [vp, C.c_int, P(GpuStats)]
    L.pbrt_gpu_group_cancel.argtypes = [vp]
    L.pbrt_gpu_group_cancel.restype = None
    L.pbrt_gpu_group_last_error.argtypes = [vp]
    L.pbrt_gpu_group_last_error.restype = C.c_char_p
    L.pbrt_gpu_group_destroy.argtypes = [vp]
    L.pbrt_gpu_group_destroy.restype = None


# ------------------------------------------------------- device-resident queries
class RaySoAOut(C.Structure):
    """pbrt_ray_soa_out: device arrays pbrt_gpu_camera_rays_device writes."""
    _fields_ = [(n, C.POINTER(C.c_double)) for n in ("ox", "oy", "oz", "dx", "dy", "dz", "tmax")]


class CameraRaysDesc(C.Structure):
    _fields_ = [
        ("x0", C.c_int64),
        ("y0", C.c_int64),
        ("x1", C.c_int64),
        ("y1", C.c_int64),
        ("film_dx", C.c_double),
        ("film_dy", C.c_double),
        ("lens_u", C.c_double),
        ("lens_v", C.c_double),
        ("time_u", C.c_double),
    ]


class QueryRecord(C.Structure):
    _fields_ = [("panics", C.c_uint64), ("first_ray", C.c_int64), ("panic_kind", C.c_int32), ("pad0", C.c_int32)]


QUERY_SYMBOLS = ("pbrt_gpu_buffer_create", "pbrt_gpu_buffer_ptr", "pbrt_gpu_buffer_size", "pbrt_gpu_buffer_upload",
                 "pbrt_gpu_buffer_download", "pbrt_gpu_buffer_destroy", "pbrt_gpu_intersect_device",
                 "pbrt_gpu_intersect_p_device", "pbrt_gpu_camera_rays_device", "pbrt_gpu_query_status")


def declare_query(L):
    """ctypes prototypes of the buffer and device-query entry points."""
    P, vp, sz = C.POINTER, C.c_void_p, C.c_size_t
    L.pbrt_gpu_buffer_create.argtypes = [vp, sz, P(vp)]
    L.pbrt_gpu_buffer_ptr.argtypes = [vp]
    L.pbrt_gpu_buffer_ptr.restype = vp
    L.pbrt_gpu_buffer_size.argtypes = [vp]
    L.pbrt_gpu_buffer_size.restype = sz
    L.pbrt_gpu_buffer_upload.argtypes = [vp, sz, vp, sz]
    L.pbrt_gpu_buffer_download.argtypes = [vp, sz, vp, sz]
    L.pbrt_gpu_buffer_destroy.argtypes = [vp]
    L.pbrt_gpu_buffer_destroy.restype = None
    L.pbrt_gpu_intersect_device.argtypes = [vp, P(RaySoA), sz, P(HitSoA)]
    L.pbrt_gpu_intersect_p_device.argtypes = [vp, P(RaySoA), sz, vp]
    L.pbrt_diag_intersect_staged_device.argtypes = [vp, P(RaySoA), sz, P(HitSoA)]   # include/pbrt_diag.h
    L.pbrt_diag_intersect_p_staged_device.argtypes = [vp, P(RaySoA), sz, vp]
    L.pbrt_gpu_cull_groups.argtypes = [vp]
    L.pbrt_gpu_camera_rays_device.argtypes = [vp, P(CameraRaysDesc), P(RaySoAOut)]
    L.pbrt_gpu_query_status.argtypes = [vp, P(QueryRecord)]


# ------------------------------------------------- batched Integrator.Li queries
class LiDesc(C.Structure):
    """pbrt_li_desc: what pbrt_gpu_li_device needs of a render desc."""
    _fields_ = [("integrator", C.c_int32), ("max_depth", C.c_int32), ("light_strategy", C.c_int32),
                ("reserved", C.c_int32), ("rr_threshold", C.c_double)]


class RngSoA(C.Structure):
    """pbrt_rng_soa: PCG32 state and increment per ray (device arrays)."""
    _fields_ = [("state", C.POINTER(C.c_uint64)), ("inc", C.POINTER(C.c_uint64))]


class RadianceSoA(C.Structure):
    """pbrt_radiance_soa: r, g, b are required; state, draws and rays may be NULL."""
    _fields_ = [("r", C.POINTER(C.c_double)), ("g", C.POINTER(C.c_double)), ("b", C.POINTER(C.c_double)),
                ("state", C.POINTER(C.c_uint64)), ("draws", C.POINTER(C.c_uint32)), ("rays", C.POINTER(C.c_uint32))]


LI_SYMBOLS = ("pbrt_gpu_li_device",)


def li_desc(max_depth=10, light_strategy=PBRT_LIGHT_STRATEGY_UNIFORM, rr_threshold=1.0,
            integrator=PBRT_INTEGRATOR_PATH, reserved=0):
    """LiDesc with render_desc's defaults."""
    return LiDesc(integrator, max_depth, light_strategy, reserved, rr_threshold)


def declare_li(L):
    """ctypes prototype of pbrt_gpu_li_device. Apart from declare_query: a library of an
    earlier build (PBRT_GPU_LIB) loads without this entry."""
    P, vp = C.POINTER, C.c_void_p
    L.pbrt_gpu_li_device.argtypes = [vp, P(LiDesc), P(RaySoA), P(RngSoA), C.c_size_t, P(RadianceSoA)]


# --------------------------------- Path.Li one bounce at a time (include/pbrt_gpu.h)
PBRT_PATH_UNUSED, PBRT_PATH_ALIVE, PBRT_PATH_ENDED, PBRT_PATH_PANICKED = 0, 1, 2, 3


class PathSoA(C.Structure):
    """pbrt_path_soa: the loop-carried state of Path.Li per path (device arrays; tmax may be NULL).
    141 bytes a path, 133 without tmax."""
    _fields_ = ([(n, C.POINTER(C.c_double)) for n in ("ox", "oy", "oz", "dx", "dy", "dz", "tmax", "lr", "lg", "lb",
                                                      "br", "bg", "bb", "eta_scale")] +
                [("state", C.POINTER(C.c_uint64)), ("inc", C.POINTER(C.c_uint64)), ("draws", C.POINTER(C.c_uint32)),
                 ("rays", C.POINTER(C.c_uint32)), ("bounces", C.POINTER(C.c_int32)), ("status", C.POINTER(C.c_uint8))])


class PathQueue(C.Structure):
    """pbrt_path_queue: n path indices and their count, both on the device."""
    _fields_ = [("index", C.POINTER(C.c_int32)), ("count", C.POINTER(C.c_uint32))]


class PathStepSoA(C.Structure):
    """pbrt_path_step_soa: what one step surfaces (every pointer optional)."""
    _fields_ = [("hit", HitSoA), ("material", C.POINTER(C.c_int32)), ("ar", C.POINTER(C.c_double)),
                ("ag", C.POINTER(C.c_double)), ("ab", C.POINTER(C.c_double))]


PATH_SYMBOLS = ("pbrt_gpu_path_begin_device", "pbrt_gpu_path_step_device")


def declare_path(L):
    """ctypes prototypes of pbrt_gpu_path_begin_device and pbrt_gpu_path_step_device (apart, like declare_li)."""
    P, vp = C.POINTER, C.c_void_p
    L.pbrt_gpu_path_begin_device.argtypes = [vp, P(RaySoA), P(RngSoA), C.c_size_t, P(PathSoA)]
    L.pbrt_gpu_path_step_device.argtypes = [vp, P(LiDesc), P(PathSoA), P(PathQueue), P(PathQueue), C.c_size_t,
                                            P(PathStepSoA)]


class DirectLiDesc(C.Structure):
    """pbrt_direct_li_desc: what pbrt_gpu_direct_li_device needs of a DirectLighting render desc."""
    _fields_ = [("max_depth", C.c_int32), ("dl_strategy", C.c_int32), ("reserved", C.c_int32 * 2)]


DIRECT_LI_SYMBOLS = ("pbrt_gpu_direct_li_device", "pbrt_gpu_direct_li_scratch_bytes")


def direct_li_desc(max_depth=5, dl_strategy=PBRT_DL_UNIFORM_SAMPLE_ALL, reserved=(0, 0)):
    """DirectLiDesc with render_desc's strategy and the DirectLighting integrator's default depth."""
    return DirectLiDesc(max_depth, dl_strategy, (C.c_int32 * 2)(*reserved))


def declare_direct_li(L):
    """ctypes prototypes of pbrt_gpu_direct_li_device and its diagnostic (apart, like declare_li)."""
    P, vp = C.POINTER, C.c_void_p
    L.pbrt_gpu_direct_li_device.argtypes = [vp, P(DirectLiDesc), P(RaySoA), P(RngSoA), C.c_size_t, P(RadianceSoA)]
    L.pbrt_gpu_direct_li_scratch_bytes.argtypes = [vp]
    L.pbrt_gpu_direct_li_scratch_bytes.restype = C.c_size_t


# --------------------------------- a frame from public pieces (include/pbrt_gpu.h)
PBRT_FILM_ADD_CLEAR = 1


class FrameDesc(C.Structure):
    """pbrt_frame_desc: a tile range of the frame layout."""
    _fields_ = [("tile_size", C.c_int32), ("ns", C.c_int32), ("tile_begin", C.c_int64), ("tile_end", C.c_int64),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class FrameSamplesSoA(C.Structure):
    """pbrt_frame_samples_soa: what pbrt_gpu_frame_samples_device writes; tmax, px, py may be NULL."""
    _fields_ = ([(n, C.POINTER(C.c_double)) for n in ("ox", "oy", "oz", "dx", "dy", "dz", "tmax", "pfilm_x", "pfilm_y")]
                + [("state", C.POINTER(C.c_uint64)), ("inc", C.POINTER(C.c_uint64)),
                   ("px", C.POINTER(C.c_int32)), ("py", C.POINTER(C.c_int32))])


class FilmSamplesSoA(C.Structure):
    """pbrt_film_samples_soa: what pbrt_gpu_film_add_device reads."""
    _fields_ = [(n, C.POINTER(C.c_double)) for n in ("pfilm_x", "pfilm_y", "r", "g", "b")]


FRAME_SYMBOLS = ("pbrt_gpu_frame_count", "pbrt_gpu_frame_samples_device", "pbrt_gpu_film_add_device",
                 "pbrt_gpu_film_rgba8_device", "pbrt_gpu_film_scratch_bytes")


def frame_desc(tile_size, ns, tile_begin, tile_end, flags=0, reserved=0):
    return FrameDesc(tile_size, ns, tile_begin, tile_end, flags, reserved)


def declare_frame(L):
    """ctypes prototypes of the frame calls (apart, like declare_li: an earlier build has none)."""
    P, vp = C.POINTER, C.c_void_p
    L.pbrt_gpu_frame_count.argtypes = [vp, P(FrameDesc)]
    L.pbrt_gpu_frame_count.restype = C.c_int64
    L.pbrt_gpu_frame_samples_device.argtypes = [vp, P(FrameDesc), P(FrameSamplesSoA)]
    L.pbrt_gpu_film_add_device.argtypes = [vp, P(FrameDesc), P(FilmSamplesSoA), vp]
    L.pbrt_gpu_film_rgba8_device.argtypes = [vp, vp, C.c_int64, C.c_int64, vp]
    L.pbrt_gpu_film_scratch_bytes.argtypes = [vp]
    L.pbrt_gpu_film_scratch_bytes.restype = C.c_size_t


# ------------------- the same pieces under sampler.Stratified (include/pbrt_gpu.h)
class StratSamplerDesc(C.Structure):
    """pbrt_strat_sampler_desc: sampler.NewStratified(sampler_x, sampler_y, jitter, n_dims)."""
    _fields_ = [("sampler_x", C.c_int32), ("sampler_y", C.c_int32), ("n_dims", C.c_int32), ("jitter", C.c_int32),
                ("reserved", C.c_int32)]


class StratSamplesSoA(C.Structure):
    """pbrt_strat_samples_soa: k and table per sample, s1d per pixel of the range (all required)."""
    _fields_ = [("k", C.POINTER(C.c_int32)), ("table", C.POINTER(C.c_int32)), ("s1d", C.POINTER(C.c_double))]


class StratSoA(C.Structure):
    """pbrt_strat_soa: the tables, the per-ray table and sample indices and the per-call cursors."""
    _fields_ = [("s1d", C.POINTER(C.c_double)), ("table", C.POINTER(C.c_int32)), ("k", C.POINTER(C.c_int32)),
                ("n_tables", C.c_int32), ("spp", C.c_int32), ("n_dims", C.c_int32), ("first_1d", C.c_int32),
                ("first_2d", C.c_int32), ("reserved", C.c_int32)]


STRAT_SYMBOLS = ("pbrt_gpu_frame_samples_stratified_device", "pbrt_gpu_li_stratified_device")


def strat_sampler_desc(sampler_x, sampler_y, n_dims, jitter=False, reserved=0):
    return StratSamplerDesc(sampler_x, sampler_y, n_dims, 1 if jitter else 0, reserved)


def camera_cursors(n_dims):
    """(first_1d, first_2d) of a path after GetCameraSample: pFilm, pLens (Get2D) and the time (Get1D)."""
    return min(1, n_dims), min(2, n_dims)


def declare_strat(L):
    """ctypes prototypes of the stratified calls (apart, like declare_li: an earlier build has none)."""
    P, vp = C.POINTER, C.c_void_p
    L.pbrt_gpu_frame_samples_stratified_device.argtypes = [vp, P(FrameDesc), P(StratSamplerDesc), P(FrameSamplesSoA),
                                                           P(StratSamplesSoA)]
    L.pbrt_gpu_li_stratified_device.argtypes = [vp, P(LiDesc), P(RaySoA), P(RngSoA), C.c_size_t, P(RadianceSoA),
                                                P(StratSoA)]


# pbrt_gpu_probe ops (include/pbrt_diag.h): one device function on a batch of inputs
PBRT_PROBE_SIN = 1
PBRT_PROBE_COS = 2
PBRT_PROBE_TAN = 3
PBRT_PROBE_ATAN = 4
PBRT_PROBE_ATAN2 = 5
PBRT_PROBE_ASIN = 6
PBRT_PROBE_ACOS = 7
PBRT_PROBE_SQRT = 8
PBRT_PROBE_DIV = 9
PBRT_PROBE_NEXTAFTER = 10
PBRT_PROBE_MAX = 11
PBRT_PROBE_MIN = 12
PBRT_PROBE_OFFSET_RAY_ORIGIN = 13
PBRT_PROBE_EFLOAT_ADD = 14
PBRT_PROBE_TRANSFORM_RAY = 15
PBRT_PROBE_SPAWN_RAY_TO = 16
PBRT_PROBE_PCG = 17
PBRT_PROBE_NEXT_FLOAT_UP = 18
PBRT_PROBE_NEXT_FLOAT_DOWN = 19
PBRT_PROBE_MIN_NONAN = 20
PBRT_PROBE_MAX_NONAN = 21
PBRT_PROBE_EFLOAT_MUL = 22
PBRT_PROBE_EFLOAT_DIV = 23
PBRT_PROBE_SINCOS = 24            # in a -> Sin(a), Cos(a) from one evaluation
PBRT_PROBE_CONCENTRIC_DISK = 25   # in u[2] -> ConcentricSampleDisk(u)[2]


def declare_probe(L):
    """ctypes prototype of pbrt_gpu_probe."""
    P = C.POINTER
    L.pbrt_gpu_probe.argtypes = [C.c_int, C.c_int, P(C.c_double), C.c_size_t, C.c_int, P(C.c_double), C.c_int]
    L.pbrt_gpu_probe.restype = C.c_int

/*
 * pbrt_gpu.h — C ABI of the MI355X-native go-pbrt hot path.
 *
 * This is the drop-in boundary for go-pbrt's ray–scene intersection and
 * path-tracing inner loop. A cgo shim binds exactly these entry points (see
 * INTEGRATION.md). Every call is frame- or batch-granular: the reference's
 * per-ray interfaces (pbrt.Integrator.Li, pbrt.Aggregate.Intersect) cost a
 * cgo hop each and can never be the device boundary.
 *
 * Reference interfaces replaced (paths relative to ssttuu/go-pbrt):
 *   pbrt_gpu_render       <- pbrt.Render(ctx, Integrator, Scene, tileSize)
 *                            pkg/pbrt/integrator.go:291-350 (with Path.Li
 *                            pkg/integrator/path.go:32-157 and
 *                            DirectLighting.Li pkg/integrator/directlighting.go:62-104
 *                            executed on the device)
 *   pbrt_gpu_intersect    <- (*accelerator.BVH).Intersect  pkg/accelerator/bvh.go:659-712
 *   pbrt_gpu_intersect_p  <- (*accelerator.BVH).IntersectP pkg/accelerator/bvh.go:713-765
 *   pbrt_gpu_cancel       <- ctx.Done() / errgroup cancellation, integrator.go:305-345
 *   PBRT_E_REF_PANIC      <- the places where the reference panics instead of
 *                            returning: integrator.go:73-75 (Ld > 10),
 *                            pkg/efloat/efloat.go:102-111 (EFloat Check)
 *
 * Conventions: plain C11, no exceptions across the ABI, caller-owned output
 * buffers, every function returns a pbrt_status (0 = OK). All arithmetic is
 * IEEE-754 binary64 with Go (amd64) semantics; descriptors carry matrices
 * exactly as the Go host computed them.
 */
#ifndef PBRT_GPU_H
#define PBRT_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status */
typedef enum pbrt_status {
    PBRT_OK = 0,
    PBRT_E_INVALID = 1,      /* bad descriptor / argument                     */
    PBRT_E_HIP = 2,          /* HIP runtime failure                           */
    PBRT_E_RCCL = 3,         /* reserved: the library links no collective; a
                                device group merges over peer access        */
    PBRT_E_CANCELLED = 4,    /* pbrt_gpu_cancel() observed                    */
    PBRT_E_REF_PANIC = 5,    /* the Go reference would have panicked here     */
    PBRT_E_UNSUPPORTED = 6   /* descriptor uses a feature not on the hot path */
} pbrt_status;

/* panic kinds reported in pbrt_gpu_stats.panic_kind */
enum {
    PBRT_PANIC_NONE = 0,
    PBRT_PANIC_LD_GT_10 = 1,     /* integrator.go:73-75                      */
    PBRT_PANIC_EFLOAT = 2,       /* efloat.go:102-111                        */
    PBRT_PANIC_BVH_STACK = 3,    /* bvh.go:670 fixed [64] stack overflow     */
    PBRT_PANIC_NIL_DEREF = 4     /* rough Glass: TrowbridgeReitz.SampleWH returns nil
                                    (its wh is shadowed, microfacet.go:79-115), so a
                                    microfacet BxDF's SampleF dereferences nil in
                                    Reflect/Refract (reflection.go:102-118, 706-811) */
};

/* --------------------------------------------------------------- transform */
/* pkg/pbrt/transform.go:27 Matrix4x4, :144 Transform{Matrix, MatrixInverse} */
typedef struct pbrt_matrix4x4 { double m[4][4]; } pbrt_matrix4x4;
typedef struct pbrt_transform { pbrt_matrix4x4 m, m_inv; } pbrt_transform;

/* ------------------------------------------------------------------ shapes */
enum { PBRT_SHAPE_SPHERE = 1, PBRT_SHAPE_DISK = 2 };

/* pkg/pbrt/sphere.go:8-17 Sphere, pkg/shapes/disk.go:14-20 Disk.
 * world_to_object is object_to_world.Inverse() (matrix/inverse swapped). */
typedef struct pbrt_shape_desc {
    int32_t type;
    int32_t reverse_orientation;
    int32_t transform_swaps_handedness;
    int32_t pad0;
    pbrt_transform object_to_world;
    double radius;
    double z_min, z_max, theta_min, theta_max, phi_max;   /* sphere           */
    double height, inner_radius;                          /* disk             */
} pbrt_shape_desc;

/* --------------------------------------------------------------- materials */
enum { PBRT_TEX_CONSTANT = 1, PBRT_TEX_CHECKERBOARD2D = 2 };
enum { PBRT_MAT_MATTE = 0, PBRT_MAT_MIRROR = 1, PBRT_MAT_GLASS = 2 };

/* type PBRT_MAT_MATTE: pkg/materials/matte.go:8-37 MatteMaterial with Kd either a
 * ConstantSpectrumTexture (pkg/pbrt/texture.go:133-145) or a Checkerboard2D
 * over PlanarMapping2D (pkg/textures/checkerboard.go, texture.go:105-123) whose
 * two sub-textures are constants. sigma is a ConstantFloatTexture.
 * type PBRT_MAT_MIRROR: pkg/materials/mirror.go:9-32 (constant Kr; NewMirror uses 0.9).
 * type PBRT_MAT_GLASS: pkg/materials/glass.go:15-75 with constant Kr, Kt, index
 * (eta) and roughness textures. Path.Li asks for multiple lobes (path.go:74), so
 * smooth glass (both roughnesses 0) is one FresnelSpecular lobe; rough glass is
 * MicrofacetReflection + MicrofacetTransmission over TrowbridgeReitz(u, v)
 * (microfacet.go, reflection.go:670-835), whose sampling panics in the reference
 * (PBRT_PANIC_NIL_DEREF). Path renders of Mirror, smooth Glass and OrenNayar
 * scenes run on the wave pipeline (its kX instantiations, LDS-sized trees);
 * rough glass, DirectLighting through these materials and panic fidelity run
 * on the serial kernel. */
typedef struct pbrt_material_desc {
    int32_t kd_type;
    int32_t type;                  /* PBRT_MAT_* (0 = Matte)                  */
    double kd[3];
    double vs[3], vt[3], ds, dt;
    double tex1[3], tex2[3];
    double sigma;
    double kr[3], kt[3];           /* Mirror: Kr; Glass: Kr, Kt               */
    double eta, u_roughness, v_roughness;   /* Glass                          */
} pbrt_material_desc;

/* -------------------------------------------------------------- primitives */
enum { PBRT_PRIM_GEOMETRIC = 1, PBRT_PRIM_TRANSFORMED = 2 };

/* GeometricPrimitive (pkg/pbrt/primitive.go:22-78), optionally wrapped in a
 * TransformedPrimitive with a non-animated AnimatedTransform (primitive.go:89-129). */
typedef struct pbrt_primitive_desc {
    int32_t kind;
    int32_t shape;
    int32_t material;
    int32_t pad0;
    pbrt_transform prim_to_world;
} pbrt_primitive_desc;

/* flattened BVH node, pkg/accelerator/bvh.go:80-87 LinearBVHNode */
typedef struct pbrt_bvh_node {
    double bmin[3], bmax[3];
    uint32_t offset;      /* primitiveOffset (leaf) | secondChildOffset (interior) */
    uint16_t n_prims;     /* 0 => interior */
    uint8_t axis;
    uint8_t pad0;
} pbrt_bvh_node;

/* ----------------------------------------------------------- triangle meshes */
/* EXTENSION (BASELINE configs D/E): go-pbrt has no triangle shape (pkg/shapes
 * holds only disk.go) and its BVH builder is O(n^2) (bvh.go:272-411), so a
 * triangle mesh is not part of the reference's semantics. Semantics here are
 * pbrt-v3's Triangle::Intersect (watertight, Woop et al.; default uv), in
 * float64 after exact widening of float32 world-space vertices, with error
 * bounds from the real machine epsilon 2^-53 (go-pbrt's own Gamma() is
 * denormal). Meshes are traversed through their own BVH, built
 * on the device (LBVH); a closest hit is the smallest (t, triangle index)
 * over all triangles, so results do not depend on that BVH. Triangles of
 * mesh m carry the global index mesh_first(m) + i and report prim =
 * n_prims + that index. */
typedef struct pbrt_mesh_desc {
    int32_t n_vertices, n_triangles;
    int32_t material;              /* index into materials                      */
    int32_t reverse_orientation;   /* flips the geometric normal                */
    const float* p;                /* n_vertices * 3 world-space positions     */
    const int32_t* indices;        /* n_triangles * 3 vertex indices            */
} pbrt_mesh_desc;

/* ------------------------------------------------------------------ lights */
enum { PBRT_LIGHT_POINT = 1, PBRT_LIGHT_DISTANT = 2, PBRT_LIGHT_DIFFUSE_AREA = 3 };

/* pkg/lights/{point,distant,diffuse}.go */
typedef struct pbrt_light_desc {
    int32_t type;
    int32_t shape;          /* DIFFUSE_AREA: index into shapes (a sphere)    */
    int32_t two_sided;      /* DIFFUSE_AREA                                  */
    int32_t pad0;
    double spectrum[3];     /* Point.I | Distant.L | DiffuseAreaLight.LEmit  */
    double p_light[3];      /* Point: lightToWorld(0,0,0)                    */
    double w_light[3];      /* Distant: normalized world direction           */
    double world_radius;    /* Distant: set by Preprocess (BoundingSphere)   */
} pbrt_light_desc;

/* ------------------------------------------------------------------ camera */
/* PerspectiveCamera (pkg/pbrt/camera.go:128-242). shutter_close is stored as
 * the reference leaves it: NewProjectiveCamera passes shutterOpen twice
 * (camera.go:116), so both fields hold shutterOpen. */
typedef struct pbrt_camera_desc {
    pbrt_transform camera_to_world;
    pbrt_transform raster_to_camera;
    double lens_radius, focal_distance, shutter_open, shutter_close;
} pbrt_camera_desc;

/* -------------------------------------------------------------------- film */
/* pkg/pbrt/film.go:27-76 (CroppedPixelBounds, BoxFilter radius, filter table) */
typedef struct pbrt_film_desc {
    int64_t res_x, res_y;
    int64_t crop_min_x, crop_min_y, crop_max_x, crop_max_y;
    double filter_radius_x, filter_radius_y;
    double max_sample_luminance;
    double filter_table[16 * 16];
} pbrt_film_desc;

/* light-selection distribution (pkg/pbrt/sampling.go:5-55 Distribution1D),
 * computed by the host from the integrator's LightSampleStrategy
 * (lightdistribution.go). func has n entries, cdf n+1. */
#define PBRT_MAX_DIST 64
typedef struct pbrt_distribution_desc {
    int32_t count;
    int32_t pad0;
    double func_int;
    double func[PBRT_MAX_DIST];
    double cdf[PBRT_MAX_DIST + 1];
} pbrt_distribution_desc;

/* ------------------------------------------------------------------- scene */
typedef struct pbrt_scene_desc {
    int32_t n_shapes, n_materials, n_prims, n_nodes, n_lights, pad0;
    const pbrt_shape_desc* shapes;
    const pbrt_material_desc* materials;
    const pbrt_primitive_desc* prims;      /* BVH order (orderedPrims)        */
    const pbrt_bvh_node* nodes;            /* depth-first, bvh.go:632-651     */
    const pbrt_light_desc* lights;
    pbrt_camera_desc camera;
    pbrt_film_desc film;
    double world_min[3], world_max[3];     /* Scene.WorldBound (BVH root)     */
    int32_t n_meshes, pad1;                /* extension: triangle meshes      */
    const pbrt_mesh_desc* meshes;
} pbrt_scene_desc;

/* ------------------------------------------------------------------ render */
enum { PBRT_INTEGRATOR_PATH = 1, PBRT_INTEGRATOR_DIRECT_LIGHTING = 2 };
enum { PBRT_LIGHT_STRATEGY_UNIFORM = 1, PBRT_LIGHT_STRATEGY_POWER = 2 };
enum { PBRT_DL_UNIFORM_SAMPLE_ALL = 1, PBRT_DL_UNIFORM_SAMPLE_ONE = 2 };

/* Execution modes.
 *  EXACT: the reference's per-tile RNG stream replayed bit-for-bit
 *         (integrator.go:318,328; one sampler clone per 16-px tile).
 *  THROUGHPUT: identical arithmetic, but every (pixel, sample) path gets its
 *         own PCG32 stream => statistically (not bitwise) equal images. */
enum { PBRT_MODE_EXACT = 0, PBRT_MODE_THROUGHPUT = 1 };

typedef struct pbrt_render_desc {
    /* sampler: sampler.NewStratified(x, y, jitter, nDims) (stratified.go:12-19) */
    int32_t sampler_x, sampler_y, jitter, n_dims;
    /* integrator */
    int32_t integrator;      /* PBRT_INTEGRATOR_*                               */
    int32_t max_depth;
    int32_t light_strategy;  /* Path: PBRT_LIGHT_STRATEGY_*                     */
    int32_t dl_strategy;     /* DirectLighting: PBRT_DL_*                       */
    double rr_threshold;
    int64_t tile_size;       /* pbrt.Render tileSize (16 in internal/render)    */
    /* tile subset (multi-GPU sharding): tiles t = tile_begin, tile_begin +
     * tile_stride, ... < tile_end (tile_end <= 0 means all tiles). */
    int64_t tile_begin, tile_end, tile_stride;
    int32_t mode;            /* PBRT_MODE_*                                     */
    int32_t flags;           /* PBRT_FLAG_* (diagnostics), normally 0           */
} pbrt_render_desc;

typedef struct pbrt_gpu_stats {
    uint64_t tiles_rendered;
    uint64_t camera_samples;     /* W*H*(spp-1) over rendered tiles           */
    uint64_t paths_traced;       /* camera rays that reached Li               */
    double kernel_ms;            /* device time of the tile render kernel      */
    double merge_ms;             /* device time of the film merge kernel       */
    double total_ms;             /* host wall time of the call                */
    int32_t panic_kind;          /* PBRT_PANIC_*                              */
    int32_t panic_tile;
    int64_t panic_pixel_x, panic_pixel_y;
    int32_t panic_sample, panic_bounce;
    int32_t kernel;          /* PBRT_KERNEL_SERIAL / _WAVE / _WAVEFRONT (last render) */
    int32_t batches;         /* WAVE/WAVEFRONT: tile batches of the frame         */
    double chain_ms;         /* WAVE/WAVEFRONT: sample-offset chain time, summed  */
    double paths_ms;         /* WAVE/WAVEFRONT: k_paths time (full paths), summed */
    /* The reference's ray segments for the rendered paths, counted in-kernel
     * (SURVEY 8(d)): closest-hit queries of Path.Li's loop (path.go:44-45, one per
     * iteration, incl. the one at bounces == maxDepth; DirectLighting: one per
     * Li call, directlighting.go:67) and any-hit visibility rays of light
     * sampling (VisibilityTester.Unoccluded, integrator.go:112-119), on every
     * kernel. EstimateDirect's BSDF-sampled ray, which always adds 0, is not
     * counted. Equal to the oracle's counts. */
    uint64_t rays_closest;
    uint64_t rays_shadow;
} pbrt_gpu_stats;

/* ----------------------------------------------------------- ray batches */
typedef struct pbrt_ray_soa {
    const double *ox, *oy, *oz, *dx, *dy, *dz;
    const double *tmax;          /* may be NULL => +Inf                      */
} pbrt_ray_soa;

typedef struct pbrt_hit_soa {
    uint8_t* hit;
    double* t_max;               /* ray.TMax after Intersect (tHit if hit)    */
    int32_t* prim;               /* index into scene prims (BVH order), -1    */
    double *px, *py, *pz;        /* SurfaceInteraction.Point                  */
    double *nx, *ny, *nz;        /* SurfaceInteraction.Normal (geometric)     */
} pbrt_hit_soa;

/* ------------------------------------------------------------------ opts */
typedef struct pbrt_gpu_opts {
    int32_t device;              /* HIP device ordinal (-1 => current)       */
    int32_t lanes_per_wave;      /* serial kernel: tiles per 64-lane wave (0=auto) */
    int32_t occupancy;           /* serial kernel: waves/SIMD build variant (0,1,2,4,8) */
    int32_t kernel;              /* PBRT_KERNEL_*                               */
    int32_t reserved[4];
} pbrt_gpu_opts;

/* Kernels. All replay the reference bit for bit:
 *  SERIAL     one lane per tile, the tile's PCG32 stream consumed in order
 *             (any render; the only one for n_dims < 3 Path renders,
 *             zero-pdf lights, filter radius >= 1.5 and PBRT_FLAG_PANIC_FIDELITY);
 *  WAVE_CI    the wave pipeline (Path integrator, n_dims >= 3, every light
 *             pdf > 0, filter radius < 1.5, no rough glass; Matte, Mirror,
 *             smooth Glass and OrenNayar on a tree of any size): per-pixel shared bounce 1, the
 *             tile's path offsets found by a continuous-issue chain of
 *             speculative trajectories + jump-ahead (k_chain_ci; trees of more
 *             than 64 nodes: its instantiations with the reference's [64]
 *             traversal stack), then the
 *             samples as full paths (k_paths_ci, or the per-bounce path
 *             wavefront k_pw_* for mesh scenes, large trees and more than
 *             16 lights; up to PBRT_MAX_DIST lights);
 *  WAVE_DL    DirectLighting (n_dims >= 1): pixel-order StartPixel +
 *             jump-ahead, one lane per sample;
 *  WAVE, WAVEFRONT  (round 1's window and wavefront chains, since replaced)
 *             request the wave pipeline; st.kernel reports WAVE_CI;
 *  WAVE_CAM   the wave pipeline for renders whose camera ray belongs to the
 *             sample, not to the pixel: n_dims == 0 (Stratified without sampled
 *             dimensions, pbrt_random_sampler; pinhole or thin lens) or
 *             n_dims == 1 with a thin lens. Path integrator, Matte scenes on
 *             a tree of any size, any light count, every light pdf > 0. Every trajectory of
 *             the chain (k_chain_cam) and every path (k_paths_cam) starts at
 *             the camera; trees of more than 64 nodes run k_chain_cam_stack and
 *             k_paths_cam_stack, the same kernels with the [64] traversal stack;
 *             with n_dims == 0 the film footprint is per sample
 *             (k_film_cam). Opt-in: AUTO keeps such renders on SERIAL, and
 *             anything else requested with WAVE_CAM is PBRT_E_UNSUPPORTED
 *             (DirectLighting, n_dims >= 2, n_dims == 1 with a pinhole,
 *             Mirror / Glass / OrenNayar, meshes, panic fidelity).
 * THROUGHPUT mode reports WAVE for the wave pipeline (no chain), and WAVE_CAM
 * for a WAVE_CAM request. */
/* WAVE kernel: always replay StartPixel serially (the path normally taken
 * only after a pcg_bounded rejection); results are identical. */
#define PBRT_FLAG_SERIAL_START_PIXEL 1
/* Panic fidelity: also trace the rays whose results never reach the film but
 * whose traversal can panic in the reference -- EstimateDirect's BSDF-sampled
 * MIS ray for an area light (integrator.go:132-192, incl. Sphere.PdfWi) and
 * the closest hit at bounces == maxDepth (path.go:44-45,66). Serial kernel. */
#define PBRT_FLAG_PANIC_FIDELITY 2

enum { PBRT_KERNEL_AUTO = 0, PBRT_KERNEL_SERIAL = 1, PBRT_KERNEL_WAVE = 2, PBRT_KERNEL_WAVEFRONT = 3,
       PBRT_KERNEL_WAVE_CI = 4, /* wave pipeline, continuous-issue offset chain */
       PBRT_KERNEL_WAVE_DL = 5, /* DirectLighting: pixel-order StartPixel + jump-ahead, one lane per sample */
       PBRT_KERNEL_WAVE_CAM = 6 /* wave pipeline with per-sample camera rays (n_dims 0, or 1 with a thin lens); opt-in */ };

typedef struct pbrt_gpu_ctx pbrt_gpu_ctx;

/* Copies the scene to device memory. The descriptor may be freed afterwards. */
int pbrt_gpu_create(const pbrt_scene_desc* scene, const pbrt_gpu_opts* opts,
                    pbrt_gpu_ctx** out);

/* Renders the frame (or the tile subset in rd) and writes the fp64 XYZ film,
 * res_x*res_y*3 doubles in raster order, to film_xyz (host memory) before
 * returning. Equivalent of pbrt.Render minus WriteImage. */
int pbrt_gpu_render(pbrt_gpu_ctx* ctx, const pbrt_render_desc* rd,
                    double* film_xyz, pbrt_gpu_stats* stats);

/* Same, but leaves the film in device memory (pbrt_gpu_film_device) and does
 * not synchronize with the host: the bench's timed region. */
int pbrt_gpu_render_async(pbrt_gpu_ctx* ctx, const pbrt_render_desc* rd);
/* Same, merging the film into a caller-owned device buffer of res_x*res_y*3
 * doubles (e.g. a torch tensor's storage). For one frame over several GPUs
 * see pbrt_gpu_group below. */
int pbrt_gpu_render_async_into(pbrt_gpu_ctx* ctx, const pbrt_render_desc* rd, double* film_device);
int pbrt_gpu_synchronize(pbrt_gpu_ctx* ctx, pbrt_gpu_stats* stats);
/* device pointer to the res_x*res_y*3 fp64 film of the last render */
double* pbrt_gpu_film_device(pbrt_gpu_ctx* ctx);
int pbrt_gpu_film_download(pbrt_gpu_ctx* ctx, double* film_xyz);
/* HIP stream the context launches on (hipStream_t as void*) */
void* pbrt_gpu_stream(pbrt_gpu_ctx* ctx);

/* Batch closest hit / any hit through the device BVH (Aggregate interface). */
int pbrt_gpu_intersect(pbrt_gpu_ctx* ctx, const pbrt_ray_soa* rays, size_t n,
                       pbrt_hit_soa* hits);
int pbrt_gpu_intersect_p(pbrt_gpu_ctx* ctx, const pbrt_ray_soa* rays, size_t n,
                         uint8_t* occluded);

/* ---------------------------------------------------- device-resident queries */
/* Device memory owned by a context, for callers that cannot allocate on the
 * device themselves (Go) or should not hand the library memory whose lifetime
 * another runtime manages. A buffer is freed by pbrt_gpu_buffer_destroy or, at
 * the latest, by pbrt_gpu_destroy of its context (after the context's streams
 * have been synchronised); using a handle after its context is destroyed is
 * undefined. bytes == 0 is PBRT_E_INVALID. upload and download are ordered on
 * the context's stream and synchronise it: they return when the host memory
 * may be reused (upload) or is valid (download). A range outside the buffer is
 * PBRT_E_INVALID. buffer_destroy synchronises the stream first. */
typedef struct pbrt_gpu_buffer pbrt_gpu_buffer;
int pbrt_gpu_buffer_create(pbrt_gpu_ctx* ctx, size_t bytes, pbrt_gpu_buffer** out);
void* pbrt_gpu_buffer_ptr(const pbrt_gpu_buffer* b);
size_t pbrt_gpu_buffer_size(const pbrt_gpu_buffer* b);
int pbrt_gpu_buffer_upload(pbrt_gpu_buffer* b, size_t offset, const void* host, size_t bytes);
int pbrt_gpu_buffer_download(pbrt_gpu_buffer* b, size_t offset, void* host, size_t bytes);
void pbrt_gpu_buffer_destroy(pbrt_gpu_buffer* b);

/* pbrt_gpu_intersect[_p] over arrays that already live on the device: every
 * pointer of rays and hits (and occluded) is a DEVICE pointer to n elements,
 * from pbrt_gpu_buffer_ptr or any allocation of the context's device. The calls
 * only enqueue a kernel on the context's stream (pbrt_gpu_stream), after
 * everything already on it: no allocation, copy or synchronisation (but one
 * small allocation for the panic record on a context's first query), so the
 * outputs are valid once the stream has been synchronised (pbrt_gpu_query_status,
 * pbrt_gpu_buffer_download, or the caller's own stream wait).
 *
 * rays->tmax may be NULL (+Inf). hits->hit is required, every other pointer of
 * hits is optional. Values are those of pbrt_gpu_intersect: on a miss hit 0,
 * t_max the ray's own TMax, prim -1, point and normal 0; occluded is 1 or 0. A
 * ray on which the reference panics is written as a miss (occluded 0) and
 * counted in the context's panic record. n == 0 is PBRT_OK and launches
 * nothing. PBRT_E_INVALID, before any device call: a NULL context, rays, ray
 * pointer other than tmax, hits->hit or occluded; n > 2^31 - 1; or a render in
 * flight on the context (between render_async and its synchronize), which is
 * left untouched. */
int pbrt_gpu_intersect_device(pbrt_gpu_ctx* ctx, const pbrt_ray_soa* rays, size_t n,
                              const pbrt_hit_soa* hits);
int pbrt_gpu_intersect_p_device(pbrt_gpu_ctx* ctx, const pbrt_ray_soa* rays, size_t n,
                                uint8_t* occluded);

/* Camera rays of a pixel window, written to device arrays in raster order:
 * ray (y - y0) * (x1 - x0) + (x - x0) is PerspectiveCamera.GenerateRay
 * (camera.go:192-242) for pFilm = (x + film_dx, y + film_dy), pLens = (lens_u,
 * lens_v) and time sample time_u, with TMax +Inf (tmax may be NULL: not
 * written). Enqueue-only and ordered like the intersect calls, so an
 * intersect_device on its output needs no host step in between. A window
 * outside 0 <= x0 < x1 <= res_x (same for y) is PBRT_E_INVALID. */
typedef struct pbrt_ray_soa_out {
    double *ox, *oy, *oz, *dx, *dy, *dz;
    double *tmax;                /* may be NULL                              */
} pbrt_ray_soa_out;
typedef struct pbrt_camera_rays_desc {
    int64_t x0, y0, x1, y1;
    double film_dx, film_dy;
    double lens_u, lens_v, time_u;
} pbrt_camera_rays_desc;
int pbrt_gpu_camera_rays_device(pbrt_gpu_ctx* ctx, const pbrt_camera_rays_desc* desc,
                                const pbrt_ray_soa_out* rays);

/* The panic record of every query since the last pbrt_gpu_query_status:
 * panics counts the rays on which the reference would have panicked,
 * first_ray is the smallest index (within its call) of such a ray, -1 when
 * there was none, and panic_kind that ray's PBRT_PANIC_*. The call synchronises
 * the context's stream, copies the record to *out (may be NULL) and clears it;
 * it returns PBRT_E_REF_PANIC when panics > 0, else PBRT_OK, and
 * PBRT_E_INVALID for a NULL context or a render in flight. */
typedef struct pbrt_query_record {
    uint64_t panics;
    int64_t first_ray;
    int32_t panic_kind, pad0;
} pbrt_query_record;
int pbrt_gpu_query_status(pbrt_gpu_ctx* ctx, pbrt_query_record* out);

/* Integrator.Li over arrays that live on the device: ray i of the batch gets
 * Path.Li(ray_i, scene, sampler, depth 0) (path.go:32-157), where the sampler is
 * sampler.RandomSampler on the PCG32 stream (rng->state[i], rng->inc[i]): every
 * Get1D / Get2D is a draw of that stream, in Path.Li's order, and no dimension
 * is stratified. The ray's time is 0 (it reaches no draw and no output);
 * rays->tmax may be NULL (+Inf). One kernel (k_li) runs the paths of the batch
 * with the arithmetic of the render kernels (path_step), so a value is the bits
 * a frame would add to its film for the same ray and stream.
 *
 * out->r/g/b receive Li's return value. The optional outputs (each may be NULL):
 * state, the ray's PCG32 state after its path; draws, the number of PCG32 draws
 * the path consumed (state is rng->state[i] advanced by draws steps); rays, the
 * reference's ray counts of the path, closest-hit queries in the low 16 bits and
 * visibility rays in the high 16. Li does not replace a NaN radiance: that is
 * the Render loop's (integrator.go:256-262), and so the caller's.
 *
 * A ray on which the reference panics has r = g = b = 0 and is counted in the
 * context's query record (pbrt_gpu_query_status) like a panicking ray of
 * pbrt_gpu_intersect_device. Its rays output holds the counts at the panic.
 * state and draws hold the stream at the panic where the closest-hit query of
 * an iteration panics (it precedes the iteration's draws). Where the light
 * sample panics (its visibility ray, or UniformSampleOneLight's Ld > 10), the
 * kernel has already drawn what the reference would have drawn next had it
 * gone on: the two values of the iteration's BSDF sample and, where Russian
 * roulette applies (from the fourth iteration on), its one value; the kernels
 * trace an iteration's visibility ray last. state is rng->state[i] advanced by
 * draws steps in either case.
 *
 * Ordering and memory are pbrt_gpu_intersect_device's: every pointer is a device
 * pointer to n elements; the call only enqueues on the context's stream, after
 * everything already on it; n == 0 is PBRT_OK and launches nothing. The light
 * distribution of desc->light_strategy is kept in a buffer of the query's own
 * and uploaded only when the strategy differs from the one last uploaded, so a
 * call in the steady state is one kernel launch: no allocation, copy or
 * synchronisation.
 *
 * PBRT_E_INVALID, before any device call: a NULL context, desc, rays, ray
 * pointer other than tmax, rng, rng->state, rng->inc, out, out->r/g/b;
 * n > 2^31 - 1; max_depth < 1; reserved != 0; or a render in flight (left
 * untouched). PBRT_E_UNSUPPORTED, with the reason in pbrt_gpu_last_error, where
 * the kernel is not the reference: integrator other than PBRT_INTEGRATOR_PATH,
 * max_depth > 2048, a scene with rough glass, an unknown light strategy, or a
 * light distribution that mixes lights of pdf 0 with others. The reference's
 * Power distribution is served: its entries are all 0 (SURVEY #28), so every
 * picked light has pdf 0 and UniformSampleOneLight returns black after its one
 * draw (integrator.go:56-58); k_li draws as it does, and no light reaches L. */
typedef struct pbrt_li_desc {
    int32_t integrator;      /* PBRT_INTEGRATOR_PATH                              */
    int32_t max_depth;       /* 1..2048                                           */
    int32_t light_strategy;  /* PBRT_LIGHT_STRATEGY_*                             */
    int32_t reserved;        /* 0                                                 */
    double  rr_threshold;
} pbrt_li_desc;
typedef struct pbrt_rng_soa {
    const uint64_t *state, *inc;   /* PCG32 state and increment per ray          */
} pbrt_rng_soa;
typedef struct pbrt_radiance_soa {
    double *r, *g, *b;       /* required                                          */
    uint64_t *state;         /* optional                                          */
    uint32_t *draws;         /* optional                                          */
    uint32_t *rays;          /* optional: closest | shadow << 16                  */
} pbrt_radiance_soa;
int pbrt_gpu_li_device(pbrt_gpu_ctx* ctx, const pbrt_li_desc* desc, const pbrt_ray_soa* rays,
                       const pbrt_rng_soa* rng, size_t n, const pbrt_radiance_soa* out);

/* The Integrator interface's other implementation over the same arrays: ray i
 * of the batch gets DirectLighting.Li(ray_i, scene, sampler, depth 0)
 * (directlighting.go:62-104, integrator.go:23-77, 352-422), where the sampler is
 * sampler.RandomSampler on the PCG32 stream (rng->state[i], rng->inc[i]): every
 * Get1D / Get2D is a draw of that stream, in the reference's order, and no
 * dimension is stratified. Per level: UniformSampleAllLights (4 draws a light)
 * or UniformSampleOneLight without a distribution (5 draws, and its "> 10"
 * panic), then, where depth + 1 < max_depth, the Get2D of SpecularReflect
 * (black for every supported material) and of SpecularTransmit, which recurses
 * at depth + 2 through smooth glass with the local-frame wi (SURVEY #7, #23).
 * One kernel (k_li_direct) runs the batch with the arithmetic of the render
 * kernels, so a value is the bits a DirectLighting frame would add to its film
 * for the same ray and stream. The ray's time is 0; rays->tmax may be NULL
 * (+Inf).
 *
 * The outputs are pbrt_gpu_li_device's: out->r/g/b receive Li's return value;
 * the optional state, draws and rays (closest-hit queries in the low 16 bits,
 * visibility rays in the high 16) may each be NULL. Li does not replace a NaN
 * radiance. A ray on which the reference panics (PBRT_PANIC_LD_GT_10 of
 * UniformSampleOneLight included) has r = g = b = 0, its optional outputs hold
 * the values at the panic, and it is counted in the context's query record
 * (pbrt_gpu_query_status).
 *
 * Ordering and memory are pbrt_gpu_intersect_device's: every pointer is a device
 * pointer to n elements; the call only enqueues on the context's stream, after
 * everything already on it; n == 0 is PBRT_OK and launches nothing.
 * DirectLighting has no light distribution: nothing is uploaded and every call
 * is one kernel launch. On a scene with Mirror / Glass / OrenNayar materials the
 * kernel keeps the recursion's level records (56 B a level and lane) in a buffer
 * the context owns, sized by the launch's capped grid and max_depth and never by
 * n; it grows on demand (a second call at the same or a smaller size allocates
 * nothing; pbrt_gpu_direct_li_scratch_bytes, pbrt_diag.h) and is freed with the
 * context. A Matte-only scene has no such buffer.
 *
 * PBRT_E_INVALID, before any device call: a NULL context, desc, rays, ray
 * pointer other than tmax, rng, rng->state, rng->inc, out, out->r/g/b;
 * n > 2^31 - 1; max_depth < 1; a reserved field != 0; or a render in flight
 * (left untouched). PBRT_E_UNSUPPORTED, with the reason in pbrt_gpu_last_error:
 * an unknown dl_strategy; a scene with rough glass; max_depth > 64 on a scene
 * with Mirror / Glass / OrenNayar materials (a DirectLighting render's own rule:
 * the level records hold 32 levels). On a Matte-only scene the recursion cannot
 * start and any max_depth >= 1 is served. The rays that only PBRT_FLAG_PANIC_FIDELITY
 * traces are not traced, as in pbrt_gpu_li_device. */
typedef struct pbrt_direct_li_desc {
    int32_t max_depth;    /* >= 1                                               */
    int32_t dl_strategy;  /* PBRT_DL_UNIFORM_SAMPLE_ALL | PBRT_DL_UNIFORM_SAMPLE_ONE */
    int32_t reserved[2];  /* 0                                                  */
} pbrt_direct_li_desc;
int pbrt_gpu_direct_li_device(pbrt_gpu_ctx* ctx, const pbrt_direct_li_desc* desc, const pbrt_ray_soa* rays,
                              const pbrt_rng_soa* rng, size_t n, const pbrt_radiance_soa* out);

/* ------------------------------------------------ Path.Li, one bounce at a time
 * pbrt_gpu_li_device with its loop opened: the loop-carried state of Path.Li
 * (path.go:32-157) as device arrays the caller owns, a call that gives every
 * path its fresh state, and a call that advances every live path by exactly one
 * iteration of the loop (path_step, the code k_li runs in registers). Between
 * two steps the state is the caller's to read, split, regroup or end.
 *
 * Path state: every pointer of pbrt_path_soa is a device pointer to n elements
 * and required, but tmax. 141 bytes a path, 133 without tmax:
 *   ox..dz, tmax  the ray the next step traces (tmax NULL: +Inf; where present
 *                 it is read by a step and written with +Inf after a scatter);
 *                 the ray's time is 0                              48 + 8 B
 *   lr, lg, lb    the radiance sum so far                              24 B
 *   br, bg, bb    beta, the path's throughput                          24 B
 *   eta_scale     Path.Li's etaScale                                    8 B
 *   state, inc    the PCG32 stream (inc is only read)               8 + 8 B
 *   draws         PCG32 draws so far (pbrt_radiance_soa's meaning)      4 B
 *   rays          closest-hit queries | visibility rays << 16           4 B
 *   bounces       iterations of Path.Li's loop begun                    4 B
 *   status        PBRT_PATH_*: a zero-filled array is not live          1 B
 *
 * pbrt_gpu_path_begin_device writes the state a path has before its first
 * iteration (one launch, k_path_begin): L = 0, beta = 1, eta_scale = 1, bounces,
 * draws and rays 0, status ALIVE, the ray and the stream copied from rays and
 * rng (pbrt_gpu_li_device's arguments; rays->tmax NULL: +Inf).
 *
 * pbrt_gpu_path_step_device runs one iteration (one launch, k_path_step) for
 * every path the call covers whose status is PBRT_PATH_ALIVE; a path of any
 * other status is skipped and left untouched. in == NULL covers the paths
 * 0 .. n-1; otherwise the paths in->index[0 .. *in->count - 1], where *in->count
 * is read on the device (no host synchronisation) and n bounds it and is the
 * length of every array, the queues' index arrays included. An index outside
 * 0 .. n-1 is skipped. After its iteration a path is ALIVE with its next ray in
 * the state, ENDED, or PANICKED: the reference panics in this iteration, lr/lg/lb
 * are set to 0 (as pbrt_gpu_li_device reports such a ray, state and draws
 * included) and the path is counted
 * in the context's query record (pbrt_gpu_query_status) under its index, with
 * its PBRT_PANIC_*. A path that is ENDED or PANICKED keeps the ray, beta and
 * eta_scale its last iteration started from. Every value of the state is the
 * caller's to set between two steps: a step reads eta_scale on every scene
 * (Russian roulette compares beta * eta_scale, path.go:145-146), also where no
 * material of the scene would ever change it. With out != NULL the call first zeroes *out->count on the
 * stream, then the kernel appends the index of every covered path that is ALIVE
 * after the step; the order within out is unspecified, the set is determined.
 * in and out must not share an index or a count array, and the indices of an
 * in queue are distinct (an out queue's are).
 *
 * step (may be NULL, as may every pointer in it) receives, at the index of each
 * path this call advanced and nowhere else: hit, the closest hit of the
 * iteration with pbrt_gpu_intersect_device's values for the step's input ray (a
 * miss's values where the iteration traced nothing because bounces reached
 * max_depth, and on a traversal panic); material, the material index of the hit
 * primitive or mesh (-1 on a miss); ar/ag/ab, the term the iteration added to L:
 * L_after == L_before + added as one float64 addition per channel, and where
 * the iteration adds nothing added is 0 and L unchanged (a PANICKED path's L is
 * 0 and its added 0).
 *
 * The contract with pbrt_gpu_li_device: begin followed by desc->max_depth steps
 * leaves every path ENDED or PANICKED, and lr/lg/lb, state, draws and rays are
 * then the bits pbrt_gpu_li_device writes to r/g/b, state, draws and rays for
 * the same rays, streams and desc. A path's values depend on its own state
 * only: never on its index, its lane, the order of a queue or how the caller
 * partitions the paths over calls.
 *
 * desc is pbrt_gpu_li_device's, with its checks, its refusals
 * (PBRT_E_UNSUPPORTED: DirectLighting, max_depth > 2048, rough glass, an unknown
 * strategy, a mixed distribution) and its light-distribution buffer, uploaded
 * only when the strategy differs from the one last uploaded. Ordering and memory
 * are pbrt_gpu_intersect_device's: both calls only enqueue on the context's
 * stream and allocate nothing in the steady state; n == 0 is PBRT_OK and
 * launches nothing. PBRT_E_INVALID, before any device call: a NULL context,
 * desc, paths or required pointer (of paths, rays, rng, or of a queue that is
 * given); n > 2^31 - 1; max_depth < 1; reserved != 0; in and out aliased; or a
 * render in flight (left untouched). */
enum { PBRT_PATH_UNUSED = 0, PBRT_PATH_ALIVE = 1, PBRT_PATH_ENDED = 2, PBRT_PATH_PANICKED = 3 };
typedef struct pbrt_path_soa {
    double *ox, *oy, *oz, *dx, *dy, *dz;
    double *tmax;            /* may be NULL => +Inf                               */
    double *lr, *lg, *lb;
    double *br, *bg, *bb;
    double *eta_scale;
    uint64_t *state;
    const uint64_t *inc;
    uint32_t *draws;
    uint32_t *rays;          /* closest | shadow << 16                            */
    int32_t *bounces;
    uint8_t *status;         /* PBRT_PATH_*                                       */
} pbrt_path_soa;
typedef struct pbrt_path_queue {
    int32_t* index;          /* n elements                                        */
    uint32_t* count;         /* one element, on the device                        */
} pbrt_path_queue;
typedef struct pbrt_path_step_soa {
    pbrt_hit_soa hit;        /* every pointer optional, hit.hit included          */
    int32_t* material;
    double *ar, *ag, *ab;
} pbrt_path_step_soa;
int pbrt_gpu_path_begin_device(pbrt_gpu_ctx* ctx, const pbrt_ray_soa* rays, const pbrt_rng_soa* rng, size_t n,
                               const pbrt_path_soa* paths);
int pbrt_gpu_path_step_device(pbrt_gpu_ctx* ctx, const pbrt_li_desc* desc, const pbrt_path_soa* paths,
                              const pbrt_path_queue* in, const pbrt_path_queue* out, size_t n,
                              const pbrt_path_step_soa* step);

/* ---------------------------------------------- a frame from public pieces
 * Three enqueue-only calls that, with pbrt_gpu_li_device between the first two,
 * build a frame on the device: samples, Li, film, RGBA8. The composed film is a
 * THROUGHPUT render's with n_dims = 0, bit for bit; a caller may replace any
 * stage (their own camera, their own treatment of the radiances) and keep the
 * others. Ordering and memory are pbrt_gpu_intersect_device's: every pointer is
 * a device pointer, a call only enqueues on the context's stream after
 * everything already on it, and it neither synchronises nor copies.
 * pbrt_gpu_film_add_device keeps the tile films of a range in a scratch buffer
 * the context owns, which grows on demand (the one allocation of these calls: a
 * second call at the same or a smaller size allocates nothing) and is freed
 * with the context.
 *
 * THE FRAME LAYOUT, shared by frame_samples and film_add. Tiles in index order
 * over the film's cropped pixel bounds at tile_size (integrator.go:316-325:
 * tile t covers x0 = crop_min_x + (t % ntx) * tile_size .. min(x0 + tile_size,
 * crop_max_x), likewise y with t / ntx); pixels row-major inside their tile;
 * ns consecutive samples per pixel; dense, no padding. With W the crop width,
 * ts the tile size and h(ty) = min(ts, H - ty * ts) the height of tile row ty,
 * ty * ts * W + tx * ts * h(ty) pixels come before tile (tx, ty). A call covers
 * the tiles [tile_begin, tile_end); element 0 of every array is the first
 * sample of tile_begin's first pixel. pbrt_gpu_frame_count returns the element
 * count of the range (what every array must hold), or -PBRT_E_INVALID where
 * the call itself would return PBRT_E_INVALID for the desc.
 *
 * PBRT_E_INVALID of the frame calls, before any device call: a NULL context,
 * desc or required pointer; tile_size < 1; ns < 1; flags other than
 * PBRT_FILM_ADD_CLEAR; reserved != 0; a tile range outside 0 <= tile_begin <=
 * tile_end <= ntx * nty; more than 2^31 - 1 elements; or a render in flight
 * (left untouched). An empty range (tile_begin == tile_end) is PBRT_OK and
 * launches nothing, except that film_add with PBRT_FILM_ADD_CLEAR still clears.
 * PBRT_E_UNSUPPORTED, with the reason in pbrt_gpu_last_error: tile_size > 256 or
 * ns > 2^20 - 1. */
enum { PBRT_FILM_ADD_CLEAR = 1 };   /* film_add: zero the film first            */
typedef struct pbrt_frame_desc {
    int32_t tile_size;       /* 1..256                                            */
    int32_t ns;              /* samples per pixel in the arrays, 1..2^20 - 1      */
    int64_t tile_begin, tile_end;
    int32_t flags;           /* film_add: PBRT_FILM_ADD_CLEAR; else 0             */
    int32_t reserved;        /* 0                                                 */
} pbrt_frame_desc;
int64_t pbrt_gpu_frame_count(const pbrt_gpu_ctx* ctx, const pbrt_frame_desc* desc);

/* The traced samples of a THROUGHPUT render with n_dims = 0 (sampler.RandomSampler
 * semantics) and spp = ns + 1, in the frame layout: sample 0 of a pixel is never
 * traced (sampler.go:29-34), so position j of a pixel holds its sample k = j + 1.
 * Sample k of pixel pi of tile t starts at the PCG32 state mb_state(t, pi, k)
 * (three rounds of splitmix64: csrc/pbrt_path.h) on the stream inc = 2 t + 1,
 * draws pFilm x, pFilm y, pLens x, pLens y and the time (sampler.go:75-80), and
 * its ray is PerspectiveCamera.GenerateRay of those (pbrt_gpu_camera_rays_device's
 * arithmetic). Written per sample: the ray (tmax may be NULL; it is +Inf);
 * pfilm_x, pfilm_y, the absolute raster position (double)px + the drawn offset;
 * state, the stream after the five draws, where pbrt_gpu_li_device begins; inc;
 * and, where not NULL, the pixel px, py. One kernel launch (k_frame_samples).
 * The samples of n_dims >= 1, whose camera values are stratified, are
 * pbrt_gpu_frame_samples_stratified_device's. Not served: EXACT mode, where a
 * tile's samples share one stream. */
typedef struct pbrt_frame_samples_soa {
    double *ox, *oy, *oz, *dx, *dy, *dz;
    double *tmax;                /* may be NULL                              */
    double *pfilm_x, *pfilm_y;
    uint64_t *state, *inc;
    int32_t *px, *py;            /* may be NULL                              */
} pbrt_frame_samples_soa;
int pbrt_gpu_frame_samples_device(pbrt_gpu_ctx* ctx, const pbrt_frame_desc* desc,
                                  const pbrt_frame_samples_soa* out);

/* Adds the film of the samples of a tile range, in the frame layout with the
 * caller's ns, to film_device: (H, W, 3) float64 XYZ over the cropped bounds,
 * the buffer pbrt_gpu_render_async_into fills. PBRT_FILM_ADD_CLEAR zeroes the
 * whole film first. Values and order are the reference's, as a frame's own
 * kernels (k_film_cam, k_merge_film) compute them: a radiance with a NaN
 * component becomes (0.1, 0.1, 0.1) (integrator.go:256-262); FilmTile.AddSample
 * with sample weight 1 (film.go:211-248, its maxSampleLuminance test included);
 * a tile-film pixel is the sum of the samples whose footprint holds it, source
 * pixels in tile order and samples in order; RGBToXYZ per tile-film pixel
 * (MergeFilmTile, film.go:115-132); the tiles of the range are added to a film
 * pixel in ascending tile index, continuing from the value it holds. Ascending
 * tile ranges over several calls (the first with the clear flag) therefore give
 * the bits of one call over all tiles, which is how a caller bounds the memory
 * of a frame. Two launches: k_film_add_tiles, k_film_add_merge.
 *
 * pfilm_x must lie in [px, px + 1) of its pixel, likewise pfilm_y; outside that
 * range, or for a non-finite value, the sample's contribution is unspecified
 * (other samples are unaffected: the kernel gathers, and no address is derived
 * from a caller's value). PBRT_E_UNSUPPORTED besides the frame calls': a filter
 * radius outside (0, tile_size), where a tile film would reach beyond its
 * neighbouring tiles (pbrt_gpu_render refuses the same). */
typedef struct pbrt_film_samples_soa {
    const double *pfilm_x, *pfilm_y;
    const double *r, *g, *b;
} pbrt_film_samples_soa;
int pbrt_gpu_film_add_device(pbrt_gpu_ctx* ctx, const pbrt_frame_desc* desc,
                             const pbrt_film_samples_soa* samples, double* film_device);

/* Film.WriteImage's pixel conversion (film.go:157-159) of a device film of w x h
 * pixels to a device buffer of w * h * 4 bytes: pbrt_film_to_rgba8's bytes on
 * every input (uint8(Clamp(v, 0, 1) * 255), a NaN as Go on amd64 converts it: 0;
 * alpha 255). Any device film: a render's, a caller's, film_add's. One launch
 * (k_film_rgba8), which stores a pixel's four bytes at once: rgba_device must
 * be 4-byte aligned. PBRT_E_INVALID: a NULL or misaligned pointer, w or
 * h <= 0, more than 2^31 - 1 pixels, a render in flight. */
int pbrt_gpu_film_rgba8_device(pbrt_gpu_ctx* ctx, const double* film_device, int64_t w, int64_t h,
                               uint8_t* rgba_device);

/* ------------------------------------ the same pieces under sampler.Stratified
 * pbrt_gpu_frame_samples_device and pbrt_gpu_li_device speak sampler.RandomSampler:
 * every Get1D / Get2D is a PCG32 draw. The two calls below are their forms under
 * sampler.NewStratified(sampler_x, sampler_y, jitter, n_dims) (pixel.go:60-80,
 * stratified.go:21-48): a pixel has n_dims shuffled 1D arrays of spp = sampler_x
 * * sampler_y values, made by StartPixel; Get1D returns samples1D[cur1d++][k]
 * while cur1d < n_dims and is a draw beyond; Get2D returns samples2D[cur2d++][k]
 * while cur2d < n_dims and is two draws beyond, and every stratified 2D value is
 * (0, 0) (StratifiedSample2D writes into a copy, sampling.go:122-124). A path is
 * therefore described by its ray, its PCG32 stream, its pixel's table of n_dims x
 * spp doubles, its sample index k and the two dimension cursors it starts from.
 * With pbrt_gpu_film_add_device the composed film is a THROUGHPUT render's with
 * the same sampler, bit for bit. Ordering and memory are the frame calls'.
 *
 * pbrt_gpu_frame_samples_stratified_device: the traced samples of a THROUGHPUT
 * render with n_dims >= 1 in the frame layout, ns = spp - 1, position j of a
 * pixel holding its sample k = j + 1. StartPixel of pixel pi of tile t runs on
 * the stream mb_state(t, pi, 0), sample k on mb_state(t, pi, k), both with inc =
 * 2 t + 1. The camera sample is GetCameraSample's (sampler.go:75-80): pFilm is
 * the stratified (0, 0); pLens is (0, 0) for n_dims >= 2 and two draws for
 * n_dims = 1 (drawn with or without a lens, used only with one); the time is
 * s1d[0][k], which reaches no draw and no output. Written per sample, in out: the
 * ray, pfilm_x / pfilm_y = (double)px, (double)py, state (the stream after the
 * camera sample's draws, where Li begins), inc, and px / py where not NULL; in
 * strat: k, the sample index, and table, the index of the sample's pixel within
 * the range (its position in the frame layout with one element a pixel). Written
 * per pixel of the range, in layout order: its table s1d[pixel][d * spp + k], the
 * values StartPixel leaves, all spp columns (pbrt_gpu_frame_count with ns = 1
 * gives the pixel count). After the camera sample the cursors of a path are
 * (min(1, n_dims), min(2, n_dims)): what pbrt_gpu_li_stratified_device takes as
 * first_1d, first_2d. One kernel launch (k_strat_pixels), one wave per pixel.
 *
 * PBRT_E_INVALID: the frame calls' own cases; a NULL sampler; sampler_x or
 * sampler_y < 1; the sampler's reserved != 0; ns != sampler_x * sampler_y - 1; a
 * NULL out, strat or required pointer (all of strat's are required).
 * PBRT_E_UNSUPPORTED, with the reason in pbrt_gpu_last_error: the frame calls'
 * own; n_dims < 1 (that frame is pbrt_gpu_frame_samples_device's); and the wave
 * StartPixel's limits, as for a render: spp > 4096, n_dims * spp > 8192, or a
 * StartPixel staging beyond 48 KB of LDS. */
typedef struct pbrt_strat_sampler_desc {
    int32_t sampler_x, sampler_y;   /* >= 1; spp = sampler_x * sampler_y          */
    int32_t n_dims;                 /* >= 1                                       */
    int32_t jitter;                 /* 0 / 1                                      */
    int32_t reserved;               /* 0                                          */
} pbrt_strat_sampler_desc;
typedef struct pbrt_strat_samples_soa {
    int32_t *k, *table;          /* per sample                                    */
    double *s1d;                 /* per pixel of the range: n_dims * spp          */
} pbrt_strat_samples_soa;
int pbrt_gpu_frame_samples_stratified_device(pbrt_gpu_ctx* ctx, const pbrt_frame_desc* desc,
                                             const pbrt_strat_sampler_desc* sampler,
                                             const pbrt_frame_samples_soa* out,
                                             const pbrt_strat_samples_soa* strat);

/* pbrt_gpu_li_device under the stratified sampler: ray i gets Path.Li(ray_i,
 * scene, sampler, 0), where the sampler is a PixelSampler with the tables
 * s1d[table[i]] (n_dims * spp doubles each, value [d * spp + k]), at sample
 * k[i], with its cursors at (first_1d, first_2d) -- the dimensions the ray's
 * first Get1D / Get2D read -- on the stream (rng->state[i], rng->inc[i]).
 * out->draws counts PCG32 draws only (a stratified value consumes none);
 * out->state is the input state advanced by draws. The panic record, the
 * optional outputs, the light distributions and the refusals are
 * pbrt_gpu_li_device's. With n_dims = 0, or both cursors equal to n_dims, no
 * value is stratified and every output is pbrt_gpu_li_device's, bit for bit
 * (with n_dims = 0, s1d, table and k are not read and may be NULL).
 *
 * table[i] and k[i] index memory: the kernel clamps them into [0, n_tables) and
 * [0, spp). A ray whose values were out of range gets an unspecified radiance;
 * other rays are unaffected, and no address outside the caller's arrays is
 * formed. One kernel launch (k_li_strat) in the steady state, as k_li.
 *
 * PBRT_E_INVALID: pbrt_gpu_li_device's cases; a NULL strat; strat->reserved !=
 * 0; n_dims < 0; a cursor outside [0, n_dims]; and, while n_dims > 0, a NULL
 * s1d, table or k, spp < 1 or n_tables < 1. */
typedef struct pbrt_strat_soa {
    const double* s1d;           /* [n_tables][n_dims * spp]                      */
    const int32_t *table, *k;    /* per ray                                       */
    int32_t n_tables, spp, n_dims;
    int32_t first_1d, first_2d;  /* 0..n_dims                                     */
    int32_t reserved;            /* 0                                             */
} pbrt_strat_soa;
int pbrt_gpu_li_stratified_device(pbrt_gpu_ctx* ctx, const pbrt_li_desc* desc, const pbrt_ray_soa* rays,
                                  const pbrt_rng_soa* rng, size_t n, const pbrt_radiance_soa* out,
                                  const pbrt_strat_soa* strat);

/* Cancels the render in flight on ctx (from pbrt_gpu_render[_async[_into]]
 * entry until its pbrt_gpu_synchronize returns): the kernels poll a flag between
 * units of work (a pixel's chain, every 128 chain steps, a workgroup of paths),
 * so the frame stops within milliseconds and its synchronize returns
 * PBRT_E_CANCELLED (the caller's film buffer is then left undefined: the final
 * merge is skipped when the kernels saw the cancel). Like the reference's
 * errgroup, which stops issuing tiles once ctx is done (integrator.go:332-335),
 * it ends that render only: the flag is cleared when the render ends, so the
 * next render on the context runs normally. With no render in flight it does
 * nothing. Thread-safe. */
void pbrt_gpu_cancel(pbrt_gpu_ctx* ctx);
const char* pbrt_gpu_last_error(const pbrt_gpu_ctx* ctx);
void pbrt_gpu_destroy(pbrt_gpu_ctx* ctx);

/* ------------------------------------------------------------ device groups */
/* One scene resident on several GPUs, rendered as one frame. The group splits
 * the tiles rd names over its members (the k-th of them goes to member k mod N),
 * every member renders its share through the single-context path, and one
 * kernel on the leader (member 0) reads all members' tile films -- over peer
 * access, or from a staging copy on the leader where peer access is refused
 * or PBRT_GROUP_STAGE=1 is set when the group is created -- and adds them in
 * tile-index order, as Film.MergeFilmTile does. The film is therefore
 * bit-identical to the one a single context renders, whatever the member
 * count; a sum of per-shard films is not (it adds in shard order).
 *
 * devices holds 1..PBRT_GROUP_MAX HIP ordinals. An ordinal MAY REPEAT:
 * {0, 0, 0} is three members on one GPU. Members that share a GPU render one
 * after the other, so repeats bring no speed; they exist so that the whole
 * mechanism can be exercised on a machine with one GPU. opts->device is
 * ignored. A NULL scene, devices or out, n_devices outside 1..PBRT_GROUP_MAX
 * or a negative ordinal is PBRT_E_INVALID before any device call.
 *
 * The calls mirror the context's. render_async starts the frame and returns;
 * errors of the frame (a bad render desc included) are reported by
 * synchronize, which waits for every member, then merges. film_device, when
 * not NULL, is a caller-owned buffer of res_x*res_y*3 doubles on the leader's
 * device. Stats: counts are summed over the members; kernel_ms, chain_ms,
 * paths_ms and batches are the maximum over them; merge_ms is the device time
 * of the group merge (staging copies included); total_ms is host wall time. A
 * reference panic is reported for the lowest panicking tile over all members
 * and no film is merged. cancel cancels every member: the frame's synchronize
 * returns PBRT_E_CANCELLED without merging, the next frame runs normally. A
 * group serves one frame at a time, from one thread; only cancel may be
 * called from another. */
typedef struct pbrt_gpu_group pbrt_gpu_group;
#define PBRT_GROUP_MAX 8
int pbrt_gpu_group_create(const pbrt_scene_desc* scene, const pbrt_gpu_opts* opts,
                          const int32_t* devices, int32_t n_devices, pbrt_gpu_group** out);
int pbrt_gpu_group_render(pbrt_gpu_group* g, const pbrt_render_desc* rd, double* film_xyz,
                          pbrt_gpu_stats* stats);
int pbrt_gpu_group_render_async(pbrt_gpu_group* g, const pbrt_render_desc* rd, double* film_device);
int pbrt_gpu_group_synchronize(pbrt_gpu_group* g, pbrt_gpu_stats* stats);
/* device pointer (on the leader) to the film of the last frame */
double* pbrt_gpu_group_film_device(pbrt_gpu_group* g);
int pbrt_gpu_group_film_download(pbrt_gpu_group* g, double* film_xyz);
int pbrt_gpu_group_size(const pbrt_gpu_group* g);
/* diagnostics: member i's context (schedule source, counters) and its stats of
 * the last frame. Do not render on or destroy a member. */
pbrt_gpu_ctx* pbrt_gpu_group_member(pbrt_gpu_group* g, int i);
int pbrt_gpu_group_member_stats(pbrt_gpu_group* g, int i, pbrt_gpu_stats* stats);
void pbrt_gpu_group_cancel(pbrt_gpu_group* g);
const char* pbrt_gpu_group_last_error(const pbrt_gpu_group* g);
void pbrt_gpu_group_destroy(pbrt_gpu_group* g);

/* PNG-byte conversion of film.go:142-179 WriteImage: uint8(clamp(XYZ,0,1)*255),
 * no XYZ->RGB and no gamma, exactly as the reference. rgba: w*h*4 bytes. */
int pbrt_film_to_rgba8(const double* film_xyz, int64_t w, int64_t h, uint8_t* rgba);

#ifdef __cplusplus
}
#endif
#endif /* PBRT_GPU_H */

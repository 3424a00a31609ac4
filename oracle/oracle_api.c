/*
 * oracle/oracle_api.c — TEST INFRASTRUCTURE (oracle). Not part of the product.
 *
 * C exports used from tests/ (ctypes), __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg. Nothing in go-pbrt_amd/ links or loads this library.
 *
 * Besides the render (oracle_render) and the intersection tests on caller rays
 * (oracle_intersect), the integrators run on caller rays too: oracle_path_li is
 * Path.Li per ray, from a fresh or a caller's loop state, to the end or for a
 * limited number of iterations, and oracle_direct_li is DirectLighting.Li per
 * ray. Both run the functions the render runs (path_li_iteration, direct_li)
 * with sampler.RandomSampler on each ray's own PCG32 stream, and catch a
 * reference panic per ray.
 */
#include <stdlib.h>
#include <string.h>

#include "oracle_render.h"
#include "oracle_scene.h"

/* ------------------------------------------------------------ Go math KATs */
double oracle_go_sin(double x) { return go_sin(x); }
double oracle_go_cos(double x) { return go_cos(x); }
double oracle_go_tan(double x) { return go_tan(x); }
double oracle_go_atan(double x) { return go_atan(x); }
double oracle_go_atan2(double y, double x) { return go_atan2(y, x); }
double oracle_go_asin(double x) { return go_asin(x); }
double oracle_go_acos(double x) { return go_acos(x); }
double oracle_go_nextafter(double x, double y) { return go_nextafter(x, y); }
double oracle_go_max(double x, double y) { return go_max(x, y); }
double oracle_go_min(double x, double y) { return go_min(x, y); }
double oracle_go_radians(double d) { return go_radians(d); }
int64_t oracle_go_f2i(double x) { return go_f2i(x); }

/* ray.go:57-74 */
void oracle_offset_ray_origin(const double p[3], const double e[3], const double n[3], const double w[3],
                              double out[3]) {
    v3 r = offset_ray_origin(V3(p[0], p[1], p[2]), V3(e[0], e[1], e[2]), V3(n[0], n[1], n[2]),
                             V3(w[0], w[1], w[2]));
    out[0] = r.x; out[1] = r.y; out[2] = r.z;
}
/* efloat.go:10-40: returns 0 on success, 1 if Check() would panic */
int oracle_efloat_add(double v1, double e1, double v2, double e2, double out[3]) {
    panic_ctx pc;
    if (setjmp(pc.jb)) return 1;
    ef_t a = ef_new(&pc, v1, e1), b = ef_new(&pc, v2, e2);
    ef_t r = ef_add(&pc, a, b);
    out[0] = r.v; out[1] = r.lo; out[2] = r.hi;
    return 0;
}
/* efloat.go Mul / Div with the same contract as oracle_efloat_add */
int oracle_efloat_mul(double v1, double e1, double v2, double e2, double out[3]) {
    panic_ctx pc;
    if (setjmp(pc.jb)) return 1;
    ef_t a = ef_new(&pc, v1, e1), b = ef_new(&pc, v2, e2);
    ef_t r = ef_mul(&pc, a, b);
    out[0] = r.v; out[1] = r.lo; out[2] = r.hi;
    return 0;
}
int oracle_efloat_div(double v1, double e1, double v2, double e2, double out[3]) {
    panic_ctx pc;
    if (setjmp(pc.jb)) return 1;
    ef_t a = ef_new(&pc, v1, e1), b = ef_new(&pc, v2, e2);
    ef_t r = ef_div(&pc, a, b);
    out[0] = r.v; out[1] = r.lo; out[2] = r.hi;
    return 0;
}
/* transform.go */
void oracle_translate(double x, double y, double z, pbrt_transform* out) { *out = orc_translate(x, y, z); }
void oracle_scale(double x, double y, double z, pbrt_transform* out) { *out = orc_scale(x, y, z); }
void oracle_rotate(int axis, double deg, pbrt_transform* out) { *out = orc_rotate(axis, deg); }
void oracle_xf_mul(const pbrt_transform* a, const pbrt_transform* b, pbrt_transform* out) { *out = orc_xf_mul(a, b); }
int oracle_matrix_inverse(const pbrt_matrix4x4* m, pbrt_matrix4x4* out) { return orc_m_inverse(m, out); }
int oracle_look_at(const double pos[3], const double look[3], const double up[3], pbrt_transform* out) {
    return orc_look_at(V3(pos[0], pos[1], pos[2]), V3(look[0], look[1], look[2]), V3(up[0], up[1], up[2]), out);
}
void oracle_perspective(double fov, double n, double f, pbrt_transform* out) { *out = orc_perspective(fov, n, f); }
void oracle_transform_point(const pbrt_transform* t, const double p[3], const double e[3], double op[3], double oe[3]) {
    v3 err;
    v3 r = xf_point(t, V3(p[0], p[1], p[2]), V3(e[0], e[1], e[2]), &err);
    op[0] = r.x; op[1] = r.y; op[2] = r.z;
    oe[0] = err.x; oe[1] = err.y; oe[2] = err.z;
}
void oracle_transform_ray(const pbrt_transform* t, const double o[3], const double d[3], double oo[3], double od[3]) {
    ray_t r;
    r.o = V3(o[0], o[1], o[2]); r.d = V3(d[0], d[1], d[2]); r.tmax = INFINITY; r.time = 0;
    ray_t w = xf_ray(t, &r, NULL, NULL);
    oo[0] = w.o.x; oo[1] = w.o.y; oo[2] = w.o.z;
    od[0] = w.d.x; od[1] = w.d.y; od[2] = w.d.z;
}
void oracle_make_sphere(const pbrt_transform* o2w, int rev, double r, double zmin, double zmax, double phimax,
                        pbrt_shape_desc* out) {
    *out = orc_sphere(*o2w, rev, r, zmin, zmax, phimax);
}
void oracle_make_disk(const pbrt_transform* o2w, double h, double r, double ri, double phimax, pbrt_shape_desc* out) {
    *out = orc_disk(*o2w, h, r, ri, phimax);
}

/* ------------------------------------------------------------------ RNG */
void oracle_pcg_stream(uint64_t seed, int n, uint32_t* out) {
    orc_pcg r;
    orc_pcg_set_sequence(&r, seed);
    for (int i = 0; i < n; i++) out[i] = orc_pcg_next(&r);
}
void oracle_pcg_floats(uint64_t seed, int n, double* out) {
    orc_pcg r;
    orc_pcg_set_sequence(&r, seed);
    for (int i = 0; i < n; i++) out[i] = orc_pcg_float(&r);
}

/* ---------------------------------------------------------------- scenes */
void* oracle_scene_new(void) { return calloc(1, sizeof(orc_scene)); }
void* oracle_scene_readme(int64_t w, int64_t h) { return orc_scene_readme(w, h); }
void* oracle_scene_cornell(int64_t w, int64_t h) { return orc_scene_cornell(w, h); }
void* oracle_scene_heightfield(int64_t w, int64_t h, int quads, uint64_t seed) {
    return orc_scene_heightfield(w, h, quads, seed);
}
void* oracle_scene_readme_glass(int64_t w, int64_t h, int special, int mirror) {
    return orc_scene_readme_glass(w, h, special, mirror);
}
int oracle_scene_add_shape(void* s, const pbrt_shape_desc* d) { return orc_add_shape((orc_scene*)s, *d); }
int oracle_scene_add_material(void* s, const pbrt_material_desc* d) { return orc_add_material((orc_scene*)s, *d); }
int oracle_scene_add_primitive(void* s, const pbrt_primitive_desc* d) {
    orc_scene* sc = (orc_scene*)s;
    sc->prims_in[sc->n_prims_in] = *d;
    return sc->n_prims_in++;
}
int oracle_scene_add_light(void* s, const pbrt_light_desc* d) {
    orc_scene* sc = (orc_scene*)s;
    sc->lights[sc->n_lights] = *d;
    return sc->n_lights++;
}
void oracle_scene_set_camera_film(void* s, const pbrt_camera_desc* c, const pbrt_film_desc* f) {
    orc_scene* sc = (orc_scene*)s;
    sc->camera = *c; sc->film = *f;
}
int oracle_scene_finalize(void* s, int max_prims) { return orc_scene_finalize((orc_scene*)s, max_prims); }
void oracle_scene_desc(void* s, pbrt_scene_desc* out) { orc_scene_desc((orc_scene*)s, out); }
void oracle_scene_order(void* s, int32_t* out) {
    orc_scene* sc = (orc_scene*)s;
    for (int i = 0; i < sc->n_prims_in; i++) out[i] = sc->order[i];
}
void oracle_scene_free(void* s) { orc_scene_free((orc_scene*)s); }

/* ---------------------------------------------------------------- render */
int oracle_render(const pbrt_scene_desc* sc, const pbrt_render_desc* rd, int n_threads, int flags,
                  double* film_xyz, orc_stats* stats) {
    return orc_render(sc, rd, n_threads, flags, film_xyz, stats);
}
int64_t oracle_num_tiles(const pbrt_scene_desc* sc, const pbrt_render_desc* rd) { return orc_num_tiles(sc, rd); }
int oracle_tile_draws(const pbrt_scene_desc* sc, const pbrt_render_desc* rd, int64_t tile, int64_t* out) {
    return orc_tile_draws(sc, rd, tile, out);
}
int oracle_intersect(const pbrt_scene_desc* sc, const double* rays, size_t n, int closest, double* out) {
    return orc_intersect(sc, rays, n, closest, out);
}
void oracle_light_distribution(const pbrt_scene_desc* sc, const pbrt_render_desc* rd, pbrt_distribution_desc* d) {
    orc_light_distribution(sc, rd, d);
}
/* the integrators on caller rays (oracle_render.h): the layouts are orc_path_li's and orc_direct_li's */
int oracle_path_li(const pbrt_scene_desc* sc, int max_depth, int light_strategy, double rr_threshold, size_t n,
                   const double* rays, const uint64_t* state, const uint64_t* inc, const double* start_f,
                   const int32_t* start_i, int k, double* out_f, uint64_t* out_state, int32_t* out_i) {
    return orc_path_li(sc, max_depth, light_strategy, rr_threshold, n, rays, state, inc, start_f, start_i, k, out_f,
                       out_state, out_i);
}
int oracle_direct_li(const pbrt_scene_desc* sc, int max_depth, int dl_strategy, size_t n, const double* rays,
                     const uint64_t* state, const uint64_t* inc, double* out_L, uint64_t* out_state, int32_t* out_i) {
    return orc_direct_li(sc, max_depth, dl_strategy, n, rays, state, inc, out_L, out_state, out_i);
}

/* interaction.go:91-102 SpawnRayToInteraction: in p0 perr0 n0 p1 perr1 n1; out o d tmax */
void oracle_spawn_ray_to(const double in[18], double out[7]) {
    v3 p0 = V3(in[0], in[1], in[2]), e0 = V3(in[3], in[4], in[5]), n0 = V3(in[6], in[7], in[8]);
    v3 p1 = V3(in[9], in[10], in[11]), e1 = V3(in[12], in[13], in[14]), n1 = V3(in[15], in[16], in[17]);
    v3 origin = offset_ray_origin(p0, e0, n0, v_sub(p1, p0));
    v3 target = offset_ray_origin(p1, e1, n1, v_sub(origin, p1));
    v3 d = v_sub(target, origin);
    out[0] = p0.x; out[1] = p0.y; out[2] = p0.z;
    out[3] = d.x; out[4] = d.y; out[5] = d.z;
    out[6] = 1 - 0.0001;
}

/* ------------------------------------------------ triangle extension (mesh) */
/* oracle_mesh.c orc_triangle_hit: ray = o[3] d[3] tmax; out = t, b0, b1, b2 */
#include "oracle_mesh.h"
int oracle_triangle_hit(const double v[9], const double ray[7], double out[4]) {
    ray_t r;
    r.o = V3(ray[0], ray[1], ray[2]);
    r.d = V3(ray[3], ray[4], ray[5]);
    r.tmax = ray[6];
    r.time = 0;
    return orc_triangle_hit(v, &r, &out[0], &out[1], &out[2], &out[3]);
}
/* (input triangles, triangles kept in the oracle's tree) of the scene's meshes */
void oracle_mesh_counts(const pbrt_scene_desc* sc, int64_t out[2]) { orc_mesh_counts(orc_mesh_get(sc), out); }
/* the same test of one ray against n triangles (brute force, no accelerator):
 * hit[i] and, where hit, t[i]; returns the number of hits */
int64_t oracle_triangle_hits(const double* v, int64_t n, const double ray[7], uint8_t* hit, double* t) {
    ray_t r;
    r.o = V3(ray[0], ray[1], ray[2]);
    r.d = V3(ray[3], ray[4], ray[5]);
    r.tmax = ray[6];
    r.time = 0;
    int64_t count = 0;
    for (int64_t i = 0; i < n; i++) {
        double b0, b1, b2;
        t[i] = 0;
        hit[i] = (uint8_t)orc_triangle_hit(v + 9 * i, &r, &t[i], &b0, &b1, &b2);
        count += hit[i];
    }
    return count;
}

/* ---------------------------------- pkg/geometry/xyz_test.go, spectrum_test.go */
#include "../include/pbrt_diag.h"
/* the oracle's XYZFloat64 (xyz.go:424-614) and Spectrum (spectrum.go:35-233)
 * operations, op codes of include/pbrt_diag.h */
int oracle_vec_op(int op, const double* a, const double* b, double s, double* out) {
    v3 x = V3(a[0], a[1], a[2]), y = b ? V3(b[0], b[1], b[2]) : V3(0, 0, 0), r = V3(0, 0, 0);
    spec p = S3(a[0], a[1], a[2]), q = b ? S3(b[0], b[1], b[2]) : S3(0, 0, 0), t = S3(0, 0, 0);
    int vec = 1, sp = 0;
    double sc = 0;
    switch (op) {
        case PBRT_VOP_ABS: r = v_abs(x); break;
        case PBRT_VOP_ABSDOT: sc = v_absdot(x, y); vec = 0; break;
        case PBRT_VOP_ADD: r = v_add(x, y); break;
        case PBRT_VOP_CROSS: r = v_cross(x, y); break;
        case PBRT_VOP_DISTANCE: sc = v_dist(x, y); vec = 0; break;
        case PBRT_VOP_DISTANCE_SQUARED: sc = v_dist2(x, y); vec = 0; break;
        case PBRT_VOP_DIV: r = v_divv(x, y); break;
        case PBRT_VOP_DIV_SCALAR: r = v_divs(x, s); break;
        case PBRT_VOP_DOT: sc = v_dot(x, y); vec = 0; break;
        case PBRT_VOP_LENGTH: sc = v_len(x); vec = 0; break;
        case PBRT_VOP_LENGTH_SQUARED: sc = v_len2(x); vec = 0; break;
        case PBRT_VOP_MUL: r = v_mul(x, y); break;
        case PBRT_VOP_MUL_SCALAR: r = v_muls(x, s); break;
        case PBRT_VOP_NORMALIZED: r = v_normalized(x); break;
        case PBRT_VOP_SUB: r = v_sub(x, y); break;
        case PBRT_SOP_ADD: t = s_add(p, q); sp = 1; break;
        case PBRT_SOP_MUL: t = s_mul(p, q); sp = 1; break;
        case PBRT_SOP_DIV_SCALAR: t = s_divs(p, s); sp = 1; break;
        case PBRT_SOP_MUL_SCALAR: t = s_muls(p, s); sp = 1; break;
        case PBRT_SOP_IS_BLACK: sc = s_is_black(p); vec = 0; break;
        default: return 1;
    }
    if (sp) { out[0] = t.c[0]; out[1] = t.c[1]; out[2] = t.c[2]; }
    else if (vec) { out[0] = r.x; out[1] = r.y; out[2] = r.z; }
    else { out[0] = sc; out[1] = out[2] = 0; }
    return 0;
}

int64_t orc_partition_at_x(int32_t* prim, double* cx, int64_t n, int64_t start, int64_t end, int64_t pivot);
int64_t oracle_partition_at(int32_t* prim, double* cx, int64_t n, int64_t start, int64_t end, int64_t pivot) {
    return orc_partition_at_x(prim, cx, n, start, end, pivot);
}

// Package pbrtgpu is the cgo binding a go-pbrt maintainer adds to call the
// MI355X hot path (include/pbrt_gpu.h, include/pbrt_scene.h) from Go.
//
// It replaces, frame-granular:
//   - pbrt.Render / renderWorker (pkg/pbrt/integrator.go:228-350) with
//     Renderer.RenderFrame (Path.Li and DirectLighting.Li run on the device);
//   - (*accelerator.BVH).Intersect / IntersectP (pkg/accelerator/bvh.go:659-765)
//     with Renderer.Intersect / IntersectP over ray batches, and with
//     IntersectDevice / IntersectPDevice / CameraRaysDevice over DeviceBuffers
//     for rays and results that stay on the device;
//   - Film.WriteImage's pixel conversion (pkg/pbrt/film.go:142-179) with FilmToRGBA.
//
// The reference's constructors (internal/render/server.go:32-164) keep their
// parameters in unexported fields, so a scene is described through the
// SceneBuilder below, which mirrors them one call each.
//
// No Go toolchain exists in the build image of this repository: this file is
// not compiled here. tests/test_go_shim.py compiles its cgo preamble and every
// C identifier it uses against the headers with gcc.
package pbrtgpu

// #cgo CFLAGS: -I${SRCDIR}/../../../include
// #cgo LDFLAGS: -L${SRCDIR}/../../../go-pbrt_amd/lib -lpbrt_gpu -Wl,-rpath,${SRCDIR}/../../../go-pbrt_amd/lib
// #include <stdlib.h>
// #include "pbrt_gpu.h"
// #include "pbrt_scene.h"
import "C"

import (
	"context"
	"fmt"
	"image"
	"unsafe"
)

// ---------------------------------------------------------------- scenes

// SceneBuilder records a scene as server.go builds it (pbrt_sb_*).
type SceneBuilder struct {
	b    *C.pbrt_scene_builder
	desc *C.pbrt_scene_desc
}

// Transform is pbrt.Transform (transform.go:144): matrix and inverse.
type Transform = C.pbrt_transform

func NewSceneBuilder() *SceneBuilder { return &SceneBuilder{b: C.pbrt_sb_create()} }

// ReadmeScene is internal/render/server.go:32-164 at w x h.
func ReadmeScene(w, h int64) (*SceneBuilder, error) {
	var b *C.pbrt_scene_builder
	if rc := C.pbrt_scene_readme(C.int64_t(w), C.int64_t(h), &b); rc != C.PBRT_OK {
		return nil, fmt.Errorf("pbrt_scene_readme: status %d", int(rc))
	}
	return &SceneBuilder{b: b}, nil
}

func Translate(x, y, z float64) Transform {
	var t Transform
	C.pbrt_translate(C.double(x), C.double(y), C.double(z), &t)
	return t
}

func RotateX(deg float64) Transform {
	var t Transform
	C.pbrt_rotate_x(C.double(deg), &t)
	return t
}

func Mul(a, b Transform) Transform {
	var t Transform
	C.pbrt_transform_mul(&a, &b, &t)
	return t
}

func d3(v [3]float64) *C.double { return (*C.double)(unsafe.Pointer(&v[0])) }

// AddSphere is pbrt.NewSphereShape (sphere.go:19-35); returns the shape index.
func (s *SceneBuilder) AddSphere(o2w Transform, reverse bool, radius, zMin, zMax, phiMax float64) int {
	var sd C.pbrt_shape_desc
	rev := C.int(0)
	if reverse {
		rev = 1
	}
	C.pbrt_make_sphere(&o2w, rev, C.double(radius), C.double(zMin), C.double(zMax), C.double(phiMax), &sd)
	return int(C.pbrt_sb_add_shape(s.b, &sd))
}

// AddDisk is shapes.NewDisk (pkg/shapes/disk.go:22-35).
func (s *SceneBuilder) AddDisk(o2w Transform, height, radius, inner, phiMax float64) int {
	var sd C.pbrt_shape_desc
	C.pbrt_make_disk(&o2w, C.double(height), C.double(radius), C.double(inner), C.double(phiMax), &sd)
	return int(C.pbrt_sb_add_shape(s.b, &sd))
}

// AddMatte is materials.NewMatteMaterial with a constant Kd (sigma > 0: OrenNayar).
func (s *SceneBuilder) AddMatte(kd [3]float64, sigma float64) int {
	var m C.pbrt_material_desc
	C.pbrt_make_matte_constant(C.double(kd[0]), C.double(kd[1]), C.double(kd[2]), C.double(sigma), &m)
	return int(C.pbrt_sb_add_material(s.b, &m))
}

// AddCheckerMatte is NewMatteMaterial(textures.NewCheckerboard2D(NewPlanarMapping2D(vs, vt, ds, dt), tex1, tex2)).
func (s *SceneBuilder) AddCheckerMatte(vs, vt [3]float64, ds, dt float64, tex1, tex2 [3]float64, sigma float64) int {
	var m C.pbrt_material_desc
	C.pbrt_make_matte_checkerboard(d3(vs), d3(vt), C.double(ds), C.double(dt), d3(tex1), d3(tex2), C.double(sigma), &m)
	return int(C.pbrt_sb_add_material(s.b, &m))
}

// AddMirror is materials.NewMirror (mirror.go:9-14) with Kr.
func (s *SceneBuilder) AddMirror(kr [3]float64) int {
	var m C.pbrt_material_desc
	C.pbrt_make_mirror(d3(kr), &m)
	return int(C.pbrt_sb_add_material(s.b, &m))
}

// AddGlass is materials.NewGlass (glass.go:15-26) with constant textures.
func (s *SceneBuilder) AddGlass(kr, kt [3]float64, uRough, vRough, eta float64) int {
	var m C.pbrt_material_desc
	C.pbrt_make_glass(d3(kr), d3(kt), C.double(uRough), C.double(vRough), C.double(eta), &m)
	return int(C.pbrt_sb_add_material(s.b, &m))
}

// AddPrimitive is NewGeometricPrimitive, wrapped in NewTransformedPrimitive when
// primToWorld is non-nil (primitive.go:22-129).
func (s *SceneBuilder) AddPrimitive(shape, material int, primToWorld *Transform) int {
	var p C.pbrt_primitive_desc
	p.shape = C.int32_t(shape)
	p.material = C.int32_t(material)
	p.kind = C.PBRT_PRIM_GEOMETRIC
	if primToWorld != nil {
		p.kind = C.PBRT_PRIM_TRANSFORMED
		p.prim_to_world = *primToWorld
	}
	return int(C.pbrt_sb_add_primitive(s.b, &p))
}

// AddPointLight is lights.NewPointLight (point.go:19-30).
func (s *SceneBuilder) AddPointLight(l2w Transform, I [3]float64) int {
	var l C.pbrt_light_desc
	C.pbrt_make_point_light(&l2w, d3(I), &l)
	return int(C.pbrt_sb_add_light(s.b, &l))
}

// AddDistantLight is lights.NewDistantLight (distant.go:19-34).
func (s *SceneBuilder) AddDistantLight(l2w Transform, L, w [3]float64) int {
	var l C.pbrt_light_desc
	C.pbrt_make_distant_light(&l2w, d3(L), d3(w), &l)
	return int(C.pbrt_sb_add_light(s.b, &l))
}

// AddAreaLight is lights.NewDiffuseAreaLight (diffuse.go:19-34) over a sphere shape.
func (s *SceneBuilder) AddAreaLight(Lemit [3]float64, shape int, twoSided bool) int {
	var l C.pbrt_light_desc
	ts := C.int(0)
	if twoSided {
		ts = 1
	}
	C.pbrt_make_diffuse_area_light(d3(Lemit), C.int(shape), ts, &l)
	return int(C.pbrt_sb_add_light(s.b, &l))
}

// Build is accelerator.NewBVH(prims, maxPrimsInNode, SplitSAH) + pbrt.NewScene.
func (s *SceneBuilder) Build(maxPrimsInNode int) error {
	var d *C.pbrt_scene_desc
	if rc := C.pbrt_sb_build(s.b, C.int(maxPrimsInNode), &d); rc != C.PBRT_OK {
		return fmt.Errorf("pbrt_sb_build: status %d", int(rc))
	}
	s.desc = d
	return nil
}

func (s *SceneBuilder) Close() { C.pbrt_sb_destroy(s.b) }

// ------------------------------------------------------------- rendering

// PathDesc is integrator.NewPath(maxDepth, camera, sampler, ...) with
// sampler.NewStratified(xs, ys, jitter, nDims) (server.go:142-164).
func PathDesc(xs, ys int32, jitter bool, nDims, maxDepth int32, rrThreshold float64, strategy int32) C.pbrt_render_desc {
	var rd C.pbrt_render_desc
	rd.sampler_x, rd.sampler_y, rd.n_dims = C.int32_t(xs), C.int32_t(ys), C.int32_t(nDims)
	if jitter {
		rd.jitter = 1
	}
	rd.integrator = C.PBRT_INTEGRATOR_PATH
	rd.max_depth = C.int32_t(maxDepth)
	rd.rr_threshold = C.double(rrThreshold)
	rd.light_strategy = C.int32_t(strategy)
	rd.tile_size = 16
	rd.mode = C.PBRT_MODE_EXACT
	return rd
}

// DirectLightingDesc is integrator.NewDirectLighting(strategy, maxDepth, camera,
// sampler, ...) with sampler.NewStratified(xs, ys, jitter, nDims); strategy is
// integrator.UniformSampleAll (1) or UniformSampleOne (2), PBRT_DL_*'s values.
func DirectLightingDesc(xs, ys int32, jitter bool, nDims, maxDepth, strategy int32) C.pbrt_render_desc {
	rd := PathDesc(xs, ys, jitter, nDims, maxDepth, 1, C.PBRT_LIGHT_STRATEGY_UNIFORM)
	rd.integrator = C.PBRT_INTEGRATOR_DIRECT_LIGHTING
	rd.dl_strategy = C.int32_t(strategy)
	return rd
}

// WithRandomSampler switches rd to sampler.NewRandomSampler(ns, seed) (random.go:12-57).
func WithRandomSampler(rd *C.pbrt_render_desc, ns int32) { C.pbrt_random_sampler(C.int32_t(ns), rd) }

// Renderer owns a device-resident scene (one per GPU).
type Renderer struct {
	ctx  *C.pbrt_gpu_ctx
	w, h int // CroppedPixelBounds extent of the scene's film
	bufs map[*DeviceBuffer]struct{} // its open device buffers (NewDeviceBuffer)
}

// Kernel requests (pbrt_gpu_opts.kernel). KernelAuto picks per render;
// KernelWaveCam opts renders with per-sample camera rays (WithRandomSampler,
// nDims 0, or nDims 1 with a thin lens; Path, Matte scenes) into the wave
// pipeline, which KernelAuto keeps on the serial kernel.
const (
	KernelAuto    = int32(C.PBRT_KERNEL_AUTO)
	KernelWaveCam = int32(C.PBRT_KERNEL_WAVE_CAM)
)

func NewRenderer(s *SceneBuilder, device int) (*Renderer, error) {
	return NewRendererKernel(s, device, KernelAuto)
}

// NewRendererKernel is NewRenderer with a kernel request (Kernel*).
func NewRendererKernel(s *SceneBuilder, device int, kernel int32) (*Renderer, error) {
	if s.desc == nil {
		return nil, fmt.Errorf("pbrtgpu: scene not built")
	}
	var opts C.pbrt_gpu_opts
	opts.device = C.int32_t(device)
	opts.kernel = C.int32_t(kernel)
	var ctx *C.pbrt_gpu_ctx
	if rc := C.pbrt_gpu_create(s.desc, &opts, &ctx); rc != C.PBRT_OK {
		return nil, fmt.Errorf("pbrt_gpu_create: status %d", int(rc))
	}
	f := s.desc.film
	return &Renderer{ctx: ctx, w: int(f.crop_max_x - f.crop_min_x), h: int(f.crop_max_y - f.crop_min_y)}, nil
}

// RenderFrame is pbrt.Render for one frame: film receives the merged XYZ sums
// Film.MergeFilmTile would hold, row-major W*H*3 float64. ctx cancellation maps
// to pbrt_gpu_cancel, as errgroup cancels the CPU workers (integrator.go:305-345).
func (r *Renderer) RenderFrame(ctx context.Context, rd *C.pbrt_render_desc, film []float64) error {
	if len(film) < r.w*r.h*3 || len(film) == 0 {
		return fmt.Errorf("pbrtgpu: film holds %d values, the frame needs %d", len(film), r.w*r.h*3)
	}
	if err := ctx.Err(); err != nil {
		return err
	}
	// pbrt_gpu_cancel acts on the render in flight only: a cancel that lands
	// before the render starts or after it ends is a no-op (include/pbrt_gpu.h)
	// The watcher is joined before RenderFrame returns: a cancel racing the end
	// of the render must not reach pbrt_gpu_cancel after the caller's Close
	// (pbrt_gpu_destroy frees the context the cancel locks).
	// a context cancelled before the frame starts renders nothing (the
	// reference's tile producer returns gtx.Err(), integrator.go:333-336)
	if err := ctx.Err(); err != nil {
		return err
	}
	done := make(chan struct{})
	exited := make(chan struct{})
	go func() {
		defer close(exited)
		select {
		case <-ctx.Done():
			C.pbrt_gpu_cancel(r.ctx)
		case <-done:
		}
	}()
	var st C.pbrt_gpu_stats
	rc := C.pbrt_gpu_render(r.ctx, rd, (*C.double)(unsafe.Pointer(&film[0])), &st)
	close(done)
	<-exited
	switch rc {
	case C.PBRT_OK:
		// the frame is complete: a cancel that reached the device while the
		// render was in flight returns PBRT_E_CANCELLED instead, and one that
		// came after the last kernel (or in the instant before the render was
		// in flight) leaves a valid film, as the reference's g.Wait() returns
		// nil once every tile was handed out (integrator.go:311-347)
		return nil
	case C.PBRT_E_CANCELLED:
		if err := ctx.Err(); err != nil {
			return err
		}
		return context.Canceled
	case C.PBRT_E_REF_PANIC: // the CPU reference panics here; keep that contract
		panic(fmt.Sprintf("go-pbrt panic kind %d at tile %d pixel (%d,%d) sample %d bounce %d",
			int(st.panic_kind), int(st.panic_tile), int64(st.panic_pixel_x), int64(st.panic_pixel_y),
			int(st.panic_sample), int(st.panic_bounce)))
	default:
		return fmt.Errorf("pbrt_gpu_render: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
}

// Intersect is BVH.Intersect over a batch (rays and hits are caller-owned SoA).
func (r *Renderer) Intersect(rays *C.pbrt_ray_soa, n int, hits *C.pbrt_hit_soa) error {
	if rc := C.pbrt_gpu_intersect(r.ctx, rays, C.size_t(n), hits); rc != C.PBRT_OK {
		return fmt.Errorf("pbrt_gpu_intersect: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
	return nil
}

// IntersectP is BVH.IntersectP over a batch; occluded[i] is 0 or 1.
func (r *Renderer) IntersectP(rays *C.pbrt_ray_soa, n int, occluded []uint8) error {
	if n <= 0 {
		return nil
	}
	if len(occluded) < n {
		return fmt.Errorf("pbrtgpu: %d results for %d rays", len(occluded), n)
	}
	if rc := C.pbrt_gpu_intersect_p(r.ctx, rays, C.size_t(n), (*C.uint8_t)(unsafe.Pointer(&occluded[0]))); rc != C.PBRT_OK {
		return fmt.Errorf("pbrt_gpu_intersect_p: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
	return nil
}

// Close destroys the context. Its device buffers go with it (pbrt_gpu_destroy
// frees what is left), so every DeviceBuffer still open is marked closed first
// and can no longer reach the library.
func (r *Renderer) Close() {
	for d := range r.bufs {
		d.b = nil
	}
	r.bufs = nil
	C.pbrt_gpu_destroy(r.ctx)
}

// ---------------------------------------------------- device-resident queries

// DeviceBuffer is pbrt_gpu_buffer: device memory the Renderer's context owns.
// Go cannot allocate on the device, so rays and results that stay there live
// in these. A buffer is closed by Close or by its Renderer's Close, whichever
// comes first; a closed buffer fails every call.
type DeviceBuffer struct {
	r *Renderer
	b *C.pbrt_gpu_buffer
}

func (r *Renderer) NewDeviceBuffer(bytes int) (*DeviceBuffer, error) {
	if bytes <= 0 {
		return nil, fmt.Errorf("pbrtgpu: device buffer of %d bytes", bytes)
	}
	var b *C.pbrt_gpu_buffer
	if rc := C.pbrt_gpu_buffer_create(r.ctx, C.size_t(bytes), &b); rc != C.PBRT_OK {
		return nil, fmt.Errorf("pbrt_gpu_buffer_create: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
	d := &DeviceBuffer{r: r, b: b}
	if r.bufs == nil {
		r.bufs = map[*DeviceBuffer]struct{}{}
	}
	r.bufs[d] = struct{}{}
	return d, nil
}

// Size is the buffer's size in bytes (0 once closed).
func (d *DeviceBuffer) Size() int { return int(C.pbrt_gpu_buffer_size(d.b)) }

func (d *DeviceBuffer) copy(offset int, host unsafe.Pointer, bytes int, up bool) error {
	if d.b == nil {
		return fmt.Errorf("pbrtgpu: device buffer is closed")
	}
	if offset < 0 || bytes < 0 || offset+bytes > d.Size() {
		return fmt.Errorf("pbrtgpu: bytes [%d, %d) outside a buffer of %d", offset, offset+bytes, d.Size())
	}
	rc := C.int(C.PBRT_OK)
	if up {
		rc = C.pbrt_gpu_buffer_upload(d.b, C.size_t(offset), host, C.size_t(bytes))
	} else {
		rc = C.pbrt_gpu_buffer_download(d.b, C.size_t(offset), host, C.size_t(bytes))
	}
	if rc != C.PBRT_OK {
		return fmt.Errorf("pbrt_gpu_buffer copy: %s", C.GoString(C.pbrt_gpu_last_error(d.r.ctx)))
	}
	return nil
}

// Upload copies src to the buffer at byte offset; it returns once src may be reused.
func (d *DeviceBuffer) Upload(offset int, src []float64) error {
	if len(src) == 0 {
		return nil
	}
	return d.copy(offset, unsafe.Pointer(&src[0]), 8*len(src), true)
}

// UploadBytes, DownloadBytes: the same for uint8 (hit flags) or raw int32 data.
func (d *DeviceBuffer) UploadBytes(offset int, src []byte) error {
	if len(src) == 0 {
		return nil
	}
	return d.copy(offset, unsafe.Pointer(&src[0]), len(src), true)
}

// Download fills dst from the buffer at byte offset (synchronises the context's stream).
func (d *DeviceBuffer) Download(offset int, dst []float64) error {
	if len(dst) == 0 {
		return nil
	}
	return d.copy(offset, unsafe.Pointer(&dst[0]), 8*len(dst), false)
}

func (d *DeviceBuffer) DownloadBytes(offset int, dst []byte) error {
	if len(dst) == 0 {
		return nil
	}
	return d.copy(offset, unsafe.Pointer(&dst[0]), len(dst), false)
}

func (d *DeviceBuffer) Close() {
	if d.b == nil {
		return
	}
	delete(d.r.bufs, d)
	C.pbrt_gpu_buffer_destroy(d.b)
	d.b = nil
}

// DeviceRays are the ray arrays of a device query (float64 each); TMax may be
// nil (+Inf on input, not written by CameraRaysDevice).
type DeviceRays struct{ Ox, Oy, Oz, Dx, Dy, Dz, TMax *DeviceBuffer }

// DeviceHits are the outputs of IntersectDevice: Hit (uint8) is required, TMax,
// Point, Normal (float64) and Prim (int32) may be nil.
type DeviceHits struct{ Hit, TMax, Prim, Px, Py, Pz, Nx, Ny, Nz *DeviceBuffer }

// devPtr is the only bounds protection a device query gets: the buffer must be
// open, belong to this Renderer and hold n elements of elem bytes.
func (r *Renderer) devPtr(d *DeviceBuffer, n, elem int, optional bool) (unsafe.Pointer, error) {
	if d == nil {
		if optional {
			return nil, nil
		}
		return nil, fmt.Errorf("pbrtgpu: a required device buffer is nil")
	}
	if d.b == nil || d.r != r {
		return nil, fmt.Errorf("pbrtgpu: device buffer closed or of another Renderer")
	}
	if n < 0 || n > 1<<31-1 || n*elem > d.Size() {
		return nil, fmt.Errorf("pbrtgpu: %d elements of %d bytes in a buffer of %d", n, elem, d.Size())
	}
	return C.pbrt_gpu_buffer_ptr(d.b), nil
}

func (r *Renderer) raySoA(rays DeviceRays, n int) (C.pbrt_ray_soa, error) {
	var soa C.pbrt_ray_soa
	p := [7]unsafe.Pointer{}
	for k, d := range []*DeviceBuffer{rays.Ox, rays.Oy, rays.Oz, rays.Dx, rays.Dy, rays.Dz, rays.TMax} {
		q, err := r.devPtr(d, n, 8, k == 6)
		if err != nil {
			return soa, err
		}
		p[k] = q
	}
	soa.ox, soa.oy, soa.oz = (*C.double)(p[0]), (*C.double)(p[1]), (*C.double)(p[2])
	soa.dx, soa.dy, soa.dz = (*C.double)(p[3]), (*C.double)(p[4]), (*C.double)(p[5])
	soa.tmax = (*C.double)(p[6])
	return soa, nil
}

// IntersectDevice enqueues BVH.Intersect for rays[0:n] on the context's stream
// (pbrt_gpu_intersect_device): nothing is copied or waited for. Results are
// valid after QueryStatus or a Download.
func (r *Renderer) IntersectDevice(rays DeviceRays, n int, hits DeviceHits) error {
	soa, err := r.raySoA(rays, n)
	if err != nil {
		return err
	}
	var hs C.pbrt_hit_soa
	p := [9]unsafe.Pointer{}
	elem := [9]int{1, 8, 4, 8, 8, 8, 8, 8, 8}
	for k, d := range []*DeviceBuffer{hits.Hit, hits.TMax, hits.Prim, hits.Px, hits.Py, hits.Pz, hits.Nx, hits.Ny, hits.Nz} {
		if p[k], err = r.devPtr(d, n, elem[k], k > 0); err != nil {
			return err
		}
	}
	hs.hit, hs.t_max, hs.prim = (*C.uint8_t)(p[0]), (*C.double)(p[1]), (*C.int32_t)(p[2])
	hs.px, hs.py, hs.pz = (*C.double)(p[3]), (*C.double)(p[4]), (*C.double)(p[5])
	hs.nx, hs.ny, hs.nz = (*C.double)(p[6]), (*C.double)(p[7]), (*C.double)(p[8])
	if rc := C.pbrt_gpu_intersect_device(r.ctx, &soa, C.size_t(n), &hs); rc != C.PBRT_OK {
		return fmt.Errorf("pbrt_gpu_intersect_device: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
	return nil
}

// IntersectPDevice is BVH.IntersectP the same way; occluded holds n uint8.
func (r *Renderer) IntersectPDevice(rays DeviceRays, n int, occluded *DeviceBuffer) error {
	soa, err := r.raySoA(rays, n)
	if err != nil {
		return err
	}
	occ, err := r.devPtr(occluded, n, 1, false)
	if err != nil {
		return err
	}
	if rc := C.pbrt_gpu_intersect_p_device(r.ctx, &soa, C.size_t(n), (*C.uint8_t)(occ)); rc != C.PBRT_OK {
		return fmt.Errorf("pbrt_gpu_intersect_p_device: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
	return nil
}

// DeviceRNG holds the PCG32 stream of each ray of a LiDevice batch: State and Inc,
// uint64 each.
type DeviceRNG struct{ State, Inc *DeviceBuffer }

// DeviceRadiance are the outputs of LiDevice: R, G, B (float64) are required;
// State (uint64: the ray's stream after its path), Draws (uint32: the PCG32 draws
// the path consumed) and Rays (uint32: closest | shadow << 16) may be nil.
type DeviceRadiance struct{ R, G, B, State, Draws, Rays *DeviceBuffer }

// LiDevice enqueues Path.Li(ray, scene, sampler, 0) for rays[0:n] on the
// context's stream (pbrt_gpu_li_device): ray i samples with a RandomSampler on the
// stream (State[i], Inc[i]). Nothing is copied or waited for; results are valid
// after QueryStatus or a Download. A ray on which the reference panics has L = 0
// and is counted in QueryStatus' record. DirectLighting, maxDepth > 2048 and
// rough glass are refused with the reason.
func (r *Renderer) LiDevice(rays DeviceRays, rng DeviceRNG, n int, maxDepth int32, rrThreshold float64,
	strategy int32, out DeviceRadiance) error {
	soa, gs, rs, err := r.liSoAs(rays, rng, n, out)
	if err != nil {
		return err
	}
	ld := liDesc(maxDepth, rrThreshold, strategy)
	if rc := C.pbrt_gpu_li_device(r.ctx, &ld, &soa, &gs, C.size_t(n), &rs); rc != C.PBRT_OK {
		return fmt.Errorf("pbrt_gpu_li_device: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
	return nil
}

// liSoAs are the ray, rng and radiance structs of a Li query over buffers checked to hold n elements.
func (r *Renderer) liSoAs(rays DeviceRays, rng DeviceRNG, n int, out DeviceRadiance) (C.pbrt_ray_soa, C.pbrt_rng_soa,
	C.pbrt_radiance_soa, error) {
	var gs C.pbrt_rng_soa
	var rs C.pbrt_radiance_soa
	soa, err := r.raySoA(rays, n)
	if err != nil {
		return soa, gs, rs, err
	}
	p := [8]unsafe.Pointer{}
	elem := [8]int{8, 8, 8, 8, 8, 8, 4, 4}
	for k, d := range []*DeviceBuffer{rng.State, rng.Inc, out.R, out.G, out.B, out.State, out.Draws, out.Rays} {
		if p[k], err = r.devPtr(d, n, elem[k], k > 4); err != nil {
			return soa, gs, rs, err
		}
	}
	gs.state, gs.inc = (*C.uint64_t)(p[0]), (*C.uint64_t)(p[1])
	rs.r, rs.g, rs.b = (*C.double)(p[2]), (*C.double)(p[3]), (*C.double)(p[4])
	rs.state, rs.draws, rs.rays = (*C.uint64_t)(p[5]), (*C.uint32_t)(p[6]), (*C.uint32_t)(p[7])
	return soa, gs, rs, nil
}

func liDesc(maxDepth int32, rrThreshold float64, strategy int32) C.pbrt_li_desc {
	var ld C.pbrt_li_desc
	ld.integrator, ld.max_depth = C.PBRT_INTEGRATOR_PATH, C.int32_t(maxDepth)
	ld.light_strategy, ld.reserved = C.int32_t(strategy), 0
	ld.rr_threshold = C.double(rrThreshold)
	return ld
}

// LiStratifiedDevice is LiDevice under the stratified sampler
// (pbrt_gpu_li_stratified_device): ray i samples with a PixelSampler whose tables
// are strat.S1D[strat.Table[i]] (nTables tables of nDims * spp values), at sample
// strat.K[i], with its cursors at (first1D, first2D), on the stream (State[i],
// Inc[i]). Draws counts PCG32 draws only. Table and K are clamped on the device:
// an out-of-range value gives that ray an unspecified radiance and touches no
// other. With nDims 0 strat may be empty, and the call is LiDevice.
func (r *Renderer) LiStratifiedDevice(rays DeviceRays, rng DeviceRNG, n int, maxDepth int32, rrThreshold float64,
	strategy int32, out DeviceRadiance, strat DeviceStrat, nTables, spp, nDims, first1D, first2D int32) error {
	soa, gs, rs, err := r.liSoAs(rays, rng, n, out)
	if err != nil {
		return err
	}
	var st C.pbrt_strat_soa
	if nDims > 0 {
		if nTables < 1 || spp < 1 {
			return fmt.Errorf("pbrtgpu: LiStratifiedDevice: nTables and spp must be >= 1")
		}
		p := [3]unsafe.Pointer{}
		if p[0], err = r.devPtr(strat.S1D, int(nTables)*int(nDims)*int(spp), 8, false); err != nil {
			return err
		}
		for k, d := range []*DeviceBuffer{strat.Table, strat.K} {
			if p[1+k], err = r.devPtr(d, n, 4, false); err != nil {
				return err
			}
		}
		st.s1d, st.table, st.k = (*C.double)(p[0]), (*C.int32_t)(p[1]), (*C.int32_t)(p[2])
	}
	st.n_tables, st.spp, st.n_dims = C.int32_t(nTables), C.int32_t(spp), C.int32_t(nDims)
	st.first_1d, st.first_2d, st.reserved = C.int32_t(first1D), C.int32_t(first2D), 0
	ld := liDesc(maxDepth, rrThreshold, strategy)
	if rc := C.pbrt_gpu_li_stratified_device(r.ctx, &ld, &soa, &gs, C.size_t(n), &rs, &st); rc != C.PBRT_OK {
		return fmt.Errorf("pbrt_gpu_li_stratified_device: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
	return nil
}

// DirectLiDevice enqueues DirectLighting.Li(ray, scene, sampler, 0) for rays[0:n]
// on the context's stream (pbrt_gpu_direct_li_device), with LiDevice's buffers and
// outputs: ray i samples with a RandomSampler on the stream (State[i], Inc[i]).
// strategy is PBRT_DL_UNIFORM_SAMPLE_ALL (1) or PBRT_DL_UNIFORM_SAMPLE_ONE (2).
// A ray on which the reference panics (UniformSampleOneLight's "> 10" included)
// has L = 0 and is counted in QueryStatus' record. An unknown strategy, rough
// glass and maxDepth > 64 on a scene with Mirror / Glass / OrenNayar materials are
// refused with the reason.
func (r *Renderer) DirectLiDevice(rays DeviceRays, rng DeviceRNG, n int, maxDepth int32, strategy int32,
	out DeviceRadiance) error {
	soa, err := r.raySoA(rays, n)
	if err != nil {
		return err
	}
	var gs C.pbrt_rng_soa
	var rs C.pbrt_radiance_soa
	p := [8]unsafe.Pointer{}
	elem := [8]int{8, 8, 8, 8, 8, 8, 4, 4}
	for k, d := range []*DeviceBuffer{rng.State, rng.Inc, out.R, out.G, out.B, out.State, out.Draws, out.Rays} {
		if p[k], err = r.devPtr(d, n, elem[k], k > 4); err != nil {
			return err
		}
	}
	gs.state, gs.inc = (*C.uint64_t)(p[0]), (*C.uint64_t)(p[1])
	rs.r, rs.g, rs.b = (*C.double)(p[2]), (*C.double)(p[3]), (*C.double)(p[4])
	rs.state, rs.draws, rs.rays = (*C.uint64_t)(p[5]), (*C.uint32_t)(p[6]), (*C.uint32_t)(p[7])
	var dd C.pbrt_direct_li_desc // (reserved stays zero)
	dd.max_depth, dd.dl_strategy = C.int32_t(maxDepth), C.int32_t(strategy)
	if rc := C.pbrt_gpu_direct_li_device(r.ctx, &dd, &soa, &gs, C.size_t(n), &rs); rc != C.PBRT_OK {
		return fmt.Errorf("pbrt_gpu_direct_li_device: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
	return nil
}

// Path statuses of DevicePaths.Status (PBRT_PATH_*): a zero-filled array is not live.
const (
	PathUnused   = uint8(C.PBRT_PATH_UNUSED)
	PathAlive    = uint8(C.PBRT_PATH_ALIVE)
	PathEnded    = uint8(C.PBRT_PATH_ENDED)
	PathPanicked = uint8(C.PBRT_PATH_PANICKED)
)

// DevicePaths is the loop-carried state of Path.Li per path (pbrt_path_soa), 141
// bytes a path (133 without TMax): the next ray (float64; TMax may be nil: +Inf),
// the radiance sum Lr/Lg/Lb, the throughput Br/Bg/Bb and EtaScale (float64), the
// PCG32 stream State and Inc (uint64), Draws and Rays (uint32: closest | shadow <<
// 16), Bounces (int32) and Status (uint8).
type DevicePaths struct {
	Ox, Oy, Oz, Dx, Dy, Dz, TMax             *DeviceBuffer
	Lr, Lg, Lb, Br, Bg, Bb, EtaScale         *DeviceBuffer
	State, Inc, Draws, Rays, Bounces, Status *DeviceBuffer
}

// DevicePathQueue names paths by index (pbrt_path_queue): Index holds n int32,
// Count one uint32, both on the device.
type DevicePathQueue struct{ Index, Count *DeviceBuffer }

// DevicePathStep is what a step surfaces at the index of each path it advanced
// (pbrt_path_step_soa); every buffer may be nil: the iteration's closest hit,
// the hit's material index (int32, -1 on a miss) and the term added to L (float64).
type DevicePathStep struct {
	Hit        DeviceHits
	Material   *DeviceBuffer
	Ar, Ag, Ab *DeviceBuffer
}

func (r *Renderer) pathSoA(paths DevicePaths, n int) (C.pbrt_path_soa, error) {
	var ps C.pbrt_path_soa
	p := [20]unsafe.Pointer{}
	elem := [20]int{8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 4, 4, 4, 1}
	var err error
	for k, d := range []*DeviceBuffer{paths.Ox, paths.Oy, paths.Oz, paths.Dx, paths.Dy, paths.Dz, paths.TMax,
		paths.Lr, paths.Lg, paths.Lb, paths.Br, paths.Bg, paths.Bb, paths.EtaScale,
		paths.State, paths.Inc, paths.Draws, paths.Rays, paths.Bounces, paths.Status} {
		if p[k], err = r.devPtr(d, n, elem[k], k == 6); err != nil {
			return ps, err
		}
	}
	ps.ox, ps.oy, ps.oz = (*C.double)(p[0]), (*C.double)(p[1]), (*C.double)(p[2])
	ps.dx, ps.dy, ps.dz = (*C.double)(p[3]), (*C.double)(p[4]), (*C.double)(p[5])
	ps.tmax = (*C.double)(p[6])
	ps.lr, ps.lg, ps.lb = (*C.double)(p[7]), (*C.double)(p[8]), (*C.double)(p[9])
	ps.br, ps.bg, ps.bb = (*C.double)(p[10]), (*C.double)(p[11]), (*C.double)(p[12])
	ps.eta_scale = (*C.double)(p[13])
	ps.state, ps.inc = (*C.uint64_t)(p[14]), (*C.uint64_t)(p[15])
	ps.draws, ps.rays = (*C.uint32_t)(p[16]), (*C.uint32_t)(p[17])
	ps.bounces, ps.status = (*C.int32_t)(p[18]), (*C.uint8_t)(p[19])
	return ps, nil
}

// PathBeginDevice enqueues the fresh state of n paths (pbrt_gpu_path_begin_device):
// L 0, beta 1, EtaScale 1, no bounce, draw or ray, PathAlive, the ray and the
// stream copied from LiDevice's rays and rng.
func (r *Renderer) PathBeginDevice(rays DeviceRays, rng DeviceRNG, n int, paths DevicePaths) error {
	soa, err := r.raySoA(rays, n)
	if err != nil {
		return err
	}
	var gs C.pbrt_rng_soa
	st, err := r.devPtr(rng.State, n, 8, false)
	if err != nil {
		return err
	}
	inc, err := r.devPtr(rng.Inc, n, 8, false)
	if err != nil {
		return err
	}
	gs.state, gs.inc = (*C.uint64_t)(st), (*C.uint64_t)(inc)
	ps, err := r.pathSoA(paths, n)
	if err != nil {
		return err
	}
	if rc := C.pbrt_gpu_path_begin_device(r.ctx, &soa, &gs, C.size_t(n), &ps); rc != C.PBRT_OK {
		return fmt.Errorf("pbrt_gpu_path_begin_device: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
	return nil
}

func (r *Renderer) pathQueue(q *DevicePathQueue, n int) (C.pbrt_path_queue, error) {
	var pq C.pbrt_path_queue
	idx, err := r.devPtr(q.Index, n, 4, false)
	if err != nil {
		return pq, err
	}
	cnt, err := r.devPtr(q.Count, 1, 4, false)
	if err != nil {
		return pq, err
	}
	pq.index, pq.count = (*C.int32_t)(idx), (*C.uint32_t)(cnt)
	return pq, nil
}

// PathStepDevice enqueues one iteration of Path.Li's loop for every PathAlive
// path the call covers (pbrt_gpu_path_step_device): paths 0 .. n-1 when in is
// nil, else those in names (its count is read on the device). The paths that are
// alive afterwards are appended to out (nil: no queue; its count is zeroed
// first). step may be nil. After PathBeginDevice and maxDepth steps every path
// has ended and Lr/Lg/Lb, State, Draws and Rays are LiDevice's outputs, bit for
// bit. A path on which the reference panics is PathPanicked with L = 0 and counted
// in QueryStatus' record. LiDevice's refusals apply; in and out must not alias.
func (r *Renderer) PathStepDevice(paths DevicePaths, in, out *DevicePathQueue, n int, maxDepth int32,
	rrThreshold float64, strategy int32, step *DevicePathStep) error {
	ps, err := r.pathSoA(paths, n)
	if err != nil {
		return err
	}
	var qi, qo C.pbrt_path_queue
	var pi, po *C.pbrt_path_queue
	if in != nil {
		if qi, err = r.pathQueue(in, n); err != nil {
			return err
		}
		pi = &qi
	}
	if out != nil {
		if qo, err = r.pathQueue(out, n); err != nil {
			return err
		}
		po = &qo
	}
	if in != nil && out != nil && (in.Index == out.Index || in.Count == out.Count) {
		return fmt.Errorf("pbrtgpu: the in and out queues alias")
	}
	var ss C.pbrt_path_step_soa
	var pss *C.pbrt_path_step_soa
	if step != nil {
		h := step.Hit
		p := [13]unsafe.Pointer{}
		elem := [13]int{1, 8, 4, 8, 8, 8, 8, 8, 8, 4, 8, 8, 8}
		for k, d := range []*DeviceBuffer{h.Hit, h.TMax, h.Prim, h.Px, h.Py, h.Pz, h.Nx, h.Ny, h.Nz,
			step.Material, step.Ar, step.Ag, step.Ab} {
			if p[k], err = r.devPtr(d, n, elem[k], true); err != nil {
				return err
			}
		}
		var hs C.pbrt_hit_soa
		hs.hit, hs.t_max, hs.prim = (*C.uint8_t)(p[0]), (*C.double)(p[1]), (*C.int32_t)(p[2])
		hs.px, hs.py, hs.pz = (*C.double)(p[3]), (*C.double)(p[4]), (*C.double)(p[5])
		hs.nx, hs.ny, hs.nz = (*C.double)(p[6]), (*C.double)(p[7]), (*C.double)(p[8])
		ss.hit = hs
		ss.material = (*C.int32_t)(p[9])
		ss.ar, ss.ag, ss.ab = (*C.double)(p[10]), (*C.double)(p[11]), (*C.double)(p[12])
		pss = &ss
	}
	var ld C.pbrt_li_desc
	ld.integrator, ld.max_depth = C.PBRT_INTEGRATOR_PATH, C.int32_t(maxDepth)
	ld.light_strategy, ld.reserved = C.int32_t(strategy), 0
	ld.rr_threshold = C.double(rrThreshold)
	if rc := C.pbrt_gpu_path_step_device(r.ctx, &ld, &ps, pi, po, C.size_t(n), pss); rc != C.PBRT_OK {
		return fmt.Errorf("pbrt_gpu_path_step_device: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
	return nil
}

// CameraRaysDevice writes the camera rays of the pixel window [x0, x1) x [y0, y1)
// in raster order (pbrt_gpu_camera_rays_device), pFilm = pixel + filmOffset; an
// IntersectDevice on them needs no host step in between.
func (r *Renderer) CameraRaysDevice(x0, y0, x1, y1 int64, filmOffset, lens [2]float64, timeU float64, rays DeviceRays) error {
	if x0 < 0 || y0 < 0 || x0 >= x1 || y0 >= y1 {
		return fmt.Errorf("pbrtgpu: empty pixel window")
	}
	soa, err := r.raySoA(rays, int((x1-x0)*(y1-y0)))
	if err != nil {
		return err
	}
	var out C.pbrt_ray_soa_out
	out.ox, out.oy, out.oz, out.dx, out.dy, out.dz, out.tmax = soa.ox, soa.oy, soa.oz, soa.dx, soa.dy, soa.dz, soa.tmax
	var cd C.pbrt_camera_rays_desc
	cd.x0, cd.y0, cd.x1, cd.y1 = C.int64_t(x0), C.int64_t(y0), C.int64_t(x1), C.int64_t(y1)
	cd.film_dx, cd.film_dy = C.double(filmOffset[0]), C.double(filmOffset[1])
	cd.lens_u, cd.lens_v, cd.time_u = C.double(lens[0]), C.double(lens[1]), C.double(timeU)
	if rc := C.pbrt_gpu_camera_rays_device(r.ctx, &cd, &out); rc != C.PBRT_OK {
		return fmt.Errorf("pbrt_gpu_camera_rays_device: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
	return nil
}

// FrameRange is pbrt_frame_desc: the tiles [TileBegin, TileEnd) of the frame
// layout (tiles in index order at TileSize, pixels row-major in their tile, Ns
// consecutive samples per pixel; include/pbrt_gpu.h).
type FrameRange struct {
	TileSize, Ns       int32
	TileBegin, TileEnd int64
}

func (f FrameRange) desc(flags int32) C.pbrt_frame_desc {
	var d C.pbrt_frame_desc
	d.tile_size, d.ns = C.int32_t(f.TileSize), C.int32_t(f.Ns)
	d.tile_begin, d.tile_end = C.int64_t(f.TileBegin), C.int64_t(f.TileEnd)
	d.flags, d.reserved = C.int32_t(flags), 0
	return d
}

// FrameCount is the element count of a tile range (pbrt_gpu_frame_count): what
// every array of FrameSamplesDevice and FilmAddDevice must hold.
func (r *Renderer) FrameCount(f FrameRange) (int, error) {
	d := f.desc(0)
	n := int64(C.pbrt_gpu_frame_count(r.ctx, &d))
	if n < 0 {
		return 0, fmt.Errorf("pbrt_gpu_frame_count: tile range outside the film, or more than 2^31 - 1 samples")
	}
	return int(n), nil
}

// DeviceSamples are the outputs of FrameSamplesDevice: the rays (TMax may be
// nil), PFilmX, PFilmY (float64: absolute raster positions), the stream after
// the camera draws (DeviceRNG, where LiDevice begins) and, optionally, the
// pixel (int32 each).
type DeviceSamples struct {
	Rays           DeviceRays
	PFilmX, PFilmY *DeviceBuffer
	RNG            DeviceRNG
	Px, Py         *DeviceBuffer
}

// FrameSamplesDevice enqueues the traced samples (k = 1 .. Ns, spp = Ns + 1) of
// a THROUGHPUT render with nDims = 0 over a tile range, in the frame layout
// (pbrt_gpu_frame_samples_device). One kernel; nothing is copied or waited for.
func (r *Renderer) FrameSamplesDevice(f FrameRange, out DeviceSamples) error {
	n, err := r.FrameCount(f)
	if err != nil {
		return err
	}
	s, err := r.samplesSoA(out, n)
	if err != nil {
		return err
	}
	d := f.desc(0)
	if rc := C.pbrt_gpu_frame_samples_device(r.ctx, &d, &s); rc != C.PBRT_OK {
		return fmt.Errorf("pbrt_gpu_frame_samples_device: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
	return nil
}

// samplesSoA is pbrt_frame_samples_soa over the buffers of out, each checked to hold n elements.
func (r *Renderer) samplesSoA(out DeviceSamples, n int) (C.pbrt_frame_samples_soa, error) {
	var s C.pbrt_frame_samples_soa
	soa, err := r.raySoA(out.Rays, n)
	if err != nil {
		return s, err
	}
	p := [6]unsafe.Pointer{}
	elem := [6]int{8, 8, 8, 8, 4, 4}
	for k, d := range []*DeviceBuffer{out.PFilmX, out.PFilmY, out.RNG.State, out.RNG.Inc, out.Px, out.Py} {
		if p[k], err = r.devPtr(d, n, elem[k], k > 3); err != nil {
			return s, err
		}
	}
	s.ox, s.oy, s.oz, s.dx, s.dy, s.dz, s.tmax = soa.ox, soa.oy, soa.oz, soa.dx, soa.dy, soa.dz, soa.tmax
	s.pfilm_x, s.pfilm_y = (*C.double)(p[0]), (*C.double)(p[1])
	s.state, s.inc = (*C.uint64_t)(p[2]), (*C.uint64_t)(p[3])
	s.px, s.py = (*C.int32_t)(p[4]), (*C.int32_t)(p[5])
	return s, nil
}

// StratSampler is pbrt_strat_sampler_desc: sampler.NewStratified(X, Y, Jitter, NDims).
type StratSampler struct {
	X, Y, NDims int32
	Jitter      bool
}

// CameraCursors are the dimensions a path's first Get1D / Get2D read after
// GetCameraSample (pFilm, pLens, time): what LiStratifiedDevice takes as
// first1D, first2D for the samples of FrameSamplesStratified.
func (s StratSampler) CameraCursors() (first1D, first2D int32) {
	first1D, first2D = 1, 2
	if s.NDims < 1 {
		first1D = s.NDims
	}
	if s.NDims < 2 {
		first2D = s.NDims
	}
	return
}

// DeviceStrat are the stratified sampler's arrays: S1D (float64) holds the
// tables, NDims * spp values each; Table and K (int32) are the table and the
// sample index of each sample or ray.
type DeviceStrat struct{ S1D, Table, K *DeviceBuffer }

// FrameSamplesStratified enqueues the traced samples (k = 1 .. spp - 1) of a
// THROUGHPUT render under the stratified sampler s, NDims >= 1, over a tile range
// (pbrt_gpu_frame_samples_stratified_device): f.Ns must be spp - 1. It writes
// FrameSamplesDevice's outputs, K and Table per sample, and the table of every
// pixel of the range to strat.S1D. One kernel; nothing is copied or waited for.
func (r *Renderer) FrameSamplesStratified(f FrameRange, s StratSampler, out DeviceSamples, strat DeviceStrat) error {
	n, err := r.FrameCount(f)
	if err != nil {
		return err
	}
	soa, err := r.samplesSoA(out, n)
	if err != nil {
		return err
	}
	if f.Ns < 1 || s.X < 1 || s.Y < 1 || s.NDims < 0 {
		return fmt.Errorf("pbrtgpu: FrameSamplesStratified: bad sampler or ns")
	}
	var ss C.pbrt_strat_samples_soa
	pixels := n / int(f.Ns)
	p := [3]unsafe.Pointer{}
	for k, d := range []*DeviceBuffer{strat.K, strat.Table} {
		if p[k], err = r.devPtr(d, n, 4, false); err != nil {
			return err
		}
	}
	if p[2], err = r.devPtr(strat.S1D, pixels*int(s.NDims)*int(s.X)*int(s.Y), 8, false); err != nil {
		return err
	}
	ss.k, ss.table, ss.s1d = (*C.int32_t)(p[0]), (*C.int32_t)(p[1]), (*C.double)(p[2])
	var sd C.pbrt_strat_sampler_desc
	sd.sampler_x, sd.sampler_y, sd.n_dims, sd.reserved = C.int32_t(s.X), C.int32_t(s.Y), C.int32_t(s.NDims), 0
	if s.Jitter {
		sd.jitter = 1
	}
	d := f.desc(0)
	if rc := C.pbrt_gpu_frame_samples_stratified_device(r.ctx, &d, &sd, &soa, &ss); rc != C.PBRT_OK {
		return fmt.Errorf("pbrt_gpu_frame_samples_stratified_device: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
	return nil
}

// FilmAddDevice adds the film of the samples of a tile range (PFilmX, PFilmY and
// the radiances L.R, L.G, L.B, in the frame layout) to film, the (H, W, 3)
// float64 XYZ film on the device; clear zeroes it first
// (pbrt_gpu_film_add_device). Ascending ranges over several calls give the bits
// of one call over all tiles. Two kernels; nothing is copied or waited for.
func (r *Renderer) FilmAddDevice(f FrameRange, pFilmX, pFilmY *DeviceBuffer, L DeviceRadiance, film *DeviceBuffer, clear bool) error {
	n, err := r.FrameCount(f)
	if err != nil {
		return err
	}
	p := [5]unsafe.Pointer{}
	for k, d := range []*DeviceBuffer{pFilmX, pFilmY, L.R, L.G, L.B} {
		if p[k], err = r.devPtr(d, n, 8, false); err != nil {
			return err
		}
	}
	fp, err := r.devPtr(film, r.w*r.h*3, 8, false)
	if err != nil {
		return err
	}
	var s C.pbrt_film_samples_soa
	s.pfilm_x, s.pfilm_y = (*C.double)(p[0]), (*C.double)(p[1])
	s.r, s.g, s.b = (*C.double)(p[2]), (*C.double)(p[3]), (*C.double)(p[4])
	flags := int32(0)
	if clear {
		flags = C.PBRT_FILM_ADD_CLEAR
	}
	d := f.desc(flags)
	if rc := C.pbrt_gpu_film_add_device(r.ctx, &d, &s, (*C.double)(fp)); rc != C.PBRT_OK {
		return fmt.Errorf("pbrt_gpu_film_add_device: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
	return nil
}

// FilmRGBA8Device converts a device film of w x h pixels to w * h * 4 bytes in
// rgba, Film.WriteImage's conversion (pbrt_gpu_film_rgba8_device): the bytes of
// FilmToRGBA's pixels on the host. One kernel; nothing is copied or waited for.
func (r *Renderer) FilmRGBA8Device(film *DeviceBuffer, w, h int, rgba *DeviceBuffer) error {
	if w <= 0 || h <= 0 || w > (1<<31-1)/h {
		return fmt.Errorf("pbrtgpu: %d x %d pixels", w, h)
	}
	fp, err := r.devPtr(film, w*h*3, 8, false)
	if err != nil {
		return err
	}
	op, err := r.devPtr(rgba, w*h*4, 1, false)
	if err != nil {
		return err
	}
	if rc := C.pbrt_gpu_film_rgba8_device(r.ctx, (*C.double)(fp), C.int64_t(w), C.int64_t(h), (*C.uint8_t)(op)); rc != C.PBRT_OK {
		return fmt.Errorf("pbrt_gpu_film_rgba8_device: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
	return nil
}

// QueryPanics is pbrt_query_record: how many rays of the queries since the last
// QueryStatus the reference panics on, the smallest such ray index (-1: none)
// and its PBRT_PANIC_* kind.
type QueryPanics struct {
	Panics   uint64
	FirstRay int64
	Kind     int32
}

// QueryStatus waits for the context's stream and returns (and clears) the panic
// record. Unlike RenderFrame it does not panic: a batch reports, the caller decides.
func (r *Renderer) QueryStatus() (QueryPanics, error) {
	var rec C.pbrt_query_record
	rc := C.pbrt_gpu_query_status(r.ctx, &rec)
	qp := QueryPanics{Panics: uint64(rec.panics), FirstRay: int64(rec.first_ray), Kind: int32(rec.panic_kind)}
	if rc != C.PBRT_OK && rc != C.PBRT_E_REF_PANIC {
		return qp, fmt.Errorf("pbrt_gpu_query_status: %s", C.GoString(C.pbrt_gpu_last_error(r.ctx)))
	}
	return qp, nil
}

// RendererGroup owns the scene resident on several GPUs (pbrt_gpu_group): the
// frame's tiles are split over the devices and merged on the first of them in
// tile-index order, so the film is bit-identical to a single Renderer's.
type RendererGroup struct {
	g    *C.pbrt_gpu_group
	w, h int
}

// NewRendererGroup creates one member per entry of devices (HIP ordinals, 1..8
// of them; an ordinal may repeat, which only serves tests on one GPU).
func NewRendererGroup(s *SceneBuilder, devices []int) (*RendererGroup, error) {
	if s.desc == nil {
		return nil, fmt.Errorf("pbrtgpu: scene not built")
	}
	if len(devices) == 0 || len(devices) > C.PBRT_GROUP_MAX {
		return nil, fmt.Errorf("pbrtgpu: a group has 1..%d devices, got %d", int(C.PBRT_GROUP_MAX), len(devices))
	}
	devs := make([]C.int32_t, len(devices))
	for i, d := range devices {
		devs[i] = C.int32_t(d)
	}
	var opts C.pbrt_gpu_opts
	var g *C.pbrt_gpu_group
	if rc := C.pbrt_gpu_group_create(s.desc, &opts, &devs[0], C.int32_t(len(devs)), &g); rc != C.PBRT_OK {
		return nil, fmt.Errorf("pbrt_gpu_group_create: status %d", int(rc))
	}
	f := s.desc.film
	return &RendererGroup{g: g, w: int(f.crop_max_x - f.crop_min_x), h: int(f.crop_max_y - f.crop_min_y)}, nil
}

// Size is the number of members.
func (r *RendererGroup) Size() int { return int(C.pbrt_gpu_group_size(r.g)) }

// RenderFrame is Renderer.RenderFrame over the group: same film, same
// cancellation (ctx maps to pbrt_gpu_group_cancel, which cancels every member)
// and the same panic contract (the lowest panicking tile over all members).
func (r *RendererGroup) RenderFrame(ctx context.Context, rd *C.pbrt_render_desc, film []float64) error {
	if len(film) < r.w*r.h*3 || len(film) == 0 {
		return fmt.Errorf("pbrtgpu: film holds %d values, the frame needs %d", len(film), r.w*r.h*3)
	}
	if err := ctx.Err(); err != nil {
		return err
	}
	// as in Renderer.RenderFrame: the watcher is joined before returning, so no
	// cancel can reach the group after the caller's Close
	done := make(chan struct{})
	exited := make(chan struct{})
	go func() {
		defer close(exited)
		select {
		case <-ctx.Done():
			C.pbrt_gpu_group_cancel(r.g)
		case <-done:
		}
	}()
	var st C.pbrt_gpu_stats
	rc := C.pbrt_gpu_group_render(r.g, rd, (*C.double)(unsafe.Pointer(&film[0])), &st)
	close(done)
	<-exited
	switch rc {
	case C.PBRT_OK:
		return nil
	case C.PBRT_E_CANCELLED:
		if err := ctx.Err(); err != nil {
			return err
		}
		return context.Canceled
	case C.PBRT_E_REF_PANIC: // the CPU reference panics here; keep that contract
		panic(fmt.Sprintf("go-pbrt panic kind %d at tile %d pixel (%d,%d) sample %d bounce %d",
			int(st.panic_kind), int(st.panic_tile), int64(st.panic_pixel_x), int64(st.panic_pixel_y),
			int(st.panic_sample), int(st.panic_bounce)))
	default:
		return fmt.Errorf("pbrt_gpu_group_render: %s", C.GoString(C.pbrt_gpu_group_last_error(r.g)))
	}
}

// MemberStats is member i's pbrt_gpu_stats of the last frame.
func (r *RendererGroup) MemberStats(i int) (C.pbrt_gpu_stats, error) {
	var st C.pbrt_gpu_stats
	if rc := C.pbrt_gpu_group_member_stats(r.g, C.int(i), &st); rc != C.PBRT_OK {
		return st, fmt.Errorf("pbrt_gpu_group_member_stats: status %d", int(rc))
	}
	return st, nil
}

func (r *RendererGroup) Close() { C.pbrt_gpu_group_destroy(r.g) }

// FilmToRGBA is Film.WriteImage's pixel loop (film.go:156-161): uint8(Clamp(v, 0, 1) * 255)
// of the XYZ sums, NaN -> 0, alpha 255; encode the result with image/png as WriteImage does.
func FilmToRGBA(film []float64, w, h int) (*image.RGBA, error) {
	if w <= 0 || h <= 0 || len(film) < w*h*3 {
		return nil, fmt.Errorf("pbrtgpu: film holds %d values, %dx%d needs %d", len(film), w, h, w*h*3)
	}
	img := image.NewRGBA(image.Rect(0, 0, w, h))
	if rc := C.pbrt_film_to_rgba8((*C.double)(unsafe.Pointer(&film[0])), C.int64_t(w), C.int64_t(h),
		(*C.uint8_t)(unsafe.Pointer(&img.Pix[0]))); rc != C.PBRT_OK {
		return nil, fmt.Errorf("pbrt_film_to_rgba8: status %d", int(rc))
	}
	return img, nil
}

"""Edge shapes on every render route, against the oracle on the uint64 view of the film.

tests/test_gpu_edges.py renders partial spheres, disks with an inner radius and a
phi_max, negative-scale transforms and reversed two-sided area lights on a
7-primitive Matte scene: the LDS-staged Matte chain, k_paths_ci, k_dl_* and the
serial kernel. Here the same shapes (tests/edge_routes.py's edge_crowd(): with
Mirror / Glass / OrenNayar on them, among filler spheres until the tree passes 64
nodes, and with one more area light on a partial sphere that has lit points inside
its radius) run on the routes for large trees, for more than 16 lights, for the kX
instantiations and on the camera-start route; the small tree runs the kX LDS chain.

Every render is 48x32, 2x2 spp, max_depth 5. Before a device comparison the oracle's
film must differ from the film of the same scene with the edge flags off. Each
comparison covers the film's bits, paths_traced, rays_closest and rays_shadow
(camera_samples too on the camera-start route); st.kernel and the launch log are
asserted (launch_checks), the log through check_invariants.
"""
import numpy as np
import pytest

import edge_routes as R
import pbrtgpu as G
from launch_checks import assert_launched, chain, names
from pbrtgpu import abi
from test_gpu_large_trees import CAM, CI, SERIAL, bits, cam_kernels, chains, checked_log, knobs

pytestmark = pytest.mark.gpu

WAVE, DL = abi.PBRT_KERNEL_WAVE, abi.PBRT_KERNEL_WAVE_DL
PW = ("k_pw_trace<false>", "k_pw_shade<false>", "k_pw_shadow<false>")
PW_KX = ("k_pw_trace<false>", "k_pw_shade<true>", "k_pw_shadow<false>")


def edges_in_view(name):
    rc, film, _ = R.oracle(name)
    rc0, plain, _ = R.oracle(name, False)
    assert rc == 0 and rc0 == 0 and np.isfinite(film).all()
    differ = int((film != plain).any(axis=-1).sum())
    assert differ > film.shape[0] * film.shape[1] // 10, (name, differ)   # (the oracle's own: 235 pixels or more of 1536)


def frames(name, family, n=1, cam=False, **opts):
    """n frames of RENDERS[name] on one context, each the oracle's; returns the checked launch logs."""
    edges_in_view(name)
    _, ofilm, ost = R.oracle(name)
    logs = []
    with G.Renderer(R.scene(name), **opts) as r:
        for frame in range(n):
            film, st = r.render(R.make_rd(name))
            print(f"{name} frame {frame}: st.kernel {st.kernel}, launched {sorted(names(r.launches()))}")
            assert st.kernel == family, (name, frame, st.kernel)
            assert np.array_equal(bits(film), bits(ofilm)), (name, frame, int((film != ofilm).any(axis=-1).sum()))
            assert (st.paths_traced, st.rays_closest, st.rays_shadow) == (ost.paths, ost.closest_rays, ost.shadow_rays), name
            if cam:
                assert st.camera_samples == ost.camera_samples, name
            logs.append(checked_log(r))
    return logs


# ------------------------------------------------------------------ the scene
def test_the_scene_is_what_the_routes_need():
    big, small = R.scene("kx"), R.scene("small_kx")
    assert big.desc.n_nodes == 73 and small.desc.n_nodes == 13   # beyond kLdsNodes (64), and LDS-staged
    assert R.scene("matte_l20").desc.n_lights == 21
    d = big.desc
    mats = [d.materials[d.prims[i].material].type for i in range(d.n_prims)]
    shapes = [d.shapes[d.prims[i].shape] for i in range(d.n_prims)]
    is_partial = [s.type == abi.PBRT_SHAPE_SPHERE and s.z_max < s.radius and s.phi_max < 6.28 for s in shapes]
    is_holed = [s.type == abi.PBRT_SHAPE_DISK and s.inner_radius > 0 for s in shapes]
    assert any(p and m == abi.PBRT_MAT_GLASS for p, m in zip(is_partial, mats))     # a partial sphere is Glass
    assert any(h and m == abi.PBRT_MAT_MIRROR for h, m in zip(is_holed, mats))      # a holed disk is Mirror
    lights = [d.lights[i] for i in range(d.n_lights) if d.lights[i].type == abi.PBRT_LIGHT_DIFFUSE_AREA]
    on_partial = [lt for lt in lights if d.shapes[lt.shape].z_max < d.shapes[lt.shape].radius
                  and d.shapes[lt.shape].phi_max < 6.28]
    assert len(lights) == 2 and len(on_partial) == 1 and any(lt.two_sided for lt in lights)
    # a lit surface inside the partial light sphere's radius: the floor plane y = 0 passes 0.75 below its centre
    sd = d.shapes[on_partial[0].shape]
    assert abs(sd.object_to_world.m.m[1][3]) < sd.radius
    # and the light shows: without it the oracle's film differs
    _, film, _ = R.oracle("matte")
    dark = R.edge_crowd(kinds=R.MATTE, partial_light=False)
    rc, without, _ = R.O.render(dark.desc, R.make_rd("matte"), threads=R.THREADS)
    assert rc == 0 and int((film != without).any(axis=-1).sum()) > 100


def test_a_disk_is_refused_as_an_area_lights_shape():
    """pbrt_gpu_create takes spheres as area lights (scene_tables.h validate_scene): PBRT_E_UNSUPPORTED."""
    with pytest.raises(G.PbrtError) as e:
        G.Renderer(R.disk_light_scene())
    assert e.value.code == abi.PBRT_E_UNSUPPORTED


# ------------------------------------------------------------- the large tree
def test_matte_exact(monkeypatch):
    knobs(monkeypatch)
    logs = frames("matte", CI, n=2)   # the cold frame and the learned one
    for log in logs:
        assert chains(log) and all(", 64, false, " in k for k in chains(log)), chains(log)
        assert_launched(log, PW, "matte")
        assert not [k for k in names(log) if k.startswith("k_paths_ci")]
    assert "k_tile_cost<false>" in names(logs[0])


def test_matte_throughput(monkeypatch):
    knobs(monkeypatch)
    for log in frames("matte_tp", WAVE):
        assert_launched(log, ("k_mb_setup<false>",) + PW, "matte_tp")
        assert not chains(log)


@pytest.mark.parametrize("w", [1, 4])
def test_kx_exact(w, monkeypatch):
    knobs(monkeypatch, PBRT_CI_WAVES=str(w))
    for log in frames("kx", CI):
        assert chain(w, 64, kx=True, multi=(w == 1)) in chains(log), chains(log)
        assert all(", 64, true, " in k for k in chains(log)), chains(log)
        assert_launched(log, PW_KX, "kx")


def test_kx_throughput(monkeypatch):
    knobs(monkeypatch)
    for log in frames("kx_tp", WAVE):
        assert_launched(log, ("k_mb_setup<true>",) + PW_KX, "kx_tp")


def test_matte_20_lights(monkeypatch):
    knobs(monkeypatch)
    for log in frames("matte_l20", CI):
        assert_launched(log, PW, "matte_l20")
        assert not [k for k in names(log) if k.startswith("k_paths_ci")]


@pytest.mark.parametrize("name,kernel", [("dl_matte", "k_dl_samples<false>"), ("dl_kx", "k_dl_samples<true>")])
def test_direct_lighting(name, kernel, monkeypatch):
    knobs(monkeypatch)
    for log in frames(name, DL):
        assert_launched(log, ("k_dl_setup", kernel), name)


@pytest.mark.parametrize("name", ["cam", "cam_tp", "cam_lens", "cam_crop"])
def test_camera_start(name, monkeypatch):
    knobs(monkeypatch)
    tp = name.endswith("_tp")
    for log in frames(name, CAM, cam=True, kernel="wave_cam"):
        assert cam_kernels(log) == {"k_cam_setup" if tp else "k_chain_cam_stack",
                                    f"k_paths_cam_stack<64, {'true' if tp else 'false'}>"}, (name, cam_kernels(log))


def test_kx_serial(monkeypatch):
    knobs(monkeypatch)
    for log in frames("kx", SERIAL, kernel="serial"):
        assert_launched(log, ("k_render_exact<1>",))
        assert not chains(log)


# ------------------------------------------------------------- the small tree
def test_small_kx_exact(monkeypatch):
    knobs(monkeypatch)
    for log in frames("small_kx", CI):
        assert chains(log) and all(", 0, true, " in k for k in chains(log)), chains(log)   # the kX LDS chain
        assert_launched(log, ("k_paths_ci<8, false, true>",), "small_kx")


def test_small_kx_path_wavefront(monkeypatch):
    knobs(monkeypatch, PBRT_PATHS_WF="1")
    for log in frames("small_kx", CI):
        assert_launched(log, PW_KX, "small_kx PBRT_PATHS_WF=1")
        assert not [k for k in names(log) if k.startswith("k_paths_ci")]


def test_small_kx_two_tiles_per_wave(monkeypatch):
    knobs(monkeypatch)
    for log in frames("small_kx", CI, lanes_per_wave=2):
        assert chains(log) == {chain(1, 0, kx=True, multi=True)}, chains(log)


def test_small_kx_throughput(monkeypatch):
    knobs(monkeypatch)
    for log in frames("small_kx_tp", WAVE):
        assert_launched(log, ("k_mb_setup<true>", "k_paths_ci<8, true, true>"), "small_kx_tp")

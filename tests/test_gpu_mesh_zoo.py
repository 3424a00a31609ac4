"""The device LBVH and the mesh walk on tests/mesh_zoo.py's families: meshes
that are not a height field (exact ties, duplicated and zero-area triangles,
one to five triangles, several meshes, degenerate Morton keys, extreme scales,
subnormal vertices, a coplanar analytic primitive). The tree's structure, the
queries (host-array and device-resident, fewer rays than a wave included) and
the renders are compared bit for bit with the oracle, which
tests/test_mesh_zoo.py pins on the same inputs against brute force; three
relations (appended copies, power-of-two scaling, the reverse flag) hold
whatever the oracle says.
"""
import functools
import os

import numpy as np
import pytest

import mesh_zoo as Z
import oracle_lib as O
import pbrtgpu as G
from pbrtgpu import abi
from test_gpu_mesh import check_lbvh
from test_gpu_query import CLEAN, any_hit, bits, closest, same_bits, status
from test_mesh_zoo import NAMES, RELATION_CASES, flip, scaled_tmax_back

pytestmark = pytest.mark.gpu

THREADS = max(1, min(int(os.environ.get("OMP_NUM_THREADS", "16") or 16), os.cpu_count() or 1))
MESH_ONLY_NAMES = [n for n in NAMES if n.startswith("scaled") or n == "subnormal"]   # no analytic variant
VARIANTS = [(n, False) for n in NAMES] + [(n, True) for n in NAMES if n not in MESH_ONLY_NAMES]
SMALL_QUERIES = ("grid_ties", "duplicates")   # also queried with 1, 63 and 65 rays


@functools.lru_cache(maxsize=None)
def oracle_rows(name, mixed):
    """(closest rows, any-hit flags) of the oracle on Case `name`, computed once."""
    c = Z.query_cases()[name]
    desc = c.scene(mixed=mixed).desc
    want, wocc = O.intersect(desc, c.rays, closest=True), O.intersect(desc, c.rays, closest=False)
    assert not np.isnan(want).any()
    for a in (want, wocc):
        a.setflags(write=False)
    return want, wocc


def test_variants_are_the_zoo():
    cases = Z.query_cases()
    assert set(NAMES) == set(cases)
    assert {n for n in NAMES if not cases[n].has_mixed} == set(MESH_ONLY_NAMES)


# --------------------------------------------------------------- structure
@pytest.mark.parametrize("name", NAMES)
def test_structure(name):
    c = Z.query_cases()[name]
    tris_in, n_kept = c.tris_in, int(c.kept.sum())
    with G.Renderer(c.scene()) as r:
        info = r.mesh_info()
        nodes, gid, tris = r.mesh_download()
        rc, got = r.intersect(c.rays) if n_kept == 0 else (0, None)
    print(f"{name}: {info}")
    assert info["tris"] == n_kept and info["meshes"] == len(c.meshes)
    assert O.mesh_counts(c.scene().desc) == (len(tris_in), n_kept)   # the oracle drops the same triangles
    if n_kept == 0:   # an all-degenerate mesh: no tree, and nothing to hit
        assert info["nodes"] == 0 and len(gid) == 0 and tris.shape == (0, 9)
        assert rc == 0 and (got[:, 0] == 0).all() and (got[:, 2] == -1).all()
        return
    check_lbvh(nodes, gid, tris, info, tris_in)
    if n_kept == 1:
        assert info["nodes"] == 1 and info["depth"] <= 1   # the root is the leaf


# ----------------------------------------------------------------- queries
@pytest.mark.parametrize("name,mixed", VARIANTS, ids=[f"{n}-{'mixed' if m else 'mesh'}" for n, m in VARIANTS])
def test_queries_match_the_oracle(name, mixed):
    """Closest and any-hit, through the host-array calls and through the
    device-resident calls (padded, sentinel-checked buffers), bit for bit."""
    c = Z.query_cases()[name]
    scene = c.scene(mixed=mixed)
    want, wocc = oracle_rows(name, mixed)
    n_prims = scene.desc.n_prims
    assert (n_prims > 0) == mixed   # mixed: the kernels with the analytic walk; else kMeshOnly (matte) ones
    n_all = c.rays.shape[0]
    sizes = (1, 63, 65, n_all) if name.startswith(SMALL_QUERIES) else (n_all,)
    with G.Renderer(scene) as r:
        for n in sizes:
            rays = c.rays[:n]
            got = closest(r, rays)
            occ = any_hit(r, rays)
            assert status(r) == CLEAN
            assert same_bits(got, want[:n]), (n, int((bits(got) != bits(want[:n])).any(axis=1).sum()))
            assert np.array_equal(occ.astype(bool), wocc[:n].astype(bool)) and set(np.unique(occ)) <= {0, 1}
            rc, host = r.intersect(rays)
            rc_p, hocc = r.intersect_p(rays)
            assert rc == 0 and rc_p == 0
            assert same_bits(host, want[:n]) and np.array_equal(hocc, occ)
    hit = want[:, 0] == 1
    tri = hit & (want[:, 2] >= n_prims)
    print(f"{name} {'mixed' if mixed else 'mesh'}: {int(tri.sum())} triangle hits, {int((hit & ~tri).sum())} analytic "
          f"hits, {int((~hit).sum())} misses")
    if name.startswith("duplicates"):   # every reported triangle lies in the first copy
        first = 1 if name.startswith("duplicates[x") else c.tris_in.shape[0] // 2
        assert tri.any() and (got[tri, 2] < n_prims + first).all() and (got[tri, 2] >= n_prims).all()
    if name == "mixed_tie" and mixed:
        assert (got[hit, 1] == 4.0).all() and (hit & ~tri).any() and tri.any()


# --------------------------------------------------------------- relations
def device_rows(scene, rays):
    with G.Renderer(scene) as r:
        got, occ = closest(r, rays), any_hit(r, rays)
        assert status(r) == CLEAN
    return got, occ


def device_film(scene, rd, **kw):
    with G.Renderer(scene, **kw) as r:
        return r.render(rd)


@pytest.mark.parametrize("name", RELATION_CASES)
def test_appended_copies_change_nothing(name):
    c = Z.query_cases()[name]
    mixed = c.has_mixed
    base = c.scene(mixed=mixed, size=(40, 32))
    twice = c.scene(mixed=mixed, size=(40, 32), meshes=c.with_copies())
    a, aocc = device_rows(base, c.rays)
    b, bocc = device_rows(twice, c.rays)
    assert same_bits(a, b) and np.array_equal(aocc, bocc)
    assert (a[:, 0] == 1).sum() > 100
    if c.view is None:
        return
    rd = abi.render_desc(2, 2, max_depth=5)
    film1, st1 = device_film(base, rd)
    film2, st2 = device_film(twice, rd)
    assert st1.paths_traced == st2.paths_traced and film1.max() > 0
    assert same_bits(film1, film2)
    front = c.scene(mixed=mixed, size=(40, 32), meshes=c.with_copies()[len(c.meshes):] + c.meshes)
    film3, _ = device_film(front, rd)
    assert not same_bits(film1, film3)   # in front, the copies win the ties with their own material


def test_power_of_two_scaling():
    s = Z.soup()
    want, wocc = device_rows(s.scene(), s.rays)
    assert (want[:, 0] == 1).sum() > 4000
    for k, c in Z.scaled().items():
        got, occ = device_rows(c.scene(), c.rays)
        assert same_bits(scaled_tmax_back(got, s.rays, k), want), k
        assert np.array_equal(occ, wocc), k


def test_reverse_flag_changes_the_film_and_the_normal():
    c = Z.multi()
    base = c.scene(mixed=True, size=(40, 32))
    flipped = c.scene(mixed=True, size=(40, 32), meshes=flip(c.meshes, 0))
    rd = abi.render_desc(2, 2, max_depth=5)
    film1, _ = device_film(base, rd)
    film2, _ = device_film(flipped, rd)
    assert film1.max() > 0 and not same_bits(film1, film2)
    (a, _), (b, _) = device_rows(base, c.rays), device_rows(flipped, c.rays)
    n_prims, first = base.desc.n_prims, c.mesh_first
    on0 = (a[:, 0] == 1) & (a[:, 2] >= n_prims) & (a[:, 2] < n_prims + first[1])
    assert on0.sum() > 50
    assert same_bits(a[:, :6], b[:, :6]) and same_bits(a[~on0], b[~on0])
    assert same_bits(b[on0, 6:9], -a[on0, 6:9])


# ----------------------------------------------------------------- renders
KERNEL_NAMES = {abi.PBRT_KERNEL_SERIAL: "serial", abi.PBRT_KERNEL_WAVE: "wave", abi.PBRT_KERNEL_WAVE_CI: "wave_ci",
                abi.PBRT_KERNEL_WAVE_DL: "wave_dl", abi.PBRT_KERNEL_WAVEFRONT: "wavefront"}


@functools.lru_cache(maxsize=None)
def multi_oracle(mode, integrator):
    scene = Z.multi().scene(mixed=True, size=(40, 32))
    rd = abi.render_desc(3, 3, max_depth=6, mode=mode, integrator=integrator)
    rc, film, st = O.render(scene.desc, rd, threads=THREADS)
    assert rc == 0 and np.isfinite(film).all()
    film.setflags(write=False)
    return scene, rd, film, st.paths


# (kernel, PBRT_PATHS_WF, PBRT_PW_SORT); None leaves the variable alone
MULTI_CONFIGS = [("serial", None, None), ("auto", None, "0"), ("auto", None, "1"), ("auto", "0", "0"), ("auto", "0", "1")]


@pytest.mark.parametrize("kernel,paths_wf,sort", MULTI_CONFIGS,
                         ids=[f"{k}-wf{w or 'default'}-sort{s or 'default'}" for k, w, s in MULTI_CONFIGS])
@pytest.mark.parametrize("mode", [abi.PBRT_MODE_EXACT, abi.PBRT_MODE_THROUGHPUT])
def test_render_multi_bitexact(mode, kernel, paths_wf, sort, monkeypatch):
    """Five meshes of four materials and mixed reverse flags over the checker
    floor: the path wavefront (the default for mesh scenes), unsorted and
    sorted by material, k_paths_ci (PBRT_PATHS_WF=0) and the serial kernel."""
    if paths_wf is not None:
        monkeypatch.setenv("PBRT_PATHS_WF", paths_wf)
    if sort is not None:
        monkeypatch.setenv("PBRT_PW_SORT", sort)
    scene, rd, ofilm, opaths = multi_oracle(mode, abi.PBRT_INTEGRATOR_PATH)
    film, st = device_film(scene, rd, kernel=kernel)
    print(f"multi mode {mode} {kernel} wf {paths_wf} sort {sort}: kernel {KERNEL_NAMES.get(st.kernel, st.kernel)}")
    if kernel == "auto":
        assert st.kernel in (abi.PBRT_KERNEL_WAVE, abi.PBRT_KERNEL_WAVE_CI)
    else:
        assert st.kernel == abi.PBRT_KERNEL_SERIAL
    assert st.paths_traced == opaths
    assert same_bits(film, ofilm), int((film != ofilm).sum())
    assert film.max() > 0


def test_render_multi_direct_lighting():
    scene, rd, ofilm, opaths = multi_oracle(abi.PBRT_MODE_EXACT, abi.PBRT_INTEGRATOR_DIRECT_LIGHTING)
    film, st = device_film(scene, rd)
    print(f"multi DirectLighting: kernel {KERNEL_NAMES.get(st.kernel, st.kernel)}")
    assert st.paths_traced == opaths
    assert same_bits(film, ofilm), int((film != ofilm).sum())
    assert film.max() > 0


TOP_RENDERS = [("grid_ties[6]", False), ("grid_ties[6]", True), ("duplicates[two_meshes]", False),
               ("duplicates[two_meshes]", True), ("degenerates[interleaved]", False),
               ("degenerates[interleaved]", True), ("degenerates[between]", True), ("degenerates[all]", True)]


@pytest.mark.parametrize("name,mixed", TOP_RENDERS, ids=[f"{n}-{'mixed' if m else 'mesh'}" for n, m in TOP_RENDERS])
def test_render_down_the_axis(name, mixed):
    """A camera looking straight down the grid's normal: primary rays meet the
    grid's vertices and edges head on. The duplicated grid stands beside the
    plain one: the same film (test_appended_copies_change_nothing) from twice
    the triangles."""
    c = Z.query_cases()[name]
    scene = c.scene(mixed=mixed, size=(48, 32))
    rd = abi.render_desc(2, 2, max_depth=5)
    rc, ofilm, ost = O.render(scene.desc, rd, threads=THREADS)
    assert rc == 0
    film, st = device_film(scene, rd)
    print(f"{name} {'mixed' if mixed else 'mesh'}: kernel {KERNEL_NAMES.get(st.kernel, st.kernel)}")
    assert st.paths_traced == ost.paths
    assert same_bits(film, ofilm), int((film != ofilm).sum())
    assert film.max() > 0

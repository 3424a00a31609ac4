"""The routes for trees beyond 64 BVH nodes without a GPU: every render
tests/test_gpu_large_trees.py compares with the oracle is a fit witness as
tests/test_large_scenes_host.py defines it (the tree is as large as the test
says, the oracle renders it, and the film has light in it), and the library
compiles the kernels those routes launch.
"""
import numpy as np
import pytest

import large_trees as T
import pbrtgpu as G
from launch_checks import chain
from pbrtgpu import abi

KX_STACK_CHAINS = [chain(1, 64, kx=True, multi=True), chain(2, 64, kx=True), chain(4, 64, kx=True)]
CAM_STACK = ["k_chain_cam_stack"] + [f"k_paths_cam_stack<{p}, {mb}>" for p in (4, 16, 64) for mb in ("false", "true")]


@pytest.mark.parametrize("name", list(T.RENDERS))
def test_render_is_a_witness(name):
    r = T.RENDERS[name]
    assert r.point == "nodes" and r.scene().desc.n_nodes > 64
    rc, film, st = T.oracle(name)
    assert np.isfinite(film).all()
    if r.panics:   # Ld > 10 at the first traced sample's first bounce, in the first tile
        assert rc == abi.PBRT_E_REF_PANIC
        assert (st.panic_kind, st.panic_tile, st.panic_sample, st.panic_bounce) == (1, 0, 1, 1)
        return
    assert rc == 0
    lit = (film.reshape(-1, 3) != 0).any(axis=1).mean()
    assert lit >= 0.5, lit   # the oracle's own share is 0.80 or more: only a broken scene is caught


def test_the_tables_split():
    assert len(T.A_RENDERS) == 8 and len(T.B_RENDERS) == 7
    assert all(T.RENDERS[n].rd.get("mode", abi.PBRT_MODE_EXACT) == abi.PBRT_MODE_EXACT for n in T.A_RENDERS)


def test_the_mesh_render_has_a_mesh_and_it_shows():
    d = T.crowd_mesh().desc
    assert d.n_meshes == 1 and d.n_prims == 61 and d.n_nodes == 121
    differ = (T.oracle("kx_exact_mesh")[1] != T.oracle("kx_exact")[1]).any(axis=-1).sum()
    assert differ > 48 * 32 // 4, differ   # the patch fills a good part of the frame


def test_the_library_compiles_the_stack_kernels():
    names = set(G.kernel_names())
    missing = [k for k in KX_STACK_CHAINS + CAM_STACK if k not in names]
    assert not missing, missing
    # the small-tree camera kernels keep their names
    assert {"k_chain_cam", "k_cam_setup", "k_film_cam<false>", "k_film_cam<true>"} <= names
    assert {f"k_paths_cam<{p}, {mb}>" for p in (4, 16, 64) for mb in ("false", "true")} <= names

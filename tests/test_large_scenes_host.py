"""The large-scene routes without a GPU: every render tests/test_gpu_large_scenes.py
compares with the oracle is a fit witness (its scene is as large as the test says,
the oracle renders it, and the film has light in it).
"""
import numpy as np
import pytest

import large_scenes as L
from pbrtgpu import abi


@pytest.mark.parametrize("name", list(L.RENDERS))
def test_render_is_a_witness(name):
    r = L.RENDERS[name]
    d = r.scene().desc
    if r.point == "nodes":
        assert d.n_nodes > 64
    elif r.point == "lights":
        assert 16 < d.n_lights <= 64
    elif r.point == "lights16":
        assert d.n_lights == 16 and d.n_nodes > 64
    else:
        assert d.n_nodes <= 64 and d.n_lights <= 16
    rc, film, st = L.oracle(name)
    assert np.isfinite(film).all()
    if r.panics:   # (a panicking render's film is whatever the tiles before the panic left)
        assert rc == abi.PBRT_E_REF_PANIC and st.panic_kind != 0
        return
    assert rc == 0
    lit = (film.reshape(-1, 3) != 0).any(axis=1).mean()
    assert lit >= 0.5, lit   # the oracle's own share is 0.89 or more: only a broken scene is caught


def test_crowd_is_the_size_the_tests_rely_on():
    d = L.crowd().desc
    assert (d.n_prims, d.n_nodes, d.n_lights) == (61, 121, 2)
    assert L.crowd(lights=64, kinds=L.MATTE).desc.n_lights == 64
    assert L.crowd(n=4, lights=20).desc.n_nodes <= 64


def test_the_extra_lights_change_the_film():
    """a route that dropped the lights beyond 16 (or all but two) would still be finite and lit"""
    f2, f20, f17 = L.oracle("matte_l2")[1], L.oracle("matte_l20")[1], L.oracle("matte_l17")[1]
    differ = lambda a, b: int((a != b).any(axis=-1).sum())   # noqa: E731
    assert differ(f2, f20) > f2.shape[0] * f2.shape[1] // 2
    assert differ(f17, L.oracle("matte_l16")[1]) > 0

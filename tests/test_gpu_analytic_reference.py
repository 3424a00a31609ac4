"""Every BVH walk of the device against tests/analytic_reference.py directly, not through
the oracle: on every decided ray the hit flag and the primitive are the reference's, t, p
and n agree within test_analytic_reference_host.TOL (measured there between the oracle and
the reference on the CPU, times 50), the any-hit flag is the closest-hit flag and the panic
record stays empty.

Per scene and family (analytic_reference.COMPARED: `aimed`, `offsets`, `shadowing`, and
adversarial_rays' `inside`, `random` and the decided rays of `axis`):

- Renderer.intersect and intersect_p: the host-array batch (k_intersect);
- intersect_device and intersect_p_device: the [64]-stack walk (k_query_hit), with
  sentinel-padded buffers that must survive;
- on the two small scenes, intersect_device(staged=True) and its any-hit: the LDS-staged
  walk (k_query_hit_staged), with the context's own culling groups, with PBRT_CULL_GROUPS=0
  and with PBRT_CULL_GROUP=2.
"""
import pytest

import adversarial_rays as A
import analytic_reference as R
import pbrtgpu as G
from test_analytic_reference_host import same_as_reference
from test_gpu_adversarial_rays import STAGED, knobs, query_kernels, staged_any, staged_closest
from test_gpu_query import CLEAN, any_hit, closest, status

pytestmark = pytest.mark.gpu


def check(key, family, rows, occ, what):
    return same_as_reference(A.SCENES[key](), R.rays(key, family), R.reference(key, family), rows, occ,
                             f"{key} {family} {what}")


@pytest.mark.parametrize("key", list(A.SCENES))
def test_host_array_batch(key, monkeypatch):
    """pbrt_gpu_intersect and pbrt_gpu_intersect_p: k_intersect."""
    knobs(monkeypatch)
    with G.Renderer(A.SCENES[key]()) as r:
        before = len(r.launches(outside=True))
        for family in R.COMPARED:
            rays = R.rays(key, family)
            rc, rows = r.intersect(rays)
            assert rc == 0, family
            rc, occ = r.intersect_p(rays)
            assert rc == 0, family
            check(key, family, rows, occ, "host-array batch")
        assert any(k.startswith("k_intersect") for k in query_kernels(r, before))


@pytest.mark.parametrize("key", list(A.SCENES))
def test_stack_walk(key, monkeypatch):
    """pbrt_gpu_intersect_device and pbrt_gpu_intersect_p_device: the [64] stack of k_query_hit."""
    knobs(monkeypatch)
    with G.Renderer(A.SCENES[key]()) as r:
        assert status(r) == CLEAN
        before = len(r.launches(outside=True))
        for family in R.COMPARED:
            rays = R.rays(key, family)
            rows = closest(r, rays)     # (sentinel-padded buffers: test_gpu_query.head checks the tails)
            assert status(r) == CLEAN, family
            occ = any_hit(r, rays)
            assert status(r) == CLEAN, family
            check(key, family, rows, occ, "stack walk")
        assert query_kernels(r, before) == {"k_query_hit<false, false>", "k_query_hit<true, false>"}


@pytest.mark.parametrize("walk", list(STAGED))
@pytest.mark.parametrize("key", ["small1", "small4"])
def test_staged_walk(key, walk, monkeypatch):
    """The LDS-staged walk: culling groups, the plain leaf scan, and groups of two leaves."""
    env, grouped = STAGED[walk]
    knobs(monkeypatch, **env)
    with G.Renderer(A.SCENES[key]()) as r:
        assert (r.cull_groups() > 0) == grouped
        before = len(r.launches(outside=True))
        for family in R.COMPARED:
            rays = R.rays(key, family)
            rows = staged_closest(r, rays)
            assert status(r) == CLEAN, family
            occ = staged_any(r, rays)
            assert status(r) == CLEAN, family
            check(key, family, rows, occ, f"staged walk ({walk})")
        assert {"k_query_hit_staged<false>", "k_query_hit_staged<true>"} <= query_kernels(r, before)

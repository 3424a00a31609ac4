"""The device's film of the one-bounce render of tests/onebounce_reference.py against its
closed form, not through the oracle, within test_onebounce_host.TOL (50 times the gap
measured there between the oracle and the closed form), on every route that accepts the
render:

- the default wave pipeline (kernel="auto": the EXACT chain);
- kernel="serial";
- PBRT_MODE_THROUGHPUT: nothing random reaches a film of maxDepth 2 with one point light
  (the order of the samples differs, their values do not), so this film matches too.

Left out: kernel="wave_cam" with n_dims = 0. Without sampled dimensions pFilm is a PCG32
draw per sample, so the camera ray no longer goes through the pixel's corner (#3 does not
apply) and the film depends on the random stream: it has no closed form. That route is
held to the oracle by tests/test_gpu_wave_cam.py.
"""
import numpy as np
import pytest

import onebounce_reference as B
import pbrtgpu as G
from pbrtgpu import abi
from test_onebounce_host import same_as_closed_form

pytestmark = pytest.mark.gpu

ROUTES = {
    "default": ("auto", abi.PBRT_MODE_EXACT, {abi.PBRT_KERNEL_WAVE_CI}),
    "serial": ("serial", abi.PBRT_MODE_EXACT, {abi.PBRT_KERNEL_SERIAL}),
    "throughput": ("auto", abi.PBRT_MODE_THROUGHPUT, {abi.PBRT_KERNEL_WAVE}),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_device_film_is_the_closed_form(route):
    kernel, mode, ran = ROUTES[route]
    with G.Renderer(B.scene(), kernel=kernel) as r:
        film, st = r.render(B.render_desc(mode=mode))
    assert st.kernel in ran, (route, st.kernel)
    assert st.paths_traced == B.RES[0] * B.RES[1] * (B.SPP[0] * B.SPP[1] - 1)      # #2
    same_as_closed_form(film, route)


def test_routes_agree_bit_for_bit_where_the_order_is_the_same():
    """The EXACT routes sum a pixel's samples in the reference's order: their films are equal bit for bit."""
    films = []
    for kernel in ("auto", "serial"):
        with G.Renderer(B.scene(), kernel=kernel) as r:
            films.append(r.render(B.render_desc())[0])
    assert np.array_equal(films[0].view(np.uint64), films[1].view(np.uint64))

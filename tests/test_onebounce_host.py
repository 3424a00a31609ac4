"""The oracle's film of a one-bounce render against the closed form of
tests/onebounce_reference.py (no GPU): the first check of camera -> hit -> BSDF -> light
-> visibility -> film that does not come from the oracle itself.

Film 16 x 12, spp 2 x 2, maxDepth 2, a pinhole camera; a floor disk, a reversed and a
plain sphere, an occluder sphere between the light and the floor, one point light.

TOL. Measured on the CPU, the largest gap between the oracle's film and the closed form,
per channel and relative to the channel's value, was 1.46e-13 (no pixel is left out; the
gap is largest on a pixel one of whose corner rays meets the occluder sphere at 82 degrees
to the light, |wi . n| = 0.13, where the hit point's rounding weighs most; the next
largest are 4e-14 to 6e-14). TOL is FACTOR = 50 times that: the oracle's hit points (EFloat's
t, float64 matrices), Go's trig in the camera matrices against numpy's and the order of
the sums are the sources. A wrong weight, a wrong side test or a wrong shadow ray shows at
1e-2 or more.
"""
import numpy as np
import pytest

import onebounce_reference as B
import oracle_lib as O

MEASURED = 1.46e-13
FACTOR = 50
TOL = FACTOR * MEASURED
LEFT_OUT_CAP = 0.10
KINDS = ("lit floor", "shadowed floor", "reversed", "plain", "background")


def same_as_closed_form(film, what):
    """The assertion for the oracle's film and for any device route's."""
    f = B.film()
    assert film.shape == f.xyz.shape and np.isfinite(film).all(), what
    gap = B.gap(film, f.xyz)
    print(f"{what}: largest gap {gap:.3g} over {int(f.compared.sum())} of {f.compared.size} pixels")
    assert gap <= TOL, (what, gap, TOL)
    return gap


def test_tolerance_is_the_measured_maximum_times_the_factor():
    assert TOL == 50 * MEASURED and TOL < 1e-9


def test_the_closed_form_covers_every_kind_of_pixel():
    f = B.film()
    assert f.xyz.shape == (12, 16, 3) and B.SPP == (2, 2) and B.MAX_DEPTH == 2
    left_out = 1 - f.compared.mean()
    print(f"left out: {left_out:.3f}")
    assert left_out <= LEFT_OUT_CAP
    seen = set()
    pure = set()          # pixels all of whose corners are of one kind
    for y in range(f.compared.shape[0]):
        for x in range(f.compared.shape[1]):
            if f.compared[y, x]:
                seen |= f.labels[y][x]
                if len(f.labels[y][x]) == 1:
                    pure |= f.labels[y][x]
    assert set(KINDS) <= seen, seen
    assert {"lit floor", "shadowed floor", "plain", "background"} <= pure, pure
    # lit pixels are lit and the rest is black, by the labels alone
    lit = np.isin(f.corner_labels, ("lit floor",))
    assert (f.L[lit] > 0).all() and not f.L[np.isin(f.corner_labels, ("shadowed floor", "background"))].any()
    # both spheres have lit corners, and the reversed one is lit like a sphere that is not reversed (#22)
    for name in ("reversed", "plain"):
        assert (f.L[f.corner_labels == name].max(axis=1) > 0).sum() >= 2, name


def test_camera_matrices_are_the_descriptors():
    """The camera of the closed form, built from camera.go and transform.go with the reference's own products,
    is the host builder's to rounding."""
    d = B.scene().desc
    r2c = np.array([list(r) for r in d.camera.raster_to_camera.m.m])
    c2w = np.array([list(r) for r in d.camera.camera_to_world.m.m])
    assert np.abs(r2c - B.raster_to_camera()).max() < 1e-15 and np.abs(c2w - B.camera_to_world()).max() < 1e-15
    assert r2c[3, 2] == 0 and r2c[3, 3] == 1     # #18: the projective row is lost


def test_film_spreads_a_corner_sample_over_four_pixels():
    """#6 and #2 on a film of one radiance: pixel (x, y) sums the corners (x, y), (x + 1, y), (x, y + 1) and
    (x + 1, y + 1) that are sampled, spp - 1 times each."""
    f = B.film()
    W, H = B.RES
    want = np.zeros((H, W, 3))
    for y in range(H):
        for x in range(W):
            for cy in (y, y + 1):
                for cx in (x, x + 1):
                    if cx < W and cy < H:
                        want[y, x] += 3 * f.L[cy, cx]
    assert np.allclose(B.rgb_to_xyz(want), f.xyz, rtol=1e-14, atol=0)


@pytest.mark.parametrize("tile_size", [16, 8])
def test_oracle_film_is_the_closed_form(tile_size):
    """(tile_size 8: the film is merged from four tiles, whose edge pixels sum two tiles' shares)"""
    sc = B.scene()
    rc, film, st = O.render(sc.desc, B.render_desc(tile_size=tile_size), threads=2)
    assert rc == 0 and st.panic_kind == 0
    assert st.paths == B.RES[0] * B.RES[1] * (B.SPP[0] * B.SPP[1] - 1)      # #2
    same_as_closed_form(film, f"oracle, tile_size {tile_size}")

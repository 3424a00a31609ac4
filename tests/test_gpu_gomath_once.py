"""The one-evaluation trig of go-pbrt_amd/csrc/gomath.h on the device.

One array of arguments (the special values, the neighbourhoods of every range
threshold and octant boundary, random values and random bit patterns; the host
check tests/gomath_once_check.cpp runs the same classes) goes through the SIN,
COS, ASIN, ACOS, ATAN, ATAN2 and SINCOS probes once:

- SINCOS is the device's own SIN and COS bit for bit, NaN payloads included;
- every routine is the oracle's Go math bit for bit (NaN as a class): Atan, Atan2,
  Asin and Acos on the whole array, Sin and Cos below Go's reduceThreshold (2^29),
  up to which the oracle and the device restate sin.go's Cody-Waite reduction;
- the CONCENTRIC_DISK probe on a 256 x 256 grid of u (its centre and both
  diagonals |ux| == |uy| are grid points) and on random u is sampling.go:173-198
  evaluated in numpy float64 (IEEE operations in Go's order, no contraction) with
  Sin and Cos from the device's own probes.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import pbrtgpu as G
from pbrtgpu import abi

pytestmark = pytest.mark.gpu


def probe(op, inp, out_stride=1):
    inp = np.ascontiguousarray(inp, dtype=np.float64)
    if inp.ndim == 1:
        inp = inp[:, None]
    out = np.zeros((inp.shape[0], out_stride))
    rc = G.lib().pbrt_gpu_probe(-1, op, inp.ctypes.data_as(C.POINTER(C.c_double)), inp.shape[0], inp.shape[1],
                                out.ctypes.data_as(C.POINTER(C.c_double)), out_stride)
    assert rc == 0
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits_nan_class(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return (np.isnan(got) & np.isnan(want)) | (bits(got) == bits(want))


def around(c, ulps=8):
    """±ulps doubles around c and around -c."""
    k = np.arange(-ulps, ulps + 1)
    u = np.array([c, -c]).view(np.uint64)
    return (u[:, None] + k[None, :].astype(np.int64).view(np.uint64)).reshape(-1).view(np.float64)


def arguments():
    rng = np.random.default_rng(20)
    one = np.array([1.0, -1.0]).view(np.uint64)
    sp = np.concatenate([
        [0.0, -0.0, 1.0, -1.0, np.nan, np.inf, -np.inf],
        np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64),    # a NaN with sign and payload
        np.concatenate([one + np.uint64(1), one - np.uint64(1)]).view(np.float64),   # beside ±1
        np.array([1, 1 << 63 | 1, 0x000FFFFFFFFFFFFF, 1 << 63 | 0x000FFFFFFFFFFFFF],   # smallest, largest denormals
                 dtype=np.uint64).view(np.float64),
        [2.2250738585072014e-308, 1.7976931348623157e308, -1.7976931348623157e308]])
    h = np.sqrt(1 + 0.66 * 0.66)
    thr = [around(t) for t in (0.66, 0.7, 2.41421356237309504880)] + [around(0.66 / h, 64), around(1 / h, 64)]
    octants = [around(k * (np.pi / 4)) for k in range(17)]
    large = [around(2.0 ** e) for e in range(30, 41)]
    rnd = [rng.uniform(-8 * np.pi, 8 * np.pi, 30000), rng.uniform(-1, 1, 30000),
           rng.choice([-1.0, 1.0], 20000) * np.ldexp(1 + rng.random(20000), rng.integers(-1074, 40, 20000)),
           rng.integers(0, 2 ** 64, 10000, dtype=np.uint64).view(np.float64)]
    a = np.concatenate([sp] + thr + octants + large + rnd)
    assert a.size <= 100_000
    return a


@pytest.fixture(scope="module")
def trig():
    """The argument array and every probe's output on it (computed once, not modified)."""
    a = arguments()
    y = np.roll(a, 1)   # Atan2's pairs: every argument beside its neighbour
    out = {"a": a, "y": y}
    for name in ("SIN", "COS", "ASIN", "ACOS", "ATAN"):
        out[name] = probe(getattr(abi, "PBRT_PROBE_" + name), a)[:, 0]
    out["ATAN2"] = probe(abi.PBRT_PROBE_ATAN2, np.stack([y, a], 1))[:, 0]
    out["SINCOS"] = probe(abi.PBRT_PROBE_SINCOS, a, 2)
    for v in out.values():
        v.setflags(write=False)
    return out


def test_sincos_is_the_devices_sin_and_cos_bit_for_bit(trig):
    assert abi.PBRT_PROBE_SINCOS == 24 and abi.PBRT_PROBE_CONCENTRIC_DISK == 25 and abi.PBRT_PROBE_EFLOAT_DIV == 23
    s, c = trig["SINCOS"][:, 0], trig["SINCOS"][:, 1]
    bad_s, bad_c = bits(s) != bits(trig["SIN"]), bits(c) != bits(trig["COS"])
    print("sincos vs sin, cos: %d and %d of %d differ" % (bad_s.sum(), bad_c.sum(), s.size))
    assert not bad_s.any(), trig["a"][bad_s][:8]
    assert not bad_c.any(), trig["a"][bad_c][:8]
    # the array does reach every class: all 8 octants, special values, large arguments
    a = trig["a"]
    fin = np.isfinite(a) & (np.abs(a) < 2.0 ** 40)
    assert set(np.unique((np.floor(np.abs(a[fin]) * (4 / np.pi)).astype(np.int64)) & 7)) == set(range(8))
    assert np.isnan(s[np.isinf(a)]).all() and np.isnan(c[np.isinf(a)]).all()
    assert np.signbit(s[1]) and s[1] == 0 and not np.signbit(s[0]) and c[0] == 1.0 and c[1] == 1.0


@pytest.mark.parametrize("name", ["SIN", "COS", "SINCOS", "ATAN", "ASIN", "ACOS", "ATAN2"])
def test_trig_is_the_oracles(trig, name):
    L = O.lib()
    a, y = trig["a"], trig["y"]
    if name in ("SIN", "COS", "SINCOS"):
        use = np.isnan(a) | np.isinf(a) | (np.abs(a) < 2.0 ** 29)   # (Go reduces by Payne-Hanek beyond)
        got = [trig[name]] if name != "SINCOS" else [trig[name][:, 0], trig[name][:, 1]]
        fs = {"SIN": [L.oracle_go_sin], "COS": [L.oracle_go_cos], "SINCOS": [L.oracle_go_sin, L.oracle_go_cos]}[name]
        for g, f in zip(got, fs):
            want = np.array([f(x) for x in a[use]])
            ok = same_bits_nan_class(g[use], want)
            print(name, "differ from the oracle: %d of %d" % ((~ok).sum(), ok.size))
            assert ok.all(), a[use][~ok][:8]
        return
    if name == "ATAN2":
        want = np.array([L.oracle_go_atan2(p, q) for p, q in zip(y, a)])
    else:
        f = getattr(L, "oracle_go_" + name.lower())
        want = np.array([f(x) for x in a])
    ok = same_bits_nan_class(trig[name], want)
    print(name, "differ from the oracle: %d of %d" % ((~ok).sum(), ok.size))
    assert ok.all(), a[~ok][:8]


def test_concentric_disk_probe_is_sampling_go():
    g = np.arange(256) / 256.0
    ux, uy = [v.reshape(-1) for v in np.meshgrid(g, g, indexing="ij")]
    rng = np.random.default_rng(21)
    u = np.concatenate([np.stack([ux, uy], 1), rng.random((4096, 2))])
    got = probe(abi.PBRT_PROBE_CONCENTRIC_DISK, u, 2)
    # sampling.go:173-198
    ox, oy = u[:, 0] * 2.0 - 1, u[:, 1] * 2.0 - 1
    centre = (ox == 0) & (oy == 0)
    wide = np.abs(ox) > np.abs(oy)
    with np.errstate(all="ignore"):
        theta = np.where(wide, (np.pi / 4.0) * (oy / ox), (np.pi / 2.0) - (np.pi / 4.0) * (ox / oy))
    theta[centre] = 0.0
    r = np.where(wide, ox, oy)
    want = np.stack([probe(abi.PBRT_PROBE_COS, theta)[:, 0] * r, probe(abi.PBRT_PROBE_SIN, theta)[:, 0] * r], 1)
    want[centre] = 0.0
    assert centre.sum() == 1 and (np.abs(ox) == np.abs(oy)).sum() >= 2 * 255
    bad = (bits(got) != bits(want)).any(axis=1)
    print("concentric disk: %d of %d differ" % (bad.sum(), bad.size))
    assert not bad.any(), u[bad][:8]

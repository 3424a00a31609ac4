"""The Li queries on rays their caller owns, against the oracle's integrators on the same rays
(oracle_path_li, oracle_direct_li), bit for bit.

The scenes, ray families and PCG32 streams are tests/li_rays.py's (checked on the oracle alone by
tests/test_li_rays_host.py): non-unit and zero-component directions, finite, zero, negative and NaN
TMax, origins on and inside shapes, and path states a caller has edited. Per scene and family, on
one context:

- li_device: r, g, b, state, draws and rays, the query record, and the launch;
- path_begin and max_depth dense steps, and the same through ping-pong queues: every state array
  after each step is the oracle's after as many iterations, and the end is li_device's;
- the `state` family: path_step from the edited arrays;
- direct_li_device with both strategies.
max_depth is 5, and 12 once per kernel on `secondary`; the batch sizes are the adversarial test's.

Comparison rule (tests/test_gpu_adversarial_rays.py's): bit for bit on the uint64 view; where the
oracle's element is NaN the device's must be NaN. A row on which the reference panics has L = 0,
its ray counts as at the panic, and the query record is (PBRT_E_REF_PANIC, count, first, kind) of
the oracle's panics. Its stream: a panic of the closest-hit walk comes before any draw of the
iteration and state and draws are the oracle's. The path kernels trace an iteration's visibility
ray after its BSDF sample and Russian roulette (csrc/pbrt_spec.h path_step), so at a panic of that
ray or of Ld > 10 they have drawn the BSDF sample's two values more than the reference had, and
a third where Russian roulette drew (from the fourth iteration on): include/pbrt_gpu.h says so,
and state is the oracle's advanced by that many draws. k_li_direct draws in the reference's order.
"""
import numpy as np
import pytest

import li_rays as LR
import li_reference as R
import oracle_lib as O
import pbrtgpu as G
import test_gpu_li as T
import test_gpu_query as Q
from pbrtgpu import abi
from test_gpu_adversarial_rays import SIZES, knobs

pytestmark = pytest.mark.gpu

padded, head = T.padded, T.head
RAY_KEYS = T.RAY_KEYS
KEYS = list(LR.SCENES)
RAY_FAMILIES = list(LR.FAMILIES)
DL = {"all": abi.PBRT_DL_UNIFORM_SAMPLE_ALL, "one": abi.PBRT_DL_UNIFORM_SAMPLE_ONE}


def test_the_scenes_select_every_instantiation():
    for base in ("k_li", "k_path_step", "k_li_direct"):
        assert {LR.kernel(k, base) for k in KEYS} == {f"{base}<{kx}, {d}>" for kx in ("false", "true") for d in (0, 64)}


# ------------------------------------------------------------------ comparison
def same(got, want, what):
    """The comparison rule for one array."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype != np.float64:
        bad = got != want
    else:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (what, "NaN", np.flatnonzero(np.isnan(got) != nan)[:5])
        bad = (got.view(np.uint64) != want.view(np.uint64)) & ~nan
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:5], got[bad][:3], want[bad][:3])


def same_stream(got_state, got_draws, o, inc, late, what):
    """state and draws against the oracle's; the late panics by the rule of the module docstring."""
    same(got_draws[~late], o.draws[~late], what + " draws")
    same(got_state[~late], o.state[~late], what + " state")
    if late.any():
        extra = got_draws[late].astype(np.int64) - o.draws[late].astype(np.int64)
        assert (np.isin(extra, (2, 3)) & ((extra == 2) | (o.bounces[late] > 3))).all(), (what, extra, o.bounces[late])
        same(got_state[late], R.pcg_advance(o.state[late], inc[late], extra), what + " state after a late panic")


def record_of(panic, status=None):
    """The query record of a call whose rows panic with these kinds (0: none)."""
    pan = panic != 0 if status is None else status == O.PANICKED
    if not pan.any():
        return Q.CLEAN
    first = int(np.argmax(pan))
    return (abi.PBRT_E_REF_PANIC, int(pan.sum()), first, int(panic[first]))


def packed(o):
    assert o.closest.max(initial=0) < 1 << 16 and o.shadow.max(initial=0) < 1 << 16
    return o.closest | (o.shadow << np.uint32(16))


def cut(t, n):
    return type(t)(*[a[:n] for a in t])


def launched(r, before, name, count=1):
    names = [rec.name for rec in r.launches(outside=True)[before:]]
    assert names == [name] * count, names


# ------------------------------------------------------------------ li_device
def check_li(r, key, family, n=None, max_depth=LR.MAX_DEPTH):
    b, o, late = LR.batch(key, family), LR.oracle_li(key, family, max_depth), LR.late_panics(key, family, max_depth)
    n = b.rays.shape[0] if n is None else min(n, b.rays.shape[0])
    o, late = cut(o, n), late[:n]
    what = f"{key} {family} li_device n={n} depth={max_depth}"
    rb, gb = T.upload_batch(r, b.rays[:n], b.state[:n], b.inc[:n])
    before = len(r.launches(outside=True))
    got = T.li(r, rb, gb, n, max_depth=max_depth)
    assert Q.status(r) == record_of(o.panic, o.status), what
    launched(r, before, LR.kernel(key, "k_li"))
    for c, k in enumerate("rgb"):
        same(got[k], o.L[:, c], f"{what} {k}")   # (a panicking row: the oracle's L is 0 too)
    same(got["rays"], packed(o), what + " rays")
    same_stream(got["state"], got["draws"], o, b.inc[:n], late, what)
    pan = o.status == O.PANICKED
    assert not got["r"][pan].any() and not got["g"][pan].any() and not got["b"][pan].any()
    return got, n


# --------------------------------------------------------------- path stepping
def oracle_state(o):
    """A PathLi as pbrt_path_soa's arrays (inc apart)."""
    out = {k: o.ray[:, i] for i, k in enumerate(RAY_KEYS)}
    out.update(lr=o.L[:, 0], lg=o.L[:, 1], lb=o.L[:, 2], br=o.beta[:, 0], bg=o.beta[:, 1], bb=o.beta[:, 2],
               eta_scale=o.eta_scale, rays=packed(o), bounces=o.bounces.astype(np.int32), status=o.status.astype(np.uint8))
    return out


def start_buffers(r, b, n):
    """The path state a batch starts from: path_begin's, or (the `state` family) the caller's own arrays, all ALIVE."""
    if b.start is None:
        rb, gb = T.upload_batch(r, b.rays[:n], b.state[:n], b.inc[:n])
        pb = {k: padded(r, n, dt) for k, dt in G.PATH_DTYPES.items()}
        before = len(r.launches(outside=True))
        assert r.path_begin(rb, gb, n, pb) == 0, r.last_error()
        launched(r, before, "k_path_begin")
        return pb
    s = cut(b.start, n)
    host = {k: b.rays[:n, i] for i, k in enumerate(RAY_KEYS)}
    host.update(lr=s.L[:, 0], lg=s.L[:, 1], lb=s.L[:, 2], br=s.beta[:, 0], bg=s.beta[:, 1], bb=s.beta[:, 2], eta_scale=s.eta_scale,
                state=b.state[:n], inc=b.inc[:n], draws=s.draws.astype(np.uint32),
                rays=(s.closest.astype(np.uint32) | (s.shadow.astype(np.uint32) << np.uint32(16))),
                bounces=s.bounces.astype(np.int32), status=np.full(n, abi.PBRT_PATH_ALIVE, dtype=np.uint8))
    return {k: padded(r, n, dt, host[k]) for k, dt in G.PATH_DTYPES.items()}


def check_steps(r, key, family, n=None, max_depth=LR.MAX_DEPTH, queues=False):
    b, steps, late = LR.batch(key, family), LR.oracle_steps(key, family, max_depth), LR.late_panics(key, family, max_depth)
    n = b.rays.shape[0] if n is None else min(n, b.rays.shape[0])
    late = late[:n]
    pb = start_buffers(r, b, n)
    qs = [{"index": padded(r, n, np.int32), "count": padded(r, 1, np.uint32)} for _ in range(2)] if queues else None
    panicked = np.zeros(n, dtype=bool)
    before = len(r.launches(outside=True))
    for k in range(max_depth):
        o = cut(steps[k], n)
        what = f"{key} {family} {'queued' if queues else 'dense'} step {k + 1} of {max_depth} n={n}"
        kw = dict(in_queue=None if k == 0 else qs[k % 2], out_queue=qs[(k + 1) % 2]) if queues else {}
        assert r.path_step(pb, n, max_depth=max_depth, **kw) == 0, r.last_error()
        new = (o.status == O.PANICKED) & ~panicked   # this step's panics, under their indices
        assert Q.status(r) == record_of(np.where(new, o.panic, 0)), what
        panicked |= new
        got = {key_: head(buf, n) for key_, buf in pb.items()}
        for name, want in oracle_state(o).items():
            same(got[name], want, f"{what} {name}")
        same_stream(got["state"], got["draws"], o, b.inc[:n], late & panicked, what)
        same(got["inc"], b.inc[:n], what + " inc")
        if queues:
            cnt = int(head(qs[(k + 1) % 2]["count"], 1)[0])
            idx = np.sort(head(qs[(k + 1) % 2]["index"], n)[:cnt])
            same(idx, np.flatnonzero(o.status == O.ALIVE).astype(np.int32), what + " out queue")
    assert (got["status"] != abi.PBRT_PATH_ALIVE).all()
    launched(r, before, LR.kernel(key, "k_path_step"), max_depth)
    return got


@pytest.mark.parametrize("family", LR.ALL)
@pytest.mark.parametrize("key", KEYS)
def test_family(key, family, monkeypatch):
    knobs(monkeypatch)
    with G.Renderer(LR.SCENES[key]()) as r:
        assert Q.status(r) == Q.CLEAN
        dense = check_steps(r, key, family)
        queued = check_steps(r, key, family, queues=True)
        for k in dense:   # how the caller covers the paths changes nothing
            assert dense[k].tobytes() == queued[k].tobytes(), k
        if family != LR.STATE:
            li, n = check_li(r, key, family)
            for a, k in (("lr", "r"), ("lg", "g"), ("lb", "b"), ("state", "state"), ("draws", "draws"), ("rays", "rays")):
                assert dense[a].tobytes() == li[k].tobytes(), (a, k)   # the end state is li_device's
        assert Q.status(r) == Q.CLEAN


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("key", KEYS)
def test_ragged_sizes(key, n, monkeypatch):
    """The head of every family at sizes that end inside a wave and inside a block."""
    knobs(monkeypatch)
    with G.Renderer(LR.SCENES[key]()) as r:
        for family in LR.ALL:
            check_steps(r, key, family, n=n, queues=(n % 2 == 1))
            if family != LR.STATE:
                check_li(r, key, family, n=n)


@pytest.mark.parametrize("key", KEYS)
def test_secondary_deep(key, monkeypatch):
    """max_depth 12: the paths that live on decide Russian roulette in every iteration from the fourth."""
    knobs(monkeypatch)
    with G.Renderer(LR.SCENES[key]()) as r:
        check_steps(r, key, "secondary", max_depth=LR.DEEP)
        check_steps(r, key, "secondary", max_depth=LR.DEEP, queues=True)
        check_li(r, key, "secondary", max_depth=LR.DEEP)


# ------------------------------------------------------------ direct_li_device
def check_direct(r, key, family, strategy, n=None, max_depth=LR.MAX_DEPTH):
    b, o = LR.batch(key, family), LR.oracle_direct(key, family, DL[strategy], max_depth)
    n = b.rays.shape[0] if n is None else min(n, b.rays.shape[0])
    o = cut(o, n)
    what = f"{key} {family} direct_li_device {strategy} n={n} depth={max_depth}"
    rb, gb = T.upload_batch(r, b.rays[:n], b.state[:n], b.inc[:n])
    ob = {k: padded(r, n, dt) for k, dt in G.LI_DTYPES.items()}
    before = len(r.launches(outside=True))
    assert r.direct_li_device(rb, gb, n, ob, max_depth=max_depth, dl_strategy=DL[strategy]) == 0, r.last_error()
    got = {k: head(buf, n) for k, buf in ob.items()}
    assert Q.status(r) == record_of(o.panic), what
    launched(r, before, LR.kernel(key, "k_li_direct"))
    for c, k in enumerate("rgb"):
        same(got[k], o.L[:, c], f"{what} {k}")
    same(got["rays"], packed(o), what + " rays")
    same(got["draws"], o.draws, what + " draws")
    same(got["state"], o.state, what + " state")
    return o


@pytest.mark.parametrize("strategy", sorted(DL))
@pytest.mark.parametrize("key", KEYS)
def test_direct(key, strategy, monkeypatch):
    knobs(monkeypatch)
    deepest = 0
    with G.Renderer(LR.SCENES[key]()) as r:
        for family in RAY_FAMILIES:
            o = check_direct(r, key, family, strategy)
            deepest = max(deepest, int(o.closest.max()))
            for n in SIZES:
                check_direct(r, key, family, strategy, n=n)
        check_direct(r, key, "secondary", strategy, max_depth=LR.DEEP)
        assert Q.status(r) == Q.CLEAN
    # SpecularTransmit recursed through Glass (from inside it too: `secondary`, `inside`); Matte never recurses
    assert (deepest > 1) == LR.KX[key], deepest

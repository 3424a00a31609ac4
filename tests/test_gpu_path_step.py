"""pbrt_gpu_path_begin_device / pbrt_gpu_path_step_device (Renderer.path_begin, path_step;
k_path_begin, k_path_step) on the GPU: Path.Li one iteration at a time over path state that
lives on the device.

1. begin + max_depth dense steps give pbrt_gpu_li_device's bits (L, state, draws, rays).
2. After k steps L is li_device's at max_depth k + 1.
3. Ping-pong queues: each out queue is the set of ALIVE paths, counts never grow, the final
   values are the dense form's; batches around the wave and work-list sizes.
4. A path's values do not depend on where it lies: the survivors of step 1, permuted into
   fresh buffers, end with the bits they have in place.
5. frame_samples -> path_begin -> steps -> film_add is the oracle's film.
6. The one-bounce closed form (tests/onebounce_reference.py), independent of the oracle.
7. The step outputs: the hit is intersect_device's, the material the descriptor's,
   L_before + added == L_after.
8. Panics, 9. refusals and edges, 10. launches and allocations.

The batches are tests/test_gpu_li.py's (about 2k rays at Stratified(3, 1)); every buffer is
64 elements longer than the call and pre-filled with a sentinel that must come back unchanged.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import li_reference as R
import onebounce_reference as B
import oracle_lib as O
import pbrtgpu as G
import test_gpu_li as T
import test_gpu_query as Q
from pbrtgpu import abi
from scenes import material_scene
from test_gpu_wave_cam import efloat_scene
from test_onebounce_host import TOL

pytestmark = pytest.mark.gpu

PAD, SENTINEL = T.PAD, T.SENTINEL
padded, head, same, bits = T.padded, T.head, T.same, T.bits
ALIVE, ENDED, PANICKED = abi.PBRT_PATH_ALIVE, abi.PBRT_PATH_ENDED, abi.PBRT_PATH_PANICKED
INV, UNS = abi.PBRT_E_INVALID, abi.PBRT_E_UNSUPPORTED
STATE_KEYS = tuple(G.PATH_DTYPES)
LI_OF = {"lr": "r", "lg": "g", "lb": "b", "state": "state", "draws": "draws", "rays": "rays"}   # state key -> li output
CASE_NAMES = ("readme40x24", "glass", "crowd_matte", "crowd_kx", "readme_d10_power", "lights20", "mesh_spheres", "edges")
KERNEL = {name: T.CASES[name].kernel.replace("k_li<", "k_path_step<") for name in CASE_NAMES}


def test_the_cases_launch_all_four_instantiations():
    assert set(KERNEL.values()) == {f"k_path_step<{kx}, {d}>" for kx in ("false", "true") for d in (0, 64)}


# ------------------------------------------------------------------ helpers
def path_buffers(r, n, tmax=True):
    return {k: padded(r, n, dt) for k, dt in G.PATH_DTYPES.items() if tmax or k != "tmax"}


def begin(r, rb, gb, n, tmax=True):
    pb = path_buffers(r, n, tmax)
    assert r.path_begin(rb, gb, n, pb) == 0, r.last_error()
    return pb


def state(pb, n):
    """The first n elements of every state array (the sentinel tails checked)."""
    return {k: head(b, n) for k, b in pb.items()}


def queue(r, n):
    return {"index": padded(r, n, np.int32), "count": padded(r, 1, np.uint32)}


def queue_set(q, n):
    """(count, the sorted indices) of a queue of capacity n."""
    cnt = int(head(q["count"], 1)[0])
    assert 0 <= cnt <= n
    idx = head(q["index"], n)   # (beyond the count: the sentinel, or what an earlier step of the ping-pong left)
    return cnt, np.sort(idx[:cnt])


def step(r, pb, n, case, **kw):
    rc = r.path_step(pb, n, max_depth=kw.pop("max_depth", case.max_depth), light_strategy=case.strategy, **kw)
    assert rc == 0, (rc, r.last_error())


def desc_of(case):
    return dict(max_depth=case.max_depth, light_strategy=case.strategy)


@functools.lru_cache(maxsize=None)
def batch(name):
    """The case's rays and streams, li_device's outputs at every max_depth 2 .. D, and the dense
    stepped form: the state after begin and after each of D steps, then after one step more."""
    case = T.CASES[name]
    scene = case.scene()
    s = R.samples(scene.desc.film, T.SPP)
    n = len(s.k)
    D = case.max_depth
    with G.Renderer(scene) as r:
        rb0 = T.sample_rays(r, s)
        rays = np.stack([head(rb0[k], n) for k in T.RAY_KEYS], axis=1)
        rb, gb = T.upload_batch(r, rays, s.state, s.inc)
        ref = {d: T.li(r, rb, gb, n, max_depth=d, light_strategy=case.strategy) for d in range(2, D + 1)}
        pb = begin(r, rb, gb, n)
        states = [state(pb, n)]
        before = len(r.launches(outside=True))
        for _ in range(D + 1):
            step(r, pb, n, case)
            states.append(state(pb, n))
        recs = r.launches(outside=True)[before:]
        assert Q.status(r) == Q.CLEAN
        for k in T.RAY_KEYS:   # begin and the steps leave their inputs alone
            assert same(head(rb[k], n), rays[:, T.RAY_KEYS.index(k)])
        assert same(head(gb["state"], n), s.state) and same(head(gb["inc"], n), s.inc)
    for st in states:
        for a in st.values():
            a.setflags(write=False)
    return scene, s, rays, ref, states, recs


# ------------------------------------------------ 1. composed equals li_device
@pytest.mark.parametrize("name", CASE_NAMES)
def test_dense_steps_are_li_device(name):
    case = T.CASES[name]
    scene, s, rays, ref, states, recs = batch(name)
    n, D = len(s.k), case.max_depth
    fresh = states[0]
    for i, k in enumerate(T.RAY_KEYS):
        assert same(fresh[k], rays[:, i]), k
    assert same(fresh["state"], s.state) and same(fresh["inc"], s.inc)
    for k in ("lr", "lg", "lb"):
        assert same(fresh[k], np.zeros(n)), k
    for k in ("br", "bg", "bb", "eta_scale"):
        assert same(fresh[k], np.ones(n)), k
    assert not fresh["draws"].any() and not fresh["rays"].any() and not fresh["bounces"].any()
    assert (fresh["status"] == ALIVE).all()
    end = states[D]
    for k, o in LI_OF.items():
        assert same(end[k], ref[D][o]), k
    assert (end["status"] == ENDED).all()
    assert (states[1]["status"] == ALIVE).any() and (states[1]["status"] == ENDED).any()
    for k in STATE_KEYS:   # one more step changes no byte
        assert same(states[D + 1][k], end[k]), k
    # 10. each step is one launch of the instantiation the scene selects, one wave a workgroup
    assert [rec.name for rec in recs] == [KERNEL[name]] * (D + 1)
    assert all(rec.block == (64, 1, 1) and rec.grid == ((n + 255) // 256, 1, 1) and rec.lds == 0 for rec in recs)


# ------------------------------------------------------------ 2. prefix property
@pytest.mark.parametrize("name", CASE_NAMES)
def test_k_steps_are_li_device_at_depth_k_plus_1(name):
    """Russian roulette depends on bounces, not on max_depth: stopping li_device one bounce
    earlier is stopping the stepper one step earlier."""
    case = T.CASES[name]
    _, _, _, ref, states, _ = batch(name)
    for k in range(1, case.max_depth):
        for a, o in (("lr", "r"), ("lg", "g"), ("lb", "b")):
            assert same(states[k][a], ref[k + 1][o]), (k, a)
        assert (states[k]["bounces"] <= k).all() and (states[k]["bounces"][states[k]["status"] == ALIVE] == k).all()


# -------------------------------------------------------------------- 3. queues
def run_queued(r, rb, gb, n, case):
    """begin, then D steps through ping-pong queues; returns the final state. Each out queue is
    the ALIVE set; the counts never grow."""
    pb = begin(r, rb, gb, n)
    qs = [queue(r, n), queue(r, n)]
    last = n
    for k in range(case.max_depth):
        step(r, pb, n, case, in_queue=None if k == 0 else qs[k % 2], out_queue=qs[(k + 1) % 2])
        cnt, idx = queue_set(qs[(k + 1) % 2], n)
        assert same(idx, np.flatnonzero(head(pb["status"], n) == ALIVE).astype(np.int32)), k
        assert cnt <= last
        last = cnt
    assert last == 0
    return state(pb, n)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_queues(name):
    case = T.CASES[name]
    scene, s, rays, ref, states, _ = batch(name)
    end = states[case.max_depth]
    N = 1000
    with G.Renderer(scene) as r:
        for order in (slice(None), slice(None, None, -1)):
            rb, gb = T.upload_batch(r, rays[:N][order], s.state[:N][order], s.inc[:N][order])
            for n in (1, 63, 64, 65, 255, 256, 257, N):
                got = run_queued(r, rb, gb, n, case)
                for k in LI_OF:
                    assert same(got[k], end[k][:N][order][:n]), (n, k)
                assert same(got["status"], end["status"][:N][order][:n])
        assert Q.status(r) == Q.CLEAN


# ------------------------------------------------------ 4. position independence
@pytest.mark.parametrize("name", ("readme40x24", "glass", "crowd_kx"))
def test_survivors_moved_to_fresh_buffers_end_with_the_same_bits(name):
    case = T.CASES[name]
    scene, s, rays, ref, states, _ = batch(name)
    one, end = states[1], states[case.max_depth]
    alive = np.flatnonzero(one["status"] == ALIVE)
    perm = np.random.default_rng(11).permutation(alive)
    m = len(perm)
    assert m > 64 and not np.array_equal(perm, alive)
    with G.Renderer(scene) as r:
        pb = {k: padded(r, m, dt, one[k][perm]) for k, dt in G.PATH_DTYPES.items()}
        for _ in range(case.max_depth - 1):
            step(r, pb, m, case)
        got = state(pb, m)
        assert Q.status(r) == Q.CLEAN
    for k in tuple(LI_OF) + ("status", "bounces"):
        assert same(got[k], end[k][perm]), k


# ------------------------------------------------- 5. against the oracle directly
@pytest.mark.parametrize("name", ("readme40x24", "glass"))
def test_composed_frame_is_the_oracles(name):
    case = T.CASES[name]
    scene, ofilm, ost = T.oracle_film(case)
    ns, ts = T.SPP - 1, 16
    with G.Renderer(scene) as r:
        n = r.frame_count(ns, 0, r.num_tiles(ts), ts)
        sb = {k: padded(r, n, G.SAMPLE_DTYPES[k]) for k in G.SAMPLE_REQUIRED}
        fn = r.hgt * r.w * 3
        fb = padded(r, fn, np.float64)
        assert r.frame_samples(sb, ns, 0, None, ts) == 0, r.last_error()
        pb = begin(r, {k: sb[k] for k in G.RAY_KEYS}, {k: sb[k] for k in G.RNG_KEYS}, n, tmax=False)
        qs = [queue(r, n), queue(r, n)]
        for k in range(case.max_depth):
            step(r, pb, n, case, in_queue=None if k == 0 else qs[k % 2], out_queue=qs[(k + 1) % 2])
        fs = dict(pfilm_x=sb["pfilm_x"], pfilm_y=sb["pfilm_y"], r=pb["lr"], g=pb["lg"], b=pb["lb"])
        assert r.film_add(fs, ns, fb, 0, None, ts, clear=True) == 0, r.last_error()
        film = head(fb, fn).reshape(r.hgt, r.w, 3)
        nrays = head(pb["rays"], n)
        assert Q.status(r) == Q.CLEAN
    assert np.array_equal(bits(film), bits(ofilm)), int((bits(film) != bits(ofilm)).sum())
    assert (int((nrays & 0xFFFF).sum()), int((nrays >> 16).sum())) == (ost.closest_rays, ost.shadow_rays)


# ----------------------------------------- 6. independently of the oracle: one bounce
def test_one_bounce_closed_form():
    """max_depth 2, one point light: L after two steps is Kd / pi * |wi . n| * I / d^2 where lit,
    else 0 (tests/test_gpu_li.py::test_one_bounce_closed_form states the reference's pixels)."""
    f = B.film()
    H, W = f.compared.shape
    want = f.L.reshape(-1, 3)
    decided = np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            decided[y, x] = any(f.compared[py, px] for py in (y - 1, y) for px in (x - 1, x) if px >= 0 and py >= 0)
    decided = decided.ravel()
    assert decided.sum() > 0.7 * decided.size
    rays = B.camera_rays()
    n = rays.shape[0]
    rng = np.random.default_rng(1)
    st = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    inc = rng.integers(0, 2**63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    with G.Renderer(B.scene()) as r:
        rb, gb = T.upload_batch(r, rays, st, inc)
        pb = begin(r, rb, gb, n)
        for _ in range(B.MAX_DEPTH):
            assert r.path_step(pb, n, max_depth=B.MAX_DEPTH) == 0, r.last_error()
        got = state(pb, n)
        assert Q.status(r) == Q.CLEAN
    assert (got["status"] == ENDED).all()
    L = np.stack([got["lr"], got["lg"], got["lb"]], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):   # as onebounce_reference.gap
        rel = np.where(want != 0, np.abs(L - want) / np.abs(want), np.where(L == want, 0.0, np.inf))
    gap = float(rel[decided].max())
    print(f"one-bounce gap {gap:.3e} (bound {TOL:.3e}) over {int(decided.sum())} of {decided.size} corner rays")
    assert gap <= TOL
    assert want[decided].max() > 0


# ---------------------------------------------------------------- 7. step outputs
def material_of(desc, prim):
    """The descriptor's material of each hit: prims[prim].material, or the mesh's for prim >= n_prims."""
    first = np.cumsum([0] + [int(desc.meshes[i].n_triangles) for i in range(desc.n_meshes)])
    out = np.full(prim.shape, -1, dtype=np.int32)
    for j, p in enumerate(prim.tolist()):
        if 0 <= p < desc.n_prims:
            out[j] = desc.prims[p].material
        elif p >= desc.n_prims:
            out[j] = desc.meshes[int(np.searchsorted(first, p - desc.n_prims, side="right")) - 1].material
    return out


@pytest.mark.parametrize("name", ("readme40x24", "glass", "mesh_spheres", "crowd_kx"))
def test_step_outputs(name):
    case = T.CASES[name]
    scene, s, rays, ref, states, _ = batch(name)
    n, D = len(s.k), case.max_depth
    miss = {"hit": 0, "prim": -1, "px": 0.0, "py": 0.0, "pz": 0.0, "nx": 0.0, "ny": 0.0, "nz": 0.0, "material": -1}
    total = np.zeros((n, 3))
    mesh_hits = n_untraced = 0
    with G.Renderer(scene) as r:
        rb, gb = T.upload_batch(r, rays, s.state, s.inc)
        pb = begin(r, rb, gb, n)
        for k in range(D):
            prev = states[k]
            adv = prev["status"] == ALIVE
            assert same(state(pb, n)["status"], prev["status"])
            hb = {key: padded(r, n, dt) for key, dt in G.HIT_DTYPES.items()}
            assert r.intersect_device({key: pb[key] for key in T.RAY_KEYS}, n, hb) == 0   # on the step's input rays
            want = {key: head(b, n) for key, b in hb.items()}
            ob = {key: padded(r, n, dt) for key, dt in G.STEP_DTYPES.items()}
            step(r, pb, n, case, step=ob)
            got = {key: head(b, n) for key, b in ob.items()}
            now = state(pb, n)
            for key in STATE_KEYS:
                assert same(now[key], states[k + 1][key]), (k, key)   # asking for the outputs changes nothing
            for key, a in got.items():   # written at the advanced paths only
                assert (a[~adv] == SENTINEL[a.dtype]).all(), (k, key)
            traced = adv & (prev["bounces"] + 1 < D)
            for key in G.HIT_DTYPES:
                assert same(got[key][traced], want[key][traced]), (k, key)
            assert same(got["material"][traced], material_of(scene.desc, want["prim"][traced])), k
            untraced = adv & ~traced
            assert k == D - 1 or not untraced.any()   # only the depth test of the last step traces nothing
            n_untraced += int(untraced.sum())
            for key, v in miss.items():
                assert (got[key][untraced] == v).all(), (k, key)
            assert same(got["t_max"][untraced], prev["tmax"][untraced])
            mesh_hits += int((got["prim"][traced] >= scene.desc.n_prims).sum())
            for c, (lk, ak) in enumerate((("lr", "ar"), ("lg", "ag"), ("lb", "ab"))):
                assert same((prev[lk] + np.where(adv, got[ak], 0.0))[adv], now[lk][adv]), (k, lk)   # one float64 addition
                assert same(now[lk][~adv], prev[lk][~adv])
                total[:, c] = total[:, c] + np.where(adv, got[ak], 0.0)
        assert Q.status(r) == Q.CLEAN
        L, st, draws, nrays, added = r.radiance_by_bounce(rays, s.state, s.inc, **desc_of(case))
        L2, st2, draws2, nrays2 = r.radiance_stepwise(rays[:, :6], s.state, s.inc, **desc_of(case))   # no tmax: +Inf
    assert (name == "mesh_spheres") == (mesh_hits > 0) and n_untraced > 0
    end = states[D]
    want_L = np.stack([end["lr"], end["lg"], end["lb"]], axis=1)
    assert same(total, want_L)
    assert added.shape == (D, n, 3)
    acc = np.zeros((n, 3))
    for k in range(D):   # the in-order sum of the terms is the final L
        acc = acc + added[k]
    assert same(acc, want_L) and same(L, want_L) and same(L2, want_L)
    for a, b_, k in ((st, st2, "state"), (draws, draws2, "draws"), (nrays, nrays2, "rays")):
        assert same(a, end[k]) and same(b_, end[k]), k


# ------------------------------------------------------------------------ 8. panics
def test_panics_are_reported_as_data():
    """tests/test_gpu_li.py's batch on the EFloat-overflow sphere: the panicking paths are PANICKED
    with L = 0, the record is li_device's for the batch, the other paths are unaffected."""
    sc = efloat_scene((20, 40, 0))
    with G.Renderer(sc) as r:
        cam = r.camera_rays()
        rays = np.stack([cam[k].download() for k in T.RAY_KEYS], axis=1)
        gx, gz = np.meshgrid(np.linspace(-3.0, 3.0, 8), np.linspace(-3.0, 3.0, 8))
        down = np.zeros((64, 7))
        down[:, 0], down[:, 1], down[:, 2], down[:, 4], down[:, 6] = gx.ravel(), 2.0, gz.ravel(), -1.0, np.inf
        rays = np.concatenate([down, rays])
        n = rays.shape[0]
        rng = np.random.default_rng(5)
        st = rng.integers(0, 2**64, size=n, dtype=np.uint64)
        inc = rng.integers(0, 2**63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        rb, gb = T.upload_batch(r, rays, st, inc)
        ref = T.li(r, rb, gb, n, max_depth=2)
        want_rec = Q.status(r)
        pan = np.isnan(O.intersect(sc.desc, rays, closest=True)[:, 0])   # the rays on which the oracle panics
        assert 0 < pan.sum() < n
        assert want_rec == (abi.PBRT_E_REF_PANIC, int(pan.sum()), int(np.argmax(pan)), abi.PBRT_PANIC_EFLOAT)
        pb = begin(r, rb, gb, n)
        ob = {k: padded(r, n, G.STEP_DTYPES[k]) for k in ("hit", "t_max", "material", "ar")}
        assert r.path_step(pb, n, step=ob, max_depth=2) == 0
        assert r.path_step(pb, n, max_depth=2) == 0
        got = state(pb, n)
        assert Q.status(r) == want_rec   # count, first ray and kind
        assert Q.status(r) == Q.CLEAN
        assert same(got["status"], np.where(pan, PANICKED, ENDED).astype(np.uint8))
        for k, o in LI_OF.items():   # L = 0 and the values at the panic; the neighbours as li_device has them
            assert same(got[k], ref[o]), k
        assert not got["lr"][pan].any() and max(got["lr"].max(), got["lg"].max(), got["lb"].max()) > 0
        hit, tm, mat, ar = (head(ob[k], n) for k in ("hit", "t_max", "material", "ar"))
        assert not hit[pan].any() and (mat[pan] == -1).all() and not ar[pan].any() and same(tm[pan], rays[pan, 6])


# ----------------------------------------------------------- 9. refusals and edges
def test_invalid_arguments_and_edges():
    scene, s, rays, ref, states, _ = batch("readme40x24")
    case = T.CASES["readme40x24"]
    n = 65
    L = G.lib()
    P = G.PATH_DTYPES
    with G.Renderer(scene) as r:
        rb, gb = T.upload_batch(r, rays[:n], s.state[:n], s.inc[:n])
        pb = path_buffers(r, n)
        qa, qb = queue(r, n), queue(r, n)
        rs = G._soa(abi.RaySoA, [(k, b, np.float64) for k, b in rb.items()])
        gs = G._soa(abi.RngSoA, [(k, b, np.uint64) for k, b in gb.items()])
        soa = lambda skip=None: G._soa(abi.PathSoA, [(k, b, P[k]) for k, b in pb.items() if k != skip])   # noqa: E731
        qsoa = lambda q, skip=None: G._soa(abi.PathQueue, [(k, b, b.dtype) for k, b in q.items() if k != skip])   # noqa: E731
        ref_ = lambda x: C.byref(x) if x is not None else None   # noqa: E731
        d = abi.li_desc(max_depth=5)

        def call_begin(rr=rs, gg=gs, nn=n, pp=soa(), h=r.h):
            return L.pbrt_gpu_path_begin_device(h, ref_(rr), ref_(gg), nn, ref_(pp))

        def call_step(dd=d, pp=soa(), qi=None, qo=None, nn=n, h=r.h):
            return L.pbrt_gpu_path_step_device(h, ref_(dd), ref_(pp), ref_(qi), ref_(qo), nn, None)

        assert call_begin(h=None) == INV and call_begin(rr=None) == INV and call_begin(gg=None) == INV
        assert call_begin(pp=None) == INV and call_begin(nn=2**31) == INV
        assert call_step(h=None) == INV and call_step(dd=None) == INV and call_step(pp=None) == INV
        assert call_step(nn=2**31) == INV
        for k in G.RAY_KEYS:
            assert call_begin(rr=G._soa(abi.RaySoA, [(q, b, np.float64) for q, b in rb.items() if q != k])) == INV, k
        for k in G.RNG_KEYS:
            assert call_begin(gg=G._soa(abi.RngSoA, [(q, b, np.uint64) for q, b in gb.items() if q != k])) == INV, k
        for k in P:
            if k != "tmax":   # every state pointer but tmax is required
                assert call_begin(pp=soa(k)) == INV and call_step(pp=soa(k)) == INV, k
        assert call_step(dd=abi.li_desc(max_depth=0)) == INV and call_step(dd=abi.li_desc(max_depth=5, reserved=1)) == INV
        assert "reserved" in r.last_error()
        for k in ("index", "count"):
            assert call_step(qi=qsoa(qa, k)) == INV and call_step(qo=qsoa(qa, k)) == INV, k
        assert call_step(qi=qsoa(qa), qo=qsoa(qa)) == INV and "alias" in r.last_error()
        mixed = G._soa(abi.PathQueue, [("index", qb["index"], np.int32), ("count", qa["count"], np.uint32)])
        assert call_step(qi=qsoa(qa), qo=mixed) == INV
        with pytest.raises(G.PbrtError):   # the wrapper's own checks
            r.path_step(pb, n, in_queue=qa, out_queue=qa)
        with pytest.raises(G.PbrtError):
            r.path_step(pb, n + PAD + 1)
        with pytest.raises(G.PbrtError):
            r.path_begin(rb, gb, n, {k: v for k, v in pb.items() if k != "bb"})
        assert call_begin(nn=0) == 0 and call_step(nn=0, qo=qsoa(qa)) == 0
        assert Q.status(r) == Q.CLEAN
        # a frame in flight: both calls are refused and leave the frame alone
        rd = abi.render_desc(2, 2)
        rc, ofilm, _ = O.render(scene.desc, rd, threads=T.THREADS)
        assert rc == 0
        r.render_async(rd)
        rc_b, rc_s = call_begin(), call_step(qo=qsoa(qa))
        r.synchronize()
        assert (rc_b, rc_s) == (INV, INV) and np.array_equal(bits(r.film()), bits(ofilm))
        for b in list(pb.values()) + list(qa.values()) + list(qb.values()):   # none of the above wrote anything
            assert (b.download() == SENTINEL[b.dtype]).all()
        # a zero-filled status array steps nothing
        for k, b in pb.items():
            b.upload(np.zeros(n, dtype=b.dtype))
        zero = state(pb, n)
        assert r.path_step(pb, n, out_queue=qa, max_depth=5) == 0
        assert all(same(a, zero[k]) for k, a in state(pb, n).items()) and queue_set(qa, n)[0] == 0
        # an index outside the arrays is skipped
        qa["index"].upload(np.array([n, -1, 2**31 - 1, 3], dtype=np.int32))
        qa["count"].upload(np.array([4], dtype=np.uint32))
        assert r.path_begin(rb, gb, n, pb) == 0
        assert r.path_step(pb, n, in_queue=qa, max_depth=5) == 0
        got = state(pb, n)
        assert got["bounces"][3] == 1 and got["bounces"].sum() == 1
        # a frame rendered before and after a stepped batch is unchanged
        film1, _ = r.render(rd)
        assert r.path_begin(rb, gb, n, pb) == 0
        for _ in range(5):
            step(r, pb, n, case)
        film2, _ = r.render(rd)
        assert np.array_equal(bits(film1), bits(ofilm)) and np.array_equal(bits(film2), bits(ofilm))
        end = state(pb, n)
        for k in LI_OF:
            assert same(end[k], states[5][k][:n]), k
        assert Q.status(r) == Q.CLEAN


REFUSALS = {
    "direct_lighting": (lambda: G.Scene.readme(32, 32), dict(integrator=abi.PBRT_INTEGRATOR_DIRECT_LIGHTING), "Path"),
    "rough_glass": (lambda: material_scene(rough=0.2), {}, "rough glass"),
    "max_depth_2049": (lambda: G.Scene.readme(32, 32), dict(max_depth=2049), "2048"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(name):
    make, desc, word = REFUSALS[name]
    n = 16
    with G.Renderer(make()) as r:
        rays = np.zeros((n, 7))
        rays[:, 5] = 1.0
        rb, gb = T.upload_batch(r, rays, np.arange(n, dtype=np.uint64), np.ones(n, dtype=np.uint64))
        pb = begin(r, rb, gb, n)
        fresh = state(pb, n)
        q = queue(r, n)
        assert r.path_step(pb, n, out_queue=q, **desc) == UNS
        assert word in r.last_error(), r.last_error()   # the reason is named
        assert Q.status(r) == Q.CLEAN
        assert all(same(a, fresh[k]) for k, a in state(pb, n).items())   # nothing was enqueued
        assert (q["count"].download() == SENTINEL[np.dtype(np.uint32)]).all()
        assert r.path_step(pb, 0, **desc) == UNS   # n = 0 is refused alike


# -------------------------------------------------------- 10. launches, allocations
def hip_free_bytes():
    hip = C.CDLL(G.hip_runtimes()[0])
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_launch_log_and_no_allocation_on_the_second_batch():
    scene, s, rays, ref, states, _ = batch("readme40x24")
    case = T.CASES["readme40x24"]
    n = 700
    with G.Renderer(scene) as r:
        rb, gb = T.upload_batch(r, rays[:n], s.state[:n], s.inc[:n])
        pb, qs = path_buffers(r, n), [queue(r, n), queue(r, n)]
        ob = {k: padded(r, n, dt) for k, dt in G.STEP_DTYPES.items()}
        free = []
        for _ in range(3):
            before = len(r.launches(outside=True))
            assert r.path_begin(rb, gb, n, pb) == 0
            for k in range(case.max_depth):
                step(r, pb, n, case, in_queue=None if k == 0 else qs[k % 2], out_queue=qs[(k + 1) % 2], step=ob)
            recs = r.launches(outside=True)[before:]
            assert [rec.name for rec in recs] == ["k_path_begin"] + [KERNEL["readme40x24"]] * case.max_depth
            assert recs[0].grid == ((n + 255) // 256, 1, 1) and recs[0].block == (256, 1, 1)
            assert Q.status(r) == Q.CLEAN
            free.append(hip_free_bytes())
        assert free[1] == free[2], free   # the steady state allocates nothing
        end = state(pb, n)
        for k in LI_OF:
            assert same(end[k], states[case.max_depth][k][:n]), k

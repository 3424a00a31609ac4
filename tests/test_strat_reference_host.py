"""tests/strat_reference.py pinned without the library, a GPU or the oracle.

- Without jitter every row of the table is a permutation of min((i + 0.5) / n, 1 - eps).
- With jitter every row is a permutation of one value per stratum [i / n, (i + 1) / n).
- The draw count is n_dims * 2 n + rejections without jitter (n picks per 1D and per 2D
  dimension) and n_dims * 5 n + rejections with it (n + 2 n jitter floats more), and the
  returned state is the start state advanced by that many literal PCG32 steps.
- pcg_bounded rejects exactly the draws below 2^32 mod b, found by stepping the stream.
- The 2D passes change no value: the table of n_dims dimensions is the first n_dims rows'
  worth of draws only when the 1D passes are replayed alone.
- frame(): layout order, k, table indices and the states after the camera sample.
"""
from collections import namedtuple

import numpy as np
import pytest

import li_reference as R
import strat_reference as S

Film = namedtuple("Film", "res_x res_y crop_min_x crop_min_y crop_max_x crop_max_y")


def film_of(w, h):
    return Film(w, h, 0, 0, w, h)


SHAPES = [(2, 2, 4), (3, 3, 1), (1, 2, 2), (11, 11, 4), (7, 7, 4), (5, 1, 6)]
STREAM = (0x853C49E6748FEA9B, 0xDA3E39CB94B95BDB)


@pytest.mark.parametrize("sx,sy,nd", SHAPES)
@pytest.mark.parametrize("jitter", [False, True])
def test_rows_are_permutations_and_draws_are_counted(sx, sy, nd, jitter):
    n = sx * sy
    sp = S.start_pixel(STREAM[0], STREAM[1], n, nd, jitter)
    assert sp.s1d.shape == (nd, n)
    for row in sp.s1d:
        if jitter:
            strata = np.floor(np.sort(row) * n).astype(int)
            assert np.array_equal(strata, np.arange(n)) and (row < 1.0).all()
        else:
            want = np.minimum((np.arange(n) + 0.5) * (1.0 / n), R.ONE_MINUS_EPS)
            assert np.array_equal(np.sort(row), want)
    events = nd * (5 * n if jitter else 2 * n)
    assert sp.draws == events + sp.rejections
    assert sp.state == R.pcg_advance(STREAM[0], STREAM[1], sp.draws)[0]   # literal stepping
    if n > 4 and nd > 1:
        assert len({row.tobytes() for row in sp.s1d}) > 1   # the dimensions are shuffled apart


def test_rejections_are_the_draws_below_the_threshold():
    """Step the stream by hand through the picks of one unjittered dimension."""
    n = 9
    sp = S.start_pixel(STREAM[0], STREAM[1], n, 1, False)
    st, inc = np.uint64(STREAM[0]), np.uint64(STREAM[1])
    perm, rejected, draws = list(range(n)), 0, 0
    for phase in range(2):   # the 1D shuffle, then the 2D pass's picks
        for i in range(n):
            b = n - i
            while True:
                new, out = R.pcg_next(st, inc)
                st, draws = new[0], draws + 1
                if int(out[0]) >= (2 ** 32) % b:
                    break
                rejected += 1
            if phase == 0:
                o = i + int(out[0]) % b
                perm[i], perm[o] = perm[o], perm[i]
    assert (rejected, draws) == (sp.rejections, sp.draws) and st == sp.state
    assert np.array_equal(sp.s1d[0], np.minimum((np.array(perm) + 0.5) * (1.0 / n), R.ONE_MINUS_EPS))


def test_stream_is_li_references_pcg32():
    s = S.Stream(*STREAM)
    st, inc = np.uint64(STREAM[0]), np.uint64(STREAM[1])
    for _ in range(200):
        new, out = R.pcg_next(st, inc)
        st = new[0]
        assert s.next() == int(out[0]) and s.state == int(st)
    _, f = R.pcg_float(st, inc)
    assert s.float() == f[0] and s.draws == 201


def test_the_reference_rotation_rejects_often():
    """(rot + 1) & 31 makes small outputs common (SURVEY #1): over many picks some are rejected."""
    total = sum(S.start_pixel(STREAM[0] + i, STREAM[1], 16, 2, False).rejections for i in range(8))
    assert total > 0


def test_camera_draws():
    assert [S.camera_draws(n) for n in range(6)] == [5, 2, 0, 0, 0, 0]


def test_frame_layout_and_states():
    f = film_of(17, 5)
    fr = S.frame(f, 2, 2, 2, False, tile_size=4)
    npx, ns = 17 * 5, 3
    assert fr.tables.shape == (npx, 2, 4) and len(fr.k) == npx * ns
    assert np.array_equal(fr.k[:6], [1, 2, 3, 1, 2, 3]) and np.array_equal(fr.table[:6], [0, 0, 0, 1, 1, 1])
    assert np.array_equal(fr.state, fr.start) and not fr.lens_u.any()   # n_dims 2: no camera draw
    # tile 4 is the ragged last column (1 pixel wide): its pixels advance in y
    first = int(np.nonzero(fr.tile == 4)[0][0])
    assert (fr.px[first], fr.py[first], fr.px[first + ns], fr.py[first + ns]) == (16, 0, 16, 1)
    one = S.frame(f, 2, 2, 1, True, tile_size=4, tile_begin=4, tile_end=6)
    assert np.array_equal(one.state, R.pcg_advance(one.start, one.inc, 2)) and one.lens_u.any()
    assert one.table[0] == 0 and one.tile[0] == 4 and one.table[-1] == 4 + 4 - 1   # tile 4: 1 x 4 pixels, tile 5: 4 x 1
    whole = S.frame(f, 2, 2, 1, True, tile_size=4)
    lo = int((whole.tile < 4).sum())
    assert np.array_equal(whole.tables[lo // ns:lo // ns + 8], one.tables)

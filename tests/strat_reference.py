"""Stratified.StartPixel restated in numpy / plain Python for one pixel on a given
PCG32 stream, from reading the reference (pkg/sampler/stratified.go:21-48,
pkg/pbrt/sampling.go:101-145, pkg/pbrt/rng.go:36-57). No GPU, no oracle and no
library here; tests/test_strat_reference_host.py pins each piece.

For each of n_dims 1D dimensions: StratifiedSample1D writes min((i + delta) / n,
1 - eps), delta a PCG32 float with jitter and 0.5 without, then ShuffleSamples1D
swaps samp[i] with samp[i + UniformUInt32(n - i)] for i = 0 .. n - 1. Then for
each of n_dims 2D dimensions StratifiedSample2D draws its 2 n jitter floats (with
jitter) into a copy, so the 2D values stay (0, 0), and the shuffle draws its n
bounded picks: only the stream advances. UniformUInt32(b) (pcg_bounded) rejects a
draw below 2^32 mod b, which the reference's (rot + 1) & 31 output rotation makes
common. Built on tests/li_reference.py's PCG32.
"""
from collections import namedtuple

import numpy as np

import li_reference as R

StartPixel = namedtuple("StartPixel", "s1d state draws rejections")


class Stream:
    """One PCG32 stream stepped literally, counting its draws."""

    def __init__(self, state, inc):
        self.state, self.inc, self.draws = int(state), int(inc), 0

    def next(self):
        """li_reference.pcg_next on Python integers (a pixel's StartPixel is thousands of dependent
        steps; tests/test_strat_reference_host.py holds the two equal)."""
        old = self.state
        self.state = (old * int(R.MULT) + self.inc) & 0xFFFFFFFFFFFFFFFF
        self.draws += 1
        xs = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
        rot = old >> 59
        return ((xs >> rot) | (xs << ((rot + 1) & 31))) & 0xFFFFFFFF

    def float(self):
        return min(self.next() * 2.3283064365386963e-10, R.ONE_MINUS_EPS)


def pcg_bounded(s, b):
    """rng.go:44-53: (the value in [0, b), the draws it rejected)."""
    threshold = ((1 << 32) - b) % b
    rejected = 0
    while True:
        v = s.next()
        if v >= threshold:
            return v % b, rejected
        rejected += 1


def start_pixel(state, inc, spp, n_dims, jitter):
    """StartPixel of one pixel on the stream (state, inc): the (n_dims, spp) table it leaves, the
    state after it, its PCG32 draws and how many of them pcg_bounded rejected."""
    s = Stream(state, inc)
    n = int(spp)
    table = np.zeros((n_dims, n))
    rejections = 0
    for d in range(n_dims):
        samp = table[d]
        for i in range(n):
            delta = s.float() if jitter else 0.5
            samp[i] = min((i + delta) * (1.0 / n), R.ONE_MINUS_EPS)
        for i in range(n):
            pick, rej = pcg_bounded(s, n - i)
            rejections += rej
            other = i + pick
            samp[i], samp[other] = samp[other], samp[i]
    for d in range(n_dims):
        if jitter:
            for _ in range(2 * n):
                s.next()
        for i in range(n):
            _, rej = pcg_bounded(s, n - i)
            rejections += rej
    return StartPixel(table, np.uint64(s.state), s.draws, rejections)


def camera_draws(n_dims):
    """PCG32 draws of GetCameraSample (pFilm, pLens: Get2D; time: Get1D) under n_dims sampled dimensions."""
    return (2 if n_dims < 1 else 0) + (2 if n_dims < 2 else 0) + (1 if n_dims < 1 else 0)


Frame = namedtuple("Frame", "tile pi px py tables k table inc start state lens_u lens_v")


def frame(film, sampler_x, sampler_y, n_dims, jitter, tile_size=16, tile_begin=0, tile_end=None):
    """What pbrt_gpu_frame_samples_stratified_device writes for the tiles [tile_begin, tile_end): per
    pixel of the range its table (StartPixel on mb_state(tile, pi, 0)), per traced sample k = 1 ..
    spp - 1 its pixel, k, table index, the start state mb_state(tile, pi, k), the state after the
    camera sample's draws and the lens values (drawn for n_dims = 1, else 0)."""
    spp = sampler_x * sampler_y
    nt = R.num_tiles(film, tile_size)
    tile_end = nt if tile_end is None else tile_end
    tiles, pis, pxs, pys, tables = [], [], [], [], []
    for t in range(tile_begin, tile_end):
        x0, y0, x1, y1 = R.tile_bounds(film, tile_size, t)
        for y in range(y0, y1):
            for x in range(x0, x1):
                pi = (y - y0) * (x1 - x0) + (x - x0)
                tiles.append(t)
                pis.append(pi)
                pxs.append(x)
                pys.append(y)
                tables.append(start_pixel(R.mb_state(t, pi, 0)[0], R.pcg_inc_of(t)[0], spp, n_dims, jitter).s1d)
    npx, ns = len(tiles), spp - 1
    rep = lambda a: np.repeat(np.asarray(a, dtype=np.int64), ns)   # noqa: E731
    tile, pi = rep(tiles), rep(pis)
    k = np.tile(np.arange(1, spp, dtype=np.int64), npx)
    inc = R.pcg_inc_of(tile)
    start = R.mb_state(tile, pi, k)
    st = start
    lens = [np.zeros(npx * ns), np.zeros(npx * ns)]
    if n_dims == 1:
        for j in range(2):
            st, lens[j] = R.pcg_float(st, inc)
    return Frame(tile, pi, rep(pxs), rep(pys), np.array(tables).reshape(npx, n_dims, spp), k.astype(np.int32),
                 rep(np.arange(npx)).astype(np.int32), inc, start, st, lens[0], lens[1])

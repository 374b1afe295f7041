"""The cases of tests/test_gpu_dtw.py and the condition that keeps them honest (tests/test_dtw_host.py): inputs by
dtw_reference.inputs at seed 1000 + 1000 T_a + T_b, the used columns set into wider rows whose other columns hold
values the call must not read.  The references are computed once per process and shared."""
import functools

import numpy as np

import dtw_reference as R

# strip and B-tile edges (64 rows of A, 64 rows of B), fewer columns than lanes, the single cell
RAGGED = ((1, 1), (1, 7), (7, 1), (2, 2), (64, 3), (3, 64), (63, 65), (64, 64), (65, 130), (129, 64), (128, 128), (200, 131))
RAGGED_SHAPE = dict(first=1, count=5, ld_a=7, ld_b=9)
WIDE = ((65, 66), (1, 1))
WIDE_SHAPE = dict(first=0, count=64, ld_a=64, ld_b=64)
# one pair of two strips at both ends of every padded count the kernel is built for (8, 16, 32, 48, 56, 64)
COUNTS = (1, 8, 9, 16, 17, 32, 33, 48, 49, 56, 57)
COUNTS_PAIR = (65, 66)
MIN_MARGIN = 1e-9


def embed(x, first, ld, fill):
    out = np.full((len(x), ld), fill, dtype=np.float32)
    out[:, first:first + x.shape[1]] = x
    return out


@functools.lru_cache(maxsize=None)
def pair(ta, tb, count):
    """(a, b) float32 over the used columns only, read-only."""
    a, b = R.inputs(ta, tb, count)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def reference(ta, tb, count, long_double=False):
    """(path, cost, margin) of pair(ta, tb, count) in float64 or long double."""
    a, b = pair(ta, tb, count)
    path, cost, margin = R.dtw(a, b, np.longdouble if long_double else np.float64)
    path.setflags(write=False)
    return path, cost, margin


def batch_rows(pairs, first, count, ld_a, ld_b):
    """The batch's two slabs: the pairs' used columns at `first` in rows of ld_a and ld_b, 1e30 in the other columns."""
    a = np.concatenate([embed(pair(ta, tb, count)[0], first, ld_a, 1e30) for ta, tb in pairs])
    b = np.concatenate([embed(pair(ta, tb, count)[1], first, ld_b, -1e30) for ta, tb in pairs])
    return a, b


def cost_bound(ta, tb, count, cost):
    """The rounding of a recursive sum of at most T_a + T_b - 1 positive terms, each the root of a count-term sum; the
    factor 2 because the library may fuse multiply-adds."""
    return 2.0 * (ta + tb - 1 + count + 2) * 2.0 ** -53 * abs(float(cost))

"""The definition of WorldMi355DtwAlign and WorldMi355FeatureDistortion (include/world_mi355.h) in numpy, written for a
dtype: np.float64 is the yardstick, np.longdouble says how far rounding can move it.  The reference tree holds no
evaluation code, so this statement is the reference.

dtw(a, b, dtype) also returns the path's margin: the smallest gap, over the cells on the path that have more than one
finite predecessor, between the best and the second-best one, divided by D at that cell.  A margin far above the rounding
of D means the path does not hang on rounding and may be compared exactly."""
import math

import numpy as np

DB = 10.0 / math.log(10.0)
CENTS = 1200.0 / math.log(2.0)


def inputs(ta, tb, width, seed=None):
    """Sequences that are worth aligning: each side takes its own sorted subset of the rows of one random walk and adds
    jitter.  float32 [ta][width], [tb][width]."""
    rng = np.random.default_rng(1000 + 1000 * ta + tb if seed is None else seed)
    n = 2 * max(ta, tb) + 4
    base = np.cumsum(0.1 * rng.standard_normal((n, width)), axis=0)
    out = []
    for t in (ta, tb):
        rows = np.sort(rng.choice(n, size=t, replace=False))
        out.append((base[rows] + 0.02 * rng.standard_normal((t, width))).astype(np.float32))
    return out[0], out[1]


def distances(a, b, dtype=np.float64):
    """d(i, j) over all the columns given, the sum in ascending k."""
    a, b = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    s = np.zeros((len(a), len(b)), dtype=dtype)
    for k in range(a.shape[1]):
        df = a[:, k][:, None] - b[:, k][None, :]
        s = s + df * df
    return np.sqrt(s)


def dtw(a, b, dtype=np.float64):
    """(path [len][2] int32 in forward order, cost, margin) of the columns given; rows of a and b, both non-empty."""
    d = distances(a, b, dtype)
    ta, tb = d.shape
    inf = dtype(np.inf)
    D = np.full((ta, tb), inf, dtype=dtype)
    for i in range(ta):
        for j in range(tb):
            if i == 0 and j == 0:
                best = dtype(0)
            else:
                best = min(D[i - 1, j - 1] if i and j else inf, D[i - 1, j] if i else inf, D[i, j - 1] if j else inf)
            D[i, j] = d[i, j] + best
    path, margin = [], math.inf
    i, j = ta - 1, tb - 1
    while True:
        path.append((i, j))
        if i == 0 and j == 0:
            break
        if i > 0 and j > 0:
            cand = [(D[i - 1, j - 1], 0), (D[i - 1, j], 1), (D[i, j - 1], 2)]
            best = min(cand, key=lambda c: (c[0], c[1]))           # on equality the diagonal, then (i-1, j)
            others = sorted(c[0] for c in cand if c[1] != best[1])
            if np.isfinite(others[0]) and D[i, j] > 0:
                margin = min(margin, float((others[0] - best[0]) / D[i, j]))
            step = best[1]
        else:
            step = 1 if j == 0 else 2
        if step == 0:
            i, j = i - 1, j - 1
        elif step == 1:
            i -= 1
        else:
            j -= 1
    return np.asarray(path[::-1], dtype=np.int32), D[ta - 1, tb - 1], margin


def brute_force_cost(a, b):
    """The smallest sum of d over every monotone path from (0, 0) to the last cell, by enumeration."""
    d = distances(a, b)
    ta, tb = d.shape

    def go(i, j):
        if i == 0 and j == 0:
            return [d[0, 0]]
        out = []
        for pi, pj in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):
            if pi >= 0 and pj >= 0:
                out.extend(c + d[i, j] for c in go(pi, pj))
        return out

    return min(go(ta - 1, tb - 1))


def truncation(ta, tb):
    n = min(ta, tb)
    return np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.int32)


def distortion(a, b, pairs, kind, mask=None, voiced_above=-1e9, dtype=np.float64):
    """The four slots of one group and one utterance along `pairs`, the sums in pair order in `dtype`.  a, b: the group's
    columns only."""
    a, b = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    s0, s1, n0, n1, n2 = dtype(0), dtype(0), 0, 0, 0
    for i, j in np.asarray(pairs).reshape(-1, 2):
        if mask is not None and not mask[j]:
            continue                                                # adds 0: the sum stays as it is
        n0 += 1
        if kind == 0:
            s = dtype(0)
            for k in range(a.shape[1]):
                df = a[i, k] - b[j, k]
                s = s + df * df
            e = dtype(DB) * np.sqrt(dtype(2) * s)
            s0, s1 = s0 + e, s1 + e * e
        else:
            va, vb = a[i, 0] > voiced_above, b[j, 0] > voiced_above
            if va and vb:
                df = a[i, 0] - b[j, 0]
                s0, n1 = s0 + df * df, n1 + 1
            elif va != vb:
                n2 += 1
    if kind == 0:
        return np.array([s0, s1, n0, 0], dtype=dtype)
    return np.array([s0, n1, n2, n0], dtype=dtype)


def pooled(rows, kinds):
    """pool_distortion's figures computed directly from [n_utt][n_groups][4] rows."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, len(kinds), 4)
    out = []
    for g, kind in enumerate(kinds):
        c = [math.fsum(rows[:, g, k].tolist()) for k in range(4)]
        if kind == 0:
            out.append({"mean_db": c[0] / c[2] if c[2] else math.nan, "pairs": int(c[2])})
        else:
            out.append({"rmse_cents": CENTS * math.sqrt(c[0] / c[1]) if c[1] else math.nan,
                        "vuv_error_percent": 100.0 * c[2] / c[3] if c[3] else math.nan, "voiced_pairs": int(c[1]),
                        "pairs": int(c[3])})
    return out

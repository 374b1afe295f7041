"""The recipe's `ffo` and `stats` stages and make_data_gv's statistic, stated in numpy: the yardstick of
tests/test_ffo_host.py, tests/test_gpu_ffo.py and tests/test_recipe_ffo.py.  A helper, not a test.

    interpolate   data/scripts/interpolate.pl:68-105 and the voicing flag of data/Makefile.in:347/:381
    window        data/scripts/window.pl:45-146 for one stream
    ffo_rows      the row of recipe.ffo_layout: per stream [voicing flag, if any][window 0 | window 1 | ...]
    moments       count, mean and sum of squared deviations per column, two passes in np.longdouble
    pooled        the variance of the union of parts, from their long-double moments
    gv            the variance across utterances of the per-utterance variances

Nothing here knows how the library orders its sums; variances divide by n.
"""
import numpy as np

LD = np.longdouble
RECIPE = [[1.0], [-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]]                        # data/win/*.win1 .. win3


def interpolate(x, ignore_value=-1.0e10):
    """x float32 [T][dim] of one utterance.  Returns (out float32 [T][dim], voiced float32 [T], status): a gap is a
    value equal to float32(ignore_value); between the valid frames lo < t < hi it becomes float32(a + step (t - lo)) in
    float64, a leading gap the first valid value, a trailing gap the last.  status 1: a column without a valid value
    (zeros), where the script dies."""
    x = np.asarray(x, dtype=np.float32)
    T, dim = x.shape
    ig = np.float32(ignore_value)
    out = x.copy()
    status = 0
    for c in range(dim):
        col = x[:, c]
        valid = np.nonzero(~(col == ig))[0]                                 # NaN is a value
        if len(valid) == 0:
            out[:, c] = 0.0
            status |= 1
            continue
        for t in range(T):
            if not (col[t] == ig):
                continue
            k = np.searchsorted(valid, t)
            if k == 0:
                out[t, c] = col[valid[0]]
            elif k == len(valid):
                out[t, c] = col[valid[-1]]
            else:
                lo, hi = int(valid[k - 1]), int(valid[k])
                a = np.float64(col[lo])
                step = (np.float64(col[hi]) - a) / np.float64(hi - lo)
                out[t, c] = np.float32(a + step * np.float64(t - lo))
    voiced = (~(x[:, 0] == ig)).astype(np.float32)
    return out, voiced, status


def window(x, windows):
    """window.pl on one utterance of one stream: float32 [T][len(windows) * dim], frames clamped to the utterance,
    float64 accumulation in tap order; -1e10 under a tap inside the window's non-zero span gives -1e10."""
    x = np.asarray(x, dtype=np.float32)
    T, dim = x.shape
    out = np.zeros((T, len(windows) * dim), dtype=np.float32)
    for i, w in enumerate(windows):
        size, h = len(w), (len(w) - 1) // 2
        nz = [k for k, v in enumerate(w) if v != 0.0]
        first, last = (nz[0], nz[-1]) if nz else (size, -1)
        for t in range(T):
            for j in range(dim):
                acc, boundary = np.float64(0.0), False
                for k in range(size):
                    v = np.float64(x[min(max(t + k - h, 0), T - 1), j])
                    if first <= k <= last and v == -1.0e10:
                        boundary = True
                    acc = acc + np.float64(w[k]) * v
                out[t, i * dim + j] = np.float32(-1.0e10) if boundary else np.float32(acc)
    return out


def ffo_rows(feats, streams, ignore_value=-1.0e10):
    """One utterance.  feats: float32 [T][dim_s] per stream; streams: [(dim, windows, msd)].  Returns (rows float32
    [T][row width], status)."""
    blocks, status = [], 0
    for x, (dim, wins, msd) in zip(feats, streams):
        x = np.asarray(x, dtype=np.float32).reshape(-1, dim)
        if msd:
            x, voiced, st = interpolate(x, ignore_value)
            status |= st
            blocks.append(voiced[:, None])
        blocks.append(window(x, wins))
    return np.concatenate(blocks, axis=1), status


def moments(x, ignore_value=None):
    """Per column of x [T][width]: (count int64, mean, m2) in long double, two passes: the mean of the kept values,
    then the sum of their squared deviations from it.  A count of 0 gives 0, 0."""
    x = np.asarray(x, dtype=np.float32)
    width = x.shape[1]
    cnt, mean, m2 = np.zeros(width, dtype=np.int64), np.zeros(width, dtype=LD), np.zeros(width, dtype=LD)
    for c in range(width):
        col = x[:, c]
        if ignore_value is not None:
            col = col[~(col == np.float32(ignore_value))]
        cnt[c] = len(col)
        if len(col):
            v = col.astype(LD)
            mean[c] = v.sum() / LD(len(v))
            m2[c] = ((v - mean[c]) ** 2).sum()
    return cnt, mean, m2


def pooled(parts):
    """(n, mean, m2) of the union of parts = [(count, mean, m2)] in long double."""
    n = sum(np.asarray(p[0], dtype=np.int64) for p in parts)
    nl = np.maximum(n, 1).astype(LD)
    mean = sum(np.asarray(p[0]).astype(LD) * np.asarray(p[1], dtype=LD) for p in parts) / nl
    m2 = sum(np.asarray(p[2], dtype=LD) + np.asarray(p[0]).astype(LD) * (np.asarray(p[1], dtype=LD) - mean) ** 2
             for p in parts)
    return n, np.where(n > 0, mean, LD(0)), np.where(n > 0, m2, LD(0))


def corpus_variance(utterances):
    """The variance of every column over all rows of all utterances (long double), `cat ffo/* | vstat -d -o 2`."""
    cnt, _, m2 = moments(np.concatenate(utterances))
    return m2 / cnt.astype(LD)


def gv(utterances):
    """The variance across utterances of the per-utterance column variances (long double)."""
    v = np.stack([m[2] / m[0].astype(LD) for m in (moments(u) for u in utterances)])
    return ((v - v.mean(axis=0)) ** 2).sum(axis=0) / LD(len(utterances))


def large_offset_case():
    """float32 [300][1] around 1e4 with a spread of 1e-2: the column that defeats sum x^2 - (sum x)^2 / T in double.
    Asserted here: that expression misses the long-double m2 by more than 1000 times the two-pass bound
    (T + 4) 2^-52."""
    rng = np.random.default_rng(11)
    x = (1.0e4 + 1.0e-2 * rng.standard_normal((300, 1))).astype(np.float32)
    v = x[:, 0].astype(np.float64)
    naive = (v * v).sum() - v.sum() ** 2 / len(v)
    ref = float(moments(x)[2][0])
    assert abs(naive - ref) / ref > 1000.0 * (len(v) + 4) * 2.0 ** -52, (naive, ref)
    return x

"""Parameter generation (SPTK `mlpg`) stated densely in numpy float64: the yardstick of tests/test_mlpg_host.py,
tests/test_gpu_mlpg.py and tests/test_recipe_gen_param.py.  A helper, not a test.

One column is one utterance, one stream and one dimension, with T frames and the stream's windows w_0 .. w_{n-1} (odd
sizes, centre tap h_i = (size_i - 1) / 2):

    W   the (n T) x T matrix whose row (t, i) holds w_i[k] at column t + k - h_i
        edge 0: a tap whose column falls outside [0, T) is dropped (SPTK mlpg)
        edge 1: the column is clamped to [0, T - 1], taps accumulate on the end frames (window.pl, cmp_compose_kernel)
    mu  the n T means, P the diagonal matrix of precisions 1 / variance
    c   solves (W' P W) c = W' P mu

W is built row by row and every column is solved by np.linalg.solve: nothing here knows that R = W' P W is banded.
"""
import functools

import numpy as np

STATIC = [[1.0]]
RECIPE = [[1.0], [-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]]                        # data/win/*.win1 .. win3
FIVE = [[1.0], [-0.2, -0.1, 0.0, 0.1, 0.2], [2 / 7, -1 / 7, -2 / 7, -1 / 7, 2 / 7]]
RAMP15 = [[1.0], [(k - 7) / 280.0 for k in range(15)]]                      # 15 taps: the widest a stream may have
ZERO_ENDS = [[0.0, 1.0, 0.0], [0.0, -0.5, 0.0, 0.5, 0.0]]                    # zero taps at both ends of a window
WINDOW_SETS = {"static": STATIC, "recipe": RECIPE, "five": FIVE, "ramp15": RAMP15, "zero_ends": ZERO_ENDS}


def window_matrix(T, windows, edge=0):
    """W, (len(windows) * T) x T, row t * n + i for frame t and window i."""
    n = len(windows)
    W = np.zeros((n * T, T))
    for t in range(T):
        for i, w in enumerate(windows):
            assert len(w) % 2 == 1
            h = (len(w) - 1) // 2
            for k, wk in enumerate(w):
                c = t + k - h
                if edge == 1:
                    W[t * n + i, min(max(c, 0), T - 1)] += wk
                elif 0 <= c < T:
                    W[t * n + i, c] += wk
    return W


def normal_matrix(W, prec):
    """R = W' P W and the factor W' P of the right-hand side, for one column's precisions (n T of them)."""
    WtP = W.T * prec[None, :]
    return WtP @ W, WtP


def precisions(var, input_type=0):
    """float64 precisions from float32 variances (input_type 0) or precisions (1), as the library reads them."""
    v = np.asarray(var, dtype=np.float32).astype(np.float64)
    return v if input_type else 1.0 / v


def mlpg(mean, var, windows, edge=0, input_type=0, want_cond=True):
    """One utterance of one stream.  mean: [T][n * dim] laid [window 0: dim | window 1: dim | ...]; var: the same
    shape, or [n * dim] for one row used at every frame.  Returns (c float64 [T][dim], cond(R) per column [dim])."""
    mean = np.asarray(mean, dtype=np.float32).astype(np.float64)
    T, n = mean.shape[0], len(windows)
    dim = mean.shape[1] // n
    assert mean.shape[1] == n * dim
    prec = np.broadcast_to(precisions(var, input_type), mean.shape)
    W = window_matrix(T, windows, edge)
    out, cond = np.zeros((T, dim)), np.zeros(dim)
    for d in range(dim):
        mu = mean[:, d::dim].reshape(-1)                                    # (t, i) order, as W's rows
        R, WtP = normal_matrix(W, np.ascontiguousarray(prec[:, d::dim]).reshape(-1))
        out[:, d] = np.linalg.solve(R, WtP @ mu)
        if want_cond:
            cond[d] = np.linalg.cond(R)
    return out, cond


def mlpg_batch(lengths, mean, var, windows, edge=0, input_type=0, var_per_frame=False, want_cond=True):
    """mlpg over the concatenated frames of a batch.  Returns (c [sum T][dim], cond [n_utt][dim])."""
    off = np.concatenate([[0], np.cumsum(lengths)])
    outs, conds = [], []
    for u in range(len(lengths)):
        a, b = off[u], off[u + 1]
        c, k = mlpg(mean[a:b], var[a:b] if var_per_frame else var, windows, edge, input_type, want_cond)
        outs.append(c)
        conds.append(k)
    return np.concatenate(outs), np.stack(conds)


def bound(c, cond):
    """The issue's error bound per column: spacing(float32(max|c|)) + 64 cond 2^-53 max|c| -- the rounding of the
    float32 output plus a banded factorisation's error in double."""
    big = np.abs(c).max(axis=0)
    return np.spacing(big.astype(np.float32)).astype(np.float64) + 64.0 * cond * 2.0 ** -53 * big


def batch_bound(lengths, c, cond):
    """bound() per utterance, spread over its frames: [sum T][dim]."""
    off = np.concatenate([[0], np.cumsum(lengths)])
    return np.concatenate([np.broadcast_to(bound(c[off[u]:off[u + 1]], cond[u]), (lengths[u], c.shape[1]))
                           for u in range(len(lengths))])


def random_walk(rng, T, dim, scale=1.0):
    """float32 [T][dim]: a random walk, the shape of a static feature track."""
    return (scale * (rng.standard_normal((1, dim)) * 3.0 + np.cumsum(rng.standard_normal((T, dim)), axis=0) * 0.3)
            ).astype(np.float32)


def make_stream(seed, lengths, dim, windows, var_per_frame=False):
    """Deterministic means and variances of one stream over a batch: static means a random walk, dynamic means the
    windows of another walk plus noise (so that they are of a track's size but not consistent with the statics),
    variances log-uniform in 1e-3 .. 1e3.  Returns (mean float32 [sum T][n dim], var float32 [n dim] or [sum T][n dim])."""
    rng = np.random.default_rng(seed)
    n = len(windows)
    rows = []
    for T in lengths:
        walk = random_walk(rng, T, dim).astype(np.float64)
        m = (window_matrix(T, windows, 1) @ walk).reshape(T, n * dim) + 0.1 * rng.standard_normal((T, n * dim))
        rows.append(m.astype(np.float32))
    mean = np.concatenate(rows)
    shape = mean.shape if var_per_frame else (n * dim,)
    var = (10.0 ** rng.uniform(-3.0, 3.0, shape)).astype(np.float32)
    return mean, var


def compose(x, windows, edge=1):
    """float32 cmp rows [T][n dim] of a float32 track x [T][dim] by the window matrix (edge 1: window.pl's)."""
    T, dim = x.shape
    return (window_matrix(T, windows, edge) @ x.astype(np.float64)).reshape(T, len(windows) * dim).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cached_reference(seed, lengths, dim, set_name, var_per_frame, edge, input_type):
    """(mean, var as given to the library, c, cond) of make_stream's case, computed once per process.  With
    input_type 1 the library is given the exact float32 reciprocals of the variances, and so is the helper."""
    mean, var = make_stream(seed, lengths, dim, WINDOW_SETS[set_name], var_per_frame)
    if input_type:
        var = (np.float32(1.0) / var).astype(np.float32)
    c, cond = mlpg_batch(list(lengths), mean, var, WINDOW_SETS[set_name], edge, input_type, var_per_frame)
    for a in (mean, var, c, cond):
        a.setflags(write=False)
    return mean, var, c, cond

"""Parameter generation considering global variance, stated in numpy: the yardstick of tests/test_mlpg_gv_host.py,
tests/test_gpu_mlpg_gv.py and the recipe tests of `gen-param-gv`.  A helper, not a test.  Parity with HTS is unpinned:
this definition (include/world_mi355.h, WorldMi355ParameterGenerationGv) is the yardstick.

A column is one utterance, one stream and one dimension with T frames and the stream's n windows.  R = W' P W and
r = W' P mu are parameter generation's (tests/mlpg_reference.py: window_matrix), built here by their bands so that a
long double evaluation stays cheap.  G is the set of frames that are voiced and not masked, N = |G|.

    start      c = c0, the float32 trajectory of parameter generation before its voicing overwrite
    moments    m = sum_G c_t / N,  e_t = c_t - m on G, else 0,  v = sum e_t^2 / N
    objective  f(c) = wh w (-1/2 c'Rc + c'r) - 1/2 wg p_v (v - mu_v)^2,  w = 1 / (n T)
    scaling    c_t <- m + sqrt(mu_v / v) e_t on G, once before the loop
    direction  g = wh w (r - Rc) - wg p_v (v - mu_v) (2 / N) e
               H = -wh w diag(R) - [G] wg (2 / N^2) p_v ((N - 1)(v - mu_v) + 2 e^2),  d = g / max(-H, 1e-3 wh w diag(R))
    loop       step = step_init; trial k = 1 .. max_iter: c' = c + step d; f(c') >= f(c): accept, step *= step_inc, stop when
               epsilon > 0 and (f(c') - f(c)) / |f(c')| < epsilon; else step *= step_dec.  d is recomputed after an accept.

Every function takes the dtype it computes in (np.float64 or np.longdouble) and works on all columns of a stream at once.
"""
import numpy as np

DEFAULTS = dict(max_iter=50, epsilon=1e-4, step_init=1.0, step_inc=1.2, step_dec=0.5, hmm_weight=1.0, gv_weight=1.0, scale=1)
STATUS_BAD_GV, STATUS_DEGENERATE = 1, 4


def normal_bands(mean, var, windows, edge, input_type, dtype):
    """(Rb [2B + 1][T][dim] with Rb[B + j][t] = R[t][t + j], r [T][dim]) of one utterance of one stream.  mean [T][n dim]
    float32; var the same shape or one row."""
    mean = np.asarray(mean, dtype=np.float32).astype(dtype)
    T, n = mean.shape[0], len(windows)
    dim = mean.shape[1] // n
    v = np.broadcast_to(np.asarray(var, dtype=np.float32).astype(dtype), mean.shape)
    prec = v if input_type else dtype(1.0) / v
    B = 2 * max((len(w) - 1) // 2 for w in windows)
    Rb, r = np.zeros((2 * B + 1, T, dim), dtype=dtype), np.zeros((T, dim), dtype=dtype)
    tau = np.arange(T)
    for i, w in enumerate(windows):
        h = (len(w) - 1) // 2
        p, mu = prec[:, i * dim:(i + 1) * dim], mean[:, i * dim:(i + 1) * dim]
        cols, ok = [], []
        for k in range(len(w)):
            c = tau + k - h
            ok.append(np.ones(T, dtype=bool) if edge == 1 else (c >= 0) & (c < T))
            cols.append(np.clip(c, 0, T - 1))
        for k1, w1 in enumerate(w):
            a1 = dtype(w1)
            np.add.at(r, cols[k1][ok[k1]], (p * a1 * mu)[ok[k1]])
            for k2, w2 in enumerate(w):
                both = ok[k1] & ok[k2]
                np.add.at(Rb, (cols[k2][both] - cols[k1][both] + B, cols[k1][both]), (p * (a1 * dtype(w2)))[both])
    return Rb, r


def band_times(Rb, c):
    """R c for the bands of normal_bands."""
    B, T = (Rb.shape[0] - 1) // 2, c.shape[0]
    out = np.zeros_like(c)
    for j in range(-B, B + 1):
        lo, hi = max(0, -j), min(T, T - j)
        if hi > lo:
            out[lo:hi] += Rb[B + j, lo:hi] * c[lo + j:hi + j]
    return out


def generate(c0, Rb, r, n_windows, member, gv_mean, gv_var, dtype=np.float64, max_iter=50, epsilon=1e-4, step_init=1.0,
             step_inc=1.2, step_dec=0.5, hmm_weight=1.0, gv_weight=1.0, scale=1):
    """The loop on all columns of one utterance of one stream.  c0 float32 [T][dim]; member bool [T] (the GV set).
    Returns a dict: c [T][dim] in dtype (before the float32 rounding and the voicing overwrite), status [dim], f0, f1,
    trials, accepts [dim], gains (per column the list of relative gains of its accepted trials) and margins (per
    column the list of |f' - f| / |f| of every trial)."""
    T, dim = c0.shape
    G = np.asarray(member, dtype=bool)
    N = int(G.sum())
    c = np.asarray(c0, dtype=np.float32).astype(dtype)
    mu_v = np.asarray(gv_mean, dtype=np.float32).astype(dtype)
    gvv = np.asarray(gv_var, dtype=np.float32).astype(dtype)
    status = np.zeros(dim, dtype=np.int64)
    bad = ~((mu_v > 0) & np.isfinite(mu_v) & (gvv > 0) & np.isfinite(gvv))
    status[bad] |= STATUS_BAD_GV
    wh, wg = dtype(hmm_weight) / (dtype(n_windows) * dtype(T)), dtype(gv_weight)
    Gc = G[:, None]

    def moments(x):
        m = np.where(Gc, x, 0).sum(axis=0) / dtype(max(N, 1))
        e = np.where(Gc, x - m, 0)
        return m, e, (e * e).sum(axis=0) / dtype(max(N, 1))

    with np.errstate(all="ignore"):
        m, e, v = moments(c)
        degenerate = ~bad & ((N < 2) | ~((v > 0) & np.isfinite(v)))
        status[degenerate] |= STATUS_DEGENERATE
        live = status == 0
        p_v = np.where(live, dtype(1.0) / np.where(live, gvv, 1), 0)
        mu_v = np.where(live, mu_v, 1)

        def objective(x):
            m, e, v = moments(x)
            return wh * (dtype(-0.5) * (x * band_times(Rb, x)).sum(axis=0) + (x * r).sum(axis=0)) \
                - dtype(0.5) * wg * p_v * (v - mu_v) ** 2

        def direction(x):
            m, e, v = moments(x)
            diag = Rb[(Rb.shape[0] - 1) // 2]
            dv = v - mu_v
            g = wh * (r - band_times(Rb, x)) - wg * p_v * dv * (dtype(2.0) / dtype(N)) * e
            H = -wh * diag - np.where(Gc, wg * (dtype(2.0) / dtype(N * N)) * p_v * (dtype(N - 1) * dv + dtype(2.0) * e * e), 0)
            return g / np.maximum(-H, dtype(1e-3) * wh * diag)

        if scale:
            k = np.sqrt(mu_v / np.where(live, v, 1))
            c = np.where(Gc & live[None, :], m + k * e, c)
        f = objective(c)
        f0 = f.copy()
        step = np.full(dim, dtype(step_init), dtype=dtype)
        trials, accepts = np.zeros(dim, dtype=np.int64), np.zeros(dim, dtype=np.int64)
        gains, margins = [[] for _ in range(dim)], [[] for _ in range(dim)]
        run = live.copy()
        d = direction(c) if max_iter > 0 else np.zeros_like(c)
        for _ in range(max_iter):
            if not run.any():
                break
            cn = c + step * d
            fn = objective(cn)
            acc = run & (fn >= f)
            rej = run & ~acc
            gain = (fn - f) / np.abs(fn)
            for j in np.nonzero(run)[0]:
                margins[j].append(float(abs(fn[j] - f[j]) / abs(f[j])) if f[j] != 0 else np.inf)
            for j in np.nonzero(acc)[0]:
                gains[j].append(float(gain[j]))
            trials[run] += 1
            accepts[acc] += 1
            c = np.where(acc[None, :], cn, c)
            f = np.where(acc, fn, f)
            step = np.where(acc, step * dtype(step_inc), np.where(rej, step * dtype(step_dec), step))
            if epsilon > 0:
                run = run & ~(acc & (gain < dtype(epsilon)))
            if acc.any():
                d = np.where(acc[None, :], direction(c), d)
    f0 = np.where(live, f0, 0)
    f = np.where(live, f, 0)
    c = np.where(live[None, :], c, np.asarray(c0, dtype=np.float32).astype(dtype))
    return dict(c=c, status=status, f0=f0, f1=f, trials=trials, accepts=accepts, gains=gains, margins=margins)


def finish(c, voiced, unvoiced_value):
    """The output: float32(c), unvoiced_value in the unvoiced frames (voiced None: a stream without msd)."""
    out = np.asarray(c, dtype=np.float64).astype(np.float32)
    if voiced is not None:
        out[~np.asarray(voiced, dtype=bool)] = np.float32(unvoiced_value)
    return out


def variance_over(c, member):
    """v of every column over the GV set: [dim]."""
    x = np.asarray(c, dtype=np.float64)[np.asarray(member, dtype=bool)]
    return ((x - x.mean(axis=0)) ** 2).mean(axis=0)


def bound(ref64, sens):
    """Per column: spacing(float32(max|c|)) + max(10 sens, 64 ulp of max|c| in double)."""
    big = np.abs(ref64).max(axis=0)
    return np.spacing(big.astype(np.float32)).astype(np.float64) + np.maximum(10.0 * sens, 64.0 * np.spacing(big))

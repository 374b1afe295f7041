"""The MGC-LSP route of include/world_mi355.h in numpy, one row at a time: lspcheck's steps, lsp2lpc, the way on to MGC
rows through tests/mgc2mgc_reference.py, and postfiltering_lsp (scripts/Training.pl:2690-2752).  SPTK's lspcheck and
lsp2lpc are not in the reference tree: this file IS the definition the library is held to (parity with SPTK's commands is
unpinned).  The check and the filter step are float64 always -- their results are defined bit for bit; lsp2lpc and what
follows it run in np.float64 (what the tests compare with) or np.longdouble (figure (b) of `sens`).

Also the seeded rows of the GPU tests, and `sens`: per row the larger of (a) the restatement's response to a last-bit
change of its input -- every checked LSP and the gain moved to a neighbouring double, the direction seeded -- and (b)
its distance from the same chain in np.longdouble."""
import math

import numpy as np

import mgc2mgc_reference as M

F64 = np.float64
LD = np.longdouble
PI = F64(np.pi)

CHANGED, RAISED, NONFINITE_IN, NONFINITE_OUT, UNORDERED = 1, 2, 4, 8, 16


def distance(m, r):
    """d = r pi / (m + 1), in that expression."""
    return F64(r) * PI / F64(m + 1)


def check(x, r=0.1, G=1e-10, log_gain=False):
    """lspcheck -c -r r -g -G G [-L] of one row: (checked row, K, status).  K is exp(x[0]) under log_gain as numpy
    rounds it; the device library's exp may round it otherwise, which only the LPC row's K sees."""
    x = np.array(x, dtype=F64)
    m = len(x) - 1
    if not np.isfinite(x).all():
        return np.zeros(m + 1), F64(0), NONFINITE_IN
    st = 0
    w = x[1:].copy()
    # range
    w = np.abs(w)
    w = np.where(w > PI, F64(2) * PI - w, w)
    changed = bool((w != x[1:]).any())
    # order
    s = np.sort(w, kind="stable")
    changed = changed or bool((s != w).any())
    w = s
    # distance: one pass
    d = distance(m, r)
    before = w.copy()
    for i in range(m - 1):
        t = w[i + 1] - w[i]
        if t < d:
            h = F64(0.5) * (d - t)
            w[i] = w[i] - h
            w[i + 1] = w[i + 1] + h
    changed = changed or bool((w != before).any())
    if changed:
        st |= CHANGED
    if not (w[0] > 0 and w[-1] < PI and (np.diff(w) > 0).all()):
        st |= UNORDERED
    # gain
    with np.errstate(all="ignore"):
        K = np.exp(x[0]) if log_gain else x[0]
    gain = x[0]
    if K < F64(G):
        K = F64(G)
        gain = F64(math.log(G)) if log_gain else F64(G)
        st |= RAISED
    return np.concatenate([[gain], w]), K, st


def factor_order(m):
    """The order in which lsp2lpc takes the quadratic factors f_1 .. f_m: P's (odd i) and Q's (even i) in turn, each
    polynomial's own in the bit-reversed order of their positions -- position j = 0, 1, ... among its factors in
    ascending i, sorted by the reversal of j's binary digits over ceil(log2 n) bits.  The partial products then have
    their roots spread around the circle and stay small; in ascending i they grow to 1e8 at order 63 and the sum
    P + Q loses every digit (tests/test_lsp_host.py measures both)."""
    def reversed_positions(n):
        bits = max(1, (n - 1).bit_length())
        return sorted(range(n), key=lambda j: int(format(j, "0%db" % bits)[::-1], 2))

    odd, even = list(range(1, m + 1, 2)), list(range(2, m + 1, 2))
    p = [odd[j] for j in reversed_positions(len(odd))]
    q = [even[j] for j in reversed_positions(len(even))] if even else []
    order = []
    for t in range(len(p)):
        order.append(p[t])
        if t < len(q):
            order.append(q[t])
    return order


def lsp2lpc(w, dt=F64, order=None):
    """a[0 .. m] of A = (P + Q) / 2, a[0] = 1: the quadratic factors in factor_order(m) (or `order`), then the further
    factor; every step (c[k] + p c[k-1]) + c[k-2]."""
    w = np.asarray(w, dtype=dt)
    m = len(w)
    n = m + 1                                            # coefficients 0 .. m; what lies beyond is never read back
    P = np.zeros(n, dtype=dt)
    Q = np.zeros(n, dtype=dt)
    P[0] = Q[0] = 1
    pw = dt(-2) * np.cos(w)

    def shifted(c, by):
        return np.concatenate([np.zeros(by, dtype=dt), c[:n - by]])

    for i in factor_order(m) if order is None else order:
        if i & 1:
            P = (P + pw[i - 1] * shifted(P, 1)) + shifted(P, 2)
        else:
            Q = (Q + pw[i - 1] * shifted(Q, 1)) + shifted(Q, 2)
    if m & 1:
        Q = Q - shifted(Q, 2)
    else:
        P = P + shifted(P, 1)
        Q = Q - shifted(Q, 1)
    return dt(0.5) * (P + Q)


def polynomials(w):
    """P and Q in full, degree m + 1 each, by np.polymul over the factors in factor_order(m): for the root tests only."""
    m = len(w)
    P, Q = np.ones(1), np.ones(1)
    for i in factor_order(m):
        f = np.array([1.0, -2.0 * np.cos(w[i - 1]), 1.0])
        if i & 1:
            P = np.polymul(P, f)
        else:
            Q = np.polymul(Q, f)
    if m & 1:
        Q = np.polymul(Q, [1.0, 0.0, -1.0])
    else:
        P = np.polymul(P, [1.0, 1.0])
        Q = np.polymul(Q, [1.0, -1.0])
    return P, Q


def lpc_of_checked(checked, K, dt=F64):
    return np.concatenate([[dt(K)], lsp2lpc(checked[1:], dt)[1:]])


def to_lpc(x, r=0.1, G=1e-10, log_gain=False, dt=F64):
    """(LPC row [K, a_1 .. a_m], checked row, status) -- zeros for a flagged row."""
    checked, K, st = check(x, r, G, log_gain)
    if st & NONFINITE_IN:
        return np.zeros(len(checked), dtype=dt), checked, st
    with np.errstate(all="ignore"):
        lpc = lpc_of_checked(checked, K, dt)
    if not np.isfinite(lpc.astype(F64)).all():
        return np.zeros(len(checked), dtype=dt), np.zeros(len(checked)), st | NONFINITE_OUT
    return lpc, checked, st


def lpc_to_mgc(lpc, alpha, gamma, out_order, out_alpha, out_gamma, dt=F64):
    """mgc2mgc -n -u of an LPC row, plain output."""
    m = len(lpc) - 1
    opt = M.option(m, alpha, gamma, out_order, out_alpha, out_gamma, n=1, u=1)
    return M.convert_rows(np.asarray(lpc, dtype=dt)[None], opt, dt)[0]


def energy(lpc, alpha, gamma, length, dt=F64):
    """1/2 ln sum_{k < L} c2[k]^2, c2 = mgc2mgc -n -u towards (L - 1, 0, 1): the sum by math.fsum."""
    c2 = lpc_to_mgc(lpc, alpha, gamma, length - 1, 0.0, 1.0, dt)
    if dt is LD:
        return np.log((c2 * c2).sum(dtype=LD)) / 2
    return F64(0.5) * F64(math.log(math.fsum(float(v) * float(v) for v in c2)))


def filter_row(x, beta):
    """[gain, p] of postfiltering_lsp, from the row as it is."""
    x = np.array(x, dtype=F64)
    m = len(x) - 1
    beta = F64(beta)
    p = x.copy()
    for i in range(2, m):
        d1 = beta * (x[i + 1] - x[i])
        d2 = beta * (x[i] - x[i - 1])
        if d1 == 0 and d2 == 0:
            continue
        p[i] = x[i - 1] + d2 + (d2 * d2 * ((x[i + 1] - x[i - 1]) - (d1 + d2))) / ((d2 * d2) + (d1 * d1))
    return p


def postfilter(x, alpha, gamma, beta, length, r=0.1, G=1e-10, log_gain=False, compensation=False, energies=False):
    """(out row, ene1, ene2, status) of one row; the energies are 0 where none is computed."""
    x = np.array(x, dtype=F64)
    m = len(x) - 1
    if beta == 1 or m <= 2:
        return x.copy(), F64(0), F64(0), 0
    if not np.isfinite(x).all():
        return np.zeros(m + 1), F64(0), F64(0), NONFINITE_IN
    with np.errstate(all="ignore"):
        out = filter_row(x, beta)
        if not np.isfinite(out).all():
            return np.zeros(m + 1), F64(0), F64(0), NONFINITE_OUT
        if not (compensation or energies):
            return out, F64(0), F64(0), 0
        lpc1, _, st1 = to_lpc(x, r, G, log_gain)
        lpc2, _, st2 = to_lpc(out, r, G, log_gain)
        st = st1 | st2
        e1 = energy(lpc1, alpha, gamma, length) if not st & 12 else F64(np.nan)
        e2 = energy(lpc2, alpha, gamma, length) if not st & 12 else F64(np.nan)
        g = out[0]
        if compensation:
            g = g + (e1 - e2) if log_gain else g * np.exp(e1 - e2)
    if st & 12 or not (np.isfinite(e1) and np.isfinite(e2) and np.isfinite(g)):
        return np.zeros(m + 1), F64(0), F64(0), st | NONFINITE_OUT
    out[0] = g
    return out, e1, e2, st


# ---- the rows of the GPU tests ------------------------------------------------------------------------------------------
SPECIAL = ("reflected", "swapped", "close", "low_gain", "nan")


def rows(m, n, seed, log_gain=False):
    """(rows [n][m+1], {kind: row index}): jittered evenly spaced sets with gains of a few decades; where the batch has
    room, one row each that is reflected (a value negated, one put beyond pi), swapped, too close, low in gain and NaN."""
    rng = np.random.default_rng(seed)
    step = np.pi / (m + 1)
    w = step * (np.arange(1, m + 1)[None] + rng.uniform(-0.3, 0.3, (n, m)))
    gain = rng.uniform(-3.0, 2.0, n)
    x = np.concatenate([(gain if log_gain else np.exp(gain))[:, None], w], axis=1)
    where = {}
    if n >= 8:
        at = rng.choice(np.arange(1, n - 1), len(SPECIAL), replace=False)
        where = dict(zip(SPECIAL, (int(a) for a in at)))
        i = where["reflected"]
        x[i, 1] = -x[i, 1]
        x[i, m] = 2 * np.pi - x[i, m]
        i = where["swapped"]
        if m >= 2:
            x[i, [1, m]] = x[i, [m, 1]]
        i = where["close"]
        if m >= 2:
            x[i, 2] = x[i, 1] + 0.01 * step
        if m >= 4:
            x[i, 4] = x[i, 3]                            # equal values: the sort keeps their order, d1 or d2 is 0
        x[where["low_gain"], 0] = -40.0 if log_gain else 1e-12
        x[where["nan"], rng.integers(0, m + 1)] = np.nan
    return np.ascontiguousarray(x), where


def neighbour(v, seed):
    """Every value moved to a neighbouring double, up or down by the seed."""
    v = np.asarray(v, dtype=F64)
    up = np.random.default_rng(seed).integers(0, 2, v.shape).astype(bool)
    return np.nextafter(v, np.where(up, np.inf, -np.inf))


def sens(fn, checked, K, seed=1):
    """fn(checked row, K, dtype) -> vector or number.  max over the result of the larger of figure (a) and (b)."""
    base = np.atleast_1d(np.asarray(fn(checked, K, F64), dtype=F64))
    moved = neighbour(np.concatenate([[K], checked[1:]]), seed)
    pert = np.concatenate([[checked[0]], moved[1:]])
    a = np.abs(np.atleast_1d(np.asarray(fn(pert, moved[0], F64), dtype=F64)) - base).max()
    b = np.abs(np.atleast_1d(fn(checked, K, LD)).astype(LD) - base.astype(LD)).max()
    return float(max(a, F64(b)))


def tol(want, s):
    """The project's rule (tests/mgc2mgc_reference.row_tol) for one row or one number."""
    return max(10.0 * s, 64.0 * float(np.spacing(np.abs(np.atleast_1d(want)).max())))

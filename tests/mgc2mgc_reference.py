"""SPTK's mgc2mgc in numpy: the core of the CLIs' SPTK port (test/sptkfunctions.cpp:221-254: freqt :596-631, gnorm
:313-328, gc2gc :347-385, ignorm :330-345) expression by expression in its order, and the four flags of SPTK's command
as include/world_mi355.h defines them (flag semantics unpinned against SPTK's command).  One row at a time, in
np.float64 (what the tests compare with) or np.longdouble (figure (b) of the fixture's `sens`)."""
import numpy as np

F64 = np.float64
LD = np.longdouble

# the fields of WorldMi355MgcConvertOption, in the header's order; an option set is a tuple of them
FIELDS = ("in_order", "in_alpha", "in_gamma", "in_normalized", "in_multiplied", "out_order", "out_alpha", "out_gamma",
          "out_normalized", "out_multiplied")


def option(m1, a1, g1, m2, a2, g2, n=0, u=0, N=0, U=0):
    return (int(m1), float(a1), float(g1), int(n), int(u), int(m2), float(a2), float(g2), int(N), int(U))


def warp(a1, a2):
    """:238, in float64 whatever the chain's precision: the branch is chosen by `a == 0`, exactly."""
    a1, a2 = F64(a1), F64(a2)
    return (a2 - a1) / (1 - a1 * a2)


def _seq_sum(terms, dt):
    """ss += term over the terms in their order (np.sum would add pairwise)."""
    return np.add.accumulate(terms, dtype=dt)[-1] if len(terms) else dt(0)


def freqt(c1, m2, a, dt=F64):
    """:596-631."""
    a = dt(a)
    b = 1 - a * a
    g = np.zeros(m2 + 1, dtype=dt)
    for c in np.asarray(c1, dtype=dt)[::-1]:
        d = g.copy()
        g[0] = c + a * d[0]
        if m2 >= 1:
            g[1] = b * d[0] + a * d[1]
        for j in range(2, m2 + 1):
            g[j] = d[j - 1] + a * (d[j] - g[j - 1])
    return g


def gnorm(c, m, g, dt=F64):
    """:313-328 over c[0 .. m]; what lies beyond m stays."""
    c = np.array(c, dtype=dt)
    g = dt(g)
    if g != 0:
        k = 1 + g * c[0]
        c[1:m + 1] = c[1:m + 1] / k
        c[0] = np.power(k, 1 / g)
    else:
        c[0] = np.exp(c[0])
    return c


def ignorm(c, m, g, dt=F64):
    """:330-345."""
    c = np.array(c, dtype=dt)
    g = dt(g)
    if g != 0:
        k = np.power(c[0], g)
        c[1:m + 1] = k * c[1:m + 1]
        c[0] = (k - 1) / g
    else:
        c[0] = np.log(c[0])
    return c


def gc2gc(c1, m1, g1, m2, g2, dt=F64):
    """:347-385: ss2 and ss1 accumulate over k = 1 .. min in that order."""
    ca = np.asarray(c1, dtype=dt)[:m1 + 1]
    g1, g2 = dt(g1), dt(g2)
    c2 = np.zeros(m2 + 1, dtype=dt)
    c2[0] = ca[0]
    for i in range(1, m2 + 1):
        mn = m1 if m1 < i else i - 1
        k = np.arange(1, mn + 1)
        mk = i - k
        cc = ca[k] * c2[mk]
        ss2 = _seq_sum(k.astype(dt) * cc, dt)
        ss1 = _seq_sum(mk.astype(dt) * cc, dt)
        s = (g2 * ss2 - g1 * ss1) / i
        c2[i] = ca[i] + s if i <= m1 else s
    return c2


def mgc2mgc(c1, m1, a1, g1, m2, a2, g2, dt=F64):
    """:221-254."""
    a = warp(a1, a2)
    c1 = np.asarray(c1, dtype=dt)
    if a == 0:
        ca = gnorm(c1, m1, g1, dt)
        c2 = gc2gc(ca, m1, g1, m2, g2, dt)
    else:
        c2 = freqt(c1, m2, a, dt)
        c2 = gnorm(c2, m2, g1, dt)
        c2 = gc2gc(c2, m2, g1, m2, g2, dt)
    return ignorm(c2, m2, g2, dt)


def plain_input(c, opt, dt=F64):
    """The flag steps before the core: -n ignorm, -u the division by gamma 1."""
    m1, _, g1, n, u = opt[:5]
    c = np.array(c, dtype=dt)
    if n:
        c = ignorm(c, m1, g1, dt)
    elif u:
        c[0] = (c[0] - 1) / dt(g1)
    if u:
        c[1:] = c[1:] / dt(g1)
    return c


def flagged_output(c, opt, dt=F64):
    """The flag steps after the core: -N gnorm, -U the product with gamma 2."""
    m2, _, g2, N, U = opt[5:]
    c = np.array(c, dtype=dt)
    if N:
        c = gnorm(c, m2, g2, dt)
    elif U:
        c[0] = c[0] * dt(g2) + 1
    if U:
        c[1:] = c[1:] * dt(g2)
    return c


def convert(c, opt, dt=F64):
    """One row through flags, core and flags."""
    m1, a1, g1, _, _, m2, a2, g2, _, _ = opt
    return flagged_output(mgc2mgc(plain_input(c, opt, dt), m1, a1, g1, m2, a2, g2, dt), opt, dt)


def convert_rows(rows, opt, dt=F64):
    with np.errstate(all="ignore"):
        return np.stack([convert(r, opt, dt) for r in rows])


def row_tol(want, sens):
    """The project's rule for a chain through gc2gc (tests/test_gpu_mgc2sp.py): per row, ten times the reference's own
    rounding error or 64 ulp of the row's largest value."""
    return np.maximum(10.0 * np.asarray(sens), 64.0 * np.spacing(np.abs(want).max(axis=1)))

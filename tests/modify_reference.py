"""ParameterModification (externs/WORLD_v2/test/test.cpp:201-238) restated in numpy float64: the yardstick of
WorldMi355ModifyFeatures.  test.cpp itself does not compile against its tree and asserts nothing, so this file is pinned
instead (tests/test_modify_host.py): against tests/golden/modify_handmade.npz, whose interpolation step ran in the
compiled reference's interp1, and against that function directly where it is built.

Also the hand-made inputs the tests share: the shapes, the ratios, the row families.
"""
import numpy as np

SHAPES = [(8000, 512), (16000, 1024), (48000, 2048), (96000, 4096)]          # (fs, fft_size)
F0_SCALES = [0.5, 1.0, 1.37, 2.0]
FAMILIES = ("speech", "wide", "flat", "zeros", "nan", "inf")
FINITE_FAMILIES = ("speech", "wide", "flat")
ROWS = 3                                                                       # rows per family


def ratios(F):
    """The test list: around 1, plain ones below and above, the two smallest legal ones (the fill starts at bin 1) and
    the two largest."""
    return [1.0, 1.0 - 2.0 ** -30, 1.0 + 2.0 ** -30, 0.5, 0.75, 1.0 / 3.0, 0.8, 0.999, 1.001, 1.2, 2.0, 3.0,
            2.0 / F, 2.0 / F * (1.0 + 2.0 ** -20), F / 2.0, float(F)]


def refused_ratios(F):
    return [0.0, -1.0, float("nan"), 2.0 / F * (1.0 - 2.0 ** -20), F * (1.0 + 2.0 ** -20)]


def interp1(x, y, xi):
    """src/matlabfunctions.cpp:157-182 with histc (:136-155) on an increasing x: the count of knots <= the query,
    clamped to [1, n - 1]; the fraction over the knot distance h[k-1] = x[k] - x[k-1]; y[k-1] + s (y[k] - y[k-1])."""
    x, y, xi = (np.asarray(a, dtype=np.float64) for a in (x, y, xi))
    k = np.clip(np.searchsorted(x, xi, side="right"), 1, len(x) - 1)
    with np.errstate(all="ignore"):
        s = (xi - x[k - 1]) / (x[k] - x[k - 1])
        return y[k - 1] + s * (y[k] - y[k - 1])


def axes(ratio, fs, F):
    """freq_axis1 and freq_axis2 (test.cpp:217-220), each product and quotient rounded in the reference's order."""
    j = np.arange(F // 2 + 1, dtype=np.float64)
    return np.float64(ratio) * j / np.float64(F) * np.float64(fs), j / np.float64(F) * np.float64(fs)


def fill_start(ratio, F):
    """c of test.cpp:229 for ratio < 1, else the row's length (nothing is filled)."""
    return int(F / 2.0 * ratio) if ratio < 1.0 else F // 2 + 1


def modify_sp(sp, ratio, fs, F, interp=interp1):
    """test.cpp:211-233 on rows sp [T][F/2+1]; interp: the interpolation step (this file's, or the compiled one)."""
    sp = np.atleast_2d(np.asarray(sp, dtype=np.float64))
    x1, x2 = axes(ratio, fs, F)
    out = np.empty_like(sp)
    c = fill_start(ratio, F)
    with np.errstate(all="ignore"):
        for t, row in enumerate(sp):
            out[t] = np.exp(interp(x1, np.log(row), x2))
            if ratio < 1.0:
                out[t, c:] = out[t, c - 1]
    return out


def modify_f0(f0, shift):
    return np.asarray(f0, dtype=np.float64) * np.float64(shift)


def bound(row):
    """8 (1 + L) 2^-52 with L = max |ln sp| over the row's finite, non-zero bins: the relative error allowed at a finite
    output bin.  wm_log <= 1 ulp and libm <= 1 ulp put <= 2 ulp(L) on a knot; the convex interpolation's three roundings
    add <= 3 ulp(L); exp turns that absolute error into a relative one, with wm_exp <= 2 ulp and libm <= 1 ulp on top."""
    row = np.asarray(row, dtype=np.float64)
    ok = np.isfinite(row) & (row > 0)
    L = float(np.abs(np.log(row[ok])).max()) if ok.any() else 0.0
    return 8.0 * (1.0 + L) * 2.0 ** -52


def rows(family, F, seed=0):
    """ROWS hand-made rows [ROWS][F/2+1] of a family.
    speech: ln sp ~ N(-10, 4).  wide: spanning 1e-250 .. 1e250.  flat: constant rows.  zeros: speech with isolated zero
    bins -- row 0 at the odd index 7 and the even index 10 (at ratio 0.5 the reference then has NaN at bins 3 and 5, at
    1.0 at 6, 7, 9 and 10), row 1 at bins 0 and F/2, row 2 at all four.  nan / inf: speech, the middle row holding one
    NaN / one +inf at bin 37; its neighbours are plain speech rows."""
    n = F // 2 + 1
    rng = np.random.default_rng([seed, F, FAMILIES.index(family)])
    speech = np.exp(rng.normal(-10.0, 2.0, (ROWS, n)))
    if family == "speech":
        return speech
    if family == "wide":
        a = np.exp(rng.uniform(np.log(1e-250), np.log(1e250), (ROWS, n)))
        a[0, :2], a[0, -2:] = (1e-250, 1e250), (1e250, 1e-250)
        return a
    if family == "flat":
        return np.repeat(np.array([[1.0], [3.7e-5], [2.5e3]]), n, axis=1)
    if family == "zeros":
        speech[0, [7, 10]] = 0.0
        speech[1, [0, F // 2]] = 0.0
        speech[2, [0, 7, 10, F // 2]] = 0.0
        return speech
    speech[1, 37] = np.nan if family == "nan" else np.inf
    return speech


def f0_contour(T, seed=0):
    """A contour with unvoiced zeros at both ends and inside."""
    rng = np.random.default_rng([seed, T, 77])
    f0 = rng.uniform(71.0, 800.0, T)
    f0[rng.random(T) < 0.3] = 0.0
    f0[[0, T - 1]] = 0.0
    return f0


# ---- the golden file's part of the grid -----------------------------------------------------------------------------
GOLDEN_SHAPES = SHAPES[:2]
GOLDEN_CASES = [("speech", 1.0), ("speech", 0.5), ("speech", 1.0 / 3.0), ("speech", 1.2), ("zeros", 0.5), ("zeros", 1.0),
                ("wide", 0.8)]


def golden_key(family, ratio, F):
    return "%s_%d_%s" % (family, F, float(ratio).hex())


def same_class(a, b):
    """Where two arrays agree on what kind of value a bin holds: NaN, +inf, -inf, zero, or an ordinary number."""
    kinds = lambda v: np.select([np.isnan(v), np.isposinf(v), np.isneginf(v), v == 0], [1, 2, 3, 4], 0)
    return kinds(np.asarray(a)) == kinds(np.asarray(b))


def ulps(a, b):
    """Distance in units of the last place between two arrays of ordinary, same-signed doubles."""
    a, b = (np.ascontiguousarray(v, dtype=np.float64).view(np.int64) for v in (a, b))
    return np.abs(a - b)

#!/usr/bin/env python3
"""Writes tests/golden/sptk_mgc2sp_full.npz: mel-generalized cepstra and the COMPILED reference's mgc2sp of them
(test/sptkfunctions.cpp:186-219, built by oracle/Makefile into oracle/_ref/libsptk_ref.so), for
tests/test_mgc2sp_host.py and tests/test_gpu_mgc2sp.py.

    make -C oracle ref && python tools/gen_golden_mgc2sp.py

The port keeps static buffers sized at first use, and its sine table depends on the largest transform a process has
made, so every option set runs in a child process of its own (this file with --child) at one fft size.  Only data is
stored: input rows, their seeds, and what the reference returned.

Inputs at gamma = 0: seeded rows c[k] = N(0, 1) / (1 + k) with c0 uniform in [-3, 3], and, where
tests/golden/sptk_mcep.npz has an option set of the same order, `conv` rows of it (same alpha if it has one) in place of
half of them.
Inputs at gamma != 0: the reference's own mgc2mgc(row, m, alpha, 0, m, alpha, gamma) of such rows, which keeps
1 + gamma c0 > 0 (asserted).  gc2gc towards F/2 coefficients is a power series that need not converge: for rows of a
large dynamic range at a low order (most of sptk_mcep.npz's at m = 1, many at gamma = -1) the reference returns finite
values of 1e6 ... 1e270 whose last-bit sensitivity exceeds 1, and a comparison against them measures nothing.  So the
rows of an option set are CHOSEN from candidates (12 seeded, 6 of sptk_mcep.npz) by one rule, choose(): the first whose
reference |x| stays below X_LIMIT = 20 (a convergent row has that of its gamma = 0 original, at most 11 here).  At
gamma = 0 every candidate passes.

Per option set (`key`, OPTIONS below):
  <key>/opt     [fft_size, m, alpha, gamma]
  <key>/mc      [rows][m+1]        the rows given to mgc2sp
  <key>/x, /y   [rows][fft/2+1]    the reference's log amplitude and its imaginary part (fftr's sign: `y_sign` says which)
  <key>/sens_x, /sens_y            the larger of (a) max |change| of the reference's result when its input is multiplied
                                   by 1 + 4 * 2^-52 * xi, xi uniform in [-1, 1] (seeded), and (b) max |reference - the
                                   same chain in np.longdouble| (freqt, gnorm, gc2gc, ignorm, a direct DFT): the
                                   reference's own rounding error, which is what a reordered gc2gc sum differs by
  <key>/sens_ab [2][2]             the two figures apart, (a) and (b) for x and y
  <key>/rt_ref                     round-trip keys only: max |mcep(exp(x)) - mc| with the reference's mcep at the same m,
                                   alpha, itr1 2, itr2 100, dd 1e-10, amplitude rows
The status case S (fft 512): four rows of which row 1 has 1 + gamma c0 < 0 and row 3 a NaN coefficient; S/status is
[0, 1, 0, 1], S/x and S/y hold zeros in the flagged rows (what the library writes), the reference's values elsewhere.
The option sets are the smallest that reach every branch (alpha 0 / not 0, gamma 0 / not 0, m of 1, mid and 63, every
fft size); the rows per set (512: 3, 1024: 4, 2048: 2, 4096: 2) keep the file under 1 MiB -- fewer rows, never lower
precision.
Also prints the compiled reference's one-thread rate at fft 1024 and 4096 (a record for DESIGN.md).
"""
import ctypes
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oracle", "_ref", "libsptk_ref.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")
PERTURB_SEED = 20241
ROWS = {512: 3, 1024: 4, 2048: 2, 4096: 2}
GAMMAS = {"g0": 0.0, "g3": -1.0 / 3.0, "g2": -0.5, "g1": -1.0}


def key_of(F, m, alpha, gname):
    return "F%d_m%d_a%s%02d_%s" % (F, m, "n" if alpha < 0 else "", round(abs(alpha) * 100), gname)


# key -> (fft_size, m, alpha, gamma)
OPTIONS = {}
for _m in (1, 24, 63):
    for _a in (0.0, 0.42, 0.55, -0.3):
        for _g in ("g0", "g3", "g2", "g1"):
            OPTIONS[key_of(512, _m, _a, _g)] = (512, _m, _a, GAMMAS[_g])
for _m, _a in ((24, 0.55), (49, 0.42)):
    for _g in ("g0", "g3"):
        OPTIONS[key_of(1024, _m, _a, _g)] = (1024, _m, _a, GAMMAS[_g])
for _g in ("g0", "g1"):
    OPTIONS[key_of(2048, 63, 0.55, _g)] = (2048, 63, 0.55, GAMMAS[_g])
for _g in ("g0", "g3"):
    OPTIONS[key_of(4096, 24, 0.55, _g)] = (4096, 24, 0.55, GAMMAS[_g])
# the round trips of tests/test_gpu_mgc2sp.py: the second is one of the sets above, the first exists for this alone
OPTIONS["F512_m8_a42_g0"] = (512, 8, 0.42, 0.0)
ROUND_TRIPS = ("F512_m8_a42_g0", "F1024_m24_a55_g0")
STATUS_OPT = (512, 24, 0.42, -1.0 / 3.0)
STATUS = (0, 1, 0, 1)
# sptk_mcep.npz's option set whose `conv` rows serve as inputs, by (fft_size, m, alpha) or (fft_size, m)
MCEP_KEYS = {(512, 1, 0.0): "A_m1_a00", (512, 1, 0.42): "A_m1_a42", (512, 1, 0.55): "A_m1_a55", (512, 1): "A_m1_a42",
             (512, 8, 0.42): "A_m8_a42", (512, 24, 0.0): "A_m24_a00", (512, 24, 0.42): "A_m24_a42",
             (512, 24, 0.55): "A_m24_a55", (512, 24): "A_m24_a42", (1024, 24, 0.55): "B_cli", (1024, 49, 0.42): "B_m49",
             (2048, 63, 0.55): "C_m63"}


def seed_of(F, m, alpha):
    return 100000 + F * 7 + m * 131 + int(round((alpha + 1.0) * 100))


X_LIMIT = 20.0
N_SEEDED, N_CONV = 12, 6


def candidates(F, m, alpha):
    """(seeded rows, rows of sptk_mcep.npz) at gamma = 0 from which an option set's rows are chosen (choose())."""
    rs = np.random.RandomState(seed_of(F, m, alpha))
    c = rs.randn(N_SEEDED, m + 1) / (1.0 + np.arange(m + 1))
    c[:, 0] = rs.uniform(-3.0, 3.0, N_SEEDED)
    mk = MCEP_KEYS.get((F, m, alpha), MCEP_KEYS.get((F, m)))
    conv = np.zeros((0, m + 1)) if mk is None else np.load(os.path.join(GOLDEN, "sptk_mcep.npz"))[mk + "/conv"][:N_CONV]
    return c, conv


def choose(usable, n_seeded, rows):
    """Indices into the candidates (seeded first): the first usable seeded rows, then up to ceil(rows / 2) usable rows
    of sptk_mcep.npz in place of the last of them."""
    seeded = [i for i in range(n_seeded) if usable[i]]
    conv = [i for i in range(n_seeded, len(usable)) if usable[i]][:(rows + 1) // 2]
    idx = seeded[:rows - len(conv)] + conv
    assert len(idx) == rows, (len(seeded), len(conv))
    return np.asarray(idx)


def perturb(c):
    xi = np.random.RandomState(PERTURB_SEED).uniform(-1.0, 1.0, c.shape)
    return c * (1.0 + 4.0 * 2.0 ** -52 * xi)


def symbol(name):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = [ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("_Z%d%sP" % (len(name), name))]
    assert len(names) == 1, (name, names)
    return names[0]


# ---- the chain in np.longdouble (sens figure (b)); the expressions of sptkfunctions.cpp in its order ----------------
LD = np.longdouble
PI_LD = LD("3.14159265358979323846264338327950288419716939937510")


def freqt_ld(c1, m2, a):
    """:596-631 on the rows of c1 [rows][m1+1] at once."""
    a = LD(a)
    b = 1 - a * a
    rows, m1 = c1.shape[0], c1.shape[1] - 1
    g = np.zeros((rows, m2 + 1), dtype=LD)
    for i in range(m1, -1, -1):
        d = g.copy()
        g[:, 0] = c1[:, i] + a * d[:, 0]
        if m2 >= 1:
            g[:, 1] = b * d[:, 0] + a * d[:, 1]
        for j in range(2, m2 + 1):
            g[:, j] = d[:, j - 1] + a * (d[:, j] - g[:, j - 1])
    return g


def gc2gc_to0_ld(ca, m2, g1):
    """gc2gc(ca, m1, g1, c2, m2, 0) (:347-385) on one row."""
    m1 = len(ca) - 1
    c2 = np.zeros(m2 + 1, dtype=LD)
    c2[0] = ca[0]
    for i in range(1, m2 + 1):
        mn = m1 if m1 < i else i - 1
        k = np.arange(1, mn + 1)
        ss1 = np.sum((i - k).astype(LD) * ca[k] * c2[i - k]) if mn >= 1 else LD(0)
        c2[i] = (ca[i] if i <= m1 else LD(0)) - LD(g1) * ss1 / i
    return c2


def mgc2sp_ld(mc, F, alpha, gamma):
    """mgc2sp (:186-274) in long double; the transform is a direct DFT with e^{-j}: (Re, Im) [rows][F/2+1]."""
    N = F // 2
    c = np.asarray(mc, dtype=LD)
    gamma_ld = LD(gamma)
    if alpha != 0:
        c = freqt_ld(c, N, -alpha)
    out = np.zeros((len(c), N + 1), dtype=LD)
    for r, row in enumerate(c):
        row = row.copy()
        if gamma != 0:
            k = 1 + gamma_ld * row[0]
            row[1:] = row[1:] / k
            row[0] = k ** (1 / gamma_ld)
            row = gc2gc_to0_ld(row, N, gamma)
            row[0] = np.log(row[0])
        out[r, :len(row)] = row
    ang = -2 * PI_LD * np.arange(F).astype(LD) / F
    cs, sn = np.cos(ang), np.sin(ang)
    idx = (np.arange(N + 1)[:, None] * np.arange(N + 1)[None, :]) % F          # [bin][n]
    return out @ cs[idx].T, out @ sn[idx].T


# ---- the compiled reference, in a child process ------------------------------------------------------------------
def child(spec_path, out_path):
    z = np.load(spec_path, allow_pickle=False)
    F, m, alpha, gamma = int(z["F"]), int(z["m"]), float(z["alpha"]), float(z["gamma"])
    lib = ctypes.CDLL(LIB)
    dp = ctypes.POINTER(ctypes.c_double)
    ci, cd = ctypes.c_int, ctypes.c_double
    mgc2sp = getattr(lib, symbol("mgc2sp"))
    mgc2sp.restype = None
    mgc2sp.argtypes = [dp, ci, cd, cd, dp, dp, ci]
    mgc2mgc = getattr(lib, symbol("mgc2mgc"))
    mgc2mgc.restype = None
    mgc2mgc.argtypes = [dp, ci, cd, cd, dp, ci, cd, cd]
    mcep = getattr(lib, symbol("mcep"))
    mcep.restype = ci
    mcep.argtypes = [dp, ci, dp, ci, cd, ci, ci, cd, ci, cd, cd, ci]

    def to_gamma(rows):
        if gamma == 0.0:
            return rows.copy()
        out = np.zeros_like(rows)
        for i, row in enumerate(rows):
            src, dst = np.ascontiguousarray(row), np.zeros(m + 1)
            mgc2mgc(src.ctypes.data_as(dp), m, alpha, 0.0, dst.ctypes.data_as(dp), m, alpha, gamma)
            out[i] = dst
        return out

    def run(rows):
        x, y = np.zeros((len(rows), F)), np.zeros((len(rows), F))
        for i, row in enumerate(rows):
            src = np.ascontiguousarray(row)
            mgc2sp(src.ctypes.data_as(dp), m, alpha, gamma, x[i].ctypes.data_as(dp), y[i].ctypes.data_as(dp), F)
        return x[:, :F // 2 + 1].copy(), y[:, :F // 2 + 1].copy()

    res = {}
    mc = to_gamma(z["base"]) if int(z["convert"]) else z["base"].copy()
    if "override" in z.files:                                    # the status case: values set after the conversion
        for r, k, v in z["override"]:
            mc[int(r), int(k)] = v
    res["mc"] = mc
    res["x"], res["y"] = run(mc)
    res["xp"], res["yp"] = run(perturb(mc))
    if int(z["round_trip"]):
        back = np.zeros_like(mc)
        buf = np.zeros(F)
        for i in range(len(mc)):
            buf[:] = 0.0
            buf[:F // 2 + 1] = np.exp(res["x"][i])
            o = np.zeros(m + 1)
            mcep(buf.ctypes.data_as(dp), F, o.ctypes.data_as(dp), m, alpha, 2, 100, 1e-10, 0, 0.0, 1e-6, 3)
            back[i] = o
        res["back"] = back
    n_rate = int(z["rate_rows"])
    if n_rate:
        t0 = time.perf_counter()
        run(np.tile(mc, (n_rate // len(mc) + 1, 1))[:n_rate])
        res["secs_per_row"] = (time.perf_counter() - t0) / n_rate
    np.savez(out_path, **res)


def run_child(base, F, m, alpha, gamma, convert=True, override=None, round_trip=False, rate_rows=0):
    with tempfile.TemporaryDirectory() as d:
        spec, out = os.path.join(d, "spec.npz"), os.path.join(d, "out.npz")
        extra = {} if override is None else {"override": np.asarray(override, dtype=np.float64)}
        np.savez(spec, base=base, F=F, m=m, alpha=alpha, gamma=gamma, convert=int(convert), round_trip=int(round_trip),
                 rate_rows=rate_rows, **extra)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", spec, out], check=True)
        z = np.load(out)
        return {k: z[k] for k in z.files}


def sens_of(r, F, alpha, gamma, rows=None):
    """((a), (b)) for x and y, and the sign that takes the e^{-j} imaginary part to the reference's y."""
    sel = slice(None) if rows is None else rows
    xl, yl = mgc2sp_ld(r["mc"][sel], F, alpha, gamma)
    x, y = r["x"][sel], r["y"][sel]
    sign = 1.0 if np.abs(y - yl).max() <= np.abs(y + yl).max() else -1.0
    a = (np.abs(r["xp"][sel] - x).max(), np.abs(r["yp"][sel] - y).max())
    b = (float(np.abs(x - xl).max()), float(np.abs(y - sign * yl).max()))
    return np.asarray([[a[0], b[0]], [a[1], b[1]]]), sign


def chosen_rows(F, m, alpha, gamma, rows, round_trip=False):
    """The reference on every candidate, cut down to the option set's rows: (results, their gamma = 0 originals)."""
    seeded, conv = candidates(F, m, alpha)
    base = np.concatenate([seeded, conv])
    r = run_child(base, F, m, alpha, gamma, round_trip=round_trip)
    with np.errstate(invalid="ignore"):
        usable = np.isfinite(r["x"]).all(axis=1) & np.isfinite(r["y"]).all(axis=1) & (np.abs(r["x"]).max(axis=1) < X_LIMIT)
    idx = choose(usable, len(seeded), rows)
    return {k: v[idx] for k, v in r.items() if np.ndim(v) >= 1 and len(v) == len(base)}, base[idx]


def main():
    assert os.path.exists(LIB), "run `make -C oracle ref` first"
    store = {"perturb_seed": PERTURB_SEED, "keys": np.asarray(sorted(OPTIONS)), "round_trips": np.asarray(ROUND_TRIPS)}
    signs = set()
    for key in sorted(OPTIONS):
        F, m, alpha, gamma = OPTIONS[key]
        r, _ = chosen_rows(F, m, alpha, gamma, ROWS[F], round_trip=key in ROUND_TRIPS)
        assert (1.0 + gamma * r["mc"][:, 0] > 0).all(), key
        assert np.isfinite(r["x"]).all() and np.isfinite(r["y"]).all(), key
        ab, sign = sens_of(r, F, alpha, gamma)
        signs.add(sign)
        store[key + "/opt"] = np.asarray([F, m, alpha, gamma])
        store[key + "/mc"], store[key + "/x"], store[key + "/y"] = r["mc"], r["x"], r["y"]
        store[key + "/sens_ab"] = ab
        store[key + "/sens_x"], store[key + "/sens_y"] = ab[0].max(), ab[1].max()
        line = "%-20s max|x| %5.2f  sens x (a) %.1e (b) %.1e  y (a) %.1e (b) %.1e" % (
            key, np.abs(r["x"]).max(), ab[0, 0], ab[0, 1], ab[1, 0], ab[1, 1])
        if key in ROUND_TRIPS:
            store[key + "/rt_ref"] = np.abs(r["back"] - r["mc"]).max()
            line += "  rt_ref %.1e" % store[key + "/rt_ref"]
        print(line, flush=True)
    assert len(signs) == 1, signs
    store["y_sign"] = signs.pop()                                # +1: y = Im sum c[n] exp(-2 pi i k n / F)
    # ---- the status case ----
    F, m, alpha, gamma = STATUS_OPT
    _, base = chosen_rows(F, m, alpha, gamma, 4)
    r = run_child(base, F, m, alpha, gamma, override=[(1, 0, 40.0), (3, 5, np.nan)])
    good = np.asarray(STATUS) == 0
    assert 1.0 + gamma * r["mc"][1, 0] < 0 and np.isnan(r["mc"][3, 5]) and np.isfinite(r["mc"][good]).all()
    assert not np.isfinite(r["x"][1]).all() and not np.isfinite(r["x"][3]).all()
    assert np.isfinite(r["x"][good]).all() and np.isfinite(r["y"][good]).all()
    ab, _ = sens_of(r, F, alpha, gamma, rows=good)
    x, y = r["x"].copy(), r["y"].copy()
    x[~good], y[~good] = 0.0, 0.0
    store.update({"S/opt": np.asarray(STATUS_OPT), "S/mc": r["mc"], "S/x": x, "S/y": y,
                  "S/status": np.asarray(STATUS, dtype=np.int32), "S/sens_ab": ab, "S/sens_x": ab[0].max(),
                  "S/sens_y": ab[1].max()})
    print("S: status %s  sens x %.1e y %.1e" % (list(STATUS), ab[0].max(), ab[1].max()))
    path = os.path.join(GOLDEN, "sptk_mgc2sp_full.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    print("wrote %s (%d bytes)" % (path, size))
    assert size < 1 << 20, "over the size limit for a committed file: store fewer rows"
    # ---- the reference's one-thread rate (a record, not a fixture) ----
    for F, n in ((1024, 64), (4096, 8)):
        for gamma in (0.0, -1.0 / 3.0):
            r = run_child(candidates(F, 24, 0.55)[0], F, 24, 0.55, gamma, rate_rows=n)
            print("reference mgc2sp, F %d, m 24, alpha 0.55, gamma %.3f: %.2f ms per row on one thread" % (
                F, gamma, 1e3 * float(r["secs_per_row"])))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main()

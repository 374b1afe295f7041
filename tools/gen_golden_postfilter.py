#!/usr/bin/env python3
"""Writes tests/golden/sptk_postfilter.npz: mel-cepstral rows and the gain term of the recipe's formant emphasis
(scripts/Training.pl:2642-2687, postfiltering_mcp) as the COMPILED reference computes it, for
tests/test_postfilter_host.py and tests/test_gpu_postfilter.py.

    make -C oracle ref && python tools/gen_golden_postfilter.py

The script runs six SPTK tools per utterance.  Of those only freqt (test/sptkfunctions.cpp:596-631) and fftr (:387-461)
exist in the compiled reference (oracle/_ref/libsptk_ref.so); the chain is composed from them here:

  E(v)   = c2acr -m co -M 0 -l L of freqt -m m -a alpha -M co -A 0 of v: freqt(v, m, ., co, -alpha), zero-padded to L,
           fftr, exp(2 Re), fftr, the first value divided by L                                     (:2654-2662)
  w      = [1, 1, beta, ..., beta]                                                                 (:2646-2651)
  delta  = 1/2 ln(E(c) / E(w c))                                                                   (:2671-2674)
  out    = b2mc(mc2b(w c) + delta e_0): mc2b b[m] = v[m], b[i] = v[i] - alpha b[i+1]; b2mc v[i] = b[i] + alpha b[i+1]
           -- in numpy; the net effect out[0] = c[0] + delta, out[k] = w[k] c[k] is asserted here to rounding level.

The port keeps static buffers sized at first use, and its sine table depends on the largest transform a process has
made, so every option set runs in a child process of its own (this file with --child), as tools/gen_golden_mgc2sp.py
does.  Only data is stored.  Per option set (`key`, OPTIONS below):
  <key>/opt      [L, co, m, alpha, beta]
  <key>/mc       [rows][m+1]   seeded rows c[k] = N(0, 1) / (1 + k), c0 uniform in [-3, 3]
  <key>/delta    [rows]        the reference's 1/2 ln(E(c) / E(w c)), in double throughout
  <key>/tail     the largest over the rows of sum_{n > co} |freqt(w c)[n]|: what the script's truncation at co leaves
                 out of the log spectrum, and so (twice, once per energy) a bound on how far its delta can lie from the
                 co -> infinity limit that the library computes.  Taken from freqt in np.longdouble carried 512 orders
                 past co and stored as a double: 0 where it lies below the double range (5e-431 at the recipe's
                 setting; freqt in double underflows to denormals of 1e-320 there).  At m = 1 the weights are all
                 ones, E(c) and E(w c) are one computation on one row and no truncation can separate them: the tail
                 is recorded as 0 there.
  <key>/sens_abc [3]           (a) max |change| of the reference's delta when its input is multiplied by
                 1 + 4 * 2^-52 * xi, xi uniform in [-1, 1] (seeded); (b) max |reference - the same chain in
                 np.longdouble| (freqt, a direct cosine sum on the L bins, exp, mean); (c) 2 * tail
  <key>/sens     max(a, b, c).  A set is ADMITTED only if (c) is not the largest of the three (one rule, asserted for
                 every set): the reference is then the accurate side at its own rounding level.
  <key>/recipe_f32_gap         a figure for DESIGN.md, not a bound: max |delta - delta of the script's pipeline with a
                 float32 rounding wherever it writes a file or a pipe|, both on the rows rounded to float32.
c2acr accepts any co < L; the small sets use co = L - 1.  co = L/2 - 1 at L = 512 with m >= 49 or alpha >= 0.77 leaves
tails of 3e-13 ... 0.3 and is not used.
Also prints the chain's one-thread rate at the recipe's setting (a record for DESIGN.md).
"""
import ctypes
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_mgc2sp import LD, LIB, PI_LD, freqt_ld, symbol  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PERTURB_SEED = 20251
TAIL_ORDERS = 512


def key_of(L, m, alpha, beta):
    return "L%d_m%d_a%s%02d_b%02d" % (L, m, "n" if alpha < 0 else "", round(abs(alpha) * 100), round(beta * 10))


# key -> (L, co, m, alpha, beta)
OPTIONS = {}
for _L, _m, _a, _co in ((512, 1, 0.55, 511), (512, 2, 0.55, 511), (512, 24, 0.42, 511), (512, 24, -0.42, 511),
                        (512, 24, 0.55, 511), (512, 49, 0.55, 511), (512, 63, 0.42, 511), (512, 24, 0.77, 511),
                        (1024, 49, 0.55, 511), (2048, 63, 0.77, 1023), (4096, 49, 0.55, 2047)):
    OPTIONS[key_of(_L, _m, _a, 1.4)] = (_L, _co, _m, _a, 1.4)
for _b in (0.7, 1.4, 2.0):
    OPTIONS[key_of(512, 24, 0.0, _b)] = (512, 511, 24, 0.0, _b)
for _b in (0.7, 2.0):
    OPTIONS[key_of(512, 24, 0.42, _b)] = (512, 511, 24, 0.42, _b)
RECIPE = key_of(4096, 49, 0.55, 1.4)


def rows_of(L):
    return 2 if L == 4096 else 3


def seed_of(L, m, alpha):
    return 200000 + L * 7 + m * 131 + int(round((alpha + 1.0) * 100))


def inputs(L, m, alpha):
    rs = np.random.RandomState(seed_of(L, m, alpha))
    n = rows_of(L)
    c = rs.randn(n, m + 1) / (1.0 + np.arange(m + 1))
    c[:, 0] = rs.uniform(-3.0, 3.0, n)
    return c


def weights(m, beta):
    w = np.full(m + 1, float(beta))
    w[:2] = 1.0
    return w


def perturb(c):
    xi = np.random.RandomState(PERTURB_SEED).uniform(-1.0, 1.0, c.shape)
    return c * (1.0 + 4.0 * 2.0 ** -52 * xi)


def mc2b(v, alpha):
    b = np.array(v, dtype=v.dtype)
    for i in range(b.shape[-1] - 2, -1, -1):
        b[..., i] = v[..., i] - alpha * b[..., i + 1]
    return b


def b2mc(b, alpha):
    v = np.array(b, dtype=b.dtype)
    v[..., :-1] = b[..., :-1] + alpha * b[..., 1:]
    return v


# ---- the chain in np.longdouble (sens figure (b)) and the truncation tail ---------------------------------------------
def energy_ld(g, L):
    """c2acr's first value of the rows of g (cepstra at warp 0): the mean over the L bins of exp(2 x_k), x_k the cosine
    sum of the row at bin k (bins k and L - k are equal)."""
    n = g.shape[1]
    ang = 2 * PI_LD * np.arange(L).astype(LD) / L
    cs = np.cos(ang)
    idx = (np.arange(L // 2 + 1)[:, None] * np.arange(n)[None, :]) % L
    x = g @ cs[idx].T
    v = np.full(L // 2 + 1, LD(2))
    v[0] = v[-1] = 1
    return (np.exp(2 * x) * v).sum(axis=1) / L


def chain_ld(c, L, co, alpha, beta):
    """(delta, tail) of the rows of c in long double."""
    m = c.shape[1] - 1
    w = weights(m, beta).astype(LD)
    c = np.asarray(c, dtype=LD)
    if alpha != 0:
        g0 = freqt_ld(c, co + TAIL_ORDERS, -alpha)
        g1 = freqt_ld(c * w, co + TAIL_ORDERS, -alpha)
    else:
        g0 = np.zeros((len(c), co + TAIL_ORDERS + 1), dtype=LD)
        g0[:, :m + 1] = c
        g1 = g0.copy()
        g1[:, :m + 1] = c * w
    delta = np.log(energy_ld(g0[:, :co + 1], L) / energy_ld(g1[:, :co + 1], L)) / 2
    tail = np.abs(g1[:, co + 1:]).sum(axis=1).max() if m > 1 else LD(0)
    return delta, float(tail)


# ---- the compiled reference, in a child process ------------------------------------------------------------------
def child(spec_path, out_path):
    z = np.load(spec_path, allow_pickle=False)
    L, co, m, alpha = int(z["L"]), int(z["co"]), int(z["m"]), float(z["alpha"])
    lib = ctypes.CDLL(LIB)
    dp = ctypes.POINTER(ctypes.c_double)
    freqt = getattr(lib, symbol("freqt"))
    freqt.restype = None
    freqt.argtypes = [dp, ctypes.c_int, dp, ctypes.c_int, ctypes.c_double]
    fftr = getattr(lib, symbol("fftr"))
    fftr.restype = ctypes.c_int
    fftr.argtypes = [dp, dp, ctypes.c_int]

    def energy(v, f32):
        """E(v); with f32 the values are rounded where the script has a pipe or a file (after freqt, after c2acr)."""
        src, g = np.ascontiguousarray(v, dtype=np.float64), np.zeros(co + 1)
        freqt(src.ctypes.data_as(dp), m, g.ctypes.data_as(dp), co, -alpha)
        if f32:
            g = g.astype(np.float32).astype(np.float64)
        x, y = np.zeros(L), np.zeros(L)
        x[:co + 1] = g
        assert fftr(x.ctypes.data_as(dp), y.ctypes.data_as(dp), L) == 0
        x = np.exp(2.0 * x)
        y[:] = 0.0
        assert fftr(x.ctypes.data_as(dp), y.ctypes.data_as(dp), L) == 0
        r = x[0] / L
        return float(np.float32(r)) if f32 else r

    res = {}
    for name in ("plain", "f32"):
        t0 = time.perf_counter()
        res[name] = np.asarray([energy(v, name == "f32") for v in z[name]])
        res["secs_" + name] = time.perf_counter() - t0
    np.savez(out_path, **res)


def run_child(L, co, m, alpha, plain, f32):
    with tempfile.TemporaryDirectory() as d:
        spec, out = os.path.join(d, "spec.npz"), os.path.join(d, "out.npz")
        np.savez(spec, L=L, co=co, m=m, alpha=alpha, plain=plain, f32=f32)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", spec, out], check=True)
        z = np.load(out)
        return {k: z[k] for k in z.files}


def reference(c, L, co, alpha, beta):
    """The reference's delta of the rows c and of their perturbed copies, the float32 pipeline's gap, seconds per frame."""
    m = c.shape[1] - 1
    w = weights(m, beta)
    f = np.float32
    c32 = c.astype(f)
    w32 = w.astype(f)
    wc32 = (c32 * w32).astype(f)                                   # vopr -m writes float32
    cp = perturb(c)
    plain = np.concatenate([c, c * w, cp, cp * w, c32.astype(np.float64), c32.astype(np.float64) * w])
    r = run_child(L, co, m, alpha, plain, np.concatenate([c32, wc32]).astype(np.float64))
    n = len(c)
    e = r["plain"].reshape(6, n)
    delta, delta_p, delta_32in = (0.5 * np.log(e[2 * i] / e[2 * i + 1]) for i in range(3))
    e32 = r["f32"].reshape(2, n).astype(f)
    delta_f32 = (np.log((e32[0] / e32[1]).astype(f)).astype(f) / f(2)).astype(f)          # vopr -d | sopr -LN -d 2
    return delta, delta_p, float(np.abs(delta_f32.astype(np.float64) - delta_32in).max()), r["secs_plain"] / (3 * n)


def main():
    assert os.path.exists(LIB), "run `make -C oracle ref` first"
    store = {"perturb_seed": PERTURB_SEED, "keys": np.asarray(sorted(OPTIONS))}
    for key in sorted(OPTIONS):
        L, co, m, alpha, beta = OPTIONS[key]
        c = inputs(L, m, alpha)
        delta, delta_p, gap, secs = reference(c, L, co, alpha, beta)
        delta_ld, tail = chain_ld(c, L, co, alpha, beta)
        abc = np.asarray([np.abs(delta_p - delta).max(), float(np.abs(delta - delta_ld).max()), 2.0 * tail])
        assert np.isfinite(delta).all() and np.isfinite(abc).all(), key
        assert abc[2] <= abc[:2].max(), (key, abc)                 # admitted: the truncation is not the largest figure
        # the net effect of mc2b, the addition and b2mc: out[0] = c0 + delta, out[k] = w[k] c[k]
        w = weights(m, beta)
        b = mc2b(c * w, alpha)
        b[:, 0] += delta
        want = c * w
        want[:, 0] += delta
        assert np.abs(b2mc(b, alpha) - want).max() <= 16 * np.spacing(np.abs(want).max()), key
        store[key + "/opt"] = np.asarray([L, co, m, alpha, beta])
        store[key + "/mc"], store[key + "/delta"] = c, delta
        store[key + "/tail"], store[key + "/sens_abc"], store[key + "/sens"] = tail, abc, abc.max()
        store[key + "/recipe_f32_gap"] = gap
        print("%-22s max|delta| %.3f  sens (a) %.1e (b) %.1e (c) %.1e  f32 gap %.1e  %.2f ms per frame" % (
            key, np.abs(delta).max(), abc[0], abc[1], abc[2], gap, 1e3 * secs), flush=True)
        if key == RECIPE:
            print("reference chain at the recipe's setting: %.0f frames/s on one thread" % (1.0 / secs))
    path = os.path.join(GOLDEN, "sptk_postfilter.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    print("wrote %s (%d bytes)" % (path, size))
    assert size < 1 << 20


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main()

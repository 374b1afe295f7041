"""The definition of WorldMi355MlsaExcitation / MlsaFilter / MlsaSynthesis (include/world_mi355.h) written out in float64:
SPTK's `excite -n | dfs`, `vopr -a` and `mglsadf -c 0` as gen_wave's first branch drives them.  SPTK is not in the
reference tree and parity with it is unpinned: this file is the yardstick, and `anchor_error` is what pins it -- at constant
coefficients the filter's impulse response must reproduce the mel-log spectrum of the coefficients.

Plain Python floats (IEEE double, the C library's log / sqrt / exp) in the order the definition gives; no vectorising
that would change a rounding."""
import math
from fractions import Fraction

import numpy as np

PADE4 = (1.0, 0.4999273, 0.1067005, 0.01170221, 0.0005656279)
PADE5 = (1.0, 0.4999391, 0.1107098, 0.01369984, 0.0009564853, 0.00003041721)


def samples(n_frames, frame_shift):
    return (n_frames - 1) * frame_shift


def pade_exact(order):
    """The plain Pade approximant's row as exact rationals."""
    f = math.factorial
    L = order
    return [Fraction(f(L) * f(2 * L - k), f(2 * L) * f(k) * f(L - k)) for k in range(L + 1)]


def pade(order):
    if order == 4:
        return list(PADE4)
    if order == 5:
        return list(PADE5)
    return [float(q) for q in pade_exact(order)]


def noise(n):
    """g[0 .. n): nrandom at seed 1."""
    state = [1]

    def rnd():
        state[0] = (state[0] * 1103515245 + 12345) & 0xFFFFFFFF
        return ((state[0] // 65536) % 32768) / 32767.0

    out = []
    while len(out) < n:
        while True:
            r1 = 2.0 * rnd() - 1.0
            r2 = 2.0 * rnd() - 1.0
            s = r1 * r1 + r2 * r2
            if not (s > 1.0 or s == 0.0):
                break
        s = math.sqrt(-2.0 * math.log(s) / s)
        out.append(r1 * s)
        out.append(r2 * s)
    return np.array(out[:n], dtype=np.float64)


def _f32(v):
    return float(np.float32(v))


def excite(pitch, P, g=None, f32=False):
    """excite -n -p P: (samples, positions of the pulses, their amplitudes, number of noise values used)."""
    pitch = [float(v) for v in pitch]
    T = len(pitch)
    if g is None:
        g = noise(samples(T, P))
    out, pos, amp = [], [], []
    p1 = pitch[0]
    cnt = p1
    used = 0
    for f in range(1, T):
        p2 = pitch[f]
        if p1 != 0.0 and p2 != 0.0:
            inc = (p2 - p1) / P
        else:
            inc = 0.0
            cnt = p2
            p1 = 0.0
        for _ in range(P):
            if p1 == 0.0:
                v = float(g[used])
                used += 1
            else:
                cnt += 1.0
                if cnt >= p1:
                    v = math.sqrt(p1)
                    pos.append(len(out))
                    amp.append(v)
                    cnt -= p1
                else:
                    v = 0.0
            p1 += inc
            out.append(_f32(v) if f32 else v)
        p1 = p2
    return np.array(out, dtype=np.float64), pos, amp, used


def fir(taps, x, f32=False):
    """dfs -b taps: taps accumulated in the order k = 0, 1, ..."""
    taps = [float(t) for t in taps]
    x = [float(v) for v in x]
    y = []
    for n in range(len(x)):
        acc = 0.0
        for k in range(min(len(taps), n + 1)):
            acc += taps[k] * x[n - k]
        y.append(_f32(acc) if f32 else acc)
    return np.array(y, dtype=np.float64)


def excitation(pitch, lowpass, highpass, P, f32=False):
    N = samples(len(pitch), P)
    g = noise(N)
    x, _, _, _ = excite(pitch, P, g, f32)
    unv = np.array([_f32(v) for v in g]) if f32 else g
    e = fir(lowpass, x, f32) + fir(highpass, unv, f32)
    return np.array([_f32(v) for v in e]) if f32 else e


def mc2b(mc, alpha):
    """Rows of mc (float32 as the files hold them, or anything else) -> rows of b, in double."""
    mc = np.asarray(mc, dtype=np.float64)
    B = np.empty_like(mc)
    m = mc.shape[1] - 1
    for t in range(mc.shape[0]):
        b = float(mc[t, m])
        B[t, m] = b
        for i in range(m - 1, -1, -1):
            b = float(mc[t, i]) - alpha * b
            B[t, i] = b
    return B


def filter_b(e, B, alpha, P, pp, f32=False):
    """mglsadf -c 0 at interpolation period 1 on rows of b (T rows give (T - 1) P samples)."""
    B = np.asarray(B, dtype=np.float64)
    T, m1 = B.shape
    m = m1 - 1
    pd = len(pp) - 1
    pp = [float(v) for v in pp]
    aa = 1.0 - alpha * alpha
    d1 = [0.0] * (pd + 1)
    pt1 = [0.0] * (pd + 1)
    pt2 = [0.0] * (pd + 1)
    D = [[0.0] * (m + 2) for _ in range(pd)]
    exp = math.exp
    y = []
    b = [float(v) for v in B[0]]
    n = 0
    for f in range(T - 1):
        bn = [float(v) for v in B[f + 1]]
        inc = [(bn[k] - b[k]) / P for k in range(m1)]
        for _ in range(P):
            x = float(e[n]) * exp(b[0])
            n += 1
            out = 0.0                                   # mlsadf1
            b1 = b[1]
            for i in range(pd, 0, -1):
                d1[i] = aa * pt1[i - 1] + alpha * d1[i]
                pt1[i] = d1[i] * b1
                v = pt1[i] * pp[i]
                x += v if i & 1 else -v
                out += v
            pt1[0] = x
            out += x
            x = out
            out = 0.0                                   # mlsadf2
            for i in range(pd, 0, -1):
                d = D[i - 1]                            # mlsafir(pt2[i-1], D[i-1])
                d[0] = pt2[i - 1]
                d[1] = aa * d[0] + alpha * d[1]
                acc = 0.0
                for k in range(2, m + 1):
                    d[k] += alpha * (d[k + 1] - d[k - 1])
                    acc += d[k] * b[k]
                for k in range(m + 1, 1, -1):
                    d[k] = d[k - 1]
                pt2[i] = acc
                v = acc * pp[i]
                x += v if i & 1 else -v
                out += v
            pt2[0] = x
            out += x
            y.append(_f32(out) if f32 else out)
            b = [b[k] + inc[k] for k in range(m1)]
        b = bn
    return np.array(y, dtype=np.float64)


def mlsa_filter(e, mc, alpha, P, pp, f32=False):
    return filter_b(e, mc2b(mc, alpha), alpha, P, pp, f32)


def sensitivity(e, B, alpha, P, pp, seed, f32=False):
    """max |change of y| when e and every b move by one ulp with random signs: the reference's own conditioning."""
    rng = np.random.default_rng(seed)
    e = np.asarray(e, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    e2 = e + np.spacing(np.abs(e)) * rng.choice([-1.0, 1.0], e.shape)
    B2 = B + np.spacing(np.abs(B)) * rng.choice([-1.0, 1.0], B.shape)
    y = filter_b(e, B, alpha, P, pp, f32)
    return y, float(np.abs(filter_b(e2, B2, alpha, P, pp, f32) - y).max())


def tolerance(y, sens):
    """The project's idiom: max(10 sens, 64 ulp of max |y|)."""
    return max(10.0 * sens, 64.0 * float(np.spacing(np.abs(y).max())))


# ---- the reference-free anchor ------------------------------------------------------------------------------------
ANCHOR_ORDER, ANCHOR_ALPHA, ANCHOR_SAMPLES = 12, 0.42, 4096
ANCHOR_BOUNDS = {4: 1e-3, 5: 1e-3, 6: 1e-8, 7: 1e-10}


def anchor_mc():
    rng = np.random.default_rng(0)
    k = np.arange(1, ANCHOR_ORDER + 1)
    return np.concatenate([[0.3], rng.normal(size=ANCHOR_ORDER) / np.sqrt(k)])


def anchor_frames(P):
    """(mc rows, impulse): constant coefficients over enough frames for ANCHOR_SAMPLES samples."""
    T = ANCHOR_SAMPLES // P + 1
    e = np.zeros(ANCHOR_SAMPLES)
    e[0] = 1.0
    return np.tile(anchor_mc(), (T, 1)), e


def anchor_error(y, mc=None, alpha=ANCHOR_ALPHA):
    """max | ln |rfft(y)| - sum_k mc[k] cos(k w~) |, w~ = w + 2 atan(alpha sin w / (1 - alpha cos w))."""
    mc = anchor_mc() if mc is None else mc
    y = np.asarray(y, dtype=np.float64)
    w = 2.0 * np.pi * np.arange(len(y) // 2 + 1) / len(y)
    wt = w + 2.0 * np.arctan(alpha * np.sin(w) / (1.0 - alpha * np.cos(w)))
    want = sum(mc[k] * np.cos(k * wt) for k in range(len(mc)))
    return float(np.abs(np.log(np.abs(np.fft.rfft(y))) - want).max())

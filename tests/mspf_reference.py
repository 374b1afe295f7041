"""The modulation-spectrum postfilter of the recipe (scripts/Training.pl:2950-3038 postfiltering_mspf / msmp2seq, its
statistics :3133-3221 make_mspf), written out step by step in numpy: the definition the device code is held to.

Settings: frame_length Lw (odd), fft_length N (even), emphasis e; S = (Lw - 1) / 2, K = N / 2 + 1.  One column x[0 .. T):
  1  mu = mean(x), y = x - mu                                              (vstat -o 1, vopr -s)
  2  J = ceil((T + S) / S) frames; frame j holds z_j[i] = w[i] y[j S - S + i], y = 0 outside [0, T)   (window -w 5, frame)
  3  w is SPTK's Bartlett window (window -w 3 -n 0): 2 i / (Lw - 1) for i < Lw / 2, else 2 - 2 i / (Lw - 1)
  4  X_j = DFT_N(z_j), m_j[k] = 1/2 ln(|X_j[k]|^2 + 1e-30)                  (spec -o 1 -e 1e-30)
  5  m' = m + e (((m - mean_gen[k]) / std_gen[k]) std_nat[k] + mean_nat[k] - m)         (:2973-2982)
  6  X'_j[k] = exp(m') X_j[k] / |X_j[k]|, exp(m') where X_j[k] = 0; v_j the inverse real transform     (phase, ifftr)
  7  seq[j S + n] += v_j[n], n < N; out[t] = seq[S + t] + mu                 (msmp2seq adds the circular tail as well)
The transforms are direct cosine / sine sums (N <= 64), so the same code runs in any floating type, np.longdouble
included.  Columns never exchange data."""
import numpy as np


def hops(Lw):
    return (Lw - 1) // 2


def n_frames(T, Lw):
    S = hops(Lw)
    return 0 if T <= 0 else (T + S + S - 1) // S


def bartlett(Lw, dtype=np.float64):
    i = np.arange(Lw).astype(dtype)
    a = dtype(2) * i / dtype(Lw - 1)
    return np.where(np.arange(Lw) < Lw // 2, a, dtype(2) - a)


def _trig(N, dtype):
    """cos and sin of 2 pi r / N, r < N, exact at the quarter turns."""
    pi = dtype(4) * np.arctan(dtype(1))
    r = np.arange(N)
    ang = dtype(2) * pi * r.astype(dtype) / dtype(N)
    c, s = np.cos(ang), np.sin(ang)
    for q, (cq, sq) in enumerate(((1, 0), (0, 1), (-1, 0), (0, -1))):
        if (q * N) % 4 == 0:
            c[q * N // 4], s[q * N // 4] = cq, sq
    return c, s


def frames(y, Lw, dtype=np.float64):
    """[J][Lw]: step 2 and 3 on a mean-free column."""
    T, S = len(y), hops(Lw)
    J = n_frames(T, Lw)
    pad = np.zeros((J - 1) * S + Lw, dtype)
    pad[S:S + T] = y
    w = bartlett(Lw, dtype)
    return np.stack([pad[j * S:j * S + Lw] * w for j in range(J)])


def forward(x, Lw, N, dtype=np.float64, mean=None):
    """Steps 1-4 for one column: (mu, re [J][K], im [J][K], m [J][K])."""
    x = np.asarray(x, dtype)
    mu = x.mean(dtype=dtype) if mean is None else dtype(mean)
    z = frames(x - mu, Lw, dtype)
    K = N // 2 + 1
    c, s = _trig(N, dtype)
    idx = (np.arange(Lw)[:, None] * np.arange(K)[None, :]) % N
    re = z @ c[idx]
    im = -(z @ s[idx])
    m = dtype(0.5) * np.log(re * re + im * im + dtype(1e-30))
    return mu, re, im, m


def postfilter_column(x, mean_gen, std_gen, mean_nat, std_nat, Lw=25, N=64, emphasis=1.0, dtype=np.float64):
    """Steps 1-7 for one column; the four tables are [K]."""
    x = np.asarray(x, dtype)
    T, S, K = len(x), hops(Lw), N // 2 + 1
    mg, sg, mn, sn = (np.asarray(t, dtype) for t in (mean_gen, std_gen, mean_nat, std_nat))
    mu, re, im, m = forward(x, Lw, N, dtype)
    m2 = m + dtype(emphasis) * ((m - mg) / sg * sn + mn - m)
    amp = np.exp(m2)
    mag = np.sqrt(re * re + im * im)
    nz = mag > 0
    safe = np.where(nz, mag, dtype(1))
    re2 = np.where(nz, amp * re / safe, amp)
    im2 = np.where(nz, amp * im / safe, dtype(0))
    c, s = _trig(N, dtype)
    idx = (np.arange(K)[:, None] * np.arange(N)[None, :]) % N          # [K][N]
    wgt = np.full(K, 2, dtype)
    wgt[0] = wgt[-1] = 1
    v = ((re2 * wgt) @ c[idx] - (im2 * wgt) @ s[idx]) / dtype(N)       # im of bins 0 and N/2 meets sin = 0
    J = len(v)
    seq = np.zeros((J - 1) * S + N, dtype)
    for j in range(J):
        seq[j * S:j * S + N] += v[j]
    return seq[S:S + T] + mu


def postfilter(x, mean_gen, std_gen, mean_nat, std_nat, Lw=25, N=64, emphasis=1.0, dtype=np.float64):
    """x [T][dim], tables [dim][K] -> [T][dim]."""
    x = np.asarray(x)
    return np.stack([postfilter_column(x[:, d], mean_gen[d], std_gen[d], mean_nat[d], std_nat[d], Lw, N, emphasis, dtype)
                     for d in range(x.shape[1])], axis=1)


def stats(seqs, Lw, N, dtype=np.float64, means=None):
    """make_mspf's sums over a list of [T][dim] sequences: (sum [dim][K], sumsq [dim][K], n = sum of J).  The all-zero
    trailing frames count.  means: per sequence [dim] or None (the sequence's own)."""
    dim, K = np.asarray(seqs[0]).shape[1], N // 2 + 1
    s1, s2, n = np.zeros((dim, K), dtype), np.zeros((dim, K), dtype), 0
    for q, x in enumerate(seqs):
        x = np.asarray(x)
        if len(x) == 0:
            continue
        for d in range(dim):
            m = forward(x[:, d], Lw, N, dtype, None if means is None else means[q][d])[3]
            s1[d] += m.sum(axis=0, dtype=dtype)
            s2[d] += (m * m).sum(axis=0, dtype=dtype)
        n += n_frames(len(x), Lw)
    return s1, s2, n


def finalize(s1, s2, n):
    """Mean and population standard deviation sqrt(E[m^2] - E[m]^2) (vstat -o 1; vstat -o 2 -d | sopr -SQRT)."""
    mean = s1 / n
    return mean, np.sqrt(np.maximum(s2 / n - mean * mean, 0))


def label_segments(lines, frame_shift_s, n_rows, silences=()):
    """Rows kept by make_mspf's silence removal: label lines "start end name" in 100 ns units; a segment's frames are
    int(start 1e-7 / shift) .. int(end 1e-7 / shift), both inclusive (bcut -s -e), clipped to the file; adjacent
    segments repeat their boundary frame."""
    keep = []
    for line in lines:
        f = line.split()
        if len(f) < 3 or f[2] in silences:
            continue
        a = int(int(f[0]) * 1e-7 / frame_shift_s)
        b = min(int(int(f[1]) * 1e-7 / frame_shift_s), n_rows - 1)
        keep.extend(range(max(a, 0), b + 1))
    return np.asarray(keep, dtype=np.int64)

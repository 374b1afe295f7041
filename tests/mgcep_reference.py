"""SPTK's `frame` and `window` in numpy, as include/world_mi355.h defines them for WorldMi355MelCepstrumOfWaveform (the
two tools are not in the reference tree; everything behind them is held to the compiled mcep).

  frame    T >= 1 samples x[0 .. T), length L, shift P, 1 <= P <= L: J = ceil((T + L // 2) / P) frames,
           z_j[i] = x[j P - L // 2 + i], i < L, zero outside [0, T).  T = 0: J = 0.
  window   a = 2 pi / (L - 1); 0 Blackman, 1 Hamming, 2 Hanning, 5 rectangular; norm 0 as is, 1 sum w^2 = 1, 2 sum w = 1.
           cos is libm's (math.cos) and the sums are exact (math.fsum): the table is good to an ulp or two.
  windowed w[i] z_j[i], one multiply, rounded to float32 once with pipe_float32, then F - L zeros.
"""
import math

import numpy as np


def n_frames(T, L, P):
    assert 1 <= P <= L and T >= 0
    return 0 if T == 0 else -(-(T + L // 2) // P)


def frames(x, L, P):
    """[J][L] float64."""
    x = np.asarray(x, dtype=np.float64)
    T, J, h = len(x), n_frames(len(x), L, P), L // 2
    pad = np.zeros(h + max(J - 1, 0) * P + L + T)
    pad[h:h + T] = x
    return np.stack([pad[j * P:j * P + L] for j in range(J)]) if J else np.zeros((0, L))


def window(kind, norm, L):
    a = 2.0 * math.pi / (L - 1)
    if kind == 0:
        w = [0.42 - 0.5 * math.cos(a * i) + 0.08 * math.cos(2.0 * a * i) for i in range(L)]
    elif kind == 1:
        w = [0.54 - 0.46 * math.cos(a * i) for i in range(L)]
    elif kind == 2:
        w = [0.5 - 0.5 * math.cos(a * i) for i in range(L)]
    elif kind == 5:
        w = [1.0] * L
    else:
        raise ValueError(kind)
    if norm == 1:
        g = 1.0 / math.sqrt(math.fsum(v * v for v in w))
    elif norm == 2:
        g = 1.0 / math.fsum(w)
    else:
        assert norm == 0
        g = None
    return np.asarray(w if g is None else [v * g for v in w])


def windowed(x, w, P, F, pipe_float32=False):
    """[J][F] float64: the rows mcep's itype 0 takes."""
    L = len(w)
    assert L <= F
    z = frames(x, L, P) * np.asarray(w, dtype=np.float64)[None, :]
    if pipe_float32:
        z = z.astype(np.float32).astype(np.float64)
    out = np.zeros((len(z), F))
    out[:, :L] = z
    return out


def windowed_batch(xs, w, P, F, pipe_float32=False):
    """The utterances' rows one after another, as a batch holds them, and the frame counts."""
    parts = [windowed(x, w, P, F, pipe_float32) for x in xs]
    return np.concatenate(parts), [len(p) for p in parts]

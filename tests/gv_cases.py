"""The inputs that tests/test_gpu_mlpg_gv.py, tests/test_gpu_caller_stream.py and tests/test_mlpg_gv_host.py share, and
the numpy reference (tests/gv_reference.py) evaluated on them, once per process.  A helper, not a test."""
import functools

import numpy as np

import gv_reference as G
import mlpg_reference as M

# shorter than a window's reach, shorter than the band, below and above one round of the workgroup's 256 lanes
LENGTHS = (1, 2, 3, 7, 33, 200, 1000)
# (dim, window set, has a voicing column)
STREAMS = ((5, "recipe", False), (1, "recipe", True), (70, "static", False))


def voicing(lengths):
    """bool [sum T]: T = 7 has ONE voiced frame, T >= 33 has unvoiced runs, the rest is voiced."""
    out = []
    for T in lengths:
        v = np.ones(T, dtype=bool)
        if T == 7:
            v[:] = False
            v[3] = True
        elif T >= 33:
            v = (np.arange(T) // 17) % 3 != 1
            v[:3] = False
        out.append(v)
    return np.concatenate(out)


def holes(lengths):
    """uint8 [sum T]: a mask with single holes and one run; T = 2 keeps both frames, T = 3 keeps two."""
    tf = int(sum(lengths))
    i = np.arange(tf)
    m = (i % 11 != 4) & ~((i >= 60) & (i < 75))
    return m.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def inputs(lengths, var_per_frame, seed=31):
    """Per stream (mean, var, gv_mean, gv_var) float32, and the voicing (bool [sum T]).  gv_mean is three times the
    variance of the static means over the batch, gv_var the square of a fifth of it."""
    out = []
    for s, (dim, name, _) in enumerate(STREAMS):
        mean, var = M.make_stream(seed + 5 * s, list(lengths), dim, M.WINDOW_SETS[name], var_per_frame)
        gm = (3.0 * mean[:, :dim].astype(np.float64).var(axis=0) + 0.01).astype(np.float32)
        gvar = ((0.2 * gm.astype(np.float64)) ** 2).astype(np.float32)
        for a in (mean, var, gm, gvar):
            a.setflags(write=False)
        out.append((mean, var, gm, gvar))
    return out, voicing(lengths)


def members(lengths, voiced, has_msd, mask):
    m = np.ones(int(sum(lengths)), dtype=bool) if not has_msd else voiced.copy()
    return m if mask is None else m & (np.asarray(mask) != 0)


def reference(lengths, data, voiced, c0s, mask, edge, dtype, **options):
    """The reference on every utterance and stream, from the library's float32 start c0s (the definition's c0).  Per
    stream a dict: c [sum T][dim] (dtype), status / f0 / f1 / trials / accepts [n_utt][dim], gains and margins
    [n_utt][dim] lists."""
    off = np.concatenate([[0], np.cumsum(lengths)])
    res = []
    for (dim, name, has_msd), (mean, var, gm, gvar), c0 in zip(STREAMS, data, c0s):
        wins = M.WINDOW_SETS[name]
        mem = members(lengths, voiced, has_msd, mask)
        per = []
        for u in range(len(lengths)):
            a, b = off[u], off[u + 1]
            Rb, r = G.normal_bands(mean[a:b], var[a:b] if var.ndim == 2 else var, wins, edge, 0, dtype)
            per.append(G.generate(c0[a:b], Rb, r, len(wins), mem[a:b], gm, gvar, dtype, **options))
        d = {k: np.stack([p[k] for p in per]) for k in ("status", "f0", "f1", "trials", "accepts")}
        d["c"] = np.concatenate([p["c"] for p in per])
        d["gains"], d["margins"] = [p["gains"] for p in per], [p["margins"] for p in per]
        res.append(d)
    return res

"""Writes tests/golden/sptk_mspf.npz: the modulation-spectrum postfilter (scripts/Training.pl:2950-3038) on small
batches, from tests/mspf_reference.py -- no compiled reference has the tools the script chains (frame, window, spec,
phase, ifftr, vstat), so the definition written out in numpy is the reference, evaluated in long double.

Per option set (frame_length, fft_length, dim, emphasis): eight utterances of T = 1, 2, S-1, S, S+1, 2S, 2S+1, 5S+7
frames (S - 1 = 0 at frame_length 3: a zero-frame utterance), "generated" columns = the 5-point moving average of AR(1)
columns with distinct offsets, rounded to float32 as the recipe's files are; the four tables from the reference's own
statistics on three short sequences (natural: the AR(1) columns, generated: their moving average); the long-double
output; and `sens` per column, the larger of
  (a) the double chain's response to a seeded input perturbation of 4 * 2^-52 relative,
  (b) the double chain's distance from the long-double chain.
Admission, asserted here: 10 sens <= 1e-9 max|x| for every column.  No column is constant: a column that is zero after
its mean has bins whose phase is rounding noise, and a std_nat / std_gen below 1 lifts them out of the 1e-30 floor --
there the script itself is unstable.

Also printed, as a record and not a bound: the gap between the double chain and the same chain rounded to float32 at
every step, which is what the script's pipes do (its `x2x +fa` rounds further, to about 6 digits).

    python tools/gen_golden_mspf.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mspf_reference as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sptk_mspf.npz")

# key -> (frame_length, fft_length, dim, emphasis): every setting, every width and both emphases at least once; the
# wide blocks ride on the short hops to keep the file small
OPTIONS = {
    "l25n64d50e10": (25, 64, 50, 1.0),
    "l25n64d1e05": (25, 64, 1, 0.5),
    "l3n16d64e10": (3, 16, 64, 1.0),
    "l3n16d65e05": (3, 16, 65, 0.5),
    "l15n16d65e10": (15, 16, 65, 1.0),
    "l15n16d1e05": (15, 16, 1, 0.5),
    "l31n32d1e10": (31, 32, 1, 1.0),
    "l31n32d50e05": (31, 32, 50, 0.5),
}


def lengths(Lw):
    S = R.hops(Lw)
    return [1, 2, S - 1, S, S + 1, 2 * S, 2 * S + 1, 5 * S + 7]


def ar1(rng, T, dim):
    """AR(1) columns (pole 0.9) around distinct offsets."""
    e = rng.standard_normal((T + 32, dim))
    x = np.zeros_like(e)
    for t in range(1, len(e)):
        x[t] = 0.9 * x[t - 1] + e[t]
    return x[32:] + (0.5 + 0.37 * np.arange(dim)) * np.where(np.arange(dim) % 2, -1.0, 1.0)


def smooth(x):
    """5-point moving average, 'valid': four rows shorter."""
    return (x[4:] + x[3:-1] + x[2:-2] + x[1:-3] + x[:-4]) / 5.0


def seed_of(key):
    Lw, N, dim, e = OPTIONS[key]
    return 7919 * Lw + 104729 * N + 31 * dim + int(10 * e)


def tables(key):
    """(mean_gen, std_gen, mean_nat, std_nat), each [dim][K], from three short sequences."""
    Lw, N, dim, _ = OPTIONS[key]
    rng = np.random.default_rng(seed_of(key) + 1)
    nat = [ar1(rng, T + 4, dim) for T in (40, 57, 33)]
    gen = [smooth(x) for x in nat]
    nat = [x[2:-2] for x in nat]
    mn, sn = R.finalize(*R.stats(nat, Lw, N))
    mg, sg = R.finalize(*R.stats(gen, Lw, N))
    return mg, sg, mn, sn


def inputs(key):
    """The batch: a list of [T][dim] float64 arrays holding float32 values."""
    Lw, N, dim, _ = OPTIONS[key]
    rng = np.random.default_rng(seed_of(key))
    return [smooth(ar1(rng, T + 4, dim)).astype(np.float32).astype(np.float64) for T in lengths(Lw)]


def run(xs, tabs, Lw, N, e, dtype):
    return np.concatenate([R.postfilter(x, *tabs, Lw, N, e, dtype) if len(x) else np.zeros((0, x.shape[1]), dtype)
                           for x in xs])


def main():
    out = {"keys": np.asarray(sorted(OPTIONS))}
    worst_gap = 0.0
    for key in sorted(OPTIONS):
        Lw, N, dim, e = OPTIONS[key]
        xs, tabs = inputs(key), tables(key)
        assert all(np.isfinite(t).all() for t in tabs) and (tabs[1] > 0).all() and (tabs[3] > 0).all()
        rng = np.random.default_rng(seed_of(key) + 2)
        xp = [x * (1.0 + 4.0 * 2.0 ** -52 * rng.choice([-1.0, 1.0], size=x.shape)) for x in xs]
        ld = run(xs, tabs, Lw, N, e, np.longdouble)
        d = run(xs, tabs, Lw, N, e, np.float64)
        dp = run(xp, tabs, Lw, N, e, np.float64)
        f32 = run(xs, tabs, Lw, N, e, np.float32)
        a = np.abs(dp - d).max(axis=0)
        b = np.abs(d - ld).astype(np.float64).max(axis=0)
        sens = np.maximum(a, b)
        xmax = np.abs(np.concatenate(xs)).max(axis=0)
        assert (10.0 * sens <= 1e-9 * xmax).all(), (key, (sens / xmax).max())
        moved = np.abs(d - np.concatenate(xs)).max()
        gap = float(np.abs(f32.astype(np.float64) - d).max() / xmax.max())
        worst_gap = max(worst_gap, gap)
        print("%-14s frames %3d  sens/max|x| %.1e (a %.1e, b %.1e)  moved by %.2f  float32 chain gap %.1e of max|x|" % (
            key, len(d), (sens / xmax).max(), a.max(), b.max(), moved, gap))
        out[key + "/opt"] = np.asarray([Lw, N, dim, e])
        out[key + "/lengths"] = np.asarray([len(x) for x in xs])
        out[key + "/x"] = np.concatenate(xs).astype(np.float32)
        for name, t in zip(("mean_gen", "std_gen", "mean_nat", "std_nat"), tabs):
            out[key + "/" + name] = t
        out[key + "/out"] = ld.astype(np.float64)
        out[key + "/sens"] = sens
    np.savez_compressed(OUT, **out)
    print("wrote %s, %d bytes; worst float32 chain gap %.1e of max|x|" % (OUT, os.path.getsize(OUT), worst_gap))


if __name__ == "__main__":
    main()

"""Writes tests/golden/recipe_ffo.npz: the recipe's gap interpolation and one `ffo` block, produced by RUNNING the
reference's own Perl scripts -- data/scripts/interpolate.pl and data/scripts/window.pl with the window files of
data/win/ -- on seeded float32 streams, as oracle/gen_golden_cmp.py does for `cmp`.  Seeds, inputs and the scripts'
outputs are stored; nothing of the scripts themselves.  SPTK is not needed: the voicing flag (`sopr -magic -1.0E+10
-m 0 -a 1 -MAGIC 0`) and the `merge` chain are one comparison and one concatenation, done here in numpy.

    WORLD_REFERENCE=<the reference's tree> python tools/gen_golden_ffo.py        (needs perl; no GPU)

Cases: dim 1 and 2, T in 1, 2, 3, 5, 63, 64, 65, 130, 257, about half of the values gaps, with at least one leading gap,
trailing gap, gap longer than 64 frames, gap across a multiple of 64, an utterance whose only valid frame is its
first and one whose only valid frame is its last.  interpolate.pl exits with "no valid value" on a column without a
valid value, so no case has one.  A numpy float64 restatement (tests/ffo_reference.py) is compared with every output
and the number of differing values printed.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ffo_reference as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "recipe_ffo.npz")
MAGIC = np.float32(-1.0e10)
LENGTHS = (1, 2, 3, 5, 63, 64, 65, 130, 257)
FFO_T = 70
FFO_STREAMS = (("mgc", 5, False), ("lf0", 1, True), ("bap", 3, False))


def gap_mask(rng, T, dim):
    """True where a value is valid.  Random halves, then the shapes the cases must hold."""
    valid = rng.random((T, dim)) < 0.5
    if T == 1:
        valid[:] = True
    elif T == 2:
        valid[:, 0] = [True, False]                                  # a trailing gap
        if dim == 2:
            valid[:, 1] = [False, True]                              # a leading gap
    elif T == 3:
        valid[:, 0] = [True, False, True]
    elif T == 65:
        valid[:, 0] = False
        valid[0, 0] = True                                           # the only valid frame is the first
        if dim == 2:
            valid[61:65, 1] = [True, False, False, False]
    elif T == 130:
        valid[:, 0] = False
        valid[T - 1 if dim == 2 else 0, 0] = True                    # ... is the last (dim 2) / the first (dim 1)
    elif T == 257:
        valid[:3, 0] = False                                         # leading, trailing
        valid[T - 2:, 0] = False
        valid[60:200, dim - 1] = False                               # longer than 64, across 64, 128 and 192
        valid[59, dim - 1] = valid[200, dim - 1] = True
    for c in range(dim):
        if not valid[:, c].any():
            valid[rng.integers(T), c] = True
    return valid


def run(scripts, name, args):
    return subprocess.run(["perl", os.path.join(scripts, name)] + [str(a) for a in args], capture_output=True,
                          check=True).stdout


def main():
    ref = os.environ.get("WORLD_REFERENCE")
    if not ref:
        raise SystemExit("set WORLD_REFERENCE to the reference's tree")
    scripts, win = os.path.join(ref, "data", "scripts"), os.path.join(ref, "data", "win")
    out, differ, n_cases = {}, 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "x.in")
        for dim in (1, 2):
            for T in LENGTHS:
                seed = 1000 * dim + T
                rng = np.random.default_rng(seed)
                x = (5.0 + rng.standard_normal((T, dim))).astype(np.float32)
                x[~gap_mask(rng, T, dim)] = MAGIC
                x.tofile(path)
                res = np.frombuffer(run(scripts, "interpolate.pl", [dim, path]), dtype=np.float32).reshape(T, dim)
                key = "ip/d%d_T%d" % (dim, T)
                out[key + "/seed"], out[key + "/x"], out[key + "/out"] = seed, x, res
                differ += int((R.interpolate(x)[0].view(np.uint32) != res.view(np.uint32)).sum())
                n_cases += 1
        feats, blocks, wins_all = [], [], []
        for s, (name, dim, msd) in enumerate(FFO_STREAMS):
            rng = np.random.default_rng(7000 + s)
            x = (rng.standard_normal((FFO_T, dim)) + (5.0 if msd else 0.0)).astype(np.float32)
            if msd:
                x[~gap_mask(rng, FFO_T, dim)] = MAGIC
                x[:4] = MAGIC
                x[FFO_T - 3:] = MAGIC
            feats.append(x)
            wfiles = [os.path.join(win, "%s.win%d" % (name, i)) for i in (1, 2, 3)]
            wins = []
            for wf in wfiles:                                         # the coefficients, as window.pl reads them
                with open(wf) as f:
                    tok = f.readline().split()
                wins.append([float(v) for v in tok[1:1 + int(tok[0])]])
            wins_all.append(wins)
            x.tofile(path)
            if msd:
                blocks.append((x[:, :1] != MAGIC).astype(np.float32))                 # sopr ... -MAGIC 0
                ip = os.path.join(tmp, "x.ip")
                with open(ip, "wb") as f:
                    f.write(run(scripts, "interpolate.pl", [dim, path]))
                src = ip
            else:
                src = path
            blocks.append(np.frombuffer(run(scripts, "window.pl", [dim, src] + wfiles), dtype=np.float32).reshape(
                FFO_T, 3 * dim))
            out["ffo/%s" % name] = x
            for i, w in enumerate(wins):
                out["ffo/%s_win%d" % (name, i + 1)] = np.asarray(w, dtype=np.float64)
        rows = np.concatenate(blocks, axis=1)                         # merge +f -s 0 -l ... -L ...: side by side
        out["ffo/rows"] = rows
        out["ffo/names"] = np.array([n for n, _, _ in FFO_STREAMS])
        out["ffo/dims"] = np.array([d for _, d, _ in FFO_STREAMS])
        out["ffo/msd"] = np.array([m for _, _, m in FFO_STREAMS])
        mine, st = R.ffo_rows(feats, [(d, w, m) for (_, d, m), w in zip(FFO_STREAMS, wins_all)])
        differ += int((mine.view(np.uint32) != rows.view(np.uint32)).sum()) + st
    np.savez_compressed(OUT, **out)
    print("recipe_ffo ok: %d interpolation cases, ffo rows %s, %d values differ from the numpy restatement, %d bytes" % (
        n_cases, rows.shape, differ, os.path.getsize(OUT)))


if __name__ == "__main__":
    sys.exit(main())

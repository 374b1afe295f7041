#!/usr/bin/env python3
"""Writes tests/golden/makefilter.npz: what the recipe's data/scripts/makefilter.pl PRINTS for the sampling rates the
tests use -- the 31 low-pass (flag 0) and high-pass (flag 1) taps gen_wave hands to `dfs -b` (scripts/Training.pl:2873-
2899).  The taps of WorldMi355MlsaExcitation / MlsaSynthesis are the caller's; the library holds no filter table, and
none goes into it from here: these are recorded outputs for tests/test_gpu_mlsa.py and tests/test_gpu_mlsa_recipe.py.

    WORLD_REFERENCE=<the reference's tree> python tools/gen_golden_makefilter.py        (needs perl; no GPU)

Runs the script with perl, once per rate and flag.  Stored per rate and flag:
  text_<rate>_<flag>   the printed line, as it is (what `recipe mlsa-synth --lowpass / --highpass` takes)
  taps_<rate>_<flag>   the same parsed to float64 [31]
"""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (16000, 22050, 44100, 48000)


def main():
    tree = os.environ.get("WORLD_REFERENCE")
    if not tree:
        raise SystemExit("set WORLD_REFERENCE to the reference's tree")
    script = os.path.join(tree, "data", "scripts", "makefilter.pl")
    out = {}
    for rate in RATES:
        for flag in (0, 1):
            text = subprocess.run(["perl", script, str(rate), str(flag)], check=True, capture_output=True,
                                  text=True).stdout
            taps = np.array([float(t) for t in text.split()], dtype=np.float64)
            assert taps.shape == (31,) and np.isfinite(taps).all(), (rate, flag, text)
            out["text_%d_%d" % (rate, flag)] = np.array(text)
            out["taps_%d_%d" % (rate, flag)] = taps
    path = os.path.join(ROOT, "tests", "golden", "makefilter.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()

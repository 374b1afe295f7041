"""Golden vectors for the feature codec on the hand-made rows of tests/codec_features.py: what the compiled reference
(make -C oracle ref -> _ref/libworld_ref.so, and _ref/libsptk_ref.so for the bap decode) gives on golden_subset(), a
fixed part of the grid with every family at every fft_size.

Inputs are that generator's (three check sums per input array are stored, so that a drift of the generator shows as
such); outputs are stored whole where they are coded and at every 8th bin where they are decoded, all in one float64
array (the recipe's float32 files widen exactly).  tests/test_golden.py holds the oracle to the file on any machine.
Run in the container that has /root/reference:  python oracle/gen_golden_codec_handmade.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import codec_features as cf  # noqa: E402
from oracle.bindings import Reference, SptkReference  # noqa: E402
from oracle.gen_golden import save_npz_fixed  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "codec_handmade.npz")


def main():
    assert Reference.available() and SptkReference.available(), "build the reference first: make -C oracle ref"
    ref, sptk = Reference(), SptkReference()
    cases = cf.golden_subset()
    parts, shapes, first, in_checks = [], [], [0], []
    for c in cases:
        outs = [cf.golden_view(c, i, a) for i, a in enumerate(cf.outputs(ref, c, sptk.mgc2sp))]
        parts += [np.asarray(a, dtype=np.float64).ravel() for a in outs]
        shapes += [(a.shape + (1,))[:2] for a in outs]
        first.append(len(parts))
        chk = cf.input_check(c)
        in_checks.append(np.concatenate([chk, np.zeros(9 - len(chk))]))
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    save_npz_fixed(OUT, cases=np.array([cf.case_id(c) for c in cases]), first=np.array(first), offset=off,
                   shape=np.array(shapes), out=np.concatenate(parts), in_check=np.array(in_checks))
    print("codec_handmade", len(cases), "cases", int(off[-1]), "values", os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 400 * 1000


if __name__ == "__main__":
    main()

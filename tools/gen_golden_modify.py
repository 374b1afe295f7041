"""tests/golden/modify_handmade.npz: ParameterModification (test.cpp:201-238) on hand-made rows, with the interpolation
step run by the compiled reference's interp1 (make -C oracle ref -> oracle/_ref/libworld_ref.so), on
tests/modify_reference.py's GOLDEN_CASES at its GOLDEN_SHAPES.  The logarithm, the exponential and the fill around that
step are numpy's, as in modify_reference.modify_sp, whose own interp1 the file pins (tests/test_modify_host.py).  The
input rows are stored beside the results: the file does not depend on the generator staying as it is.
Run where the reference tree is:  python tools/gen_golden_modify.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import modify_reference as mr  # noqa: E402
from oracle.bindings import Reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "modify_handmade.npz")


def main():
    assert Reference.available(), "build the reference first: make -C oracle ref"
    ref = Reference()
    data = {}
    for fs, F in mr.GOLDEN_SHAPES:
        for family in sorted({f for f, _ in mr.GOLDEN_CASES}):
            data["in_%s_%d" % (family, F)] = mr.rows(family, F)
        for family, ratio in mr.GOLDEN_CASES:
            data[mr.golden_key(family, ratio, F)] = mr.modify_sp(mr.rows(family, F), ratio, fs, F, interp=ref.interp1)
    np.savez_compressed(OUT, **data)
    print("modify_handmade", len(data), "arrays", os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "codec_handmade.npz"))


if __name__ == "__main__":
    main()

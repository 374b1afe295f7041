"""What the objective-evaluation stage (csrc/dtw.hip) rests on without a GPU: the numpy reference itself
(tests/dtw_reference.py) against brute force, the condition that lets tests/test_gpu_dtw.py compare paths exactly, the host
halves of the public interface (pool_distortion, dtw_workspace_bytes, the label masks and the command line of `recipe.py
evaluate`), and the new names in the header, the bindings and the list of translation units."""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import dtw_cases as K
import dtw_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("WorldMi355DtwWorkspaceBytes", "WorldMi355DtwAlign", "WorldMi355FeatureDistortion")


@pytest.fixture(scope="module")
def W(pkg):
    pkg.world.load_library()
    return pkg.world


def test_reference_cost_is_the_minimum_over_all_monotone_paths():
    for ta, tb in itertools.product(range(1, 6), repeat=2):
        a, b = R.inputs(ta, tb, 3)
        path, cost, _ = R.dtw(a, b)
        assert cost == pytest.approx(R.brute_force_cost(a, b), rel=1e-14), (ta, tb)
        d = R.distances(a, b)
        assert sum(d[i, j] for i, j in path) == pytest.approx(cost, rel=1e-14)
        assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (ta - 1, tb - 1)
        steps = np.diff(path, axis=0)
        assert ((steps >= 0) & (steps <= 1)).all() and (steps.sum(axis=1) >= 1).all()


def test_reference_tie_rule():
    one = np.ones((3, 1), np.float32)
    path, cost, _ = R.dtw(one, np.ones((5, 1), np.float32))             # every D ties: the diagonal first, then (i-1, j)
    assert cost == 0.0 and [tuple(p) for p in path] == [(0, 0), (0, 1), (0, 2), (1, 3), (2, 4)]
    path, _, _ = R.dtw(np.ones((5, 1), np.float32), one)
    assert [tuple(p) for p in path] == [(0, 0), (1, 0), (2, 0), (3, 1), (4, 2)]


@pytest.mark.parametrize("pairs,shape", [(K.RAGGED, K.RAGGED_SHAPE), (K.WIDE, K.WIDE_SHAPE)])
def test_gpu_cases_do_not_hang_on_rounding(pairs, shape):
    for ta, tb in pairs:
        p64, c64, m64 = K.reference(ta, tb, shape["count"])
        pld, cld, _ = K.reference(ta, tb, shape["count"], True)
        assert np.array_equal(p64, pld), (ta, tb)
        if ta > 1 and tb > 1:
            assert m64 >= K.MIN_MARGIN, (ta, tb, m64)
        assert abs(float(cld) - float(c64)) <= K.cost_bound(ta, tb, shape["count"], c64)


def test_gpu_count_cases_do_not_hang_on_rounding():
    ta, tb = K.COUNTS_PAIR
    for count in K.COUNTS:
        p64, c64, m64 = K.reference(ta, tb, count)
        assert np.array_equal(p64, K.reference(ta, tb, count, True)[0]) and m64 >= K.MIN_MARGIN, (count, m64)


def test_pool_distortion(W):
    rng = np.random.default_rng(5)
    rows = np.zeros((40, 3, 4))
    rows[:, 0, 0] = rng.uniform(0, 1e3, 40) * 10.0 ** rng.integers(-8, 8, 40)         # sums that plain addition reorders
    rows[:, 0, 2] = rng.integers(1, 500, 40)
    rows[:, 0, 1] = rows[:, 0, 0] ** 2 / rows[:, 0, 2] * 1.5
    rows[:, 1, 0] = rng.uniform(0, 3, 40)
    rows[:, 1, 1] = rng.integers(1, 300, 40)
    rows[:, 1, 2] = rng.integers(0, 30, 40)
    rows[:, 1, 3] = rows[:, 1, 1] + rows[:, 1, 2] + rng.integers(0, 100, 40)
    rows[:, 2] = rows[:, 0]
    kinds = (0, 1, 0)
    whole = W.pool_distortion(rows, kinds)
    want = R.pooled(rows, kinds)
    assert whole[0]["mean_db"] == want[0]["mean_db"] == math.fsum(rows[:, 0, 0]) / rows[:, 0, 2].sum()
    assert whole[0]["pairs"] == int(rows[:, 0, 2].sum()) and whole[0]["std_db"] >= 0.0
    assert whole[1]["rmse_cents"] == want[1]["rmse_cents"]
    assert whole[1]["rmse_cents"] == 1200.0 / math.log(2.0) * math.sqrt(math.fsum(rows[:, 1, 0]) / rows[:, 1, 1].sum())
    assert whole[1]["vuv_error_percent"] == 100.0 * rows[:, 1, 2].sum() / rows[:, 1, 3].sum()
    assert whole[1]["voiced_pairs"] == int(rows[:, 1, 1].sum()) and whole[1]["pairs"] == int(rows[:, 1, 3].sum())
    # however the list was split over ranks and in whatever order the parts come back: the same figures, exactly
    for cut in (1, 13, 39):
        assert W.pool_distortion(np.concatenate([rows[cut:], rows[:cut]]), kinds) == whole
    assert W.pool_distortion(rows[rng.permutation(40)], kinds) == whole
    empty = W.pool_distortion(np.zeros((2, 2, 4)), (0, 1))
    assert math.isnan(empty[0]["mean_db"]) and math.isnan(empty[1]["rmse_cents"]) and empty[1]["pairs"] == 0
    with pytest.raises(ValueError):
        W.pool_distortion(rows, (0, 2, 0))


def test_dtw_workspace_bytes(W):
    sizes = [W.dtw_workspace_bytes([t], [t]) for t in (1, 2, 63, 64, 65, 400, 1600, 32767)]
    assert all(x <= y for x, y in zip(sizes, sizes[1:]))
    for ta, tb in ((1, 1), (64, 64), (65, 3), (3, 65), (400, 1600), (1600, 400), (32767, 32767)):
        n = W.dtw_workspace_bytes([ta], [tb])
        assert 4 * n >= ta * tb                                   # at least a byte per four cells
        assert n <= 2 * (ta + 63) * (tb + 66) + (1 << 16)         # and about a byte per cell of the padded strips
        assert W.dtw_workspace_bytes([ta, ta], [tb, tb]) >= n
        if max(ta, tb) < 32767:
            assert W.dtw_workspace_bytes([ta + 1], [tb]) >= n and W.dtw_workspace_bytes([ta], [tb + 1]) >= n
    assert W.dtw_workspace_bytes([5], [0]) > 0
    for bad in (([32768], [5]), ([5], [32768]), ([-1], [5]), ([5], [-1])):
        with pytest.raises(RuntimeError, match="bad argument"):
            W.dtw_workspace_bytes(*bad)
    with pytest.raises(ValueError):
        W.dtw_workspace_bytes([5, 6], [5])


def test_label_mask_and_groups(pkg):
    rc = pkg.recipe
    lines = ["0 125000 sil\n", "125000 325000 a\n", "325000 425000 pau\n", "425000 625000 b\n"]
    mask = rc.gv_label_mask(lines, 0.005, 14, ("sil", "pau"))          # 5 ms frames: segments [0,2] [2,6] [6,8] [8,12]
    assert mask.dtype == np.uint8 and mask.tolist() == [0, 0, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0]
    assert rc.gv_label_mask(lines, 0.005, 14).tolist() == [1] * 13 + [0]
    streams = [("mgc", 6), ("lf0", 1), ("bap", 3)]
    assert rc.evaluate_groups(streams) == [(1, 5, 0), (0, 1, 1), (0, 3, 0)]
    assert rc.evaluate_groups(streams, with_c0=True) == [(0, 6, 0), (0, 1, 1), (0, 3, 0)]
    for bad in ([("lf0", 2)], [("mgc", 1)], [("bap", 65)]):
        with pytest.raises(ValueError):
            rc.evaluate_groups(bad)
    assert rc.parse_eval_stream("mgc:50") == ("mgc", 50)
    for bad in ("mgc", "mgc:", ":5", "mgc:0", "mgc:x"):
        with pytest.raises(ValueError):
            rc.parse_eval_stream(bad)


def test_evaluate_command_line(pkg, tmp_path, capsys):
    rc = pkg.recipe
    for argv in (["evaluate", "--stream", "mgc:6"],                                  # no job list
                 ["evaluate", "--scp", "x", "--stream", "mgc"],                       # a stream without its dimension
                 ["evaluate", "--scp", "x", "--stream", "mgc:6", "--align", "band"]):
        with pytest.raises(SystemExit) as e:
            rc.main(argv)
        assert e.value.code == 2
    scp = tmp_path / "jobs.scp"
    scp.write_text("gen.mgc nat.mgc\n")                                               # the label column is missing
    with pytest.raises(SystemExit):
        rc.main(["evaluate", "--scp", str(scp), "--stream", "mgc:6"])
    np.zeros((4, 3), np.float32).tofile(tmp_path / "g.bap")
    np.zeros((4, 3), np.float32).tofile(tmp_path / "n.bap")
    scp.write_text("%s %s -\n" % (tmp_path / "g.bap", tmp_path / "n.bap"))
    with pytest.raises(SystemExit) as e:                                              # dtw without an mgc stream
        rc.main(["evaluate", "--scp", str(scp), "--stream", "bap:3"])
    assert e.value.code == 2
    capsys.readouterr()


def test_names_in_header_bindings_and_units():
    header = open(os.path.join(ROOT, "include", "world_mi355.h")).read()
    capi = open(os.path.join(ROOT, "hts-train-world_amd", "capi.py")).read()
    world = open(os.path.join(ROOT, "hts-train-world_amd", "world.py")).read()
    for name in NEW:
        assert name in header and name in capi and ("L.%s.argtypes" % name) in world, name
    assert "WorldMi355DistortionGroup" in header and "WorldMi355DistortionOption" in header
    units = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "hts-train-world_amd", "csrc"), "print-units"],
                           capture_output=True, text=True, check=True).stdout.split()
    assert "dtw.hip" in units                   # tests/hostsan builds its harness from this list


def test_symbols_and_refusals_on_the_host(W):
    import ctypes as C
    L = W.load_library()
    for name in NEW + ("WorldMi355DefaultDistortionOption",):
        assert hasattr(L, name)
    o = W.DistortionOption()
    L.WorldMi355DefaultDistortionOption(C.byref(o))
    assert o.voiced_above == -1.0e9
    out = C.c_int64(-1)
    assert L.WorldMi355DtwWorkspaceBytes(1, None, None, C.byref(out)) == 2
    assert L.WorldMi355DtwWorkspaceBytes(0, None, None, C.byref(out)) == 0 and out.value >= 0
    assert L.WorldMi355DtwAlign(None, None, 1, None, 1, None, 0, 1, None, None, None, None) == 2
    assert L.WorldMi355FeatureDistortion(None, None, None, None, None, 1, None, None, None) == 2

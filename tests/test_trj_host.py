"""The trajectory training criterion (DNNDefine.trajectory_cost, data/scripts/DNNDefine.py:240-399): what can be checked
without a GPU.  Our reading of the reference's window matrix, the two references of tests/trj_reference.py against each
other (and the analytic gradients against autograd), the ABI, its refusals, and the host logic of `trj-eval` and
final_outputs."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import mlpg_reference as M
import trj_reference as R
from conftest import ROOT


def create_window_matrix(T, D=2):
    """DNNDefine.py:318-333 with transpose=False, op for op in numpy, on the window_vector DNNTraining.py:141-160 builds
    from the recipe's three windows as DNNDataIO.load_window pads them to width 3."""
    windows = [[0.0, 1.0, 0.0], [-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]]
    num_windows, window_width = 3, len(windows[0])
    window_vector = []
    for j in range(window_width - 1, -1, -1):
        for k in range(num_windows):
            window_vector.append(windows[k][j])
    window_vector = np.repeat(np.reshape(window_vector, [1, -1]), D, axis=0).astype(np.float32)
    half_window_width = (window_width - 1) // 2
    half_window_vector = window_vector.T[0:num_windows * (window_width + 1) // 2, 0:D].T
    zero_vector = np.zeros([D, num_windows * (T - half_window_width)], dtype=np.float32)
    W = np.concatenate([window_vector, zero_vector], 1)
    W = np.tile(W, [1, T - 1])
    W = np.concatenate([W, half_window_vector], 1)
    W = np.reshape(W, [D, T, -1])
    W = W[:, :, num_windows * half_window_width:num_windows * half_window_width + 3 * T]
    return np.transpose(W, (0, 2, 1))                                            # [D][3 T][T]


@pytest.mark.parametrize("T", [1, 2, 3, 5, 64])
def test_window_matrix_is_the_references(T):
    W = create_window_matrix(T)
    want = M.window_matrix(T, M.RECIPE, 0)
    assert W.shape == (2, 3 * T, T)
    for d in range(2):
        np.testing.assert_array_equal(W[d].astype(np.float64), want)


SMALL = ((3, "recipe", False), (1, "recipe", True), (2, "five", False), (2, "static", False))


@pytest.mark.parametrize("weights", [(1.0, 1e-6), (0.0, 1.0), (10.0, 10.0)])
def test_references_agree_and_gradients_match_autograd(weights):
    """(a) dense + autograd against (b) banded long double + the analytic gradients, T = 1 .. 9 and 33: every
    quantity within 1e-9 of its scale (measured: below 1e-11)."""
    worst = 0.0
    for T in (1, 2, 3, 4, 9, 33):
        pred, obs, var, gv_var = R.make_case(100 + T, (T,), SMALL)
        a = R.dense(pred, obs, var, gv_var, SMALL, *weights)
        b = R.banded(pred, obs, var, gv_var, SMALL, *weights)
        _, w = R.check_sens(a, b, SMALL)
        worst = max(worst, w)
        assert w <= 1e-9, (T, w)
    print("msd_weight %g gv_weight %g: worst sens / scale %.3g" % (weights + (worst,)))


def test_gpu_cases_are_admitted():
    """The shapes of tests/test_gpu_trj.py: sens <= 1e-9 of every quantity's scale, in every utterance."""
    _, _, _, _, refs = R.cached_case(R.SEED, R.LENGTHS, R.STREAMS)
    for T, (_, _, _, worst) in zip(R.LENGTHS, refs):
        print("T %d: worst sens / scale %.3g" % (T, worst))
    assert max(r[3] for r in refs) <= 1e-9


def test_msd_is_zero_without_a_voicing_column():
    st = ((2, "recipe", False),)
    pred, obs, var, gv_var = R.make_case(3, (6,), st)
    a, b = R.dense(pred, obs, var, gv_var, st), R.banded(pred, obs, var, gv_var, st)
    assert a["cost"][1] == 0 and b["cost"][1] == 0


def test_abi_declared_exported_with_defaults(pkg):
    text = open(os.path.join(ROOT, "include", "world_mi355.h")).read()
    assert re.search(r"\bint\s+WorldMi355TrajectoryCost\s*\(", text)
    assert re.search(r"\bvoid\s+WorldMi355DefaultTrajectoryOption\s*\(", text)
    assert "DNNDefine.py:240-399" in text and '"trj_kernel"' in text
    lib = pkg.load_library()
    assert hasattr(lib, "WorldMi355TrajectoryCost") and hasattr(lib, "WorldMi355DefaultTrajectoryOption")
    O = pkg.world.TrajectoryOption
    o = O(7, 7.0, 7.0)
    lib.WorldMi355DefaultTrajectoryOption(ctypes.byref(o))
    assert (o.edge, o.msd_weight, o.gv_weight) == (0, 1.0, 1e-6)
    assert ctypes.sizeof(O) == 24 and (O.edge.offset, O.msd_weight.offset, O.gv_weight.offset) == (0, 8, 16)
    lib.WorldMi355DefaultTrajectoryOption(None)                                  # a null option struct is left alone
    assert hasattr(pkg.world.WorldBatch, "trajectory_cost") and hasattr(pkg.recipe, "trajectory_files")
    assert hasattr(pkg.training, "TrajectoryLoss") and hasattr(pkg.training, "final_outputs")


def _c_args(dims=(2,), wins=(M.RECIPE,), ld=6, ld_grad=6, edge=0, drop=(), grad=True):
    """A complete argument set of WorldMi355TrajectoryCost over host memory (never dereferenced: the batch is NULL or
    the set is refused first).  drop: names of required pointers to pass as NULL."""
    n = len(dims)
    dp = ctypes.POINTER(ctypes.c_double)
    buf = (ctypes.c_float * 64)()
    keep = [buf]
    ptrs = lambda: (ctypes.c_void_p * max(n, 1))(*[ctypes.addressof(buf)] * n)
    wptrs, sptrs = (ctypes.POINTER(dp) * max(n, 1))(), (ctypes.POINTER(ctypes.c_int) * max(n, 1))()
    for s, ws in enumerate(wins):
        arrs = [(ctypes.c_double * len(w))(*w) for w in ws]
        pa = (dp * len(ws))(*[ctypes.cast(a, dp) for a in arrs])
        sz = (ctypes.c_int * len(ws))(*[len(w) for w in ws])
        keep += [arrs, pa, sz]
        wptrs[s], sptrs[s] = ctypes.cast(pa, ctypes.POINTER(dp)), ctypes.cast(sz, ctypes.POINTER(ctypes.c_int))
    cost = (ctypes.c_double * 3)()
    a = {"pred": ptrs(), "obs": ptrs(), "var": ptrs(), "gv_var": ptrs(), "dims": (ctypes.c_int * max(n, 1))(*dims),
         "n_windows": (ctypes.c_int * max(n, 1))(*[len(w) for w in wins]), "windows": wptrs, "window_sizes": sptrs,
         "cost": ctypes.cast(cost, ctypes.c_void_p)}
    for name in drop:
        a[name] = None
    return a, n, ld, ld_grad, edge, ptrs() if grad else None, keep + [cost]


def _call(pkg, **kw):
    lib = pkg.load_library()
    a, n, ld, ld_grad, edge, grad, keep = _c_args(**kw)
    o = pkg.world.TrajectoryOption()
    lib.WorldMi355DefaultTrajectoryOption(ctypes.byref(o))
    o.edge = edge
    return lib.WorldMi355TrajectoryCost(None, n, a["pred"], a["obs"], ld, a["var"], a["gv_var"], a["dims"],
                                        a["n_windows"], a["windows"], a["window_sizes"], None, None, None,
                                        ctypes.byref(o), a["cost"], None, grad, None, ld_grad, None, None)


@pytest.mark.parametrize("what", [dict(), dict(dims=(), wins=()), dict(dims=(1,) * 5, wins=(M.RECIPE,) * 5), dict(dims=(0,)),
                                  dict(wins=([[1.0]] * 5,), ld=10, ld_grad=10), dict(drop=("pred",)), dict(drop=("obs",)),
                                  dict(drop=("var",)), dict(drop=("gv_var",)), dict(drop=("dims",)),
                                  dict(drop=("n_windows",)), dict(drop=("windows",)), dict(drop=("window_sizes",)),
                                  dict(drop=("cost",)), dict(ld=5), dict(ld_grad=5), dict(edge=1), dict(edge=-1),
                                  dict(wins=([[1.0], [0.0] * 7],), ld=4, ld_grad=4),
                                  dict(wins=([[1.0], [0.5, 0.5]],), ld=4, ld_grad=4)],
                         ids=["null_batch", "no_streams", "five_streams", "dim_0", "five_windows", "pred", "obs", "var",
                              "gv_var", "dims", "n_windows", "windows", "window_sizes", "cost", "ld", "ld_grad", "edge_1",
                              "edge_neg", "seven_taps", "even_size"])
def test_refusals_return_bad_argument_without_a_device(pkg, what):
    assert _call(pkg, **what) == 2                                               # WM_ERR_BAD_ARG


def test_null_option_is_refused(pkg):
    lib = pkg.load_library()
    a, n, ld, ld_grad, _, grad, keep = _c_args()
    assert lib.WorldMi355TrajectoryCost(None, n, a["pred"], a["obs"], ld, a["var"], a["gv_var"], a["dims"], a["n_windows"],
                                        a["windows"], a["window_sizes"], None, None, None, None, a["cost"], None, grad,
                                        None, ld_grad, None, None) == 2


def test_final_outputs_layout(pkg):
    import torch
    T = pkg.training
    layout = [(2, M.RECIPE, False), (1, M.RECIPE, True), (3, M.STATIC, False)]
    cols, width = pkg.recipe.ffo_layout(layout)
    assert width == 6 + 4 + 3
    b = types.SimpleNamespace(total_frames=4)
    pred = torch.arange(4 * width, dtype=torch.float32).reshape(4, width)
    c = [torch.full((4, d), -float(k + 1)) for k, (d, _, _) in enumerate(layout)]
    out = T.final_outputs(b, pred, c, layout)
    assert out.dtype == torch.float32 and tuple(out.shape) == (4, 2 + 1 + 1 + 3) == (4, pkg.recipe.trajectory_rows(layout))
    np.testing.assert_array_equal(out[:, :2].numpy(), -1)
    np.testing.assert_array_equal(out[:, 2].numpy(), pred[:, 6].numpy())         # the predicted voicing column
    np.testing.assert_array_equal(out[:, 3].numpy(), -2)
    np.testing.assert_array_equal(out[:, 4:].numpy(), -3)
    with pytest.raises(ValueError):
        T.final_outputs(b, pred[:, 1:], c, layout)
    with pytest.raises(ValueError):
        T.final_outputs(b, pred, c[:2], layout)
    views = T.stream_views(pred, pred + 1, layout)
    assert [tuple(v[0].shape) for v in views] == [(4, 6), (4, 3), (4, 3)]
    assert views[0][3] is None and views[2][3] is None and torch.equal(views[1][3][1], pred[:, 6] + 1)
    assert torch.equal(views[1][0], pred[:, 7:10]) and torch.equal(views[2][1], pred[:, 10:] + 1)


def test_trj_eval_arguments(pkg, tmp_path, monkeypatch, capsys):
    rec = pkg.recipe
    scp = tmp_path / "jobs.scp"
    scp.write_text("a.ffo a.obs a.out\n# comment\nb.ffo - b.out\nc.ffo c.obs -\n")
    seen = {}

    def fake(jobs, streams, var, gv, msd_weight, gv_weight, resume=False):
        seen.update(jobs=jobs, streams=streams, var=var, gv=gv, w=(msd_weight, gv_weight), resume=resume)
        return [1.5, None, 2.5e-3]

    monkeypatch.setattr(rec, "trajectory_files", fake)
    argv = ["trj-eval", "--scp", str(scp), "--stream", "50:0:m.win1,m.win2,m.win3", "--stream", "1:1:l.win1,l.win2",
            "--var", "ffo.var", "--gv-var", "gv.var"]
    assert rec.main(argv + ["--gv-weight", "0.5", "--resume"]) == 0
    assert seen["jobs"] == [("a.ffo", "a.obs", "a.out"), ("b.ffo", None, "b.out"), ("c.ffo", "c.obs", None)]
    assert seen["streams"] == [(50, ["m.win1", "m.win2", "m.win3"], False), (1, ["l.win1", "l.win2"], True)]
    assert (seen["var"], seen["gv"], seen["w"], seen["resume"]) == ("ffo.var", "gv.var", (1.0, 0.5), True)
    lines = capsys.readouterr().out.splitlines()
    assert lines == ["Evaluation: cost = %e (a.ffo)" % 1.5, "Evaluation: cost = %e (c.ffo)" % 2.5e-3]
    rec.main(argv)
    assert seen["w"] == (1.0, 1e-6) and seen["resume"] is False
    for bad in (["trj-eval", "--scp", str(scp), "--var", "v", "--gv-var", "g"], argv[:-2]):
        with pytest.raises(SystemExit):
            rec.main(bad)
    scp.write_text("a.ffo a.obs\n")
    with pytest.raises(SystemExit):
        rec.main(argv)


def test_ld_grad_is_checked_for_grad_msd_alone(pkg):
    """grad_pred NULL, grad_msd given: the row stride of the gradients is still held to a stream's row."""
    lib = pkg.load_library()
    a, n, ld, _, _, _, keep = _c_args(grad=False)
    o = pkg.world.TrajectoryOption()
    lib.WorldMi355DefaultTrajectoryOption(ctypes.byref(o))
    gm = (ctypes.c_void_p * 1)(None)
    assert lib.WorldMi355TrajectoryCost(None, n, a["pred"], a["obs"], ld, a["var"], a["gv_var"], a["dims"], a["n_windows"],
                                        a["windows"], a["window_sizes"], None, None, None, ctypes.byref(o), a["cost"],
                                        None, None, gm, 5, None, None) == 2

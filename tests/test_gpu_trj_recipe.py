"""recipe.trajectory_files (`trj-eval`) on a temporary directory of five small utterances: the files against
final_outputs of reference (b) of tests/trj_reference.py, the costs within its bounds, and, without targets, the rows
against gen_param_files' trajectories."""
import numpy as np
import pytest

import mlpg_reference as M
import trj_reference as R

pytestmark = pytest.mark.gpu

LENGTHS = (7, 1, 12, 3, 30)
STREAMS = ((4, "recipe", False), (1, "recipe", True), (2, "recipe", False))


def write_case(tmp_path):
    pred, obs, var, gv_var = R.make_case(77, LENGTHS, STREAMS)
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    jobs = []
    for u in range(len(LENGTHS)):
        p, o, out = tmp_path / ("u%d.pred" % u), tmp_path / ("u%d.ffo" % u), tmp_path / ("u%d.out" % u)
        pred[off[u]:off[u + 1]].tofile(p)
        obs[off[u]:off[u + 1]].tofile(o)
        jobs.append((str(p), str(o), str(out)))
    var.tofile(tmp_path / "ffo.var")
    gv_var.tofile(tmp_path / "gv.var")
    return pred, obs, var, gv_var, off, jobs


def test_files_and_costs(gpu, pkg, tmp_path):
    torch, W, ctx = gpu
    pred, obs, var, gv_var, off, jobs = write_case(tmp_path)
    st = R.named(STREAMS)
    weights = (2.0, 0.5)
    costs = pkg.recipe.trajectory_files(jobs, st, tmp_path / "ffo.var", tmp_path / "gv.var", *weights, ctx=ctx)
    lay, width = R.layout(st)
    cols = pkg.recipe.trajectory_rows(st)
    assert cols == 4 + 1 + 1 + 2 and len(costs) == len(jobs)
    worst = 0.0
    for u, (p, o, out) in enumerate(jobs):
        sl = slice(off[u], off[u + 1])
        a = R.dense(pred[sl], obs[sl], var, gv_var, STREAMS, *weights)
        b = R.banded(pred[sl], obs[sl], var, gv_var, STREAMS, *weights)
        sens, w = R.check_sens(a, b, STREAMS)
        assert w <= 1e-9
        bd = R.bounds(a, b, sens, STREAMS)
        rows = np.fromfile(out, dtype=np.float32).reshape(-1, cols)
        assert rows.shape[0] == LENGTHS[u]
        want = np.concatenate([b["c"][0], pred[sl][:, lay[1][0]:lay[1][0] + 1], b["c"][1], b["c"][2]], axis=1).astype(np.float64)
        tol = np.concatenate([bd["c"][0], [0.0], bd["c"][1], bd["c"][2]])
        err = np.abs(rows.astype(np.float64) - want)
        assert (err <= tol[None, :]).all(), (u, float((err / np.maximum(tol, 1e-300)).max()))
        np.testing.assert_array_equal(rows[:, 4], pred[sl][:, lay[1][0]])            # the predicted voicing column, as it is
        total = float(b["cost"][0] + weights[0] * b["cost"][1] + weights[1] * b["cost"][2])
        tol_c = float(bd["cost"][0] + weights[0] * bd["cost"][1] + weights[1] * bd["cost"][2])
        worst = max(worst, abs(costs[u] - total) / tol_c)
        assert abs(costs[u] - total) <= tol_c, (u, costs[u], total, tol_c)
    print("trajectory_files: worst cost error / bound %.3f" % worst)
    # resume: complete files are left alone and no cost is evaluated for them
    before = [np.fromfile(j[2], dtype=np.float32) for j in jobs]
    open(jobs[2][2], "wb").close()
    again = pkg.recipe.trajectory_files(jobs, st, tmp_path / "ffo.var", tmp_path / "gv.var", *weights, ctx=ctx, resume=True)
    assert [c is None for c in again] == [True, True, False, True, True] and again[2] == costs[2]
    for j, x in zip(jobs, before):
        np.testing.assert_array_equal(np.fromfile(j[2], dtype=np.float32), x)


def test_without_targets_equals_gen_param(gpu, pkg, tmp_path):
    torch, W, ctx = gpu
    pred, obs, var, gv_var, off, jobs = write_case(tmp_path)
    st = R.named(STREAMS)
    costs = pkg.recipe.trajectory_files([(p, None, out) for p, _, out in jobs], st, tmp_path / "ffo.var",
                                        tmp_path / "gv.var", ctx=ctx)
    assert costs == [None] * len(jobs)
    gjobs = [(p, str(tmp_path / ("g%d.mgc" % u)), str(tmp_path / ("g%d.lf0" % u)), str(tmp_path / ("g%d.bap" % u)))
             for u, (p, _, _) in enumerate(jobs)]
    pkg.recipe.gen_param_files(gjobs, st, tmp_path / "ffo.var", edge=0, ctx=ctx)
    lay, _ = R.layout(st)
    for u, ((p, _, out), g) in enumerate(zip(jobs, gjobs)):
        rows = np.fromfile(out, dtype=np.float32).reshape(LENGTHS[u], -1)
        mgc, lf0, bap = [np.fromfile(f, dtype=np.float32).reshape(LENGTHS[u], -1) for f in g[1:]]
        voiced = pred[off[u]:off[u + 1], lay[1][0]] >= np.float32(0.5)              # gen_param masks the unvoiced frames
        np.testing.assert_array_equal(rows[:, :4].view(np.uint32), mgc.view(np.uint32))
        np.testing.assert_array_equal(rows[:, 6:].view(np.uint32), bap.view(np.uint32))
        np.testing.assert_array_equal(rows[voiced, 5].view(np.uint32), lf0[voiced, 0].view(np.uint32))
        assert (lf0[~voiced] == np.float32(-1e10)).all() and np.isfinite(rows).all() and (np.abs(rows[:, 5]) < 1e6).all()
        np.testing.assert_array_equal(rows[:, 4], pred[off[u]:off[u + 1], lay[1][0]])

"""tests/train_step_reference.py, the float64 statement of one whole training step and of train_files' SGD loop, held
to what can be checked without a GPU: its two statements of the frame cost against each other, its trajectory
composition against trj_reference.banded, the frame mode's derived bound against a plain float32 evaluation of the same
step, the measured float32 distances (d32) that the GPU tests of the trajectory step and of the loop take their
tolerances from, and that every wrong wiring a training loop can hide leaves those tolerances far behind."""
import numpy as np
import pytest
import torch

import train_step_reference as S
import trj_reference as J

FRAME_CASES = ((1.0, 0), (0.8, 7))


def _ratio(err, bound):
    return float(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0).max())


@pytest.mark.parametrize("p,step", FRAME_CASES)
def test_frame_cost_statements_agree(pkg, p, step):
    """The reference's batch mean with picked variances against the weighted per-utterance training.frame_cost (unequal
    lengths 31, 129, 96; the speakers' variance rows differ), and against frame_bounds' numpy statement: the cost and
    every gradient within 1e-12 of the largest entry."""
    args = S.frame_args(p, step)
    (cost, grads, out), (bcost, _, bgrads, _, fw) = S.frame_reference(p, step)
    w = np.asarray(S.FRAME_LENGTHS, dtype=np.float64) / sum(S.FRAME_LENGTHS)
    wcost, wgrads, wout = S.frame_step(*args, weights=w)
    assert (wout == out).all() and np.abs(fw["out"] - out).max() <= 1e-12 * np.abs(out).max()
    assert abs(wcost - cost) <= 1e-12 * abs(cost) and abs(bcost - cost) <= 1e-12 * abs(cost)
    assert set(grads) == set(wgrads) == set(bgrads) and len(grads) == 9
    worst = 0.0
    for k in grads:
        scale = float(np.abs(grads[k]).max())
        assert scale > 0
        for other in (wgrads, bgrads):
            err = float(np.abs(other[k] - grads[k]).max())
            assert err <= 1e-12 * scale, (k, err, scale)
            worst = max(worst, err / scale)
    print("frame statements p %.1f: worst difference / largest entry %.2e" % (p, worst))


def test_trajectory_statement_agrees_with_banded():
    """The composition of trajectory_step (per utterance the speaker's variance row and GV row, the mean over the
    utterances) on given float32 outputs against trj_reference.banded per utterance, composed here by hand: the cost and
    both gradients within the sensitivity trj_reference.check_sens admits (1e-9 of every quantity's scale)."""
    params, x, obs, lengths, spkrs, _, _, _, _, _, layout, gv_var, mw, gw = S.trajectory_args()
    (_, _, out), _ = S.trajectory_reference()
    pred = out.astype(np.float32)
    tp = torch.tensor(pred.astype(np.float64)).requires_grad_(True)
    tv = torch.tensor(np.asarray(params[S.VAR], dtype=np.float64)).requires_grad_(True)
    cost = S.trajectory_criterion(tp, obs, tv, gv_var, lengths, spkrs, layout, mw, gw)
    cost.backward()
    off = np.concatenate([[0], np.cumsum(lengths)])
    n = len(lengths)
    want, S_cost, gvar, S_var = 0.0, 0.0, np.zeros(params[S.VAR].shape), np.zeros(params[S.VAR].shape)
    worst = 0.0
    for u, s in enumerate(spkrs):
        sl = slice(int(off[u]), int(off[u + 1]))
        b = J.banded(pred[sl], obs[sl], params[S.VAR][s], gv_var[s], layout, mw, gw)
        want += float(b["cost"][0] + mw * b["cost"][1] + gw * b["cost"][2]) / n
        S_cost += float(b["S_cost"][0] + mw * b["S_cost"][1] + gw * b["S_cost"][2]) / n
        gvar[s] += b["grad_var"].astype(np.float64) / n
        S_var[s] += b["S_var"].astype(np.float64) / n
        gp = b["grad_pred"].astype(np.float64) / n
        scale = np.abs(gp).max(axis=0)
        worst = max(worst, float((np.abs(tp.grad.numpy()[sl] - gp).max(axis=0) / np.maximum(scale, 1e-300)).max()))
    worst = max(worst, abs(cost.item() - want) / S_cost, float((np.abs(tv.grad.numpy() - gvar) / np.maximum(S_var, 1e-300)).max()))
    print("trajectory statement: worst sens / scale %.3g" % worst)
    assert worst <= 1e-9


@pytest.mark.parametrize("p,step", FRAME_CASES)
def test_frame_bound_covers_a_float32_step(p, step):
    """The derived bound of train_step_reference's docstring against the same step in plain float32 on the CPU (torch's
    summation order): the cost and every gradient element, variance.variances included."""
    (cost, grads, out), (_, e_cost, _, bounds, fw) = S.frame_reference(p, step)
    tcost, tgrads, tout = S.frame_step_f32(*S.frame_args(p, step))
    assert (np.abs(tout.astype(np.float64) - out) <= fw["e_out"]).all()
    print("p %.1f step %d: cost error / bound %.4f" % (p, step, abs(tcost - cost) / e_cost))
    assert abs(tcost - cost) <= e_cost
    worst = 0.0
    for k in grads:
        assert tgrads[k].dtype == np.float32 and np.isfinite(bounds[k]).all()
        ratio = _ratio(np.abs(tgrads[k].astype(np.float64) - grads[k]), bounds[k])
        print("p %.1f step %d %s: float32 step error / bound %.4f, bound / largest entry %.2e"
              % (p, step, k, ratio, float(bounds[k].max() / np.abs(grads[k]).max())))
        assert ratio <= 1.0, (k, ratio)
        worst = max(worst, ratio)
    print("p %.1f step %d: worst float32 step error / bound %.4f" % (p, step, worst))


def test_trajectory_d32():
    """d32 per parameter tensor of the trajectory step: float32 forward and backward with trj_reference.banded on the
    float32 outputs in between, against the float64 reference.  The GPU test allows 8 d32."""
    (cost, grads, _), d32 = S.trajectory_reference()
    assert np.isfinite(cost) and set(d32) == set(grads) | {"cost"}
    for k in sorted(d32):
        print("trajectory step d32 %-22s %.3e" % (k, d32[k]))
        assert 0.0 < d32[k] < 1e-3, k               # float32: far below any wiring error, see test_wrong_wirings


FRAME_WRONG = ("uniform_weights", "variance_row", "mask_offset", "variance_scatter")
TRJ_WRONG = ("variance_row", "mask_offset", "no_division", "variance_scatter", "gv_row")


@pytest.mark.parametrize("wrong", FRAME_WRONG)
def test_wrong_wirings_leave_the_frame_bound_behind(pkg, wrong):
    """Each wiring error, applied to the reference at keep_prob 0.8, moves at least one gradient element by more than
    100 times the bound the GPU test holds that element to."""
    (_, grads, _), (_, _, _, bounds, _) = S.frame_reference(0.8, 7)
    _, bad, _ = S.frame_step(*S.frame_args(0.8, 7), wrong=(wrong,))
    moved = {k: _ratio(np.abs(bad[k] - grads[k]), bounds[k]) for k in grads}
    k = max(moved, key=moved.get)
    print("frame %s: %s moves by %.3g bounds" % (wrong, k, moved[k]))
    assert moved[k] > 100.0


@pytest.mark.parametrize("wrong", TRJ_WRONG)
def test_wrong_wirings_leave_the_trajectory_tolerance_behind(wrong):
    """The same against 8 d32 max|reference| per parameter tensor."""
    (_, grads, _), d32 = S.trajectory_reference()
    _, bad, _ = S.trajectory_step(*S.trajectory_args(), wrong=(wrong,))
    moved = {k: float(np.abs(bad[k] - grads[k]).max() / (S.FACTOR * d32[k] * np.abs(grads[k]).max())) for k in grads}
    k = max(moved, key=moved.get)
    print("trajectory %s: %s moves by %.3g tolerances" % (wrong, k, moved[k]))
    assert moved[k] > 100.0


@pytest.mark.parametrize("trajectory", [False, True], ids=["frame", "trajectory"])
def test_sgd_loop_falls_and_its_float32_twin_stays_close(pkg, tmp_path, trajectory):
    """Four SGD steps over the files the GPU test trains on: the float64 cost falls at the learning rate used there, and
    the float32 twin's distance from the float64 loop (the GPU test allows 8 times it) is printed."""
    jobs, _ = S.write_loop_corpus(tmp_path, trajectory)
    costs, params = S.loop_reference(jobs, pkg.recipe, trajectory)
    tcosts, tparams = S.loop_reference(jobs, pkg.recipe, trajectory, np.float32)
    print("float64 costs:", " ".join("%.6f" % c for c in costs))
    assert len(costs) == S.LOOP_STEPS and np.isfinite(costs).all() and costs[-1] < costs[0]
    start = S.initial_parameters(S.LOOP_SEED, *S.LOOP_NET, 2, S.HIDDEN, S.OUTPUT, S.loop_variances()[0])
    for k in sorted(params):
        d = float(np.abs(tparams[k].astype(np.float64) - params[k]).max() / np.abs(params[k]).max())
        print("loop d32 %-22s %.3e (moved %.3e)" % (k, d, float(np.abs(params[k] - start[k]).max() / np.abs(params[k]).max())))
        assert tparams[k].dtype == np.float32 and 0.0 <= d < 1e-3 and (params[k] != start[k]).any(), k
    d = float(np.abs(np.array(tcosts) - costs).max() / np.abs(costs).max())          # the logged costs as one vector
    print("loop d32 %-22s %.3e" % ("costs", d))
    assert 0.0 < d < 1e-3

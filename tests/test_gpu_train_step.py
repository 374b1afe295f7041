"""A whole training step as recipe.train_files runs it -- recipe._train_cost, recipe._train_cost_trajectory, four SGD
steps of train_files itself -- against tests/train_step_reference.py, the float64 statement of the step, on the net
37 -> 48, 130 -> 229 (sigmoid / linear, SAT, 3 speakers; the loop: 37 -> 48 -> 229, 2 speakers) and the recipe's
229-column layout.  The kernels have their own tests; this one is about the wiring between them: the weights per
pseudo-utterance, each speaker's variance row and GV row, the masks' offset, the mean over the utterances, the scatter
of the variance gradient.  tests/test_train_step_host.py shows on the CPU that each of these, done wrong, leaves the
tolerances used here behind by more than a factor of 100.

Frame step: the cost within the forward bound propagated to it, every gradient element (variance.variances included)
within the bound DERIVED in train_step_reference's docstring; a plain float32 CPU evaluation of the step reaches 0.004 of
it.  Nothing in it is measured.

Trajectory step and the loops: a derived bound would need the criterion's Hessian, so the tolerance per parameter tensor
is 8 d32 max|reference|, d32 = max|float32 CPU step - float64 reference| / max|reference| (the float32 forward and
backward with trj_reference.banded on the float32 outputs in between; for the loops the float32 twin of sgd_steps after
the four steps, and the four logged costs as one vector).  The factor covers another summation order in three chained
products.  d32 is computed where the test runs; measured on the CPU:
  trajectory step  hidden0.si_weights 5.6e-07  hidden0.si_biases 1.1e-07  hidden0.sd_weights 1.6e-07
                   hidden1.si_weights 3.9e-07  hidden1.si_biases 1.3e-07  hidden1.sd_weights 1.6e-07
                   output.si_weights  4.3e-07  output.si_biases  3.9e-09  variance.variances 4.1e-08  cost 3.9e-09
  frame loop       hidden0.si_weights 1.3e-07  hidden0.si_biases 8.7e-08  hidden0.sd_weights 1.1e-07
                   output.si_weights  1.8e-07  output.si_biases  8.0e-08  variance.variances 1.1e-07  costs 2.5e-09
  trajectory loop  hidden0.si_weights 1.2e-07  hidden0.si_biases 7.3e-08  hidden0.sd_weights 1.1e-07
                   output.si_weights  1.6e-07  output.si_biases  5.3e-08  variance.variances 9.9e-08  costs 9.2e-09"""
import numpy as np
import pytest

import mlpg_reference as M
import train_step_reference as S

pytestmark = pytest.mark.gpu

GPU_LAYOUT = [(dim, M.RECIPE, msd) for dim, _, msd in S.LAYOUT]


def _module(torch, pkg, params):
    n_in, units, n_out = S.NET
    m = pkg.training.AcousticModel(n_in, list(units), n_out, S.N_SPKRS, S.HIDDEN, S.OUTPUT)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
    return m.cuda()


def _batch(W, ctx, lengths):
    return W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=list(lengths))


def _grads(m):
    return {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}


def _ratio(err, bound):
    assert np.isfinite(err).all()
    return float(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0).max())


@pytest.mark.parametrize("p,step", [(1.0, 0), (0.8, 7)])
def test_one_frame_step(gpu, pkg, p, step):
    """recipe._train_cost(...).backward() on pseudo-utterances of 31, 129 and 96 frames of speakers 0, 1, 2."""
    torch, W, ctx = gpu
    params, x, obs, lengths, spkrs, _, _, _, seed, _ = S.frame_args(p, step)
    (cost, grads, _), (_, e_cost, _, bounds, _) = S.frame_reference(p, step)
    m = _module(torch, pkg, params)
    b = _batch(W, ctx, lengths)
    try:
        got = pkg.recipe._train_cost(m, b, torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(obs)).cuda(), lengths,
                                     spkrs, p, seed, step)
        got.backward()
    finally:
        b.close()
    assert got.dtype == torch.float64
    print("frame step p %.1f step %d: cost error / bound %.4f" % (p, step, abs(float(got.detach()) - cost) / e_cost))
    assert abs(float(got.detach()) - cost) <= e_cost
    have = _grads(m)
    assert set(have) == set(grads)
    worst = 0.0
    for k in sorted(grads):
        assert have[k].dtype == np.float32 and have[k].shape == grads[k].shape
        ratio = _ratio(np.abs(have[k].astype(np.float64) - grads[k]), bounds[k])
        print("frame step p %.1f step %d %s: worst error / bound %.4f" % (p, step, k, ratio))
        worst = max(worst, ratio)
    print("frame step p %.1f step %d: worst error / bound %.4f" % (p, step, worst))
    assert worst <= 1.0


def _parts(W, ctx, lengths, spkrs, live):
    """train_files' parts: per speaker present (its index, a batch of its utterances, its first row, its end row)."""
    off = np.concatenate([[0], np.cumsum(lengths)])
    parts = []
    for s in sorted(set(spkrs)):
        k0, k1 = spkrs.index(s), len(spkrs) - spkrs[::-1].index(s)
        live.append(_batch(W, ctx, lengths[k0:k1]))
        parts.append((s, live[-1], int(off[k0]), int(off[k1])))
    return parts


def test_one_trajectory_step(gpu, pkg):
    """recipe._train_cost_trajectory on utterances of 2, 33, 129 and 40 frames of speakers 0, 0, 1, 2 at keep_prob 0.8,
    gv_weight 1 (so that the GV rows count)."""
    torch, W, ctx = gpu
    params, x, obs, lengths, spkrs, _, _, p, seed, step, _, gv_var, mw, gw = S.trajectory_args()
    (cost, grads, _), d32 = S.trajectory_reference()
    m = _module(torch, pkg, params)
    live = [_batch(W, ctx, lengths)]
    try:
        parts = _parts(W, ctx, lengths, spkrs, live)
        got = pkg.recipe._train_cost_trajectory(m, live[0], parts, torch.from_numpy(np.array(x)).cuda(),
                                                torch.from_numpy(np.array(obs)).cuda(), spkrs, GPU_LAYOUT,
                                                torch.from_numpy(np.array(gv_var)).cuda(), mw, gw, p, seed, step)
        got.backward()
    finally:
        for b in live:
            b.close()
    ratio = abs(float(got.detach()) - cost) / (S.FACTOR * d32["cost"] * abs(cost))
    print("trajectory step cost: error / (8 d32) %.4f (d32 %.3e)" % (ratio, d32["cost"]))
    worst = ratio
    have = _grads(m)
    assert set(have) == set(grads)
    for k in sorted(grads):
        assert have[k].dtype == np.float32 and have[k].shape == grads[k].shape and np.isfinite(have[k]).all()
        ratio = float(np.abs(have[k].astype(np.float64) - grads[k]).max() / (S.FACTOR * d32[k] * np.abs(grads[k]).max()))
        print("trajectory step %s: error / (8 d32) %.4f (d32 %.3e)" % (k, ratio, d32[k]))
        worst = max(worst, ratio)
    print("trajectory step: worst error / (8 d32) %.4f" % worst)
    assert worst <= 1.0


@pytest.mark.parametrize("trajectory", [False, True], ids=["frame", "trajectory"])
def test_four_sgd_steps_through_train_files(gpu, pkg, tmp_path, trajectory):
    """recipe.train_files from files: two speakers whose ffo.var and gv.var rows differ, keep_prob 0.5, log_interval 1;
    trajectory mode in batches of 3 utterances of at most 129 frames.  The four logged costs and every saved parameter
    against sgd_steps."""
    jobs, var_dir = S.write_loop_corpus(tmp_path, trajectory)
    cfg = S.LOOP_TRJ if trajectory else S.LOOP_FRAME
    n_in, units, n_out = S.LOOP_NET
    costs, params = S.loop_reference(jobs, pkg.recipe, trajectory)
    tcosts, tparams = S.loop_reference(jobs, pkg.recipe, trajectory, np.float32)
    assert costs[-1] < costs[0]
    path = str(tmp_path / "m.npz")
    extra = {"streams": S.LOOP_LAYOUT, "gv_weight": cfg["gv_weight"]} if trajectory else {}
    log = pkg.recipe.train_files(jobs, path, n_in, units, n_out, n_spkrs=2, variance_dir=var_dir, hidden_activation=S.HIDDEN,
                                 output_activation=S.OUTPUT, keep_prob=S.LOOP_KEEP, optimizer="sgd",
                                 learning_rate=cfg["learning_rate"], batch_size=cfg["batch_size"], n_steps=S.LOOP_STEPS,
                                 seed=S.LOOP_SEED, log_interval=1, report=lambda s: None, **extra)
    assert [s for s, _ in log] == list(range(S.LOOP_STEPS))
    got = np.array([c for _, c in log])
    d = float(np.abs(np.array(tcosts) - costs).max() / np.abs(costs).max())
    worst = float(np.abs(got - costs).max() / (S.FACTOR * d * np.abs(costs).max()))
    print("loop costs: error / (8 d32) %.4f (d32 %.3e); library %s, reference %s" % (worst, d, got.tolist(), costs))
    m = pkg.training.AcousticModel.load(path)
    assert m.step == S.LOOP_STEPS
    saved = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    assert set(saved) == set(params)
    for k in sorted(params):
        d = float(np.abs(tparams[k].astype(np.float64) - params[k]).max() / np.abs(params[k]).max())
        ratio = float(np.abs(saved[k].astype(np.float64) - params[k]).max() / (S.FACTOR * d * np.abs(params[k]).max()))
        print("loop %s: error / (8 d32) %.4f (d32 %.3e)" % (k, ratio, d))
        worst = max(worst, ratio)
    print("loop: worst error / (8 d32) %.4f" % worst)
    assert worst <= 1.0


# ---- the flag paths: designed statuses ---------------------------------------------------------------------------------
def test_frame_loss_flags_a_nan_in_obs(gpu, pkg):
    """A NaN in pseudo-utterance 1's obs: FrameLoss raises and names it; with skip_flagged that utterance costs 0 and the
    gradients are, within the single step's bound, the reference's with that utterance's weight set to 0."""
    torch, W, ctx = gpu
    p, step = 0.8, 7
    params, x, obs, lengths, spkrs, hidden, output, _, seed, _ = S.frame_args(p, step)
    bad = np.array(obs)
    off = np.concatenate([[0], np.cumsum(lengths)])
    bad[off[1] + 5, 17] = np.nan
    w = np.asarray(lengths, dtype=np.float64) / sum(lengths)
    w0 = np.array(w)
    w0[1] = 0.0
    cost, grads, _ = S.frame_step(params, x, bad, lengths, spkrs, hidden, output, p, seed, step, weights=w0)
    _, e_cost, _, bounds, _ = S.frame_bounds(params, x, bad, lengths, spkrs, hidden, output, p, seed, step, weights=w0)
    m = _module(torch, pkg, params)
    b = _batch(W, ctx, lengths)
    try:
        xd, od = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(bad).cuda()
        out = m.train_outputs(b, xd, spkrs, p, seed, step)
        with pytest.raises(RuntimeError, match=r"FrameLoss: utterances \[1\] are flagged \(status \[1\]\)"):
            pkg.training.FrameLoss.apply(b, out, m.variance.variances, od, spkrs)
        with pytest.raises(RuntimeError, match=r"FrameLoss: utterances \[1\]"):
            pkg.recipe._train_cost(m, b, xd, od, lengths, spkrs, p, seed, step)
        per = pkg.training.FrameLoss.apply(b, out, m.variance.variances, od, spkrs, True)
        costs = per.detach().cpu().numpy()
        assert costs[1] == 0.0 and costs[0] > 0 and costs[2] > 0
        total = (per * torch.from_numpy(w).cuda()).sum()
        total.backward()
    finally:
        b.close()
    assert abs(float(total.detach()) - cost) <= e_cost
    have = _grads(m)
    assert (have[S.VAR][1] == 0).all() and (grads[S.VAR][1] == 0).all()         # the flagged speaker's row: no gradient
    worst = 0.0
    for k in sorted(grads):
        ratio = _ratio(np.abs(have[k].astype(np.float64) - grads[k]), bounds[k])
        assert ratio <= 1.0, (k, ratio)
        worst = max(worst, ratio)
    print("skip_flagged: worst error / bound %.4f" % worst)


def test_train_outputs_flags_a_nan_in_x(gpu, pkg):
    torch, W, ctx = gpu
    params, x, obs, lengths, spkrs, _, _, _, seed, _ = S.frame_args(0.8, 7)
    bad = np.array(x)
    bad[int(lengths[0]) + int(lengths[1]) + 3, 36] = np.nan
    m = _module(torch, pkg, params)
    b = _batch(W, ctx, lengths)
    try:
        with pytest.raises(RuntimeError, match=r"train_outputs: utterances \[2\] are flagged \(status \[1\]\)"):
            m.train_outputs(b, torch.from_numpy(bad).cuda(), spkrs, 0.8, seed, 7)
    finally:
        b.close()

"""WorldBatch.trajectory_cost and training.TrajectoryLoss (trj_kernel, csrc/trj.hip) against reference (b) of
tests/trj_reference.py, the banded long-double statement with the analytic gradients, on the same float32 inputs --
never against another run of the library, except where a test is about two runs agreeing bit for bit.

Bounds (trj_reference.bounds), per utterance: c and grad_pred (float32) within mlpg_reference.bound per column,
spacing(float32(max|x|)) + 64 cond 2^-53 max|x|; the three costs and every entry of grad_var (double) within
max(10 sens, 64 2^-53 cond S), sens = |(a) - (b)| and S the sum of the magnitudes of the terms added."""
import numpy as np
import pytest

import mlpg_reference as M
import trj_reference as R

pytestmark = pytest.mark.gpu


def frames_batch(W, ctx, lengths):
    return W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=list(lengths))


def run(gpu, pkg, lengths, streams, pred, obs, var, gv_var, weights=(1.0, 1.0e-6), **want):
    torch, W, ctx = gpu
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    b = frames_batch(W, ctx, lengths)
    views = pkg.training.stream_views(dev(pred), dev(obs), R.named(streams))
    cost, c, gp, gvr, status = b.trajectory_cost(views, dev(var), dev(gv_var), *weights, **want)
    host = lambda t: None if t is None else t.cpu().numpy()
    out = host(cost), None if c is None else [host(t) for t in c], host(gp), host(gvr), host(status)
    b.close()
    return out


def check(got, lengths, streams, refs, what, weight=None):
    """Every utterance against (b) within trj_reference.bounds; prints and returns the worst error / bound per kind."""
    cost, c, gp, gvr, status = got
    off = np.concatenate([[0], np.cumsum(lengths)])
    worst = {"c": 0.0, "cost": 0.0, "grad_var": 0.0, "grad_pred": 0.0}
    fails = []
    for u, (a, b, sens, _) in enumerate(refs):
        bd = R.bounds(a, b, sens, streams)
        sl = slice(off[u], off[u + 1])
        pairs = [("cost", cost[u], b["cost"], bd["cost"])]
        if gvr is not None:
            pairs.append(("grad_var", gvr[u], b["grad_var"], bd["grad_var"]))
        if gp is not None:
            pairs.append(("grad_pred", gp[sl], b["grad_pred"], bd["grad_pred"][None, :]))
        if c is not None:
            pairs += [("c", cs[sl], cb, bb[None, :]) for cs, cb, bb in zip(c, b["c"], bd["c"])]
        for name, g, w, tol in pairs:
            assert np.isfinite(g).all(), (what, name, u)
            ratio = float((np.abs(g.astype(np.float64) - w.astype(np.float64)) / np.maximum(tol, 1e-300)).max())
            worst[name] = max(worst[name], ratio)
            if ratio > 1.0:
                fails.append((name, lengths[u], ratio))
    print("%s: worst error / bound: %s" % (what, ", ".join("%s %.3f" % kv for kv in worst.items())))
    assert (status == 0).all(), (what, status)
    assert not fails, (what, fails)
    return worst


def test_against_banded_reference(gpu, pkg):
    """Every band instantiation, one and two 64-lane chunks, a one-lane stream with a voicing column, lengths shorter
    than a window's reach up to 257: c, the three costs, grad_pred and every entry of grad_var."""
    pred, obs, var, gv_var, refs = R.cached_case(R.SEED, R.LENGTHS, R.STREAMS)
    got = run(gpu, pkg, R.LENGTHS, R.STREAMS, pred, obs, var, gv_var)
    assert got[0].dtype == np.float64 and got[3].dtype == np.float64 and got[2].dtype == np.float32
    assert [t.shape for t in got[1]] == [(sum(R.LENGTHS), d) for d, _, _ in R.STREAMS]
    check(got, R.LENGTHS, R.STREAMS, refs, "defaults")


W_LENGTHS = (5, 65)


@pytest.mark.parametrize("weights", [(0.0, 1.0), (10.0, 10.0), (1.0, 0.0)], ids=["msd0_gv1", "msd10_gv10", "msd1_gv0"])
def test_weights(gpu, pkg, weights):
    """gv_weight 1 and 10: the GV gradient (the second solve) is no longer lost beside the trajectory's."""
    pred, obs, var, gv_var, refs = R.cached_case(R.SEED + 100, W_LENGTHS, R.STREAMS, *weights)
    assert max(r[3] for r in refs) <= 1e-9
    got = run(gpu, pkg, W_LENGTHS, R.STREAMS, pred, obs, var, gv_var, weights)
    check(got, W_LENGTHS, R.STREAMS, refs, "msd_weight %g gv_weight %g" % weights)


def test_internal_precision(gpu, pkg):
    """T = 129, the recipe's windows, static variance 1 and delta variances 1e-6: the same banded algorithm in float32
    arithmetic (the helper with LD = np.float32) misses the bounds, the library keeps them."""
    T, dim = 129, 3
    st = ((dim, "recipe", False),)
    pred, obs, _, gv_var = R.make_case(5, (T,), st)
    var = np.repeat(np.array([1.0, 1e-6, 1e-6], dtype=np.float32), dim)
    a, b = R.dense(pred, obs, var, gv_var, st, 1.0, 1.0), R.banded(pred, obs, var, gv_var, st, 1.0, 1.0)
    sens, worst = R.check_sens(a, b, st)
    print("cond %.3g, worst sens / scale %.3g" % (a["cond"].max(), worst))
    bd = R.bounds(a, b, sens, st)
    f = R.banded(pred, obs, var, gv_var, st, 1.0, 1.0, LD=np.float32)
    miss = {"c": float((np.abs(f["c"][0] - b["c"][0]).astype(np.float64) / bd["c"][0]).max()),
            "cost": float((np.abs(f["cost"] - b["cost"]).astype(np.float64)[[0, 2]] / bd["cost"][[0, 2]]).max()),
            "grad_var": float((np.abs(f["grad_var"] - b["grad_var"]).astype(np.float64) / bd["grad_var"]).max()),
            "grad_pred": float((np.abs(f["grad_pred"] - b["grad_pred"]).astype(np.float64) / bd["grad_pred"]).max())}
    print("float32 inside: error / bound %s" % ", ".join("%s %.3g" % kv for kv in miss.items()))
    assert min(miss.values()) > 1.0
    got = run(gpu, pkg, (T,), st, pred, obs, var, gv_var, (1.0, 1.0))
    check(got, (T,), st, [(a, b, sens, worst)], "static var 1, delta var 1e-6")


def test_column_views_and_unread_columns(gpu, pkg):
    """Streams as column views of wider matrices with NaN in the columns nobody owns, and NaN in the dynamic columns
    of obs, which are never read: bit for bit the packed call."""
    torch, W, ctx = gpu
    lengths = W_LENGTHS
    pred, obs, var, gv_var, refs = R.cached_case(R.SEED + 100, lengths, R.STREAMS, 0.0, 1.0)
    plain = run(gpu, pkg, lengths, R.STREAMS, pred, obs, var, gv_var, (0.0, 1.0))
    st = R.named(R.STREAMS)
    lay, width = R.layout(st)
    tf = sum(lengths)
    wide_p, wide_o = [np.full((tf, 2 * width + 8), np.nan, dtype=np.float32) for _ in range(2)]
    at, where = 3, []
    for (mcol, c0, n), (dim, wins, _) in zip(lay, st):
        if mcol is not None:
            wide_p[:, at], wide_o[:, at] = pred[:, mcol], obs[:, mcol]
        m_at = at if mcol is not None else None
        at += 1 if mcol is not None else 0
        wide_p[:, at:at + n] = pred[:, c0:c0 + n]
        wide_o[:, at:at + dim] = obs[:, c0:c0 + dim]                      # the static window alone
        where.append((m_at, at, n))
        at += n + 2                                                       # two columns nobody owns
    dp, do = torch.from_numpy(wide_p).cuda(), torch.from_numpy(wide_o).cuda()
    views = [(dp[:, c0:c0 + n], do[:, c0:c0 + n], wins, None if m_at is None else (dp[:, m_at], do[:, m_at]))
             for (m_at, c0, n), (_, wins, _) in zip(where, st)]
    assert not views[0][0].is_contiguous()
    b = frames_batch(W, ctx, lengths)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    cost, c, gp, gvr, status = b.trajectory_cost(views, dev(var), dev(gv_var), 0.0, 1.0)
    assert (status.cpu().numpy() == 0).all()
    np.testing.assert_array_equal(cost.cpu().numpy().view(np.uint64), plain[0].view(np.uint64))
    np.testing.assert_array_equal(gvr.cpu().numpy().view(np.uint64), plain[3].view(np.uint64))
    np.testing.assert_array_equal(gp.cpu().numpy().view(np.uint32), plain[2].view(np.uint32))
    for x, y in zip(c, plain[1]):
        np.testing.assert_array_equal(x.cpu().numpy().view(np.uint32), y.view(np.uint32))
    b.close()
    check(plain, lengths, R.STREAMS, refs, "packed call of the column-view test")


def test_null_outputs_change_nothing(gpu, pkg):
    lengths = W_LENGTHS
    pred, obs, var, gv_var, _ = R.cached_case(R.SEED + 100, lengths, R.STREAMS, 0.0, 1.0)
    full = run(gpu, pkg, lengths, R.STREAMS, pred, obs, var, gv_var, (0.0, 1.0))
    for drop in ("want_c", "want_grad_pred", "want_grad_var"):
        got = run(gpu, pkg, lengths, R.STREAMS, pred, obs, var, gv_var, (0.0, 1.0), **{drop: False})
        assert got[{"want_c": 1, "want_grad_pred": 2, "want_grad_var": 3}[drop]] is None
        for x, y in zip(got, full):
            if x is None:
                continue
            for p, q in zip(x, y) if isinstance(x, list) else [(x, y)]:
                np.testing.assert_array_equal(p.view(np.uint8), q.view(np.uint8), err_msg=drop)


DELTA = [[-0.5, 0.0, 0.5]]                                                # no static window: singular at odd T
F_STREAMS = ((3, "recipe", False), (1, "recipe", True), (2, DELTA, False))
F_LENGTHS = (4, 3, 6, 2, 8)


def flagged_case():
    pred, obs, var, gv_var = R.make_case(31, F_LENGTHS, F_STREAMS)
    lay, width = R.layout(R.named(F_STREAMS))
    var = var.copy()
    var[lay[2][1]:] = 1.0                                                 # unit variances: the zero pivot is exact
    return pred.copy(), obs.copy(), var, gv_var.copy(), lay, width


def test_flagged_utterances_and_untouched_neighbours(gpu, pkg):
    """Bit 1: a NaN in pred.  Bit 2: the stream without a static window at T = 3.  The flagged utterances have costs 0
    and gradients 0, and c is zeros in the flagged columns; the others equal, bit for bit, the batch without the
    flagged utterances, and an utterance run alone equals itself inside the batch."""
    pred, obs, var, gv_var, lay, width = flagged_case()
    off = np.concatenate([[0], np.cumsum(F_LENGTHS)])
    pred[off[2] + 4, lay[0][1] + 3 + 1] = np.nan                          # utterance 2: delta mean of dim 1, stream 0
    cost, c, gp, gvr, status = run(gpu, pkg, F_LENGTHS, F_STREAMS, pred, obs, var, gv_var, (1.0, 1.0))
    assert status.tolist() == [0, 2, 1, 0, 0]
    for u in (1, 2):
        assert (cost[u] == 0).all() and (gvr[u] == 0).all() and (gp[off[u]:off[u + 1]] == 0).all()
    assert (c[2][off[1]:off[2]] == 0).all() and (c[0][off[2]:off[3], 1] == 0).all()
    assert (c[0][off[1]:off[2]] != 0).all() and (c[0][off[2]:off[3], 0] != 0).all()      # unflagged columns keep c
    for u in (0, 3, 4):
        assert (cost[u] != 0).all() and np.isfinite(gp[off[u]:off[u + 1]]).all() and (gvr[u] != 0).all()
    good = [0, 3, 4]
    keep = np.concatenate([np.arange(off[u], off[u + 1]) for u in good])
    for sel, rows in ((good, keep), ([4], np.arange(off[4], off[5]))):
        cost2, c2, gp2, gvr2, status2 = run(gpu, pkg, [F_LENGTHS[u] for u in sel], F_STREAMS, pred[rows], obs[rows], var,
                                            gv_var, (1.0, 1.0))
        assert status2.tolist() == [0] * len(sel)
        np.testing.assert_array_equal(cost[sel].view(np.uint64), cost2.view(np.uint64))
        np.testing.assert_array_equal(gvr[sel].view(np.uint64), gvr2.view(np.uint64))
        np.testing.assert_array_equal(gp[rows].view(np.uint32), gp2.view(np.uint32))
        for x, y in zip(c, c2):
            np.testing.assert_array_equal(x[rows].view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("which", ["var", "gv_var", "msd_var", "obs", "msd_pred"])
def test_bad_inputs_set_bit_1(gpu, pkg, which):
    """A variance of 0 (the row is shared: every utterance is flagged), a NaN in obs' static window or in a voicing
    column (that utterance alone)."""
    pred, obs, var, gv_var, lay, width = flagged_case()
    lengths, keep = (4, 6, 2), np.r_[0:4, 7:13, 13:15]                    # without the T = 3 utterance
    pred, obs = pred[keep], obs[keep]
    want = [1, 1, 1]
    if which == "var":
        var[lay[0][1] + 2] = 0.0
    elif which == "gv_var":
        gv_var[1] = 0.0
    elif which == "msd_var":
        var[lay[1][0]] = -1.0
    elif which == "obs":
        obs[5, lay[0][1]] = np.inf
        want = [0, 1, 0]
    else:
        pred[11, lay[1][0]] = np.nan
        want = [0, 0, 1]
    cost, c, gp, gvr, status = run(gpu, pkg, lengths, F_STREAMS, pred, obs, var, gv_var)
    assert status.tolist() == want
    off = np.concatenate([[0], np.cumsum(lengths)])
    for u, flag in enumerate(want):
        if flag:
            assert (cost[u] == 0).all() and (gvr[u] == 0).all() and (gp[off[u]:off[u + 1]] == 0).all()
        else:
            assert (cost[u] != 0).all() and np.isfinite(gp[off[u]:off[u + 1]]).all()


def test_trajectory_loss(gpu, pkg):
    """Upstream weights per utterance: pred.grad equals the weighted reference gradient within the weighted bound,
    var.grad (float32) the weighted sum of the utterances' grad_var within the weighted sum of their bounds plus one
    float32 spacing of the result."""
    torch, W, ctx = gpu
    pred, obs, var, gv_var, refs = R.cached_case(R.SEED, R.LENGTHS, R.STREAMS)
    st = R.named(R.STREAMS)
    wts = np.array([0.5, 2.0, 1.0, 0.25, 3.0, 0.0, 1.5, 0.75])
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    b = frames_batch(W, ctx, R.LENGTHS)
    p, v = dev(pred).requires_grad_(True), dev(var).requires_grad_(True)
    cost = pkg.training.TrajectoryLoss.apply(b, p, v, dev(obs), dev(gv_var), st)
    assert tuple(cost.shape) == (len(R.LENGTHS),) and cost.dtype == torch.float64
    (cost * dev(wts)).sum().backward()
    assert p.grad.dtype == torch.float32 and v.grad.dtype == torch.float32 and tuple(v.grad.shape) == var.shape
    off = np.concatenate([[0], np.cumsum(R.LENGTHS)])
    gp, gv = p.grad.cpu().numpy().astype(np.float64), v.grad.cpu().numpy().astype(np.float64)
    want_v, tol_v, worst = np.zeros(var.shape), np.zeros(var.shape), 0.0
    for u, (a, bb, sens, _) in enumerate(refs):
        bd = R.bounds(a, bb, sens, R.STREAMS)
        total = float(bb["cost"][0] + bb["cost"][1] + 1e-6 * bb["cost"][2])
        assert abs(float(cost[u].detach()) - total) <= bd["cost"][0] + bd["cost"][1] + 1e-6 * bd["cost"][2]
        want = wts[u] * bb["grad_pred"].astype(np.float64)
        tol = wts[u] * bd["grad_pred"][None, :] + np.spacing(np.abs(want).max(axis=0).astype(np.float32)).astype(np.float64)
        err = np.abs(gp[off[u]:off[u + 1]] - want)
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
        assert (err <= tol).all(), (R.LENGTHS[u], float((err / np.maximum(tol, 1e-300)).max()))
        want_v += wts[u] * bb["grad_var"].astype(np.float64)
        tol_v += wts[u] * bd["grad_var"]
    tol_v += np.spacing(np.abs(want_v).astype(np.float32)).astype(np.float64)
    ratio = float((np.abs(gv - want_v) / tol_v).max())
    print("TrajectoryLoss: pred.grad worst error / bound %.3f, var.grad %.3f" % (worst, ratio))
    assert ratio <= 1.0
    b.close()


def test_trajectory_loss_skip_flagged(gpu, pkg):
    torch, W, ctx = gpu
    pred, obs, var, gv_var, lay, width = flagged_case()
    st = R.named(F_STREAMS)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    b = frames_batch(W, ctx, F_LENGTHS)
    p, v = dev(pred).requires_grad_(True), dev(var).requires_grad_(True)
    with pytest.raises(RuntimeError, match="flagged"):
        pkg.training.TrajectoryLoss.apply(b, p, v, dev(obs), dev(gv_var), st)
    cost = pkg.training.TrajectoryLoss.apply(b, p, v, dev(obs), dev(gv_var), st, 1.0, 1.0e-6, True)
    host = cost.detach().cpu().numpy()
    assert host[1] == 0.0 and (host[[0, 2, 3, 4]] != 0).all()
    cost.sum().backward()
    off = np.concatenate([[0], np.cumsum(F_LENGTHS)])
    g = p.grad.cpu().numpy()
    assert (g[off[1]:off[2]] == 0).all() and np.isfinite(g).all() and (g[off[2]:off[3]] != 0).any()
    assert np.isfinite(v.grad.cpu().numpy()).all()
    b.close()


def test_timing_name(gpu, pkg):
    torch, W, ctx = gpu
    ctx.timing_enable(True)
    try:
        assert ctx.timing_query("trj_kernel")[1] == 0
        pred, obs, var, gv_var, _, _ = flagged_case()
        run(gpu, pkg, F_LENGTHS, F_STREAMS, pred, obs, var, gv_var)
        assert ctx.timing_query("trj_kernel")[1] == 1
    finally:
        ctx.timing_enable(False)

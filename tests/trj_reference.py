"""The trajectory training criterion (DNNDefine.trajectory_cost, data/scripts/DNNDefine.py:240-399) stated twice, the
yardsticks of tests/test_trj_host.py, tests/test_gpu_trj.py and tests/test_gpu_trj_recipe.py.  A helper, not a test.
TensorFlow is not available to the tests, so the reference's own Python cannot run: these two statements, written
independently of each other and of the library, are what the library is held to.

(a) dense():  trajectory_cost line by line in torch float64 on the CPU -- the dense W of mlpg_reference.window_matrix
    (edge 0), W' S W, its Cholesky factor, the FULL inverse by cholesky_solve against eye(T), the three costs exactly as
    the reference composes them -- and torch autograd for the gradients with respect to pred and var.  dense_terms()
    is the same statement on float64 tensors as they are given, the three cost terms returned as tensors: what
    tests/train_step_reference.py chains behind the network's forward pass.
(b) banded(): a banded LDL' written out in np.longdouble gives ln det A, c and the band of A^-1 (backward recurrence);
    the cost terms and the ANALYTIC gradients of the issue are evaluated from them.  It also returns, per quantity, S:
    the sum of the magnitudes of the terms that were added to make it (in the quantity's own units).

One utterance: pred, obs float32 [T][width] in the `ffo` layout of `streams` = [(dim, windows, msd)], var float32
[width], gv_var float32 [sum dims].  sens of a quantity is |a - b|; a case is admitted when sens <= 1e-9 of the
quantity's scale (check_sens)."""
import functools

import numpy as np

import mlpg_reference as M

LD = np.longdouble
LN2PI = float(np.log(2.0 * np.pi))

# the shapes of tests/test_gpu_trj.py: every band instantiation (0, 2, 4), one and two 64-lane chunks, a one-lane stream
LENGTHS = (1, 2, 3, 5, 63, 64, 65, 257)
STREAMS = ((50, "recipe", False), (1, "recipe", True), (25, "five", False), (65, "static", False))
# make_case's seed for them: of seeds 1 .. 12 the one whose largest sens / scale is smallest (1.8e-10; the dense inverse
# of (a) loses about cond 2^-53, and cond reaches 1e6 to 5e6 with variances spread over 1e-3 .. 1e3)
SEED = 3


def layout(streams):
    """[(voicing column or None, first column, columns)], width -- recipe.ffo_layout, restated."""
    at, out = 0, []
    for dim, wins, msd in streams:
        out.append((at if msd else None, at + (1 if msd else 0), dim * len(wins)))
        at = out[-1][1] + out[-1][2]
    return out, at


def named(streams):
    return [(d, M.WINDOW_SETS[w] if isinstance(w, str) else w, m) for d, w, m in streams]


# ---- (a) dense, float64, autograd ----------------------------------------------------------------------------------
def dense_terms(p_, o_, v_, g_, streams, want_cond=False):
    """trajectory_cost of one utterance on torch float64 tensors as they are given -- nothing is cast, detached or
    differentiated here, so the tensors may carry autograd history (tests/train_step_reference.py chains the network
    in front).  p_, o_: [T][width], v_: [width], g_: [sum dims].  Returns (trj, msd, gv, cs, conds): the three cost
    terms as tensors, c per stream as numpy, the condition numbers (empty without want_cond)."""
    import torch
    streams = named(streams)
    lay, width = layout(streams)
    T = p_.shape[0]
    D = sum(d for d, _, _ in streams)
    Mn = sum(1 for _, _, m in streams if m)
    covdet = mahala = torch.zeros((), dtype=torch.float64)
    msd_covdet = msd_mahala = torch.zeros((), dtype=torch.float64)
    pvs, ovs, cs, conds = [], [], [], []
    for (mcol, c0, n), (dim, wins, _) in zip(lay, streams):
        nw = len(wins)
        W = torch.tensor(M.window_matrix(T, wins, 0))                          # [(t, i)][T]
        mu = p_[:, c0:c0 + n].reshape(T, nw, dim).permute(2, 0, 1).reshape(dim, T * nw, 1)
        prec = (1.0 / v_[c0:c0 + n]).reshape(nw, dim).t()                      # [dim][nw]
        prec = prec[:, None, :].expand(dim, T, nw).reshape(dim, T * nw)
        WS = W.t()[None] * prec[:, None, :]                                    # [dim][T][(t, i)]
        WSW = WS @ W
        L = torch.linalg.cholesky(WSW)
        P = torch.cholesky_solve(torch.eye(T, dtype=torch.float64).expand(dim, T, T), L)
        c = P @ (WS @ mu)                                                      # [dim][T][1]
        oc = o_[:, c0:c0 + dim].t()[:, :, None]
        e = oc - c
        covdet = covdet - 2.0 * torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum()
        mahala = mahala + (e.transpose(1, 2) @ (WSW @ e)).sum()
        pvs.append(((c - c.mean(1, keepdim=True)) ** 2).mean(1)[:, 0])
        ovs.append(((oc - oc.mean(1, keepdim=True)) ** 2).mean(1)[:, 0])
        cs.append(c[:, :, 0].t().detach().numpy())
        if want_cond:
            conds.append(np.linalg.cond(WSW.detach().numpy()))
        if mcol is not None:
            mp = 1.0 / v_[mcol]
            msd_covdet = msd_covdet - T * torch.log(mp)
            msd_mahala = msd_mahala + ((p_[:, mcol] - o_[:, mcol]) ** 2 * mp).sum()
    trj = (D * T * LN2PI + covdet + mahala) / (2.0 * D * T)
    msd = (Mn * T * LN2PI + msd_covdet + msd_mahala) / (2.0 * Mn * T) if Mn else torch.zeros((), dtype=torch.float64)
    pv, ov = torch.cat(pvs), torch.cat(ovs)
    gv = (D * LN2PI + torch.log(g_).sum() + ((pv - ov) ** 2 / g_).sum()) / (2.0 * D)
    return trj, msd, gv, cs, conds


def dense(pred, obs, var, gv_var, streams, msd_weight=1.0, gv_weight=1.0e-6, want_cond=True):
    import torch
    f64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float32).astype(np.float64))
    p_, v_ = f64(pred).requires_grad_(True), f64(var).requires_grad_(True)
    trj, msd, gv, cs, conds = dense_terms(p_, f64(obs), v_, f64(gv_var), streams, want_cond)
    total = trj + msd_weight * msd + gv_weight * gv
    total.backward()
    return {"cost": np.array([trj.item(), msd.item(), gv.item()]), "c": cs, "grad_pred": p_.grad.numpy(),
            "grad_var": v_.grad.numpy(), "cond": np.concatenate(conds) if want_cond else None}


# ---- (b) banded, long double, analytic gradients ---------------------------------------------------------------------
def _band_mul(w, x, LD=LD):
    """(W_i x)[tau] = sum_j w[h + j] x[tau + j], columns outside [0, T) dropped.  x: [T][dim]."""
    T, h = x.shape[0], (len(w) - 1) // 2
    y = np.zeros_like(x)
    for k, wk in enumerate(w):
        j = k - h
        lo, hi = max(0, -j), min(T, T - j)
        if hi > lo:
            y[lo:hi] += LD(wk) * x[lo + j:hi + j]
    return y


def _gram_band(T, w, B, LD=LD):
    """G[k][t] = (W_i' W_i)[t][t + k], k = 0 .. B, in long double (zeros beyond the matrix)."""
    Wi = M.window_matrix(T, [w], 0).astype(LD)
    G = Wi.T @ Wi
    out = np.zeros((B + 1, T), dtype=LD)
    for k in range(min(B, T - 1) + 1):
        out[k, :T - k] = np.diagonal(G, k)
    return out


def banded(pred, obs, var, gv_var, streams, msd_weight=1.0, gv_weight=1.0e-6, LD=LD):
    """LD: the arithmetic throughout, np.longdouble for the reference; np.float32 shows what single precision inside
    would give (tests/test_gpu_trj.py, internal precision)."""
    streams = named(streams)
    lay, width = layout(streams)
    T = pred.shape[0]
    ld = lambda a: np.asarray(a, dtype=np.float32).astype(LD)
    pred_, obs_, var_, gvv = ld(pred), ld(obs), ld(var), ld(gv_var)
    D = sum(d for d, _, _ in streams)
    Mn = sum(1 for _, _, m in streams if m)
    nT, nG = LD(2 * D * T), LD(2 * D)
    grad_pred, grad_var = np.zeros((T, width), dtype=LD), np.zeros(width, dtype=LD)
    S_var = np.zeros(width, dtype=LD)
    logdet = mahal = gvm = LD(0)
    S_trj = LD(D * T) * LD(LN2PI)
    cs, at = [], 0
    for (mcol, c0, n), (dim, wins, _) in zip(lay, streams):
        nw = len(wins)
        B = 2 * max((len(w) - 1) // 2 for w in wins)
        p = 1 / var_[c0:c0 + n].reshape(nw, dim)                               # [nw][dim]
        mu = pred_[:, c0:c0 + n].reshape(T, nw, dim)
        G = [_gram_band(T, w, B, LD) for w in wins]
        A = sum(G[i][:, :, None] * p[i][None, None, :] for i in range(nw))      # [k][t][dim]
        r = np.zeros((T, dim), dtype=LD)
        for i, w in enumerate(wins):                                           # W_i' x = the band multiply by the reversed taps
            r += _band_mul(w[::-1], p[i][None, :] * mu[:, i], LD)
        # LDL': A = L diag(d) L', l[a][t] = L[t + a][t]
        d, l = np.zeros((T, dim), dtype=LD), np.zeros((B + 1, T, dim), dtype=LD)
        for t in range(T):
            for k in range(min(B, T - 1 - t) + 1):
                v = A[k, t].copy()
                for a in range(1, min(B - k, t) + 1):                          # pivot t - a reaches t and t + k
                    v -= l[a, t - a] * d[t - a] * l[a + k, t - a]
                if k == 0:
                    d[t] = v
                else:
                    l[k, t] = v / d[t]
        assert (d > 0).all() or LD is not np.longdouble
        z = r.copy()
        for t in range(T):
            for a in range(1, min(B, t) + 1):
                z[t] -= l[a, t - a] * z[t - a]

        def back(y):
            x = y / d
            for t in range(T - 1, -1, -1):
                for a in range(1, min(B, T - 1 - t) + 1):
                    x[t] -= l[a, t] * x[t + a]
            return x

        def forw(g):
            y = g.copy()
            for t in range(T):
                for a in range(1, min(B, t) + 1):
                    y[t] -= l[a, t - a] * y[t - a]
            return y

        c = back(z)
        # the band of Z = A^-1: Z[t][t + k] = [k == 0] / d_t - sum_a l[a][t] Z[t + a][t + k]
        Z = np.zeros((B + 1, T + B + 1, dim), dtype=LD)                        # Z[k][t] = Z[t][t + k], zeros beyond T
        for t in range(T - 1, -1, -1):
            for k in range(min(B, T - 1 - t), -1, -1):
                v = 1 / d[t] if k == 0 else np.zeros(dim, dtype=LD)
                for a in range(1, min(B, T - 1 - t) + 1):
                    v = v - l[a, t] * (Z[k - a, t + a] if k >= a else Z[a - k, t + k])
                Z[k, t] = v
        o = obs_[:, c0:c0 + dim]
        e = o - c
        cbar = c.mean(0)
        pv, ov = ((c - cbar) ** 2).mean(0), ((o - o.mean(0)) ** 2).mean(0)
        gsl = gvv[at:at + dim]
        g = LD(4) / T * (pv - ov) * (c - cbar) / gsl
        s = back(forw(g))
        logdet += np.log(d).sum()
        S_trj += np.abs(np.log(d).sum(0)).sum()
        gvm += ((pv - ov) ** 2 / gsl).sum()
        for i, w in enumerate(wins):
            ye, yc, ys = _band_mul(w, e, LD), _band_mul(w, c, LD), _band_mul(w, s, LD)
            res = mu[:, i] - yc
            mahal += (p[i] * (ye * ye).sum(0)).sum()
            cols = slice(c0 + i * dim, c0 + (i + 1) * dim)
            grad_pred[:, cols] = p[i] * (-2 * ye / nT + LD(gv_weight) * ys / nG)
            wgt = np.where(np.arange(B + 1) == 0, 1, 2).astype(LD)[:, None, None]
            trs = wgt * Z[:, :T] * G[i][:, :, None]
            dp_trj = -trs.sum((0, 1)) + (ye * ye).sum(0) - 2 * (ye * res).sum(0)
            dp_gv = (ys * res).sum(0)
            grad_var[cols] = -p[i] ** 2 * (dp_trj / nT + LD(gv_weight) * dp_gv / nG)
            S_var[cols] = p[i] ** 2 * ((np.abs(trs).sum((0, 1)) + (ye * ye).sum(0) + 2 * np.abs(ye * res).sum(0)) / nT
                                       + abs(LD(gv_weight)) * np.abs(ys * res).sum(0) / nG)
        cs.append(c)
        at += dim
    S_trj += mahal
    trj = (LD(D * T) * LD(LN2PI) - logdet + mahal) / nT
    gv = (LD(D) * LD(LN2PI) + np.log(gvv).sum() + gvm) / nG
    S_gv = (LD(D) * LD(LN2PI) + np.abs(np.log(gvv)).sum() + gvm) / nG
    msd = S_msd = LD(0)
    if Mn:
        nM = LD(2 * Mn * T)
        acc = LD(Mn * T) * LD(LN2PI)
        S_msd = acc
        for (mcol, _, _) in lay:
            if mcol is None:
                continue
            v = var_[mcol]
            df = pred_[:, mcol] - obs_[:, mcol]
            sq = (df * df).sum()
            acc += T * np.log(v) + sq / v
            S_msd += T * abs(np.log(v)) + sq / v
            grad_pred[:, mcol] = LD(msd_weight) * 2 * df / v / nM
            grad_var[mcol] = LD(msd_weight) * (T / v - sq / (v * v)) / nM
            S_var[mcol] = abs(LD(msd_weight)) * (T / v + sq / (v * v)) / nM
        msd, S_msd = acc / nM, S_msd / nM
    return {"cost": np.array([trj, msd, gv], dtype=LD), "S_cost": np.array([S_trj / nT, S_msd, S_gv], dtype=LD),
            "c": cs, "grad_pred": grad_pred, "grad_var": grad_var, "S_var": S_var}


# ---- cases ---------------------------------------------------------------------------------------------------------
def make_case(seed, lengths, streams):
    """Deterministic `ffo`-layout inputs of a batch: pred and var of mlpg_reference.make_stream per stream, obs = pred
    plus noise of 0.3, voicing columns (pred in (0, 1), obs 0 or 1), gv_var about the variance over the utterances of
    the observed per-utterance variances.  Returns float32 (pred [sum T][width], obs, var [width], gv_var [D])."""
    rng = np.random.default_rng(seed)
    st = named(streams)
    lay, width = layout(st)
    tf = int(sum(lengths))
    pred, var = np.zeros((tf, width), dtype=np.float32), np.zeros(width, dtype=np.float32)
    for k, ((mcol, c0, n), (dim, wins, _)) in enumerate(zip(lay, st)):
        pred[:, c0:c0 + n], var[c0:c0 + n] = M.make_stream(seed + 7 * (k + 1), list(lengths), dim, wins)
        if mcol is not None:
            pred[:, mcol] = rng.uniform(0.05, 0.95, tf)
            var[mcol] = 10.0 ** rng.uniform(-2.0, 0.0)
    obs = (pred + 0.3 * rng.standard_normal(pred.shape)).astype(np.float32)
    for mcol, _, _ in lay:
        if mcol is not None:
            obs[:, mcol] = (rng.uniform(0, 1, tf) < 0.6).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(lengths)])
    stat = np.concatenate([np.arange(c0, c0 + dim) for (_, c0, _), (dim, _, _) in zip(lay, st)])
    ov = np.stack([obs[off[u]:off[u + 1]][:, stat].astype(np.float64).var(axis=0) for u in range(len(lengths))])
    gv_var = (ov.var(axis=0) + 1e-4).astype(np.float32)
    return pred, obs, var, gv_var


def check_sens(a, b, streams):
    """sens = |a - b| of every quantity over its scale: the costs over S, an entry of grad_var over its S, c and
    grad_pred over the column's largest magnitude.  Returns ({name: sens array}, worst sens / scale)."""
    sens = {"cost": np.abs(a["cost"] - b["cost"]).astype(np.float64), "grad_var": np.abs(a["grad_var"] - b["grad_var"]).astype(np.float64),
            "grad_pred": np.abs(a["grad_pred"] - b["grad_pred"]).astype(np.float64),
            "c": [np.abs(x - y).astype(np.float64) for x, y in zip(a["c"], b["c"])]}
    worst = 0.0
    worst = max(worst, float((sens["cost"] / np.maximum(b["S_cost"].astype(np.float64), 1e-300)).max()))
    worst = max(worst, float((sens["grad_var"] / np.maximum(b["S_var"].astype(np.float64), 1e-300)).max()))
    gp = np.abs(b["grad_pred"]).max(axis=0).astype(np.float64)
    worst = max(worst, float((sens["grad_pred"].max(axis=0) / np.maximum(gp, 1e-300)).max()))
    for s_, cb in zip(sens["c"], b["c"]):
        worst = max(worst, float((s_.max(axis=0) / np.maximum(np.abs(cb).max(axis=0).astype(np.float64), 1e-300)).max()))
    return sens, worst


@functools.lru_cache(maxsize=None)
def cached_case(seed, lengths, streams, msd_weight=1.0, gv_weight=1.0e-6):
    """(pred, obs, var, gv_var, [per utterance (dense, banded, sens)]), computed once per process and read-only."""
    pred, obs, var, gv_var = make_case(seed, lengths, streams)
    off = np.concatenate([[0], np.cumsum(lengths)])
    refs = []
    for u in range(len(lengths)):
        a = dense(pred[off[u]:off[u + 1]], obs[off[u]:off[u + 1]], var, gv_var, streams, msd_weight, gv_weight)
        b = banded(pred[off[u]:off[u + 1]], obs[off[u]:off[u + 1]], var, gv_var, streams, msd_weight, gv_weight)
        sens, worst = check_sens(a, b, streams)
        refs.append((a, b, sens, worst))
    for arr in (pred, obs, var, gv_var):
        arr.setflags(write=False)
    return pred, obs, var, gv_var, refs


def column_cond(streams, cond):
    """cond per column of a row of width: a stream's column cond for each of its windows, 1 for a voicing column."""
    st = named(streams)
    lay, width = layout(st)
    out, at = np.ones(width), 0
    for (_, c0, n), (dim, wins, _) in zip(lay, st):
        out[c0:c0 + n] = np.tile(cond[at:at + dim], len(wins))
        at += dim
    return out


def bounds(a, b, sens, streams):
    """The issue's bounds for one utterance, in the quantities' own (normalised) units:
      cost, grad_var   max(10 sens, 64 2^-53 cond S)   (cond: the utterance's largest for a cost, the column's for an
                       entry of grad_var, 1 for the voicing term),
      c, grad_pred     mlpg_reference.bound: spacing(float32(max|x|)) + 64 cond 2^-53 max|x| per column."""
    eps = 64.0 * 2.0 ** -53
    cond = a["cond"]
    ccol = column_cond(streams, cond)
    S = b["S_cost"].astype(np.float64)
    cost = np.maximum(10.0 * sens["cost"], eps * np.array([cond.max(), 1.0, cond.max()]) * S)
    gvar = np.maximum(10.0 * sens["grad_var"], eps * ccol * b["S_var"].astype(np.float64))
    gpred = M.bound(b["grad_pred"].astype(np.float64), ccol)
    cs, at = [], 0
    for cb in b["c"]:
        cs.append(M.bound(cb.astype(np.float64), cond[at:at + cb.shape[1]]))
        at += cb.shape[1]
    return {"cost": cost, "grad_var": gvar, "grad_pred": gpred, "c": cs}

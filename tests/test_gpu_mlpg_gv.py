"""WorldBatch.parameter_generation_gv (mlpg_gv_kernel, csrc/mlpg_gv.hip) against the numpy statement of
tests/gv_reference.py, which starts from the library's own parameter_generation output as the definition says.

The bound on |out - reference| per column: spacing(float32(max|c|)) + max(10 sens, 64 ulp of max|c|), sens the
difference of the reference's float64 and long double evaluations (gv_reference.bound)."""
import numpy as np
import pytest

import gv_cases as K
import gv_reference as G
import mlpg_reference as M

pytestmark = pytest.mark.gpu

LENGTHS = K.LENGTHS
UNVOICED = -1e10
_cache = {}


def frames_batch(W, ctx, lengths):
    return W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=list(lengths))


def device_streams(torch, data, voiced, with_msd=True):
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    msd = dev(np.where(voiced, 0.9, 0.1).astype(np.float32))
    streams = [(dev(m), dev(v), M.WINDOW_SETS[name], msd if (has and with_msd) else None)
               for (m, v, _, _), (_, name, has) in zip(data, K.STREAMS)]
    return streams, [dev(g) for _, _, g, _ in data], [dev(g) for _, _, _, g in data]


def start_of(torch, W, ctx, lengths, data, voiced, var_per_frame, edge):
    """c0: the library's parameter_generation without the voicing overwrite, and with it (float32 numpy per stream)."""
    key = ("c0", lengths, var_per_frame, edge)
    if key not in _cache:
        b = frames_batch(W, ctx, lengths)
        plain, _, _ = device_streams(torch, data, voiced, with_msd=False)
        masked, _, _ = device_streams(torch, data, voiced)
        c0, st = b.parameter_generation(plain, var_per_frame=var_per_frame, edge=edge)
        c0m, _ = b.parameter_generation(masked, var_per_frame=var_per_frame, edge=edge, unvoiced_value=UNVOICED)
        assert (st.cpu().numpy() == 0).all()
        _cache[key] = ([o.cpu().numpy() for o in c0], [o.cpu().numpy() for o in c0m])
        b.close()
    return _cache[key]


def reference_of(lengths, data, voiced, c0s, masked, var_per_frame, edge, dtype, **options):
    key = ("ref", lengths, masked, var_per_frame, edge, dtype, tuple(sorted(options.items())))
    if key not in _cache:
        _cache[key] = K.reference(lengths, data, voiced, c0s, K.holes(lengths) if masked else None, edge, dtype, **options)
    return _cache[key]


def run(torch, W, ctx, lengths, data, voiced, masked, var_per_frame, edge, **options):
    b = frames_batch(W, ctx, lengths)
    streams, gm, gv = device_streams(torch, data, voiced)
    mask = torch.from_numpy(K.holes(lengths)).cuda() if masked else None
    outs, status, info = b.parameter_generation_gv(streams, gm, gv, gv_mask=mask, want_info=True, var_per_frame=var_per_frame,
                                                   edge=edge, unvoiced_value=UNVOICED, **options)
    res = [o.cpu().numpy() for o in outs], status.cpu().numpy(), info.cpu().numpy()
    b.close()
    return res


def compare(lengths, voiced, outs, status, c0s, r64, rld, what):
    """Every column of every utterance within the bound on its voiced frames, the rest exactly the unvoiced value,
    columns the reference returns as c0 bit for bit, the status word the reference's.  Returns the worst error / bound."""
    off = np.concatenate([[0], np.cumsum(lengths)])
    worst, want_status = 0.0, np.zeros(len(lengths), dtype=np.int64)
    for s, (dim, name, has_msd) in enumerate(K.STREAMS):
        v = voiced if has_msd else np.ones_like(voiced)
        got = outs[s]
        assert np.isfinite(got).all() and got.dtype == np.float32
        assert (got[~v] == np.float32(UNVOICED)).all()
        for u in range(len(lengths)):
            a, b = off[u], off[u + 1]
            st = r64[s]["status"][u]
            want_status[u] |= np.bitwise_or.reduce(st)
            rows = v[a:b]
            assert (got[a:b][rows][:, st != 0] == c0s[s][a:b][rows][:, st != 0]).all(), (what, name, u)
            if not rows.any():
                continue
            c64 = r64[s]["c"][a:b]
            sens = np.abs(c64 - rld[s]["c"][a:b].astype(np.float64)).max(axis=0)
            tol = G.bound(c64, sens)
            err = np.abs(got[a:b].astype(np.float64) - c64)[rows].max(axis=0)
            ratio = float((err / tol).max())
            worst = max(worst, ratio)
            assert (err <= tol).all(), (what, name, "T", lengths[u], ratio)
    assert (status == want_status).all(), (what, status, want_status)
    print("%s: worst error / bound %.3f" % (what, worst))
    return worst


@pytest.mark.parametrize("max_iter", [1, 5, 50])
@pytest.mark.parametrize("var_per_frame", [False, True], ids=["one_var_row", "var_per_frame"])
@pytest.mark.parametrize("edge", [0, 1])
def test_fixed_trial_counts(gpu, edge, var_per_frame, max_iter):
    """epsilon 0: every column runs max_iter trials; a gv_mask with holes."""
    torch, W, ctx = gpu
    data, voiced = K.inputs(LENGTHS, var_per_frame)
    c0s, _ = start_of(torch, W, ctx, LENGTHS, data, voiced, var_per_frame, edge)
    opts = dict(max_iter=max_iter, epsilon=0.0)
    outs, status, info = run(torch, W, ctx, LENGTHS, data, voiced, True, var_per_frame, edge, **opts)
    r64 = reference_of(LENGTHS, data, voiced, c0s, True, var_per_frame, edge, np.float64, **opts)
    rld = reference_of(LENGTHS, data, voiced, c0s, True, var_per_frame, edge, np.longdouble, **opts)
    compare(LENGTHS, voiced, outs, status, c0s, r64, rld, "edge %d var_per_frame %d max_iter %d" % (edge, var_per_frame, max_iter))
    at = 0
    for s, (dim, _, _) in enumerate(K.STREAMS):
        live = r64[s]["status"] == 0
        assert (info[:, at:at + dim, 2][live] == max_iter).all()
        assert (info[:, at:at + dim, 2][~live] == 0).all()
        at += dim


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_stop_rule(gpu, masked):
    """epsilon 1e-4: the trial and accept counts are the reference's, on every column but those where the reference's
    own decisions hang on the last bits (at most 5 % of the columns)."""
    torch, W, ctx = gpu
    eps = 1e-4
    data, voiced = K.inputs(LENGTHS, False)
    c0s, _ = start_of(torch, W, ctx, LENGTHS, data, voiced, False, 0)
    outs, status, info = run(torch, W, ctx, LENGTHS, data, voiced, masked, False, 0, epsilon=eps)
    r64 = reference_of(LENGTHS, data, voiced, c0s, masked, False, 0, np.float64, epsilon=eps)
    at, n_live, n_out = 0, 0, 0
    for s, (dim, _, _) in enumerate(K.STREAMS):
        for u in range(len(LENGTHS)):
            for j in range(dim):
                if r64[s]["status"][u][j] != 0:
                    assert info[u, at + j, 2] == 0 and info[u, at + j, 3] == 0
                    continue
                n_live += 1
                near = any(abs(g - eps) <= 1e-6 * eps for g in r64[s]["gains"][u][j])
                thin = any(mg < 1e-10 for mg in r64[s]["margins"][u][j])
                if near or thin:
                    n_out += 1
                    continue
                assert info[u, at + j, 2] == r64[s]["trials"][u][j], (s, u, j)
                assert info[u, at + j, 3] == r64[s]["accepts"][u][j], (s, u, j)
                assert info[u, at + j, 1] >= info[u, at + j, 0]
        at += dim
    print("stop rule: %d of %d columns excluded" % (n_out, n_live))
    assert n_live > 300 and n_out <= 0.05 * n_live


def test_status_and_neighbours(gpu):
    """T = 1 and the column with one voiced frame come back as parameter_generation's with 4; a non-positive gv_var
    gives 1 and that column alone is parameter_generation's; a column that parameter_generation flags stays zeros;
    every other utterance and column keeps its bits."""
    torch, W, ctx = gpu
    data, voiced = K.inputs(LENGTHS, True)
    _, c0m = start_of(torch, W, ctx, LENGTHS, data, voiced, True, 0)
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    base, st0, _ = run(torch, W, ctx, LENGTHS, data, voiced, False, True, 0, max_iter=5, epsilon=0.0)
    assert (st0 == np.array([4, 0, 0, 4, 0, 0, 0])).all(), st0
    for s in range(3):
        assert (base[s][0:1] == c0m[s][0:1]).all()                      # T = 1: every stream
    assert (base[1][off[3]:off[4]] == c0m[1][off[3]:off[4]]).all()      # one voiced frame: the voiced stream alone
    assert (base[0][off[3]:off[4]] != c0m[0][off[3]:off[4]]).any()
    assert (base[0][off[5]:off[6]] != c0m[0][off[5]:off[6]]).any()      # and the loop does move the others

    b = frames_batch(W, ctx, LENGTHS)
    streams, gm, gv = device_streams(torch, data, voiced)
    gv[0] = gv[0].clone()
    gv[0][2] = 0.0
    var0 = streams[0][1].clone()
    var0[off[5] + 9, 4] = -1.0                                          # utterance 5 (T = 200), stream 0, column 4
    streams[0] = (streams[0][0], var0, streams[0][2], streams[0][3])
    outs, status = b.parameter_generation_gv(streams, gm, gv, var_per_frame=True, unvoiced_value=UNVOICED, max_iter=5, epsilon=0.0)
    outs, status = [o.cpu().numpy() for o in outs], status.cpu().numpy()
    b.close()
    assert (status == np.array([4 | 1, 1, 1, 4 | 1, 1, 1, 1])).all(), status
    assert (outs[0][:, 2] == c0m[0][:, 2]).all()
    assert (outs[0][off[5]:off[6], 4] == 0).all()
    keep = np.ones(outs[0].shape, dtype=bool)
    keep[:, 2] = False
    keep[off[5]:off[6], 4] = False
    assert (outs[0][keep] == base[0][keep]).all()
    assert (outs[1] == base[1]).all() and (outs[2] == base[2]).all()


def test_no_trials_without_scaling_is_parameter_generation(gpu):
    torch, W, ctx = gpu
    data, voiced = K.inputs(LENGTHS, False)
    _, c0m = start_of(torch, W, ctx, LENGTHS, data, voiced, False, 1)
    outs, status, _ = run(torch, W, ctx, LENGTHS, data, voiced, True, False, 1, max_iter=0, scale=0)
    for o, c in zip(outs, c0m):
        assert o.tobytes() == c.tobytes()


def test_an_utterance_does_not_see_its_batch(gpu):
    """T = 200 alone, in two other batches, and beside utterances of 2048 and 2049 frames -- the last whose state fits
    LDS and the first whose state does not, which also changes the workspace layout of the whole batch: the same bits.
    The two long utterances themselves are held to the reference."""
    torch, W, ctx = gpu
    got = []
    batches = ((200,), (33, 200), (7, 200, 1000, 3), (200, 2048, 2049))
    for lengths in batches:
        data, voiced = K.inputs((200,), False)
        rest = [K.inputs((T,), False, seed=90 + T) for T in lengths if T != 200]
        order, k = [], 0
        for T in lengths:
            if T == 200:
                order.append((data, voiced))
            else:
                order.append(rest[k])
                k += 1
        joined = [tuple(np.concatenate([o[0][s][i] for o in order]) if i == 0 else data[s][i] for i in range(4))
                  for s in range(3)]
        v = np.concatenate([o[1] for o in order])
        outs, status, _ = run(torch, W, ctx, lengths, joined, v, False, False, 0)
        a = int(sum(lengths[:lengths.index(200)]))
        got.append([o[a:a + 200].tobytes() for o in outs])
        if 2049 in lengths:
            c0s, _ = start_of(torch, W, ctx, lengths, tuple(joined), v, False, 0)
            opts = dict(max_iter=5, epsilon=0.0)
            outs, status, _ = run(torch, W, ctx, lengths, joined, v, False, False, 0, **opts)
            r64 = K.reference(lengths, joined, v, c0s, None, 0, np.float64, **opts)
            rld = K.reference(lengths, joined, v, c0s, None, 0, np.longdouble, **opts)
            compare(lengths, v, outs, status, c0s, r64, rld, "T = 2048 and 2049, state in LDS and in the workspace")
    assert all(g == got[0] for g in got[1:])


def test_effect_on_the_variance(gpu):
    """Trajectories whose variance is about a third of the GV mean come out with v / gv_mean in [0.7, 1.3]."""
    torch, W, ctx = gpu
    lengths, dim = (33, 200, 1000), 5
    mean, var, gm, gvar = effect_inputs(lengths, dim)
    b = frames_batch(W, ctx, lengths)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    streams = [(dev(mean), dev(var), M.RECIPE, None)]
    c0, _ = b.parameter_generation(streams)
    outs, status = b.parameter_generation_gv(streams, [dev(gm)], [dev(gvar)])
    assert (status.cpu().numpy() == 0).all()
    off = np.concatenate([[0], np.cumsum(lengths)])
    for u in range(len(lengths)):
        rows = slice(off[u], off[u + 1])
        before = G.variance_over(c0[0].cpu().numpy()[rows], np.ones(lengths[u], bool)) / gm
        after = G.variance_over(outs[0].cpu().numpy()[rows], np.ones(lengths[u], bool)) / gm
        print("T %d: v / gv_mean before %s after %s" % (lengths[u], np.round(before, 3), np.round(after, 3)))
        assert (before > 0.15).all() and (before < 0.5).all()      # about a third: the reference's own run gave 0.19 .. 0.33
        assert (after >= 0.7).all() and (after <= 1.3).all()
    b.close()


def effect_inputs(lengths, dim):
    """Means whose static track has unit variance in every utterance and column, moderate variances, and a GV
    mean of three times the variance the plain solve leaves (about 0.95) with a standard deviation of a tenth of it."""
    rng = np.random.default_rng(77)
    rows = []
    for T in lengths:
        x = M.random_walk(rng, T, dim).astype(np.float64)
        x = (x - x.mean(axis=0)) / x.std(axis=0)
        rows.append(M.compose(x.astype(np.float32), M.RECIPE, 1))
    mean = np.concatenate(rows)
    var = np.repeat(np.array([0.5, 0.05, 0.05], dtype=np.float32), dim)
    gm = np.full(dim, 3.0, dtype=np.float32)
    gvar = np.full(dim, 0.09, dtype=np.float32)
    return mean, var, gm, gvar


@pytest.mark.parametrize("bad", [dict(max_iter=-1), dict(epsilon=-1.0), dict(step_init=0.0), dict(step_inc=float("inf")),
                                 dict(step_dec=-0.5), dict(hmm_weight=0.0), dict(gv_weight=-1.0), dict(epsilon=float("nan"))],
                         ids=lambda d: "%s_%s" % next(iter(d.items())))
def test_options_out_of_range_are_refused(gpu, bad):
    """With a live batch, so that the refusal is the option's and not the NULL batch's."""
    torch, W, ctx = gpu
    b = frames_batch(W, ctx, (5,))
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    mean, var = M.make_stream(1, [5], 2, M.RECIPE)
    with pytest.raises(Exception, match="ParameterGenerationGv"):
        b.parameter_generation_gv([(dev(mean), dev(var), M.RECIPE, None)], [dev(np.ones(2, np.float32))],
                                  [dev(np.ones(2, np.float32))], **bad)
    b.close()

"""WorldBatch.parameter_generation (mlpg_kernel, csrc/mlpg.hip) against the dense float64 statement of
tests/mlpg_reference.py on the same float32 inputs -- never against another run of the library, except where a test is
about two runs agreeing (the voicing mask, untouched neighbours of a flagged column).

The bound on |out - c| per column (mlpg_reference.bound): spacing(float32(max|c|)) + 64 cond(R) 2^-53 max|c|, the
rounding of the float32 output plus a banded factorisation's error in double."""
import ctypes as C

import numpy as np
import pytest

import mlpg_reference as ref

pytestmark = pytest.mark.gpu

# shorter than a window's reach, shorter than the band, either side of a wave of frames, and long
LENGTHS = (1, 2, 3, 5, 63, 64, 65, 257)
# (dim, window set): every band instantiation (0, 2, 4, 14), one and two 64-lane chunks, a narrow stream
CALL_A = ((64, "static"), (50, "recipe"), (1, "zero_ends"), (65, "ramp15"))
CALL_B = ((25, "five"), (1, "recipe"))


def frames_batch(W, ctx, lengths):
    return W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=list(lengths))


def check(got, want, cond, lengths, what):
    """|got - want| within the bound, every column of every utterance; prints the worst error / bound."""
    tol = ref.batch_bound(list(lengths), want, cond)
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / tol).max())
    print("%s: max err %.3e, worst err / bound %.3f, largest cond %.3g" % (what, err.max(), ratio, cond.max()))
    assert np.isfinite(got).all(), what
    assert (err <= tol).all(), (what, ratio)
    return ratio


def case(call, var_per_frame, edge, input_type=0, seed=11):
    return [ref.cached_reference(seed + 7 * s, LENGTHS, dim, name, var_per_frame, edge, input_type)
            for s, (dim, name) in enumerate(call)]


@pytest.mark.parametrize("call", [CALL_A, CALL_B], ids=["four_streams", "two_streams"])
@pytest.mark.parametrize("var_per_frame", [False, True], ids=["one_var_row", "var_per_frame"])
@pytest.mark.parametrize("edge", [0, 1])
def test_against_dense_reference(gpu, call, var_per_frame, edge):
    torch, W, ctx = gpu
    data = case(call, var_per_frame, edge)
    b = frames_batch(W, ctx, LENGTHS)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    streams = [(dev(m), dev(v), ref.WINDOW_SETS[name], None) for (m, v, _, _), (_, name) in zip(data, call)]
    outs, status = b.parameter_generation(streams, var_per_frame=var_per_frame, edge=edge)
    assert (status.cpu().numpy() == 0).all()
    for o, (m, _, c, cond), (dim, name) in zip(outs, data, call):
        assert tuple(o.shape) == (sum(LENGTHS), dim) and o.dtype == torch.float32
        check(o.cpu().numpy(), c, cond, LENGTHS, "%s dim %d edge %d var_per_frame %d" % (name, dim, edge, var_per_frame))
    b.close()


@pytest.mark.parametrize("var_per_frame", [False, True], ids=["one_var_row", "var_per_frame"])
def test_precisions_as_input(gpu, var_per_frame):
    """input_type 1 with the exact float32 reciprocals of the variances: held to the helper fed those precisions."""
    torch, W, ctx = gpu
    data = case(CALL_B, var_per_frame, 0, input_type=1)
    b = frames_batch(W, ctx, LENGTHS)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    streams = [(dev(m), dev(p), ref.WINDOW_SETS[name], None) for (m, p, _, _), (_, name) in zip(data, CALL_B)]
    outs, status = b.parameter_generation(streams, var_per_frame=var_per_frame, input_type=1)
    assert (status.cpu().numpy() == 0).all()
    for o, (_, _, c, cond), (dim, name) in zip(outs, data, CALL_B):
        check(o.cpu().numpy(), c, cond, LENGTHS, "precisions, %s dim %d" % (name, dim))
    b.close()


def test_streams_as_columns_of_one_matrix(gpu):
    """Pointer plus one row stride: the `ffo` layout, a voicing column between the streams, nothing copied."""
    torch, W, ctx = gpu
    data = case(CALL_B, True, 0)
    (m0, v0, c0, k0), (m1, v1, c1, k1) = data
    tf = sum(LENGTHS)
    voiced = (np.arange(tf) % 3 != 0)
    msd = np.where(voiced, 0.9, 0.1).astype(np.float32)
    pad = np.full((tf, 2), np.nan, dtype=np.float32)              # columns no stream owns are never read
    rows = torch.from_numpy(np.concatenate([m0, msd[:, None], pad, m1], axis=1)).cuda()
    vrow = torch.from_numpy(np.concatenate([pad, v0, pad[:, :1], v1], axis=1)).cuda()
    n0, n1 = m0.shape[1], m1.shape[1]
    streams = [(rows[:, :n0], vrow[:, 2:2 + n0], ref.FIVE, None),
               (rows[:, n0 + 3:], vrow[:, 3 + n0:], ref.RECIPE, rows[:, n0])]
    assert not streams[0][0].is_contiguous()
    b = frames_batch(W, ctx, LENGTHS)
    outs, status = b.parameter_generation(streams, var_per_frame=True, unvoiced_value=0.0)
    assert (status.cpu().numpy() == 0).all()
    check(outs[0].cpu().numpy(), c0, k0, LENGTHS, "column views, five")
    lf0 = outs[1].cpu().numpy()
    assert (lf0[~voiced] == 0).all()
    check(np.where(voiced[:, None], lf0, c1.astype(np.float32)), c1, k1, LENGTHS, "column views, recipe with voicing")
    b.close()


@pytest.mark.parametrize("edge,dvar", [(1, 1e-6), (0, 1e-8)])
def test_internal_precision(gpu, edge, dvar):
    """T = 129, the recipe's windows, static variance 1 and delta variances 1e-6 (edge 1; cond 1.6e7) or 1e-8 (edge 0):
    float32 arithmetic inside the solve misses the bound by 5000x and 120x, float64 keeps it."""
    torch, W, ctx = gpu
    T, dim = 129, 3
    mean, _ = ref.make_stream(5, [T], dim, ref.RECIPE)
    var = np.repeat(np.array([1.0, dvar, dvar], dtype=np.float32), dim)
    c, cond = ref.mlpg(mean, var, ref.RECIPE, edge)
    b = frames_batch(W, ctx, [T])
    outs, status = b.parameter_generation([(torch.from_numpy(mean).cuda(), torch.from_numpy(var).cuda(), ref.RECIPE, None)],
                                          edge=edge)
    assert int(status[0]) == 0
    check(outs[0].cpu().numpy(), c, cond[None], [T], "static var 1, delta var %g, edge %d" % (dvar, edge))
    b.close()


@pytest.mark.parametrize("name", ["recipe", "ramp15"])
def test_round_trip_from_compose_cmp(gpu, name):
    """compose_cmp(x) -> parameter_generation(edge=1) returns x at any positive variances; the bound is the helper's
    own round-trip error on the same rows plus one float32 spacing."""
    torch, W, ctx = gpu
    wins, dim = ref.WINDOW_SETS[name], 50
    rng = np.random.default_rng(3)
    x = np.concatenate([ref.random_walk(rng, T, dim, scale=4.0) for T in LENGTHS])
    var = (10.0 ** rng.uniform(-3, 3, len(wins) * dim)).astype(np.float32)
    b = frames_batch(W, ctx, LENGTHS)
    cmp_ = b.compose_cmp([(torch.from_numpy(x).cuda(), wins)])
    outs, status = b.parameter_generation([(cmp_, torch.from_numpy(var).cuda(), wins, None)], edge=1)
    assert (status.cpu().numpy() == 0).all()
    got, rows = outs[0].cpu().numpy().astype(np.float64), cmp_.cpu().numpy()
    worst = 0.0
    for a, e in zip(b.frame_offsets[:-1], b.frame_offsets[1:]):
        helper, _ = ref.mlpg(rows[a:e], var, wins, edge=1, want_cond=False)
        xs = x[a:e].astype(np.float64)
        tol = np.abs(helper - xs).max(axis=0) + np.spacing(np.abs(x[a:e]).max(axis=0)).astype(np.float64)
        err = np.abs(got[a:e] - xs).max(axis=0)
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (name, int(e - a), float((err / tol).max()))
    print("%s: round trip, worst err / (helper's error + one spacing) %.3f" % (name, worst))
    b.close()


@pytest.mark.parametrize("unvoiced_value", [-1e10, 0.0])
def test_voicing_mask(gpu, unvoiced_value):
    """Voiced is value >= 0.5 (0, 0.49 unvoiced; 0.5, 1 voiced), flipping per frame, one utterance all unvoiced: the
    solve runs over every frame whatever the voicing, unvoiced frames then hold unvoiced_value in every dim."""
    torch, W, ctx = gpu
    lengths, dim = (9, 6, 33), 2
    mean, var = ref.make_stream(21, lengths, dim, ref.RECIPE)
    c, cond = ref.mlpg_batch(list(lengths), mean, var, ref.RECIPE)
    tf = sum(lengths)
    msd = np.array([0.0, 0.49, 0.5, 1.0], dtype=np.float32)[(np.arange(tf) * 7 + np.arange(tf) // 4) % 4]
    msd[9:15] = np.array([0.0, 0.49] * 3, dtype=np.float32)                       # utterance 1: all unvoiced
    voiced = msd >= np.float32(0.5)
    assert voiced[:9].any() and (~voiced[:9]).any() and not voiced[9:15].any()
    b = frames_batch(W, ctx, lengths)
    dev = lambda a: torch.from_numpy(a).cuda()
    plain, _ = b.parameter_generation([(dev(mean), dev(var), ref.RECIPE, None)])
    outs, status = b.parameter_generation([(dev(mean), dev(var), ref.RECIPE, dev(msd))], unvoiced_value=unvoiced_value)
    assert (status.cpu().numpy() == 0).all()
    got, plain = outs[0].cpu().numpy(), plain[0].cpu().numpy()
    assert (got[~voiced] == np.float32(unvoiced_value)).all()
    np.testing.assert_array_equal(got[voiced], plain[voiced])                     # voiced frames equal the unmasked solve
    check(plain, c, cond, lengths, "unmasked")
    check(np.where(voiced[:, None], got, c.astype(np.float32)), c, cond, lengths, "voiced frames")
    b.close()


def test_status_and_untouched_neighbours(gpu):
    """Bit 1: a NaN mean, a variance of 0.  Bit 2: a stream without a static window at T = 3 (unit variances: the
    zero pivot is exact).  Flagged columns are zeros, every other column of the batch is bit-identical to the call
    without the bad utterances."""
    torch, W, ctx = gpu
    lengths, dim = (4, 3, 6, 2, 8), 3
    off = np.concatenate([[0], np.cumsum(lengths)])
    mean, var = ref.make_stream(31, lengths, dim, ref.RECIPE, var_per_frame=True)
    mean, var = mean.copy(), var.copy()
    mean[off[2] + 4, dim + 1] = np.nan                    # utterance 2: delta mean of dim 1
    var[off[3] + 1, 2] = 0.0                              # utterance 3: static variance of dim 2
    delta = [[-0.5, 0.0, 0.5]]                            # no static window: W' P W is singular at odd T
    dmean, _ = ref.make_stream(32, lengths, 2, delta, var_per_frame=True)
    dvar = np.ones_like(dmean)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    b = frames_batch(W, ctx, lengths)
    (o, od), status = b.parameter_generation([(dev(mean), dev(var), ref.RECIPE, None), (dev(dmean), dev(dvar), delta, None)],
                                             var_per_frame=True)
    assert status.cpu().numpy().tolist() == [0, 2, 1, 1, 0]
    o, od = o.cpu().numpy(), od.cpu().numpy()
    seg = lambda a, u: a[off[u]:off[u + 1]]
    assert (seg(od, 1) == 0).all() and (seg(o, 2)[:, 1] == 0).all() and (seg(o, 3)[:, 2] == 0).all()
    # the flagged utterances' other columns, and the no-static stream at even T, against the helper
    for u, cols in ((1, [0, 1, 2]), (2, [0, 2]), (3, [0, 1])):
        c, cond = ref.mlpg(np.nan_to_num(seg(mean, u)), np.where(seg(var, u) > 0, seg(var, u), 1), ref.RECIPE)
        check(seg(o, u)[:, cols], c[:, cols], cond[cols][None], [lengths[u]], "utterance %d, unflagged columns" % u)
    for u in (0, 2, 3, 4):
        c, cond = ref.mlpg(seg(dmean, u), seg(dvar, u), delta)
        check(seg(od, u), c, cond[None], [lengths[u]], "delta window alone, T %d" % lengths[u])
    b.close()
    good = [0, 4]
    keep = np.concatenate([np.arange(off[u], off[u + 1]) for u in good])
    b = frames_batch(W, ctx, [lengths[u] for u in good])
    (o2, od2), status = b.parameter_generation([(dev(mean[keep]), dev(var[keep]), ref.RECIPE, None),
                                                (dev(dmean[keep]), dev(dvar[keep]), delta, None)], var_per_frame=True)
    assert status.cpu().numpy().tolist() == [0, 0]
    np.testing.assert_array_equal(o[keep].view(np.uint32), o2.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(od[keep].view(np.uint32), od2.cpu().numpy().view(np.uint32))
    b.close()


def test_status_of_precisions(gpu):
    """input_type 1: a negative precision sets bit 1 and zeroes its column; precision 0, an ignored observation, is
    allowed and agrees with the helper."""
    torch, W, ctx = gpu
    lengths, dim = (7, 5), 3
    mean, var = ref.make_stream(41, lengths, dim, ref.RECIPE, var_per_frame=True)
    prec = (np.float32(1.0) / var).astype(np.float32)
    prec[2, dim:2 * dim] = 0.0                            # utterance 0: the delta of frame 2 is ignored
    prec[3, 2 * dim] = 0.0
    bad = prec.copy()
    bad[7 + 2, 1] = -1.0                                  # utterance 1: a static precision of dim 1
    dev = lambda a: torch.from_numpy(a).cuda()
    b = frames_batch(W, ctx, lengths)
    (o,), status = b.parameter_generation([(dev(mean), dev(bad), ref.RECIPE, None)], var_per_frame=True, input_type=1)
    assert status.cpu().numpy().tolist() == [0, 1]
    o = o.cpu().numpy()
    assert (o[7:, 1] == 0).all()
    c, cond = ref.mlpg_batch(list(lengths), mean, prec, ref.RECIPE, input_type=1, var_per_frame=True)
    o[7:, 1] = c[7:, 1]
    check(o, c, cond, lengths, "precisions with zeros")
    b.close()


def test_limits_are_bad_arguments(gpu):
    torch, W, ctx = gpu
    b = frames_batch(W, ctx, [4])
    z = lambda n: torch.zeros(4, n, dtype=torch.float32, device="cuda")
    one = lambda n: torch.ones(n, dtype=torch.float32, device="cuda")
    ok = (z(3), one(3), ref.RECIPE, None)
    outs, status = b.parameter_generation([ok] * 4)
    assert len(outs) == 4 and int(status[0]) == 0
    for streams, opt in (([ok] * 5, {}),                                         # streams
                         ([(z(5), one(5), [[1.0]] * 5, None)], {}),              # windows
                         ([(z(2), one(2), [[1.0], [0.5, 0.5]], None)], {}),      # an even size
                         ([(z(2), one(2), [[1.0], [0.0] * 17], None)], {}),      # beyond 15 taps
                         ([ok], {"edge": 2}), ([ok], {"edge": -1}), ([ok], {"input_type": 2})):
        with pytest.raises(RuntimeError, match="bad argument"):
            b.parameter_generation(streams, **opt)
    # a row stride smaller than the stream's row, and a null stream pointer: the C call itself
    lib = W.load_library()
    o = W.MlpgOption()
    lib.WorldMi355DefaultMlpgOption(C.byref(o))
    mean, var, out = z(3), one(3), z(1)
    dp = C.POINTER(C.c_double)
    taps = [(C.c_double * len(w))(*w) for w in ref.RECIPE]
    wp = (dp * 3)(*[C.cast(a, dp) for a in taps])
    wpp = (C.POINTER(dp) * 1)(C.cast(wp, C.POINTER(dp)))
    sz = (C.c_int * 3)(1, 3, 3)
    szp = (C.POINTER(C.c_int) * 1)(C.cast(sz, C.POINTER(C.c_int)))
    one_ptr = lambda t: (C.c_void_p * 1)(C.c_void_p(t.data_ptr() if t is not None else None))
    call = lambda m, ld: lib.WorldMi355ParameterGeneration(b.handle, 1, one_ptr(m), ld, one_ptr(var), 0, (C.c_int * 1)(1),
                                                           (C.c_int * 1)(3), wpp, szp, None, C.byref(o), one_ptr(out), None)
    assert call(mean, 3) == 0
    assert call(mean, 2) == 2
    assert call(None, 3) == 2
    ctx.synchronize()
    b.close()


def test_timing_name(gpu):
    torch, W, ctx = gpu
    b = frames_batch(W, ctx, [5, 9])
    ctx.timing_enable(True)
    try:
        assert ctx.timing_query("mlpg_kernel")[1] == 0
        z = torch.zeros(14, 6, dtype=torch.float32, device="cuda")
        b.parameter_generation([(z, torch.ones(6, dtype=torch.float32, device="cuda"), ref.RECIPE, None)] * 2)
        assert ctx.timing_query("mlpg_kernel")[1] == 1
    finally:
        ctx.timing_enable(False)
    b.close()


def test_chain_to_synthesis(gpu, pkg):
    """RecipeFeatures -> ComposeCmp -> ParameterGeneration(edge 1, unvoiced 0) -> RecipeDecode -> Synthesis equals
    synthesis from the decoded original features.  The bound is what the helper's own round-trip error produces when
    the chain is run from the helper's output, plus 10 %: the kernel may sum in another order."""
    torch, W, ctx = gpu
    fs = 16000
    x = pkg.synth_data.make_utterance(31, fs, duration=0.5)
    b = W.WorldBatch(ctx, W.default_params(fs, 5.0), x_lengths=[len(x)])
    _, f0, sp, ap = b.analyze(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    lf0, mgc, bap = b.recipe_features(f0, sp, ap, 50, 25)
    assert int((lf0 != 0).sum()) > 10 and int((lf0 == 0).sum()) > 0
    feats = [lf0.reshape(-1, 1), mgc, bap]
    rows = b.compose_cmp([(f, ref.RECIPE) for f in feats])
    voiced = (lf0 != 0).float()
    at, streams = 0, []
    rng = np.random.default_rng(9)
    for k, f in enumerate(feats):
        n = 3 * f.shape[1]
        var = torch.from_numpy((10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)).cuda()
        streams.append((rows[:, at:at + n], var, ref.RECIPE, voiced if k == 0 else None))
        at += n
    outs, status = b.parameter_generation(streams, edge=1, unvoiced_value=0.0)
    assert int(status[0]) == 0
    synth = lambda l, m, a: b.synthesize(*b.recipe_decode(l.contiguous(), m.contiguous(), a.contiguous())).cpu().numpy()
    y0 = synth(lf0, mgc, bap)
    yg = synth(outs[0].reshape(-1), outs[1], outs[2])
    helper = []
    for (m, v, w, _), f in zip(streams, feats):
        c, _ = ref.mlpg(m.cpu().numpy(), v.cpu().numpy(), w, edge=1, want_cond=False)
        helper.append(torch.from_numpy(c.astype(np.float32)).cuda())
    helper[0] = helper[0] * voiced[:, None]
    yh = synth(helper[0].reshape(-1), helper[1], helper[2])
    eg, eh = float(np.abs(yg - y0).max()), float(np.abs(yh - y0).max())
    print("chain: max|y - y0| from the kernel %.3e, from the helper %.3e, peak |y0| %.3f" % (eg, eh, np.abs(y0).max()))
    assert eg <= 1.1 * eh
    b.close()

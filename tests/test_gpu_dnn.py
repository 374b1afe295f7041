"""WorldBatch.acoustic_model_forward (dnn_layer_kernel / dnn_cost_kernel, csrc/dnn.hip) against tests/dnn_reference.py,
the float64 statement of DNNDefine.inference and DNNDefine.cost, on the same float32 inputs -- never against another run
of the library, except where a test is about two runs agreeing bit for bit.

Shapes: one batch of utterances of 1, 2, 31, 32, 33, 127, 128, 129 and 257 frames (either side of a 32-row MFMA tile and
of a 128-row block tile; utterance boundaries fall inside tiles) through the nets of dnn_reference.NETS, each in SD mode,
in SAT mode with per-utterance speakers and in SAT mode with the NULL default.

Bounds: the exact test asks bit-for-bit equality on small integers (it is the one that catches a swapped row and column,
a missed tail, a wrong k pairing or a padding leak); the bound test asks |out - ref| <= e, dnn_reference's running bound
of a float32 fma-chain evaluation (nothing in it is measured); the cost is held to 64 * 2^-53 * S of the float64 sum
over the RETURNED out, S the sum of the magnitudes of the terms added."""
import ctypes as C

import numpy as np
import pytest

import dnn_reference as R
import mlpg_reference as M

pytestmark = pytest.mark.gpu


def frames_batch(W, ctx, lengths):
    return W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=list(lengths))


def model_dict(torch, params, hidden, output, sat=None):
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    n = R.n_layers(params)
    names = ["hidden%d" % i for i in range(n)] + ["output"]
    n_spkrs = params["variance.variances"].shape[0]
    sat = n_spkrs > 1 if sat is None else sat
    return {"weights": [dev(params[k + ".si_weights"]) for k in names], "biases": [dev(params[k + ".si_biases"]) for k in names],
            "spkr_weights": [dev(params["hidden%d.sd_weights" % i]) for i in range(n)] if sat else None,
            "variances": dev(params["variance.variances"]), "n_spkrs": n_spkrs,
            "hidden_activation": hidden, "output_activation": output}


def run(gpu, lengths, params, x, spkr, hidden, output, obs=None, max_chunk_frames=0, x_dev=None):
    torch, W, ctx = gpu
    b = frames_batch(W, ctx, lengths)
    xd = x_dev if x_dev is not None else torch.from_numpy(np.array(x)).cuda()
    od = None if obs is None else torch.from_numpy(np.array(obs)).cuda()
    out, cost, status = b.acoustic_model_forward(model_dict(torch, params, hidden, output), xd, spkr, od, max_chunk_frames)
    res = out.cpu().numpy(), None if cost is None else cost.cpu().numpy(), status.cpu().numpy()
    b.close()
    return res


@pytest.mark.parametrize("net", range(len(R.NETS)), ids=["37-48-130-229", "1-1-1", "3-33", "65-129-31", "700-229"])
def test_exact_on_small_integers(gpu, net):
    """Bit for bit the float64 reference, linear and ReLU hidden units, SD / SAT / SAT with the default speaker."""
    for mode in R.MODES:
        for hidden in ("linear", "relu"):
            params, x, spkr, ref = R.exact_case(net, mode, hidden)
            out, _, status = run(gpu, R.LENGTHS, params, x, spkr, hidden, "linear")
            assert out.dtype == np.float32 and out.shape == ref.shape
            assert (status == 0).all()
            wrong = np.argwhere(out.astype(np.float64) != ref)
            assert wrong.size == 0, (mode, hidden, len(wrong), wrong[:5].tolist())


@pytest.mark.parametrize("net", range(len(R.NETS)), ids=["37-48-130-229", "1-1-1", "3-33", "65-129-31", "700-229"])
def test_within_the_forward_error_bound(gpu, net):
    """Every hidden activation, linear and sigmoid outputs, the three modes: |out - ref| <= e per element."""
    worst = 0.0
    for n, mode, hidden, output in R.all_cases():
        if n != net:
            continue
        params, x, spkr, ref, e = R.cached_case(net, mode, hidden, output)
        out, _, status = run(gpu, R.LENGTHS, params, x, spkr, hidden, output)
        assert (status == 0).all() and np.isfinite(out).all()
        ratio = float((np.abs(out.astype(np.float64) - ref) / e).max())
        print("net %d %s %s/%s: worst error / bound %.4f" % (net, mode, hidden, output, ratio))
        assert ratio <= 1.0, (mode, hidden, output, ratio)
        worst = max(worst, ratio)
    print("net %d: worst error / bound %.4f" % (net, worst))


def test_chunks_do_not_change_a_bit(gpu):
    """max_chunk_frames 64 and 1 against the default call, on the SAT case of 37 -> 48, 130 -> 229."""
    params, x, spkr, _, _ = R.cached_case(0, "sat", "sigmoid", "linear")
    whole, _, _ = run(gpu, R.LENGTHS, params, x, spkr, "sigmoid", "linear")
    for chunk in (64, 1):
        part, _, status = run(gpu, R.LENGTHS, params, x, spkr, "sigmoid", "linear", max_chunk_frames=chunk)
        assert (status == 0).all()
        assert part.tobytes() == whole.tobytes(), chunk


def test_an_utterance_alone_equals_itself_in_the_batch(gpu):
    params, x, spkr, _, _ = R.cached_case(0, "sat", "tanh", "linear")
    whole, _, _ = run(gpu, R.LENGTHS, params, x, spkr, "tanh", "linear")
    off = np.concatenate([[0], np.cumsum(R.LENGTHS)])
    for u in (0, 4, 6, 8):
        sl = slice(off[u], off[u + 1])
        alone, _, _ = run(gpu, [R.LENGTHS[u]], params, x[sl], [spkr[u]], "tanh", "linear")
        assert alone.tobytes() == whole[sl].tobytes(), u


def test_column_view_with_nan_beside_it(gpu):
    """x as columns 3 .. 39 of a wider matrix whose other columns hold NaN: the row stride is passed, nothing beyond a
    row's own columns is read."""
    torch = gpu[0]
    params, x, spkr, _, _ = R.cached_case(0, "sat", "relu", "linear")
    packed, _, _ = run(gpu, R.LENGTHS, params, x, spkr, "relu", "linear")
    wide = np.full((x.shape[0], 45), np.nan, dtype=np.float32)
    wide[:, 3:40] = x
    wd = torch.from_numpy(wide).cuda()
    view = wd[:, 3:40]
    assert view.stride(0) == 45 and view.data_ptr() == wd.data_ptr() + 12
    out, _, status = run(gpu, R.LENGTHS, params, None, spkr, "relu", "linear", x_dev=view)
    assert (status == 0).all()
    assert out.tobytes() == packed.tobytes()


def make_obs(ref, seed=7):
    rng = np.random.default_rng(seed)
    return (ref + rng.standard_normal(ref.shape)).astype(np.float32)


@pytest.mark.parametrize("mode", ["sd", "sat"])
def test_cost(gpu, mode):
    """T = 1 and a batch: the float64 sum over the returned out, the targets and the speaker's variances."""
    params, x, spkr, ref, _ = R.cached_case(0, mode, "sigmoid", "linear")
    obs = make_obs(ref)
    out, cost, status = run(gpu, R.LENGTHS, params, x, spkr, "sigmoid", "linear", obs=obs)
    assert cost.dtype == np.float64 and cost.shape == (len(R.LENGTHS),) and (status == 0).all()
    off = np.concatenate([[0], np.cumsum(R.LENGTHS)])
    worst = 0.0
    for u, T in enumerate(R.LENGTHS):
        sl = slice(off[u], off[u + 1])
        s = spkr[u] if spkr is not None else params["variance.variances"].shape[0] - 1
        want, S = R.cost(out[sl], obs[sl], params["variance.variances"][s])
        ratio = abs(cost[u] - want) / (64.0 * 2.0 ** -53 * S)
        assert ratio <= 1.0, (mode, T, cost[u], want, ratio)
        worst = max(worst, ratio)
    print("cost %s: worst error / bound %.3f" % (mode, worst))
    for u in (0, 8):                                                     # T = 1 and T = 257 alone: the same bits
        sl = slice(off[u], off[u + 1])
        _, alone, _ = run(gpu, [R.LENGTHS[u]], params, x[sl], None if spkr is None else [spkr[u]], "sigmoid", "linear",
                          obs=obs[sl])
        assert alone[0] == cost[u] and alone.tobytes() == cost[u:u + 1].tobytes()


def test_non_finite_inputs_flag_their_utterance_only(gpu):
    """ReLU hidden units would swallow a NaN: the utterance is flagged from its x, its rows are zeros, the others keep
    their bits."""
    params, x, spkr, ref, _ = R.cached_case(0, "sat", "relu", "linear")
    obs = make_obs(ref)
    clean, clean_cost, _ = run(gpu, R.LENGTHS, params, x, spkr, "relu", "linear", obs=obs)
    off = np.concatenate([[0], np.cumsum(R.LENGTHS)])
    bad = np.array(x)
    bad[off[5] + 3, 36] = np.nan                                         # utterance 5 (127 frames), the last column
    bad[off[5] + 100, 0] = np.inf
    out, cost, status = run(gpu, R.LENGTHS, params, bad, spkr, "relu", "linear", obs=obs)
    assert status.tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0]
    assert (out[off[5]:off[6]] == 0).all() and cost[5] == 0.0
    keep = np.r_[0:off[5], off[6]:off[9]]
    assert out[keep].tobytes() == clean[keep].tobytes()
    assert np.delete(cost, 5).tobytes() == np.delete(clean_cost, 5).tobytes()
    out, _, status = run(gpu, R.LENGTHS, params, bad, spkr, "relu", "linear")          # without a cost: the same flag
    assert status.tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0] and (out[off[5]:off[6]] == 0).all()
    assert out[keep].tobytes() == clean[keep].tobytes()
    nobs = np.array(obs)
    nobs[off[2] + 1, 7] = np.nan                                         # a non-finite target: bit 1, with a cost only
    out, cost, status = run(gpu, R.LENGTHS, params, x, spkr, "relu", "linear", obs=nobs)
    assert status.tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0] and cost[2] == 0.0 and (out[off[2]:off[3]] == 0).all()


def test_overflowing_output_is_flagged(gpu):
    """Finite inputs whose linear output overflows float32: bit 2."""
    params = {k: np.array(v) for k, v in R.cached_case(2, "sd", "linear", "linear")[0].items()}
    x = np.array(R.cached_case(2, "sd", "linear", "linear")[1])
    lengths = (5, 40, 3)
    x = x[:sum(lengths)]
    x[7] = 3.0e38
    params["output.si_weights"][:, 4] = 3.0
    out, _, status = run(gpu, lengths, params, x, None, "linear", "linear")
    assert status.tolist() == [0, 2, 0] and (out[5:45] == 0).all() and (out[:5] != 0).any() and (out[45:] != 0).any()


def test_zero_variance_flags_only_when_a_cost_is_asked(gpu):
    params = {k: np.array(v) for k, v in R.cached_case(0, "sat", "sigmoid", "linear")[0].items()}
    _, x, spkr, ref, _ = R.cached_case(0, "sat", "sigmoid", "linear")
    params["variance.variances"][1, 200] = 0.0                           # speaker 1: utterances 0, 3, 6
    assert [u for u, s in enumerate(spkr) if s == 1] == [0, 3, 6]
    clean, _, status = run(gpu, R.LENGTHS, params, x, spkr, "sigmoid", "linear")
    assert (status == 0).all() and (clean != 0).any(axis=1).all()
    out, cost, status = run(gpu, R.LENGTHS, params, x, spkr, "sigmoid", "linear", obs=make_obs(ref))
    assert status.tolist() == [2, 0, 0, 2, 0, 0, 2, 0, 0]
    off = np.concatenate([[0], np.cumsum(R.LENGTHS)])
    for u in range(len(R.LENGTHS)):
        rows = out[off[u]:off[u + 1]]
        if status[u]:
            assert (rows == 0).all() and cost[u] == 0.0
        else:
            assert rows.tobytes() == clean[off[u]:off[u + 1]].tobytes() and cost[u] > 0.0


# ---- refusals: WM_ERR_BAD_ARG before any device call ---------------------------------------------------------------
def _c_call(gpu, change):
    """A complete, valid call through ctypes on a batch of two utterances (net 3 -> 4 -> 2, two speakers, SAT), changed
    by `change(d, a)`: d the WorldMi355AcousticModel, a the other arguments.  Returns (rc, out after the call)."""
    torch, W, ctx = gpu
    b = frames_batch(W, ctx, [3, 2])
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    t = {"w0": z(3, 4), "w1": z(4, 2), "b0": z(4), "b1": z(2), "sd0": z(2, 4), "var": z(2, 2) + 1, "x": z(5, 3), "obs": z(5, 2),
         "out": z(5, 2) + 7, "cost": torch.zeros(2, dtype=torch.float64, device="cuda"),
         "status": torch.zeros(2, dtype=torch.int32, device="cuda")}
    p = lambda k: t[k].data_ptr()
    d = W.AcousticModelDesc()
    d.n_layers, d.n_inputs, d.n_outputs, d.n_spkrs, d.hidden_activation, d.output_activation = 1, 3, 2, 2, 1, 0
    keep = {"units": (C.c_int * 1)(4), "weights": (C.c_void_p * 2)(p("w0"), p("w1")), "biases": (C.c_void_p * 2)(p("b0"), p("b1")),
            "spkr_weights": (C.c_void_p * 1)(p("sd0")), "spkr": (C.c_int * 2)(0, 1)}
    d.units, d.weights, d.biases, d.spkr_weights, d.variances = (keep["units"], keep["weights"], keep["biases"],
                                                                 keep["spkr_weights"], p("var"))
    a = {"x": p("x"), "ld_x": 3, "spkr": C.cast(keep["spkr"], C.c_void_p), "out": p("out"), "ld_out": 2, "obs": p("obs"),
         "ld_obs": 2, "cost": p("cost"), "status": p("status"), "model": C.byref(d), "keep": keep}
    change(d, a)
    v = lambda k: a[k] if not isinstance(a[k], int) else C.c_void_p(a[k])
    rc = W.load_library().WorldMi355AcousticModelForward(b.handle, a["model"], v("x"), a["ld_x"], a["spkr"], v("out"), a["ld_out"],
                                                         v("obs"), a["ld_obs"], v("cost"), v("status"))
    ctx.synchronize()
    out = t["out"].cpu().numpy()
    b.close()
    return rc, out


def _set(obj, **kw):
    for k, val in kw.items():
        if isinstance(obj, dict):
            obj[k] = val
        else:
            setattr(obj, k, val)


def _null_entry(name, i):
    def f(d, a):
        a["keep"][name][i] = None
    return f


def _spkr(*vals):
    def f(d, a):
        a["keep"]["spkr"][0], a["keep"]["spkr"][1] = vals
    return f


REFUSED = {
    "null_model": lambda d, a: _set(a, model=None), "null_x": lambda d, a: _set(a, x=None),
    "null_out": lambda d, a: _set(a, out=None), "null_units": lambda d, a: _set(d, units=None),
    "null_weights": lambda d, a: _set(d, weights=None), "null_biases": lambda d, a: _set(d, biases=None),
    "null_weight_entry": _null_entry("weights", 1), "null_bias_entry": _null_entry("biases", 0),
    "null_spkr_weight_entry": _null_entry("spkr_weights", 0),
    "layers_neg": lambda d, a: _set(d, n_layers=-1), "layers_9": lambda d, a: _set(d, n_layers=9),
    "units_0": lambda d, a: a["keep"]["units"].__setitem__(0, 0), "inputs_0": lambda d, a: _set(d, n_inputs=0),
    "outputs_0": lambda d, a: _set(d, n_outputs=0), "spkrs_0": lambda d, a: _set(d, n_spkrs=0),
    "hidden_act_4": lambda d, a: _set(d, hidden_activation=4), "hidden_act_neg": lambda d, a: _set(d, hidden_activation=-1),
    "output_act_4": lambda d, a: _set(d, output_activation=4), "output_act_neg": lambda d, a: _set(d, output_activation=-1),
    "spkr_2": _spkr(0, 2), "spkr_neg": _spkr(-1, 0),
    "ld_x": lambda d, a: _set(a, ld_x=2), "ld_out": lambda d, a: _set(a, ld_out=1), "ld_obs": lambda d, a: _set(a, ld_obs=1),
    "cost_without_obs": lambda d, a: _set(a, obs=None), "cost_without_variances": lambda d, a: _set(d, variances=None),
    "chunk_neg": lambda d, a: _set(d, max_chunk_frames=-1),
}


def test_the_unchanged_call_is_accepted(gpu):
    rc, out = _c_call(gpu, lambda d, a: None)
    assert rc == 0 and (out == 0).all()                                  # zero weights, linear output: 0, not the 7 it held
    rc, out = _c_call(gpu, lambda d, a: _set(a, cost=None, obs=None, status=None, spkr=None))
    assert rc == 0 and (out == 0).all()
    rc, out = _c_call(gpu, lambda d, a: (_set(a, cost=None), _set(d, variances=None, spkr_weights=None)))
    assert rc == 0 and (out == 0).all()


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusals(gpu, what):
    rc, out = _c_call(gpu, REFUSED[what])
    assert rc == 2, what                                                 # WM_ERR_BAD_ARG
    assert (out == 7).all()                                              # and nothing ran


# ---- the chain: forward pass -> parameter generation -> trajectory loss --------------------------------------------
RECIPE_LAYOUT = ((50, False), (1, True), (25, False))                   # mgc 50 x 3, lf0 1 x 3 behind its voicing column, bap 25 x 3
CHAIN_LENGTHS = (1, 2, 33, 129)


def test_chain_to_parameter_generation(gpu):
    """acoustic_model_forward -> parameter_generation with the speaker's variance row, on the recipe layout (229
    outputs), without leaving the device: against mlpg_reference fed the float64 forward pass, within
    mlpg_reference.bound widened by the forward bound pushed through the solve, cond * e."""
    torch, W, ctx = gpu
    params, x, spkr, ref, e = R.cached_case(0, "sat", "sigmoid", "linear", CHAIN_LENGTHS)
    assert ref.shape[1] == 229
    b = frames_batch(W, ctx, CHAIN_LENGTHS)
    out, _, status = b.acoustic_model_forward(model_dict(torch, params, "sigmoid", "linear"),
                                              torch.from_numpy(np.array(x)).cuda(), spkr)
    assert int(status.abs().sum()) == 0
    # one variance row for the batch: parameter_generation takes one.  The utterances' speakers differ ([1, 0, 2, 1]);
    # speaker 1's row is given to the library and to mlpg_reference alike, and it only weights the solve
    var = params["variance.variances"][1]
    dvar = torch.from_numpy(np.array(var)).cuda()
    streams, at = [], 0
    for dim, msd in RECIPE_LAYOUT:
        at += 1 if msd else 0
        streams.append((out[:, at:at + 3 * dim], dvar[at:at + 3 * dim], M.RECIPE, None))
        at += 3 * dim
    assert at == 229
    cs, st2 = b.parameter_generation(streams, edge=0)
    assert int(st2.abs().sum()) == 0
    off = np.concatenate([[0], np.cumsum(CHAIN_LENGTHS)])
    at, worst = 0, 0.0
    for (dim, msd), c in zip(RECIPE_LAYOUT, cs):
        at += 1 if msd else 0
        got = c.cpu().numpy().astype(np.float64)
        for u, T in enumerate(CHAIN_LENGTHS):
            sl = slice(off[u], off[u + 1])
            want, cond = M.mlpg(ref[sl, at:at + 3 * dim], var[at:at + 3 * dim], M.RECIPE, 0)
            ee = e[sl, at:at + 3 * dim] + np.spacing(np.abs(ref[sl, at:at + 3 * dim]).astype(np.float32))
            e_col = ee.reshape(T, 3, dim).max(axis=(0, 1))              # per static column: its three windows, every frame
            tol = M.bound(want, cond) + cond * e_col
            worst = max(worst, float((np.abs(got[sl] - want) / tol[None, :]).max()))
        at += 3 * dim
    b.close()
    print("chain: worst error / bound %.4f" % worst)
    assert worst <= 1.0


def test_trajectory_loss_on_infer_output(gpu, pkg):
    """TrajectoryLoss on AcousticModel.infer's output equals TrajectoryLoss on the same tensor passed directly."""
    torch, W, ctx = gpu
    T = pkg.training
    params, x, spkr, ref, _ = R.cached_case(0, "sat", "sigmoid", "linear", CHAIN_LENGTHS)
    m = T.AcousticModel(37, [48, 130], 229, R.N_SPKRS, "sigmoid", "linear")
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
    m = m.cuda()
    b = frames_batch(W, ctx, CHAIN_LENGTHS)
    out, _, status = m.infer(b, torch.from_numpy(np.array(x)).cuda(), spkr)
    assert int(status.abs().sum()) == 0
    layout = [(dim, M.RECIPE, msd) for dim, msd in RECIPE_LAYOUT]
    obs = torch.from_numpy(make_obs(ref, 11)).cuda()
    var = torch.from_numpy(np.array(params["variance.variances"][1])).cuda()
    gv = torch.ones(76, dtype=torch.float32, device="cuda")
    a = T.TrajectoryLoss.apply(b, out, var, obs, gv, layout)
    direct = torch.from_numpy(out.cpu().numpy()).cuda()
    c = T.TrajectoryLoss.apply(b, direct, var, obs, gv, layout)
    assert a.cpu().numpy().tobytes() == c.cpu().numpy().tobytes() and bool(torch.isfinite(a).all())
    with torch.no_grad():                                                # and the module's own forward states the same net
        plain = m(torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(R.spkr_rows(CHAIN_LENGTHS, spkr)).cuda())
    assert float((plain - out).abs().max()) <= 1e-4 * float(out.abs().max())
    b.close()

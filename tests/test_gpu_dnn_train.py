"""WorldBatch.acoustic_model_train_forward / acoustic_model_backward (csrc/dnn_train.hip) against
tests/dnn_train_reference.py, the float64 statement of the training pass with its Philox dropout mask, on the same float32
inputs -- never against another run of the library, except where a test is about two runs agreeing bit for bit.

Shapes: dnn_reference's five nets over its utterance lengths (612 rows; boundaries inside MFMA and block tiles).
Bounds: the exact test asks bit-for-bit equality on small integers at keep_prob 1 and 0.5 (1 / p = 2 is exact); the
bound test asks |gradient - ref| <= the reference's running bound of a float32 evaluation, element by element (nothing
in it is measured); the cost gradients are held to the forward bound / (var T D) + 2 u |value| and to 64 * 2^-53 of the
sum of the magnitudes of grad_var's terms."""
import ctypes as C

import numpy as np
import pytest

import dnn_reference as R
import dnn_train_reference as T
import test_gpu_dnn as F

pytestmark = pytest.mark.gpu

SEED, OFFSET = 20261019, 3
NET_IDS = ["37-48-130-229", "1-1-1", "3-33", "65-129-31", "700-229"]
OFF = np.concatenate([[0], np.cumsum(R.LENGTHS)])
ROWS = int(OFF[-1])


def rows_of(params, spkr):
    n_spkrs = params["variance.variances"].shape[0]
    return R.spkr_rows(R.LENGTHS, spkr if spkr is not None else [n_spkrs - 1] * len(R.LENGTHS))


def run(gpu, params, x, spkr, hidden, output, p, G, chunk=0, x_dev=None, G_dev=None, obs=None, lengths=R.LENGTHS):
    """One training forward (with the cost gradients when obs is given) and one backward pass on G.  Returns a dict:
    out, cost, status, grad_out, grad_var, grads (name -> numpy), bstatus."""
    torch, W, ctx = gpu
    b = F.frames_batch(W, ctx, lengths)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    xd = x_dev if x_dev is not None else dev(x)
    model = F.model_dict(torch, params, hidden, output)
    res = b.acoustic_model_train_forward(model, xd, spkr, None if obs is None else dev(obs), p, SEED, OFFSET, obs is not None,
                                         chunk)
    r = {"out": res[0].cpu().numpy(), "cost": None if res[1] is None else res[1].cpu().numpy(), "status": res[2].cpu().numpy()}
    if obs is not None:
        r["grad_out"], r["grad_var"] = res[3].cpu().numpy(), res[4].cpu().numpy()
    if G is not None or G_dev is not None:
        g = b.acoustic_model_backward(model, xd, spkr, G_dev if G_dev is not None else dev(G), p, SEED, OFFSET, chunk)
        r["bstatus"] = g.pop("status").cpu().numpy()
        r["grads"] = {k: v.cpu().numpy() for k, v in g.items()}
    b.close()
    return r


def same_bits(a, b):
    return set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.mark.parametrize("net", range(len(R.NETS)), ids=NET_IDS)
def test_exact_on_small_integers(gpu, net):
    """Outputs and every gradient equal the float64 reference bit for bit: linear and ReLU hidden units, the three
    modes, keep_prob 1 and 0.5.  At 0.5 the outputs show the hidden layers' zero pattern: the reference mask's."""
    for mode in R.MODES:
        for hidden in ("linear", "relu"):
            params, x, spkr, ref = R.exact_case(net, mode, hidden)
            sr = rows_of(params, spkr)
            for p in (1.0, 0.5):
                fw = T.train_forward(params, x, sr, hidden, "linear", p, SEED, OFFSET)
                for i, (Wt, bv, sd) in enumerate(R.layers(params)):          # the forward products stay exact at 1 / p = 2
                    h = fw["x"] if i == 0 else fw["h"][i - 1]
                    m = np.abs(h) @ np.abs(Wt) + np.abs(bv) + (0.0 if sd is None else np.abs(sd[sr]))
                    assert m.max() < 2.0 ** 24
                G = T.exact_G(ROWS, ref.shape[1], 8)
                if T.products_stay_exact(params, fw, G, hidden, "linear") >= 2.0 ** 24:
                    G = T.exact_G(ROWS, ref.shape[1], 16)
                worst = T.products_stay_exact(params, fw, G, hidden, "linear")
                assert worst < 2.0 ** 24, (mode, hidden, p, worst)
                want, _ = T.backward(params, fw, G, sr, hidden, "linear")
                got = run(gpu, params, x, spkr, hidden, "linear", p, G)
                assert (got["status"] == 0).all() and (got["bstatus"] == 0).all()
                if p == 1.0:
                    assert (fw["out"] == ref).all()
                assert (got["out"].astype(np.float64) == fw["out"]).all(), (mode, hidden, p)
                assert set(got["grads"]) == set(want)
                for k in want:
                    g = got["grads"][k]
                    assert g.dtype == np.float32 and g.shape == want[k].shape
                    wrong = np.argwhere(g.astype(np.float64) != want[k])
                    assert wrong.size == 0, (mode, hidden, p, k, len(wrong), wrong[:5].tolist())


@pytest.mark.parametrize("net", range(len(R.NETS)), ids=NET_IDS)
def test_within_the_backward_error_bound(gpu, net):
    """Every hidden activation, linear and sigmoid outputs, the three modes, keep_prob 1 and 0.8: every gradient element
    within the reference's bound; the outputs within the forward bound."""
    worst_net = 0.0
    for n, mode, hidden, output in R.all_cases():
        if n != net:
            continue
        params, x, spkr, _, _ = R.cached_case(net, mode, hidden, output)
        sr = rows_of(params, spkr)
        G = T.random_G(R.SEED + 900 + net, ROWS, R.NETS[net][2])
        for p in (1.0, 0.8):
            fw = T.train_forward(params, x, sr, hidden, output, p, SEED, OFFSET)
            want, bound = T.backward(params, fw, G, sr, hidden, output)
            got = run(gpu, params, x, spkr, hidden, output, p, G)
            assert (got["status"] == 0).all() and (got["bstatus"] == 0).all()
            assert (np.abs(got["out"].astype(np.float64) - fw["out"]) <= fw["e_out"]).all()
            worst = 0.0
            for k in want:
                err = np.abs(got["grads"][k].astype(np.float64) - want[k])
                assert np.isfinite(err).all()
                ratio = float(np.where(err > 0, err / np.maximum(bound[k], 1e-300), 0.0).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (mode, hidden, output, p, k, ratio)
            print("net %d %s %s/%s p %.1f: worst error / bound %.4f" % (net, mode, hidden, output, p, worst))
            worst_net = max(worst_net, worst)
    print("net %d: worst error / bound %.4f" % (net, worst_net))


def test_keep_prob_one_equals_the_forward_call(gpu):
    torch, W, ctx = gpu
    for mode, hidden in (("sat", "sigmoid"), ("sd", "tanh")):
        params, x, spkr, ref, _ = R.cached_case(0, mode, hidden, "linear")
        obs = F.make_obs(ref)
        plain, cost, status = F.run(gpu, R.LENGTHS, params, x, spkr, hidden, "linear", obs=obs)
        got = run(gpu, params, x, spkr, hidden, "linear", 1.0, None, obs=obs)
        assert got["out"].tobytes() == plain.tobytes() and got["cost"].tobytes() == cost.tobytes()
        assert (got["status"] == status).all()


def test_chunks_and_repeats_do_not_change_a_bit(gpu):
    """max_chunk_frames 64, 1 and 33 against the default call, and the default call twice: out, grad_out and every
    parameter gradient, on the SAT case of 37 -> 48, 130 -> 229 at keep_prob 0.8."""
    params, x, spkr, ref, _ = R.cached_case(0, "sat", "sigmoid", "linear")
    obs = F.make_obs(ref)
    G = T.random_G(5, ROWS, 229)
    whole = run(gpu, params, x, spkr, "sigmoid", "linear", 0.8, G, obs=obs)
    assert (whole["out"] == 0).mean() < 0.01 and (whole["bstatus"] == 0).all()
    for chunk in (0, 64, 1, 33):
        part = run(gpu, params, x, spkr, "sigmoid", "linear", 0.8, G, chunk=chunk, obs=obs)
        assert (part["status"] == 0).all() and (part["bstatus"] == 0).all()
        assert part["out"].tobytes() == whole["out"].tobytes(), chunk
        assert part["grad_out"].tobytes() == whole["grad_out"].tobytes(), chunk
        assert part["grad_var"].tobytes() == whole["grad_var"].tobytes(), chunk
        assert same_bits(part["grads"], whole["grads"]), (chunk, [k for k in whole["grads"]
                                                                  if part["grads"][k].tobytes() != whole["grads"][k].tobytes()])


def test_column_views_between_nan_columns(gpu):
    torch = gpu[0]
    params, x, spkr, _, _ = R.cached_case(0, "sat", "relu", "linear")
    G = T.random_G(6, ROWS, 229)
    packed = run(gpu, params, x, spkr, "relu", "linear", 0.8, G)
    wide = np.full((ROWS, 45), np.nan, dtype=np.float32)
    wide[:, 3:40] = x
    gwide = np.full((ROWS, 235), np.nan, dtype=np.float32)
    gwide[:, 5:234] = G
    wd, gd = torch.from_numpy(wide).cuda(), torch.from_numpy(gwide).cuda()
    xv, gv = wd[:, 3:40], gd[:, 5:234]
    assert xv.stride(0) == 45 and gv.stride(0) == 235 and gv.data_ptr() == gd.data_ptr() + 20
    got = run(gpu, params, None, spkr, "relu", "linear", 0.8, None, x_dev=xv, G_dev=gv)
    assert (got["status"] == 0).all() and (got["bstatus"] == 0).all()
    assert got["out"].tobytes() == packed["out"].tobytes() and same_bits(got["grads"], packed["grads"])


def test_non_finite_values_flag_their_utterance_only(gpu):
    """A NaN in utterance 5's x, and separately in its G: bit 1 on that utterance alone, and all gradients equal, bit
    for bit, those of the batch with that utterance's x finite and its G rows zero."""
    params, x, spkr, _, _ = R.cached_case(0, "sat", "relu", "linear")
    G = T.random_G(7, ROWS, 229)
    Gz = np.array(G)
    Gz[OFF[5]:OFF[6]] = 0.0
    want = run(gpu, params, x, spkr, "relu", "linear", 0.8, Gz)
    assert (want["bstatus"] == 0).all()
    bad = np.array(x)
    bad[OFF[5] + 3, 36] = np.nan
    bad[OFF[5] + 100, 0] = np.inf
    got = run(gpu, params, bad, spkr, "relu", "linear", 0.8, G)
    assert got["status"].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0] and got["bstatus"].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0]
    assert (got["out"][OFF[5]:OFF[6]] == 0).all()
    keep = np.r_[0:OFF[5], OFF[6]:OFF[9]]
    assert got["out"][keep].tobytes() == want["out"][keep].tobytes()
    assert same_bits(got["grads"], want["grads"])
    Gn = np.array(G)
    Gn[OFF[5] + 126, 228] = np.nan
    got = run(gpu, params, x, spkr, "relu", "linear", 0.8, Gn)
    assert (got["status"] == 0).all() and got["bstatus"].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0]
    assert same_bits(got["grads"], want["grads"])
    got = run(gpu, params, bad, spkr, "relu", "linear", 0.8, Gn, chunk=33)            # both, in chunks
    assert got["bstatus"].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0] and same_bits(got["grads"], want["grads"])


@pytest.mark.parametrize("mode", ["sd", "sat"])
def test_cost_gradients(gpu, mode):
    """T = 1 ... 257 against the reference fed the float64 forward pass."""
    params, x, spkr, ref, e = R.cached_case(0, mode, "sigmoid", "linear")
    obs = F.make_obs(ref)
    got = run(gpu, params, x, spkr, "sigmoid", "linear", 1.0, None, obs=obs)
    assert got["grad_out"].dtype == np.float32 and got["grad_var"].dtype == np.float64 and (got["status"] == 0).all()
    assert got["grad_var"].shape == (len(R.LENGTHS), 229)
    worst_o = worst_v = 0.0
    for u, Tn in enumerate(R.LENGTHS):
        sl = slice(OFF[u], OFF[u + 1])
        s = spkr[u] if spkr is not None else params["variance.variances"].shape[0] - 1
        var = params["variance.variances"][s]
        # from the float64 outputs: the returned out is within e of them
        go = (ref[sl] - obs[sl].astype(np.float64)) / (var.astype(np.float64)[None, :] * Tn * 229)
        tol = e[sl] / (var.astype(np.float64)[None, :] * Tn * 229) + 2.0 * R.U * np.abs(go)
        ratio = float((np.abs(got["grad_out"][sl] - go) / tol).max())
        assert ratio <= 1.0, (mode, Tn, "grad_out", ratio)
        worst_o = max(worst_o, ratio)
        _, gv, S = T.cost_grads(got["out"][sl], obs[sl], var)             # over the RETURNED out, as the cost test
        ratio = float((np.abs(got["grad_var"][u] - gv) / (64.0 * 2.0 ** -53 * S)).max())
        assert ratio <= 1.0, (mode, Tn, "grad_var", ratio)
        worst_v = max(worst_v, ratio)
    print("cost gradients %s: worst error / bound grad_out %.3f grad_var %.3f" % (mode, worst_o, worst_v))


# ---- refusals: WM_ERR_BAD_ARG before any device call ---------------------------------------------------------------
def _c_calls(gpu, change):
    """Complete, valid TrainForward and Backward calls through ctypes (net 3 -> 4 -> 2, two speakers, SAT, two
    utterances), changed by `change(d, a)`.  Returns (rc forward, rc backward, out, gradient of the first weights)."""
    torch, W, ctx = gpu
    b = F.frames_batch(W, ctx, [3, 2])
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    t = {"w0": z(3, 4), "w1": z(4, 2), "b0": z(4), "b1": z(2), "sd0": z(2, 4), "var": z(2, 2) + 1, "x": z(5, 3), "obs": z(5, 2),
         "out": z(5, 2) + 7, "cost": torch.zeros(2, dtype=torch.float64, device="cuda"), "go": z(5, 2),
         "gvar": torch.zeros(2, 2, dtype=torch.float64, device="cuda"), "G": z(5, 2),
         "gw0": z(3, 4) + 7, "gw1": z(4, 2), "gb0": z(4), "gb1": z(2), "gs0": z(2, 4),
         "status": torch.zeros(2, dtype=torch.int32, device="cuda")}
    p = lambda k: t[k].data_ptr()
    d = W.AcousticModelDesc()
    d.n_layers, d.n_inputs, d.n_outputs, d.n_spkrs, d.hidden_activation, d.output_activation = 1, 3, 2, 2, 1, 0
    keep = {"units": (C.c_int * 1)(4), "weights": (C.c_void_p * 2)(p("w0"), p("w1")), "biases": (C.c_void_p * 2)(p("b0"), p("b1")),
            "spkr_weights": (C.c_void_p * 1)(p("sd0")), "spkr": (C.c_int * 2)(0, 1),
            "gw": (C.c_void_p * 2)(p("gw0"), p("gw1")), "gb": (C.c_void_p * 2)(p("gb0"), p("gb1")), "gs": (C.c_void_p * 1)(p("gs0")),
            "drop": W.Dropout(0.5, 1, 0)}
    d.units, d.weights, d.biases, d.spkr_weights, d.variances = (keep["units"], keep["weights"], keep["biases"],
                                                                 keep["spkr_weights"], p("var"))
    a = {"x": p("x"), "ld_x": 3, "spkr": C.cast(keep["spkr"], C.c_void_p), "out": p("out"), "ld_out": 2, "obs": p("obs"),
         "ld_obs": 2, "cost": p("cost"), "grad_out": p("go"), "ld_grad": 2, "grad_var": p("gvar"), "G": p("G"), "ld_g": 2,
         "gw": keep["gw"], "gb": keep["gb"], "gs": keep["gs"], "drop": C.byref(keep["drop"]),
         "status": p("status"), "model": C.byref(d), "keep": keep}
    change(d, a)
    v = lambda k: a[k] if not isinstance(a[k], int) else C.c_void_p(a[k])
    L = W.load_library()
    rc_f = L.WorldMi355AcousticModelTrainForward(b.handle, a["model"], a["drop"], v("x"), a["ld_x"], a["spkr"], v("out"),
                                                 a["ld_out"], v("obs"), a["ld_obs"], v("cost"), v("grad_out"), a["ld_grad"],
                                                 v("grad_var"), v("status"))
    rc_b = L.WorldMi355AcousticModelBackward(b.handle, a["model"], a["drop"], v("x"), a["ld_x"], a["spkr"], v("G"), a["ld_g"],
                                             a["gw"], a["gb"], a["gs"], v("status"))
    ctx.synchronize()
    res = rc_f, rc_b, t["out"].cpu().numpy(), t["gw0"].cpu().numpy()
    b.close()
    return res


def _keep_prob(value):
    def f(d, a):
        a["keep"]["drop"].keep_prob = value
    return f


def _null_grad_entry(name, i):
    def f(d, a):
        a["keep"][name][i] = None
    return f


BOTH, FWD, BWD = "both", "forward", "backward"
REFUSED = {k: (BOTH, f) for k, f in F.REFUSED.items() if k not in ("null_out", "ld_out", "ld_obs", "cost_without_obs",
                                                                   "cost_without_variances")}
REFUSED.update({
    "null_out": (FWD, F.REFUSED["null_out"]), "ld_out": (FWD, F.REFUSED["ld_out"]), "ld_obs": (FWD, F.REFUSED["ld_obs"]),
    "cost_without_obs": (FWD, F.REFUSED["cost_without_obs"]),
    "cost_without_variances": (FWD, F.REFUSED["cost_without_variances"]),
    "grads_without_obs": (FWD, lambda d, a: F._set(a, obs=None, cost=None)),
    "grad_var_without_variances": (FWD, lambda d, a: (F._set(a, cost=None, grad_out=None), F._set(d, variances=None))),
    "keep_prob_0": (BOTH, _keep_prob(0.0)), "keep_prob_neg": (BOTH, _keep_prob(-0.5)), "keep_prob_above_1": (BOTH, _keep_prob(1.5)),
    "keep_prob_nan": (BOTH, _keep_prob(float("nan"))), "keep_prob_inf": (BOTH, _keep_prob(float("inf"))),
    "ld_grad_out": (FWD, lambda d, a: F._set(a, ld_grad=1)), "ld_G": (BWD, lambda d, a: F._set(a, ld_g=1)),
    "null_G": (BWD, lambda d, a: F._set(a, G=None)),
    "null_grad_weight_entry": (BWD, _null_grad_entry("gw", 1)), "null_grad_bias_entry": (BWD, _null_grad_entry("gb", 0)),
    "null_grad_spkr_weight_entry": (BWD, _null_grad_entry("gs", 0)),
    "grad_spkr_weights_without_spkr_weights": (BWD, lambda d, a: F._set(d, spkr_weights=None)),
})


def test_the_unchanged_calls_are_accepted(gpu):
    rc_f, rc_b, out, gw0 = _c_calls(gpu, lambda d, a: None)
    assert rc_f == 0 and rc_b == 0 and (out == 0).all() and (gw0 == 0).all()           # zero weights: 0, not the 7 they held
    rc_f, rc_b, out, gw0 = _c_calls(gpu, lambda d, a: F._set(a, drop=None, cost=None, obs=None, grad_out=None, grad_var=None,
                                                            status=None, spkr=None, gb=None, gs=None))
    assert rc_f == 0 and rc_b == 0 and (out == 0).all() and (gw0 == 0).all()
    rc_f, rc_b, out, gw0 = _c_calls(gpu, lambda d, a: F._set(a, gw=None))
    assert rc_f == 0 and rc_b == 0 and (gw0 == 7).all()


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusals(gpu, what):
    which, change = REFUSED[what]
    rc_f, rc_b, out, gw0 = _c_calls(gpu, change)
    if which in (BOTH, FWD):
        assert rc_f == 2 and (out == 7).all(), what                                    # WM_ERR_BAD_ARG, and nothing ran
    else:
        assert rc_f == 0, what
    if which in (BOTH, BWD):
        assert rc_b == 2 and (gw0 == 7).all(), what
    else:
        assert rc_b == 0, what


# ---- autograd wiring ------------------------------------------------------------------------------------------------
def _module(torch, pkg, params):
    m = pkg.training.AcousticModel(37, [48, 130], 229, R.N_SPKRS, "sigmoid", "linear")
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
    return m.cuda()


def test_autograd_through_frame_loss(gpu, pkg):
    """train_outputs + FrameLoss: the parameters' gradients equal the direct library calls bit for bit, and one
    torch.optim.SGD step leaves p - lr g exactly."""
    torch, W, ctx = gpu
    Tr = pkg.training
    params, x, spkr, ref, _ = R.cached_case(0, "sat", "sigmoid", "linear", F.CHAIN_LENGTHS)
    m = _module(torch, pkg, params)
    b = F.frames_batch(W, ctx, F.CHAIN_LENGTHS)
    xd, obs = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(F.make_obs(ref, 11)).cuda()
    out = m.train_outputs(b, xd, spkr, 0.5, SEED, OFFSET)
    loss = Tr.FrameLoss.apply(b, out, m.variance.variances, obs, spkr)
    assert loss.dtype == torch.float64 and tuple(loss.shape) == (len(F.CHAIN_LENGTHS),)
    loss.sum().backward()
    o2, cost, status, grad_out, grad_var = b.acoustic_model_train_forward(m, xd, spkr, obs, 0.5, SEED, OFFSET, True)
    assert int(status.abs().sum()) == 0
    assert o2.cpu().numpy().tobytes() == out.detach().cpu().numpy().tobytes()
    assert cost.cpu().numpy().tobytes() == loss.detach().cpu().numpy().tobytes()
    direct = b.acoustic_model_backward(m, xd, spkr, grad_out, 0.5, SEED, OFFSET)
    for name, p in m.train_parameters():
        assert p.grad.cpu().numpy().tobytes() == direct[name].cpu().numpy().tobytes(), name
    assert len(set(spkr)) < len(spkr)                                   # a speaker with more than one utterance
    gv, rows = np.zeros((R.N_SPKRS, 229)), grad_var.cpu().numpy()
    for u, s in enumerate(spkr):                                         # in the batch's order, in double, rounded once
        gv[s] += rows[u]
    assert m.variance.variances.grad.cpu().numpy().tobytes() == gv.astype(np.float32).tobytes()
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    grads = {k: p.grad.clone() for k, p in m.named_parameters()}
    torch.optim.SGD(m.parameters(), lr=0.125).step()
    for k, p in m.named_parameters():
        assert torch.equal(p.detach(), before[k] - 0.125 * grads[k]), k
    b.close()


def test_autograd_through_trajectory_loss(gpu, pkg):
    import mlpg_reference as M
    torch, W, ctx = gpu
    Tr = pkg.training
    params, x, spkr, ref, _ = R.cached_case(0, "sat", "sigmoid", "linear", F.CHAIN_LENGTHS)
    m = _module(torch, pkg, params)
    b = F.frames_batch(W, ctx, F.CHAIN_LENGTHS)
    xd, obs = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(F.make_obs(ref, 11)).cuda()
    layout = [(dim, M.RECIPE, msd) for dim, msd in F.RECIPE_LAYOUT]
    var = torch.from_numpy(np.array(params["variance.variances"][1])).cuda()
    gv = torch.ones(76, dtype=torch.float32, device="cuda")
    out = m.train_outputs(b, xd, spkr, 0.5, SEED, OFFSET)
    Tr.TrajectoryLoss.apply(b, out, var, obs, gv, layout).sum().backward()
    leaf = out.detach().clone().requires_grad_(True)
    Tr.TrajectoryLoss.apply(b, leaf, var, obs, gv, layout).sum().backward()
    direct = b.acoustic_model_backward(m, xd, spkr, leaf.grad, 0.5, SEED, OFFSET)
    for name, p in m.train_parameters():
        assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
        assert p.grad.cpu().numpy().tobytes() == direct[name].cpu().numpy().tobytes(), name
    b.close()

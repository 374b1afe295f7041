"""The optimiser step's host side.  tests/optimizer_reference.py against torch.optim in float64 for the four rules on
which torch and TF 1.x agree (the independent pin of those four), two hand-computed first steps for the two on which
they do not, and the measured distance of torch's Adam and RMSprop from TF's rule in units of the float32 twin's own
rounding: a kernel that implemented torch's rule could not pass tests/test_gpu_optimizer.py.  Then recipe.Tf1Optimizer's
CPU path against the twin, bit for bit, and recipe.train_files with updates="tf1" on the CPU: a continued run is the run
it continues, and ADAPT mode."""
import numpy as np
import pytest
import torch

import dnn_train_reference as T
import optimizer_reference as O
from test_dnn_train_host import _torch_cost


def _torch_run(make, dtype=torch.float64):
    """STEPS steps of a torch.optim optimiser (one parameter group per tensor, at its rate) on inputs()."""
    params, grads = O.inputs()
    ps = [torch.nn.Parameter(torch.from_numpy(np.array(p)).to(dtype)) for p in params]
    opt = make([{"params": [p], "lr": r} for p, r in zip(ps, O.rates())])
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(np.array(g)).to(dtype)
        opt.step()
    return [p.detach().numpy() for p in ps], opt, ps


@pytest.mark.parametrize("rule", ["sgd", "momentum", "adagrad", "adadelta"])
def test_four_rules_are_torchs(rule):
    """step64 over the 5 steps against torch.optim in float64 (Adagrad with accumulator 0.1 and eps 0): parameters and
    slots within 64 * 2^-53 of the tensor's largest entry."""
    make = {"sgd": lambda g: torch.optim.SGD(g, lr=1.0),
            "momentum": lambda g: torch.optim.SGD(g, lr=1.0, momentum=0.9),
            "adagrad": lambda g: torch.optim.Adagrad(g, lr=1.0, initial_accumulator_value=0.1, eps=0.0),
            "adadelta": lambda g: torch.optim.Adadelta(g, lr=1.0, rho=0.95, eps=1e-8)}[rule]
    got, opt, ps = _torch_run(make)
    want, slots, _ = O.reference(rule, np.float64)
    keys = {"momentum": ["momentum_buffer"], "adagrad": ["sum"], "adadelta": ["square_avg", "acc_delta"]}.get(rule, [])
    worst = 0.0
    for k in range(len(want)):
        pairs = [(got[k], want[k])] + [(opt.state[ps[k]][key].numpy(), slots[j][k]) for j, key in enumerate(keys)]
        for a, b in pairs:
            worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max()) if np.abs(b).max() > 0 else float(np.abs(a).max()))
    print("%s: step64 against torch.optim, worst error / largest entry %.3e (bound %.3e)" % (rule, worst, 64 * 2.0 ** -53))
    assert worst <= 64 * 2.0 ** -53


def test_adam_and_rmsprop_first_steps_by_hand():
    """Where epsilon sits, and RMSprop's slot of ones.  Adam, g = 1e-8 at rate 1: alpha = sqrt(0.001) / 0.1, m = 1e-9,
    v = 1e-19, the step 3.1623e-10 / (3.1623e-10 + 1e-8) = 0.030653; torch's rule, with epsilon beside the unscaled root,
    gives 0.5.  RMSprop, g = 0.01 at rate 0.1: s = 1 + (1e-4 - 1) 0.1 = 0.90001, the step 1e-3 / sqrt(0.90001) =
    1.05409e-3; torch's, from a slot of zeros, 0.1 / sqrt(0.1) = 0.316."""
    p, g = np.zeros(1), np.array([1e-8])
    # the float32 twin: 1 - fl(0.999) is 0.001 to 2^-25 / 0.001 = 3e-5 only, and it enters alpha and v
    for step, rel in ((O.step64, 1e-12), (O.step32, 1e-4)):
        q, (m, v) = step("adam", p, g, [np.zeros(1), np.zeros(1)], 1.0)
        want = (1e-9 * np.sqrt(0.001) / 0.1) / (np.sqrt(1e-19) + 1e-8)
        assert abs(-q[0] - want) <= rel * want and abs(want - 0.030653) < 5e-7
        assert abs(m[0] - 1e-9) <= rel * 1e-9 and abs(v[0] - 1e-19) <= rel * 1e-19
        q, (s,) = step("rmsprop", p, np.array([0.01]), [np.ones(1)], 0.1)
        want = 1e-3 / np.sqrt(0.90001 + 1e-10)
        assert abs(-q[0] - want) <= rel * want and abs(want - 1.05409e-3) < 5e-9 and abs(s[0] - 0.90001) <= rel
    t = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))
    t.grad = torch.tensor([1e-8], dtype=torch.float64)
    torch.optim.Adam([t], lr=1.0, betas=(0.9, 0.999), eps=1e-8).step()
    assert abs(-float(t.detach()) - 0.5) < 1e-6
    t = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))
    t.grad = torch.tensor([0.01], dtype=torch.float64)
    torch.optim.RMSprop([t], lr=0.1, alpha=0.9, eps=1e-10).step()
    assert abs(-float(t.detach()) - 0.1 / np.sqrt(0.1)) < 1e-6
    # the powers after three steps: beta^4, in either precision rounded step by step
    for dtype in (np.float64, np.float32):
        pw = O.initial_powers(dtype)
        for _ in range(3):
            pw = O.advance_powers(pw, dtype)
        assert type(pw[0]) is dtype and pw == (dtype(dtype(dtype(dtype(0.9) * dtype(0.9)) * dtype(0.9)) * dtype(0.9)),
                                               dtype(dtype(dtype(dtype(0.999) * dtype(0.999)) * dtype(0.999)) * dtype(0.999)))
        assert abs(pw[0] - 0.9 ** 4) < 1e-6 and abs(pw[1] - 0.999 ** 4) < 1e-6


def _distance(a, b):
    return max(float(np.abs(x - y).max()) for x, y in zip(a, b)) / max(float(np.abs(y).max()) for y in b)


def test_the_inputs_tell_torchs_rule_from_tfs():
    """d32 = max|step32 - step64| / max|step64| over the parameters after the 5 steps, per rule; torch.optim.Adam and
    torch.optim.RMSprop on the same inputs lie more than 1e4 d32 from step64."""
    d32 = {}
    for rule in O.RULES:
        d32[rule] = _distance(O.reference(rule, np.float32)[0], O.reference(rule, np.float64)[0])
        print("%s: d32 %.3e" % (rule, d32[rule]))
        assert 0 < d32[rule] < 1e-5
    for rule, make in (("adam", lambda g: torch.optim.Adam(g, lr=1.0, betas=(0.9, 0.999), eps=1e-8)),
                       ("rmsprop", lambda g: torch.optim.RMSprop(g, lr=1.0, alpha=0.9, eps=1e-10))):
        far = _distance(_torch_run(make)[0], O.reference(rule, np.float64)[0])
        print("torch.optim %s: %.3e of the largest parameter from step64, %.3e d32" % (rule, far, far / d32[rule]))
        assert far > 1e4 * d32[rule]


# ---- recipe.Tf1Optimizer on the CPU -------------------------------------------------------------------------------------
def _model_with_grads(pkg, seed):
    torch.manual_seed(seed)
    m = pkg.training.AcousticModel(5, [4, 3], 2, n_spkrs=3)
    rng = np.random.default_rng(seed)
    grads = [{k: O.make_gradient(rng, p.numel()).reshape(tuple(p.shape)) for k, p in m.named_parameters()} for _ in range(3)]
    return m, grads


def _rate_of(name, lr, adapt):
    leaf = name.split(".")[-1]
    return (0.0 if adapt else lr) if leaf.startswith("si_") else lr if leaf.startswith("sd_") else 0.01 * lr


@pytest.mark.parametrize("adapt", [False, True])
@pytest.mark.parametrize("rule", O.RULES)
def test_tf1_optimizer_cpu_path_is_the_twin(pkg, rule, adapt):
    """Three steps on AcousticModel(5, [4, 3], 2, n_spkrs=3) with hand-set gradients: every parameter, slot and power
    equals step32 at that parameter's group rate, bit for bit; with adapt the si_ parameters keep their bits while their
    slots move."""
    lr = 0.25
    m, grads = _model_with_grads(pkg, 11)
    start = {k: p.detach().numpy().copy() for k, p in m.named_parameters()}
    opt = pkg.recipe.Tf1Optimizer(m, rule, lr, None, adapt=adapt)
    assert sorted(opt.names) == sorted(start)
    want = {k: (v, O.initial_slots(rule, v, np.float32)) for k, v in start.items()}
    powers = O.initial_powers(np.float32)
    for gs in grads:
        for k, p in m.named_parameters():
            p.grad = torch.from_numpy(gs[k].copy())
        opt.step()
        want = {k: O.step32(rule, want[k][0], gs[k], want[k][1], _rate_of(k, lr, adapt), powers) for k in want}
        powers = O.advance_powers(powers, np.float32)
    state = opt.state_arrays()
    assert str(state["rule"]) == rule
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
    for k, p in m.named_parameters():
        assert (bits(p.detach().numpy()) == bits(want[k][0])).all(), k
        for j, s in enumerate(want[k][1]):
            assert (bits(state["slot%d/%s" % (j, k)]) == bits(s)).all(), (k, j)
            if s.size >= 12:                         # (a gradient below 6e-5 leaves Adagrad's 0.1 where it is)
                assert (s != O.SLOT_INIT[rule][j]).any(), (k, j)
        if adapt and k.split(".")[-1].startswith("si_"):
            assert (bits(p.detach().numpy()) == bits(start[k])).all(), k
        elif rule != "adadelta":                     # (Adadelta's first steps are of the order of sqrt(eps))
            assert (p.detach().numpy() != start[k]).any(), k
    assert state["beta1_power"].dtype == np.float32 and (float(state["beta1_power"]), float(state["beta2_power"])) == \
        (float(powers[0]), float(powers[1]))
    p0 = next(iter(m.parameters()))
    p0.grad = None
    with pytest.raises(RuntimeError, match="has no gradient"):
        opt.step()
    with pytest.raises(ValueError):
        pkg.recipe.Tf1Optimizer(m, "lbfgs", lr, None)


# ---- the loop on the CPU ------------------------------------------------------------------------------------------------
def _loop(pkg, tmp_path, path, n_steps, optimizer, lines=None, **kw):
    jobs = T.write_corpus(tmp_path, 2)
    n_in, units, n_out = T.CORPUS_NET
    log = pkg.recipe.train_files(jobs, str(path), n_in, units, n_out, n_spkrs=2, keep_prob=1.0, optimizer=optimizer,
                                 learning_rate=0.01, batch_size=T.CORPUS_BATCH, n_steps=n_steps, seed=5, log_interval=1,
                                 device="cpu", report=(lines.append if lines is not None else (lambda s: None)),
                                 **{"updates": "tf1", **kw})
    with np.load(str(path)) as z:
        return log, {k: z[k] for k in z.files}


@pytest.mark.parametrize("optimizer", ["adam", "rmsprop"])
def test_a_continued_run_is_the_run_it_continues(pkg, tmp_path, monkeypatch, optimizer):
    """4 steps straight against 2 steps, a save and 2 more from restore: the same parameters, slots, powers and logged
    costs, bit for bit.  From a file without the state the run reports one line and ends elsewhere."""
    monkeypatch.setattr(pkg.recipe, "_train_cost", _torch_cost(pkg, []))
    log4, z4 = _loop(pkg, tmp_path, tmp_path / "four.npz", 4, optimizer)
    log2, z2 = _loop(pkg, tmp_path, tmp_path / "two.npz", 2, optimizer)
    lines = []
    log22, z22 = _loop(pkg, tmp_path, tmp_path / "two_two.npz", 2, optimizer, lines, restore=str(tmp_path / "two.npz"))
    assert not [ln for ln in lines if not ln.startswith("Step")]
    assert [s for s, _ in log4] == [0, 1, 2, 3] and log2 + log22 == log4
    assert str(z4["optimizer/rule"]) == optimizer and int(z4["step"]) == 4
    n_slots = len(O.SLOT_INIT[optimizer])
    assert sorted(k for k in z4 if k.startswith("optimizer/slot")) == sorted(
        "optimizer/slot%d/%s" % (j, k) for j in range(n_slots) for k in z4 if "." in k and not k.startswith("optimizer/"))
    assert set(z4) == set(z22)
    for k in z4:
        assert z4[k].dtype == z22[k].dtype and z4[k].tobytes() == z22[k].tobytes(), k
    f = np.float32
    assert z4["optimizer/beta1_power"] == f(f(f(f(f(0.9) * f(0.9)) * f(0.9)) * f(0.9)) * f(0.9))
    # a file without the optimiser's state: one line, and another run
    pkg.training.AcousticModel.load(str(tmp_path / "two.npz")).save(str(tmp_path / "bare.npz"), 2)
    lines = []
    _, zb = _loop(pkg, tmp_path, tmp_path / "from_bare.npz", 2, optimizer, lines, restore=str(tmp_path / "bare.npz"))
    extra = [ln for ln in lines if not ln.startswith("Step")]
    assert len(extra) == 1 and "begins anew" in extra[0] and optimizer in extra[0]
    assert any(zb[k].tobytes() != z4[k].tobytes() for k in z4 if "." in k and not k.startswith("optimizer/"))
    # the state of another optimiser is no state of this one
    other = "rmsprop" if optimizer == "adam" else "adam"
    lines = []
    _loop(pkg, tmp_path, tmp_path / "other.npz", 1, other, lines, restore=str(tmp_path / "two.npz"))
    assert len([ln for ln in lines if "begins anew" in ln]) == 1


def test_a_file_without_optimizer_state_loads_as_before(pkg, tmp_path):
    """The format of before: the parameters, the activations and the step, nothing under optimizer/."""
    torch.manual_seed(3)
    m = pkg.training.AcousticModel(5, [4], 2, n_spkrs=2)
    arrays = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    arrays.update(step=np.array(7, dtype=np.int64), hidden_activation=np.array("sigmoid"), output_activation=np.array("linear"))
    np.savez(str(tmp_path / "old.npz"), **arrays)
    got = pkg.training.AcousticModel.load(str(tmp_path / "old.npz"))
    assert got.step == 7 and got.optimizer_state is None and got.sat
    for k, v in got.state_dict().items():
        assert (v.numpy() == arrays[k]).all()
    m.save(str(tmp_path / "new.npz"), 7)                                   # and save() without a state writes that format
    with np.load(str(tmp_path / "new.npz")) as z:
        assert set(z.files) == set(arrays)
    m.save(str(tmp_path / "with.npz"), 7, {"rule": np.array("sgd"), "beta1_power": np.float32(0.9), "beta2_power": np.float32(0.999)})
    got = pkg.training.AcousticModel.load(str(tmp_path / "with.npz"))
    assert str(got.optimizer_state["rule"]) == "sgd" and set(got.optimizer_state) == {"rule", "beta1_power", "beta2_power"}


@pytest.mark.parametrize("updates", ["tf1", "torch"])
def test_adapt_mode_on_the_cpu(pkg, tmp_path, monkeypatch, updates):
    """adapt with n_steps=0 saves the mean row; two steps leave every si_ parameter's bits and move the rest; adapt
    without restore, on an SD model or with one speaker raises."""
    monkeypatch.setattr(pkg.recipe, "_train_cost", _torch_cost(pkg, []))
    n_in, units, n_out = T.CORPUS_NET
    torch.manual_seed(2)
    sat = pkg.training.AcousticModel(n_in, list(units), n_out, n_spkrs=3)
    sat.save(str(tmp_path / "sat.npz"), 10)
    jobs = [(a, b, 2) for a, b, _ in T.write_corpus(tmp_path)]
    common = dict(n_spkrs=3, keep_prob=1.0, optimizer="adam", learning_rate=0.01, batch_size=T.CORPUS_BATCH, seed=5,
                  log_interval=1, device="cpu", report=lambda s: None, updates=updates)
    pkg.recipe.train_files(jobs, str(tmp_path / "a0.npz"), n_in, units, n_out, n_steps=0, restore=str(tmp_path / "sat.npz"),
                           adapt=True, **common)
    before = {k: v.numpy() for k, v in sat.state_dict().items()}
    a0 = pkg.training.AcousticModel.load(str(tmp_path / "a0.npz"))
    assert a0.step == 10
    for k, v in a0.state_dict().items():
        if k.endswith("sd_weights"):
            mean = np.mean(before[k][:-1], 0)
            assert mean.dtype == np.float32 and (v.numpy()[-1] == mean).all() and (v.numpy()[:-1] == before[k][:-1]).all()
            assert (v.numpy()[-1] != before[k][-1]).any()
        else:
            assert (v.numpy() == before[k]).all()
    log = pkg.recipe.train_files(jobs, str(tmp_path / "a2.npz"), n_in, units, n_out, n_steps=2, restore=str(tmp_path / "sat.npz"),
                                 adapt=True, **common)
    assert [s for s, _ in log] == [10, 11]
    a2 = pkg.training.AcousticModel.load(str(tmp_path / "a2.npz"))
    for k, v in a2.state_dict().items():
        leaf = k.split(".")[-1]
        if leaf.startswith("si_"):
            assert v.numpy().tobytes() == before[k].tobytes(), k
        elif leaf.startswith("sd_"):
            assert (v.numpy()[-1] != a0.state_dict()[k].numpy()[-1]).any() and (v.numpy()[:-1] == before[k][:-1]).all()
        else:
            assert (v.numpy()[2] != before[k][2]).any() and (v.numpy()[:2] == before[k][:2]).all()
    with pytest.raises(ValueError):
        pkg.recipe.train_files(jobs, str(tmp_path / "x.npz"), n_in, units, n_out, n_steps=1, adapt=True, **common)
    sd = pkg.training.AcousticModel(n_in, list(units), n_out, n_spkrs=3, sat=False)
    sd.save(str(tmp_path / "sd.npz"), 1)
    with pytest.raises(ValueError):
        pkg.recipe.train_files(jobs, str(tmp_path / "x.npz"), n_in, units, n_out, n_steps=1, restore=str(tmp_path / "sd.npz"),
                               adapt=True, **common)
    one = pkg.training.AcousticModel(n_in, list(units), n_out, n_spkrs=1)
    one.save(str(tmp_path / "one.npz"), 1)
    with pytest.raises(ValueError):
        pkg.recipe.train_files([(a, b, 0) for a, b, _ in jobs], str(tmp_path / "x.npz"), n_in, units, n_out, n_steps=1,
                               restore=str(tmp_path / "one.npz"), adapt=True, **{**common, "n_spkrs": 1})

"""The optimiser step on the device (csrc/optim.hip, world.Context.optimizer_step, recipe.Tf1Optimizer, recipe.train_files
with updates="tf1") against tests/optimizer_reference.py.  The kernel's results are compared with the float32 twin
step32 BIT FOR BIT, as int32 views: the twin performs the table's operations one rounded numpy operation each, and so
must the kernel -- a contracted multiply-add or a division that is not the correctly rounded one shows as a differing
element.  tests/test_optimizer_host.py pins the twin itself."""
import ctypes as C

import numpy as np
import pytest

import dnn_train_reference as T
import optimizer_reference as O
import train_step_reference as S

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
_aligned = {}


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _place(torch, a, offset):
    """`a` on the device: a tensor of its own (16-byte aligned), or the slice [1 : 1 + n] of a buffer whose two ends hold
    SENTINEL (4-byte aligned only).  Returns (tensor, buffer or None)."""
    if not offset:
        t = torch.from_numpy(np.array(a, dtype=np.float32)).cuda()
        assert t.data_ptr() % 16 == 0
        return t, None
    buf = torch.full((a.size + 2,), SENTINEL, dtype=torch.float32, device="cuda")
    t = buf[1:1 + a.size]
    t.copy_(torch.from_numpy(np.array(a, dtype=np.float32)))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t, buf


def _device_run(gpu, rule, offset):
    """The STEPS steps of inputs() at rates() by Context.optimizer_step: (params, slots [slot][tensor], buffers)."""
    torch, W, ctx = gpu
    params, grads = O.inputs()
    bufs = []

    def put(a):
        t, b = _place(torch, a, offset)
        bufs.append(b)
        return t
    ps = [put(p) for p in params]
    slots = [[put(np.full(p.shape, v, dtype=np.float32)) for p in params] for v in O.SLOT_INIT[rule]]
    powers = O.initial_powers(np.float32)
    for gs in grads:
        g = [put(a) for a in gs]
        o = W.default_optimizer_option(rule, beta1_power=float(powers[0]), beta2_power=float(powers[1]))
        assert ctx.optimizer_step(o, ps, g, O.rates(), *slots) is None
        powers = O.advance_powers(powers, np.float32)
    torch.cuda.synchronize()
    return ps, slots, bufs


@pytest.mark.parametrize("rule", O.RULES)
def test_six_rules_bit_for_bit(gpu, rule):
    """Every rule on the shared inputs for 5 steps: p and the slots equal step32's bits, element by element."""
    ps, slots, _ = _device_run(gpu, rule, False)
    _aligned[rule] = ([_bits(p) for p in ps], [[_bits(t) for t in s] for s in slots])
    want_p, want_s, _ = O.reference(rule, np.float32)
    assert len(slots) == len(want_s) == len(O.SLOT_INIT[rule])
    for k, n in enumerate(O.SIZES):
        for what, got, want in [("p", ps[k], want_p[k])] + [("slot%d" % j, slots[j][k], want_s[j][k]) for j in range(len(slots))]:
            diff = np.nonzero(_bits(got) != _bits(want))[0]
            assert diff.size == 0, "%s: tensor of %d elements, %s: %d elements differ, the first at %d: %r against %r" % (
                rule, n, what, diff.size, diff[0], got.cpu().numpy()[diff[0]], want[diff[0]])
        if O.rates()[k] == 0.0:
            assert (_bits(ps[k]) == _bits(O.inputs()[0][k])).all()           # rate 0: p keeps its bits, the slots move
            assert all((_bits(s[k]) != _bits(np.float32(v))).any() for s, v in zip(slots, O.SLOT_INIT[rule]) if n >= 63)


@pytest.mark.parametrize("rule", O.RULES)
def test_placement_does_not_change_a_bit(gpu, rule):
    """Every tensor the slice [1 : 1 + n] of a buffer of n + 2: the element-by-element path.  The results are the aligned
    run's bits; no sentinel of param, slots or gradients is touched."""
    if rule not in _aligned:
        ps, slots, _ = _device_run(gpu, rule, False)
        _aligned[rule] = ([_bits(p) for p in ps], [[_bits(t) for t in s] for s in slots])
    ps, slots, bufs = _device_run(gpu, rule, True)
    for k in range(len(O.SIZES)):
        assert (_bits(ps[k]) == _aligned[rule][0][k]).all(), (rule, O.SIZES[k])
        for j in range(len(slots)):
            assert (_bits(slots[j][k]) == _aligned[rule][1][j][k]).all(), (rule, O.SIZES[k], j)
    assert len(bufs) == len(O.SIZES) * (1 + len(slots) + O.STEPS)
    ends = np.array([[float(b[0]), float(b[-1])] for b in bufs])
    assert (ends == SENTINEL).all()


def test_one_launch_for_all_tensors(gpu):
    """27 tensors (a SAT net of eight hidden layers has as many), 3 calls: 3 records of optimizer_step_kernel."""
    torch, W, ctx = gpu
    rng = np.random.default_rng(O.SEED + 1)
    sizes = [2 + 37 * k for k in range(27)]          # (element 0 of a gradient is one of the exact zeros)
    ps = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda() for n in sizes]
    gs = [torch.from_numpy(O.make_gradient(rng, n)).cuda() for n in sizes]
    m, v = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    before = [p.clone() for p in ps]
    ctx.timing_enable(True)
    try:
        for _ in range(3):
            ctx.optimizer_step(W.default_optimizer_option("adam"), ps, gs, [0.5] * 27, m, v)
        ms, launches = ctx.timing_query("optimizer_step_kernel")
    finally:
        ctx.timing_enable(False)
    assert launches == 3 and ms > 0.0
    assert all((p != q).any() for p, q in zip(ps, before))


def test_status_names_the_tensors_with_a_non_finite_gradient(gpu):
    torch, W, ctx = gpu
    rule = "adam"
    sizes = (5, 4099, 64, 257, 1023)
    params, grads = O.inputs(sizes, 1, O.SEED + 2)
    g = [np.array(a) for a in grads[0]]
    g[1][4097] = np.nan
    g[3][101] = -np.inf
    ps = [torch.from_numpy(np.array(p)).cuda() for p in params]
    slots = [[torch.zeros_like(p) for p in ps] for _ in range(2)]
    status = ctx.optimizer_step(W.default_optimizer_option(rule), ps, [torch.from_numpy(a).cuda() for a in g], O.rates(5), *slots,
                                want_status=True)
    assert status.dtype == torch.int32 and status.cpu().tolist() == [0, 1, 0, 1, 0]
    for k in (0, 2, 4):
        want, ws = O.step32(rule, params[k], g[k], O.initial_slots(rule, params[k], np.float32), O.rates(5)[k])
        assert (_bits(ps[k]) == _bits(want)).all() and all((_bits(slots[j][k]) == _bits(ws[j])).all() for j in range(2))
    # the update is applied as written: the bad element's parameter is not finite, its neighbours are the twin's
    want, _ = O.step32(rule, params[1], g[1], O.initial_slots(rule, params[1], np.float32), O.rates(5)[1])
    got = ps[1].cpu().numpy()
    assert np.isnan(got[4097]) and (np.delete(_bits(got), 4097) == np.delete(_bits(want), 4097)).all()
    # and a second call zeroes the status again
    status = ctx.optimizer_step(W.default_optimizer_option("sgd"), ps[:1], [torch.from_numpy(g[0]).cuda()], [0.5], want_status=True)
    assert status.cpu().tolist() == [0]


def test_refusals_leave_the_tensors_alone(gpu):
    """Every refusal of the header: WM_ERR_BAD_ARG, and not a bit of any tensor moves."""
    torch, W, ctx = gpu
    L = W.load_library()
    n = 3
    host = [np.arange(1, 9, dtype=np.float32) * (k + 1) for k in range(4 * n)]
    dev = [torch.from_numpy(a).cuda() for a in host]
    ptr = lambda ts: (C.c_void_p * len(ts))(*[t if t is None or isinstance(t, int) else t.data_ptr() for t in ts])
    P, G, A, B = dev[:n], dev[n:2 * n], dev[2 * n:3 * n], dev[3 * n:]
    cnt = lambda v: (C.c_int64 * len(v))(*v)
    rt = lambda v: (C.c_float * len(v))(*v)

    def opt(name, **over):
        o = W.default_optimizer_option(name)
        for k, v in over.items():
            setattr(o, k, v)
        return o
    status = torch.zeros(n, dtype=torch.int32, device="cuda")

    def call(o, k, p, g, a, b, c, r):
        return L.WorldMi355OptimizerStep(ctx.handle, C.byref(o) if o is not None else None, k, p, g, a, b, c, r, status.data_ptr())
    ok_c, ok_r = cnt([8] * n), rt([0.5] * n)
    many = 65
    cases = {
        "no tensors": (opt("adam"), 0, ptr(P), ptr(G), ptr(A), ptr(B), ok_c, ok_r),
        "65 tensors": (opt("sgd"), many, ptr(P * 22), ptr(G * 22), None, None, cnt([8] * 66), rt([0.5] * 66)),
        "rule -1": (opt("adam", rule=-1), n, ptr(P), ptr(G), ptr(A), ptr(B), ok_c, ok_r),
        "rule 6": (opt("adam", rule=6), n, ptr(P), ptr(G), ptr(A), ptr(B), ok_c, ok_r),
        "no option": (None, n, ptr(P), ptr(G), ptr(A), ptr(B), ok_c, ok_r),
        "no param": (opt("adam"), n, None, ptr(G), ptr(A), ptr(B), ok_c, ok_r),
        "no grad": (opt("adam"), n, ptr(P), None, ptr(A), ptr(B), ok_c, ok_r),
        "no count": (opt("adam"), n, ptr(P), ptr(G), ptr(A), ptr(B), None, ok_r),
        "no rate": (opt("adam"), n, ptr(P), ptr(G), ptr(A), ptr(B), ok_c, None),
        "momentum without slot0": (opt("momentum"), n, ptr(P), ptr(G), None, None, ok_c, ok_r),
        "rmsprop without slot0": (opt("rmsprop"), n, ptr(P), ptr(G), None, ptr(B), ok_c, ok_r),
        "adam without slot1": (opt("adam"), n, ptr(P), ptr(G), ptr(A), None, ok_c, ok_r),
        "adadelta without slot1": (opt("adadelta"), n, ptr(P), ptr(G), ptr(A), None, ok_c, ok_r),
        "a NULL param": (opt("sgd"), n, ptr([P[0], None, P[2]]), ptr(G), None, None, ok_c, ok_r),
        "a NULL grad": (opt("sgd"), n, ptr(P), ptr([G[0], G[1], None]), None, None, ok_c, ok_r),
        "a NULL slot0": (opt("adagrad"), n, ptr(P), ptr(G), ptr([None, A[1], A[2]]), None, ok_c, ok_r),
        "a NULL slot1": (opt("adam"), n, ptr(P), ptr(G), ptr(A), ptr([B[0], None, B[2]]), ok_c, ok_r),
        "count 0": (opt("sgd"), n, ptr(P), ptr(G), None, None, cnt([8, 0, 8]), ok_r),
        "count -1": (opt("sgd"), n, ptr(P), ptr(G), None, None, cnt([8, 8, -1]), ok_r),
        "a negative rate": (opt("sgd"), n, ptr(P), ptr(G), None, None, ok_c, rt([0.5, -1e-3, 0.5])),
        "a NaN rate": (opt("sgd"), n, ptr(P), ptr(G), None, None, ok_c, rt([float("nan"), 0.5, 0.5])),
        "an infinite rate": (opt("sgd"), n, ptr(P), ptr(G), None, None, ok_c, rt([0.5, 0.5, float("inf")])),
        "epsilon NaN": (opt("adam", epsilon=float("nan")), n, ptr(P), ptr(G), ptr(A), ptr(B), ok_c, ok_r),
        "rho infinite": (opt("rmsprop", rho=float("inf")), n, ptr(P), ptr(G), ptr(A), None, ok_c, ok_r),
        "momentum NaN": (opt("momentum", momentum=float("nan")), n, ptr(P), ptr(G), ptr(A), None, ok_c, ok_r),
        "beta1 infinite": (opt("adam", beta1=float("-inf")), n, ptr(P), ptr(G), ptr(A), ptr(B), ok_c, ok_r),
        "beta2 NaN": (opt("adam", beta2=float("nan")), n, ptr(P), ptr(G), ptr(A), ptr(B), ok_c, ok_r),
        "beta1_power 0": (opt("adam", beta1_power=0.0), n, ptr(P), ptr(G), ptr(A), ptr(B), ok_c, ok_r),
        "beta1_power 1": (opt("adam", beta1_power=1.0), n, ptr(P), ptr(G), ptr(A), ptr(B), ok_c, ok_r),
        "beta2_power 0": (opt("adam", beta2_power=0.0), n, ptr(P), ptr(G), ptr(A), ptr(B), ok_c, ok_r),
        "beta2_power 1": (opt("adam", beta2_power=1.0), n, ptr(P), ptr(G), ptr(A), ptr(B), ok_c, ok_r),
        "beta2_power NaN": (opt("adam", beta2_power=float("nan")), n, ptr(P), ptr(G), ptr(A), ptr(B), ok_c, ok_r),
    }
    for name, args in cases.items():
        assert call(*args) == 2, name                                         # WM_ERR_BAD_ARG
    assert L.WorldMi355OptimizerStep(None, C.byref(opt("sgd")), n, ptr(P), ptr(G), None, None, ok_c, ok_r, None) == 2
    torch.cuda.synchronize()
    for t, a in zip(dev, host):
        assert (_bits(t) == _bits(a)).all()
    # the binding's own: float32, cuda, contiguous, as many of each
    o = opt("adam")
    for bad in (lambda: ctx.optimizer_step(o, P, G, [0.5] * n, A),
                lambda: ctx.optimizer_step(o, P, G[:2], [0.5] * n, A, B),
                lambda: ctx.optimizer_step(o, P, G, [0.5] * 2, A, B),
                lambda: ctx.optimizer_step(o, P, [g.double() for g in G], [0.5] * n, A, B),
                lambda: ctx.optimizer_step(o, P, [g.cpu() for g in G], [0.5] * n, A, B),
                lambda: ctx.optimizer_step(o, P, G, [0.5] * n, A, [torch.zeros(16, device="cuda")[::2] for _ in B]),
                lambda: ctx.optimizer_step(o, P, G, [0.5] * n, A, [torch.zeros(7, device="cuda") for _ in B])):
        with pytest.raises(ValueError):
            bad()
    # the same arrays, accepted: the call itself works on them (the powers outside the open interval are adam's alone)
    assert call(opt("sgd", beta1_power=1.0), n, ptr(P), ptr(G), None, None, ok_c, ok_r) == 0
    torch.cuda.synchronize()
    assert all((_bits(t) != _bits(a)).any() for t, a in zip(P, host[:n])) and status.cpu().tolist() == [0] * n


# ---- through recipe.train_files ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("trajectory", [False, True], ids=["frame", "trajectory"])
def test_four_sgd_steps_by_the_librarys_update(gpu, pkg, tmp_path, trajectory):
    """test_gpu_train_step's loop with updates="tf1": the four logged costs and every saved parameter against
    train_step_reference.loop_reference, within FACTOR d32 per tensor, d32 from that module's float32 twin."""
    jobs, var_dir = S.write_loop_corpus(tmp_path, trajectory)
    cfg = S.LOOP_TRJ if trajectory else S.LOOP_FRAME
    n_in, units, n_out = S.LOOP_NET
    costs, params = S.loop_reference(jobs, pkg.recipe, trajectory)
    tcosts, tparams = S.loop_reference(jobs, pkg.recipe, trajectory, np.float32)
    path = str(tmp_path / "m.npz")
    extra = {"streams": S.LOOP_LAYOUT, "gv_weight": cfg["gv_weight"]} if trajectory else {}
    log = pkg.recipe.train_files(jobs, path, n_in, units, n_out, n_spkrs=2, variance_dir=var_dir, hidden_activation=S.HIDDEN,
                                 output_activation=S.OUTPUT, keep_prob=S.LOOP_KEEP, optimizer="sgd",
                                 learning_rate=cfg["learning_rate"], batch_size=cfg["batch_size"], n_steps=S.LOOP_STEPS,
                                 seed=S.LOOP_SEED, log_interval=1, report=lambda s: None, updates="tf1", **extra)
    assert [s for s, _ in log] == list(range(S.LOOP_STEPS))
    got = np.array([c for _, c in log])
    d = float(np.abs(np.array(tcosts) - costs).max() / np.abs(costs).max())
    worst = float(np.abs(got - costs).max() / (S.FACTOR * d * np.abs(costs).max()))
    print("loop costs: error / (8 d32) %.4f (d32 %.3e)" % (worst, d))
    m = pkg.training.AcousticModel.load(path)
    assert m.step == S.LOOP_STEPS and str(m.optimizer_state["rule"]) == "sgd"
    saved = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    assert set(saved) == set(params)
    for k in sorted(params):
        d = float(np.abs(tparams[k].astype(np.float64) - params[k]).max() / np.abs(params[k]).max())
        ratio = float(np.abs(saved[k].astype(np.float64) - params[k]).max() / (S.FACTOR * d * np.abs(params[k]).max()))
        print("loop %s: error / (8 d32) %.4f (d32 %.3e)" % (k, ratio, d))
        worst = max(worst, ratio)
    print("loop: worst error / (8 d32) %.4f" % worst)
    assert worst <= 1.0


@pytest.mark.parametrize("optimizer,trajectory", [("adam", False), ("rmsprop", False), ("adam", True)],
                         ids=["adam-frame", "rmsprop-frame", "adam-trajectory"])
def test_a_continued_run_writes_the_same_bytes(gpu, pkg, tmp_path, optimizer, trajectory):
    """keep_prob 0.5: 4 steps straight against 2 steps, a save and 2 more from restore -- the same bytes of the `.npz` (the
    parameters, the slots, the powers) and the same logged costs."""
    jobs, var_dir = S.write_loop_corpus(tmp_path, trajectory)
    cfg = S.LOOP_TRJ if trajectory else S.LOOP_FRAME
    n_in, units, n_out = S.LOOP_NET
    extra = {"streams": S.LOOP_LAYOUT, "gv_weight": cfg["gv_weight"]} if trajectory else {}

    def run(name, n_steps, restore=None):
        return pkg.recipe.train_files(jobs, str(tmp_path / name), n_in, units, n_out, n_spkrs=2, variance_dir=var_dir,
                                      hidden_activation=S.HIDDEN, output_activation=S.OUTPUT, keep_prob=0.5, optimizer=optimizer,
                                      learning_rate=0.01, batch_size=cfg["batch_size"], n_steps=n_steps, seed=S.LOOP_SEED,
                                      log_interval=1, report=lambda s: None, updates="tf1", restore=restore, **extra)
    log4 = run("four.npz", 4)
    log2 = run("two.npz", 2)
    log22 = run("two_two.npz", 2, str(tmp_path / "two.npz"))
    assert [s for s, _ in log4] == [0, 1, 2, 3] and np.isfinite([c for _, c in log4]).all()
    assert log2 + log22 == log4
    assert open(str(tmp_path / "two_two.npz"), "rb").read() == open(str(tmp_path / "four.npz"), "rb").read()
    with np.load(str(tmp_path / "four.npz")) as z:
        slots = [k for k in z.files if k.startswith("optimizer/slot")]
        assert len(slots) == len(O.SLOT_INIT[optimizer]) * 6 and str(z["optimizer/rule"]) == optimizer
        assert all((z[k] != O.SLOT_INIT[optimizer][int(k[len("optimizer/slot")])]).any() for k in slots)
        f = np.float32
        assert z["optimizer/beta2_power"] == f(f(f(f(f(0.999) * f(0.999)) * f(0.999)) * f(0.999)) * f(0.999))


def test_adapt_mode(gpu, pkg, tmp_path):
    """From a 3-speaker SAT model, adam, 3 steps on the last speaker's data: every si_ tensor is the restored file's, bit
    for bit; sd_weights[-1] started at the mean row and moved; the variances moved; dnn-forward runs on the result."""
    torch = gpu[0]
    n_in, units, n_out = T.CORPUS_NET
    torch.manual_seed(4)
    pkg.training.AcousticModel(n_in, list(units), n_out, n_spkrs=3).save(str(tmp_path / "sat.npz"), 12)
    with np.load(str(tmp_path / "sat.npz")) as z:
        before = {k: z[k] for k in z.files}
    jobs = [(a, b, 2) for a, b, _ in T.write_corpus(tmp_path)]
    lines = []
    log = pkg.recipe.train_files(jobs, str(tmp_path / "adapted.npz"), n_in, units, n_out, n_spkrs=3, keep_prob=0.5,
                                 optimizer="adam", learning_rate=0.01, batch_size=T.CORPUS_BATCH, n_steps=3, seed=5,
                                 log_interval=1, report=lines.append, updates="tf1", adapt=True, restore=str(tmp_path / "sat.npz"))
    assert [s for s, _ in log] == [12, 13, 14] and np.isfinite([c for _, c in log]).all()
    assert len([ln for ln in lines if "begins anew" in ln]) == 1
    with np.load(str(tmp_path / "adapted.npz")) as z:
        after = {k: z[k] for k in z.files}
    assert int(after["step"]) == 15
    for k in before:
        leaf = k.split(".")[-1]
        if leaf.startswith("si_"):
            assert after[k].tobytes() == before[k].tobytes(), k
            assert (after["optimizer/slot0/" + k] != 0).any() and (after["optimizer/slot1/" + k] != 0).any()
        elif leaf.startswith("sd_"):
            mean = np.mean(before[k][:-1], 0)
            assert (after[k][:-1] == before[k][:-1]).all() and (after[k][-1] != mean).any()
            # three Adam steps from the mean row: (1 - beta1) / sqrt(1 - beta2) = 3.16 rates bound one
            assert np.abs(after[k][-1] - mean).max() <= 3 * 0.01 * 3.2
            assert np.abs(before[k][-1] - mean).max() > 0.1
        elif leaf == "variances":
            assert (after[k][2] != before[k][2]).any() and (after[k][:2] == before[k][:2]).all()
    evals = pkg.recipe.forward_files([(a, b) for a, b, _ in jobs], str(tmp_path / "adapted.npz"), str(tmp_path / "gen"),
                                     report=lambda s: None)
    assert all(c is not None and np.isfinite(c) for c in evals)
    with pytest.raises(ValueError):
        pkg.recipe.train_files(jobs, str(tmp_path / "x.npz"), n_in, units, n_out, n_spkrs=3, n_steps=1, updates="tf1", adapt=True)

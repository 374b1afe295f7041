"""The training pass's host side: tests/dnn_train_reference.py (numpy float64) -- its Philox mask against the generator's
known answers, its gradients against torch autograd on training.AcousticModel.double() with the same masks injected, its
cost gradients against autograd of training.frame_cost, and its error bound on plain numpy float32 passes over every case
of the GPU tests; recipe.train_files' minibatches and learning-rate groups with the library call stubbed; the ABI
struct."""
import ctypes as C

import numpy as np
import pytest
import torch

import dnn_reference as R
import dnn_train_reference as T
from test_dnn_host import module_of

SEED = 20261019
ROWS = int(sum(R.LENGTHS))


def test_philox_known_answers():
    """Philox4x32-10 of Random123's kat_vectors: counter and key all zeros, and all ones."""
    hexes = lambda w: " ".join("%08x" % int(v) for v in w)
    z = np.uint64(0)
    assert hexes(T.philox4x32_10((z, z, z, z), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    f = np.uint64(0xffffffff)
    assert hexes(T.philox4x32_10((f, f, f, f), (0xffffffff, 0xffffffff))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"


def test_mask_keeps_its_share():
    """Seed 20261019, offset 0, layers 0 .. 3 of widths 129, 48, 130, 1 over 612 rows: the kept share is within three
    binomial deviations of p.  The mask depends on (seed, offset, layer, row, unit) alone."""
    worst = 0.0
    for p in (0.25, 0.5, 0.8):
        for layer, n in enumerate((129, 48, 130, 1)):
            m = T.mask(SEED, 0, layer, ROWS, n, p)
            assert m.shape == (ROWS, n) and m.dtype == bool
            dev = abs(m.mean() - p) / np.sqrt(p * (1 - p) / m.size)
            assert dev <= 3.0, (p, layer, dev)
            worst = max(worst, dev)
    print("kept share: worst %.2f deviations" % worst)
    a = T.mask(SEED, 0, 1, ROWS, 48, 0.5)
    assert (T.mask(SEED, 0, 1, ROWS, 130, 0.5)[:, :48] == a).all() and (T.mask(SEED, 0, 1, 40, 48, 0.5) == a[:40]).all()
    assert (T.mask(SEED, 1, 1, ROWS, 48, 0.5) != a).any() and (T.mask(SEED + (1 << 32), 0, 1, ROWS, 48, 0.5) != a).any()
    assert T.mask(SEED, 0, 0, 5, 7, 1.0).all()


def _autograd(pkg, params, x, rows, hidden, output, p, ms, G):
    """Gradients of sum(out * G) by torch autograd on the module in float64, the masks injected as tensors."""
    m = module_of(pkg, params, hidden, output).double()
    act = pkg.training._activate
    h = torch.from_numpy(np.array(x)).double()
    sr = torch.from_numpy(rows)
    p = float(np.float32(p))
    for i in range(len(m.units)):
        L = m.hidden(i)
        z = h @ L.si_weights + L.si_biases
        if m.sat:
            z = z + L.sd_weights[sr]
        h = act(hidden, z)
        if p < 1.0:
            h = h / p * torch.from_numpy(ms[i]).double()
    out = act(output, h @ m.output.si_weights + m.output.si_biases)
    (out * torch.from_numpy(np.array(G)).double()).sum().backward()
    return {k: v.grad.numpy() for k, v in m.named_parameters() if not k.startswith("variance.")}, out.detach().numpy()


def test_reference_gradients_agree_with_autograd(pkg):
    """SD and SAT, every activation, n_layers 0, keep_prob 1 and 0.8: every gradient within 1e-12 of its largest entry."""
    worst = 0.0
    for net, mode, hidden, output in R.all_cases():
        if mode == "sat_default":
            continue
        params, x, spkr, _, _ = R.cached_case(net, mode, hidden, output)
        rows = R.spkr_rows(R.LENGTHS, spkr if spkr is not None else [0] * len(R.LENGTHS))
        G = T.random_G(R.SEED + 900 + net, ROWS, R.NETS[net][2])
        for p in (1.0, 0.8):
            fw = T.train_forward(params, x, rows, hidden, output, p, SEED, 3)
            got, _ = T.backward(params, fw, G, rows, hidden, output)
            want, out = _autograd(pkg, params, x, rows, hidden, output, p, fw["masks"], G)
            assert np.abs(out - fw["out"]).max() <= 1e-12 * np.abs(out).max()
            assert set(got) == set(want)
            for k in want:
                scale = float(np.abs(want[k]).max())
                err = float(np.abs(got[k] - want[k]).max())
                assert err <= 1e-12 * scale, (net, mode, hidden, output, p, k, err, scale)
                worst = max(worst, err / scale if scale else 0.0)
    print("worst |reference - autograd| / max|autograd|: %.2e" % worst)


def test_cost_gradients_agree_with_autograd(pkg):
    params, x, spkr, out, _ = R.cached_case(0, "sat", "tanh", "linear")
    rng = np.random.default_rng(5)
    obs = (out + rng.standard_normal(out.shape)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(R.LENGTHS)])
    for u in (0, 4, 8):
        sl = slice(off[u], off[u + 1])
        var = params["variance.variances"][spkr[u]]
        o32 = out[sl].astype(np.float32)
        go, gv, S = T.cost_grads(o32, obs[sl], var)
        t = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)).double().requires_grad_(True)
        to, tv = t(o32), t(var)
        pkg.training.frame_cost(to, t(obs[sl]), tv).backward()
        assert np.abs(to.grad.numpy() - go).max() <= 1e-12 * np.abs(go).max()
        assert (np.abs(tv.grad.numpy() - gv) <= 1e-12 * S).all()


def test_bound_covers_a_float32_backward_pass():
    """Plain numpy float32 (its own summation order) over every case of the GPU tests at keep_prob 1 and 0.8."""
    worst = 0.0
    for net, mode, hidden, output in R.all_cases():
        params, x, spkr, _, _ = R.cached_case(net, mode, hidden, output)
        n_spkrs = params["variance.variances"].shape[0]
        rows = R.spkr_rows(R.LENGTHS, spkr if spkr is not None else [n_spkrs - 1] * len(R.LENGTHS))
        G = T.random_G(R.SEED + 900 + net, ROWS, R.NETS[net][2])
        for p in (1.0, 0.8):
            fw = T.train_forward(params, x, rows, hidden, output, p, SEED, 3)
            want, bound = T.backward(params, fw, G, rows, hidden, output)
            got = T.backward_f32(params, x, rows, hidden, output, p, fw["masks"], G)
            for k in want:
                err = np.abs(got[k].astype(np.float64) - want[k])
                ratio = float(np.where(err > 0, err / np.maximum(bound[k], 1e-300), 0.0).max())
                assert ratio <= 1.0, (net, mode, hidden, output, p, k, ratio)
                worst = max(worst, ratio)
    print("float32 backward: worst error / bound %.4f" % worst)


def test_exact_cases_stay_exact():
    """The GPU exact test's premise: sum |a| |b| < 2^24 for every product of the backward pass at keep_prob 1 and 0.5."""
    worst = 0.0
    for net in range(len(R.NETS)):
        for mode in R.MODES:
            for hidden in ("linear", "relu"):
                params, x, spkr, ref = R.exact_case(net, mode, hidden)
                n_spkrs = params["variance.variances"].shape[0]
                rows = R.spkr_rows(R.LENGTHS, spkr if spkr is not None else [n_spkrs - 1] * len(R.LENGTHS))
                for p in (1.0, 0.5):
                    fw = T.train_forward(params, x, rows, hidden, "linear", p, SEED, 3)
                    w = T.products_stay_exact(params, fw, T.exact_G(ROWS, ref.shape[1], 8), hidden, "linear")
                    if w >= 2.0 ** 24:
                        w = T.products_stay_exact(params, fw, T.exact_G(ROWS, ref.shape[1], 16), hidden, "linear")
                    assert w < 2.0 ** 24, (net, mode, hidden, p, w)
                    worst = max(worst, w)
    print("exact cases: worst sum |a||b| %.3g" % worst)


def test_dropout_struct_layout(pkg):
    """include/world_mi355.h: WorldMi355Dropout { float keep_prob; uint64_t seed; uint32_t offset; } on LP64."""
    D = pkg.world.Dropout
    assert C.sizeof(D) == 24 and D.keep_prob.offset == 0 and D.seed.offset == 8 and D.offset.offset == 16
    lib = pkg.load_library()
    assert hasattr(lib, "WorldMi355AcousticModelTrainForward") and hasattr(lib, "WorldMi355AcousticModelBackward")


# ---- recipe.train_files with the library call stubbed ---------------------------------------------------------------
def _torch_cost(pkg, calls):
    """recipe._train_cost in plain torch float32 on the CPU (keep_prob 1): the module's forward and frame_cost per
    pseudo-utterance, weighted by its share of the frames."""
    def cost(model, ctx, x, obs, lengths, spkrs, keep_prob, seed, step):
        calls.append((list(lengths), list(spkrs), step, tuple(x.shape)))
        rows = torch.repeat_interleave(torch.tensor(spkrs), torch.tensor(lengths))
        out = model(x, rows)
        off = np.concatenate([[0], np.cumsum(lengths)])
        total = 0.0
        for u, s in enumerate(spkrs):
            sl = slice(int(off[u]), int(off[u + 1]))
            total = total + pkg.training.frame_cost(out[sl], obs[sl], model.variance.variances[s]) * (lengths[u] / off[-1])
        return total
    return cost


def test_minibatches_group_frames_by_speaker(pkg):
    frame_spkr = np.repeat([0, 2, 1, 2], [33, 129, 257, 64])
    got = list(pkg.recipe.minibatches(frame_spkr, 128, 7, 11))
    assert len(got) == 7                                                 # 483 frames: three minibatches an epoch, the tail dropped
    for rows, lengths, spkrs in got:
        assert len(rows) == 128 == sum(lengths) and spkrs == sorted(set(spkrs)) and len(spkrs) == len(lengths)
        assert (np.repeat(spkrs, lengths) == frame_spkr[rows]).all()
    for e in (0, 3):                                                     # within an epoch no frame twice
        rows = np.concatenate([g[0] for g in got[e:e + 3]])
        assert len(set(rows.tolist())) == len(rows)
    again = list(pkg.recipe.minibatches(frame_spkr, 128, 7, 11))
    assert all((a[0] == b[0]).all() for a, b in zip(got, again))
    assert any((a[0] != b[0]).any() for a, b in zip(got, pkg.recipe.minibatches(frame_spkr, 128, 7, 12)))
    with pytest.raises(ValueError):
        next(pkg.recipe.minibatches(frame_spkr[:100], 128, 1, 0))


def test_utterance_minibatches_and_continuation(pkg):
    file_spkr = [0, 2, 1, 2, 0]
    got = list(pkg.recipe.utterance_minibatches(file_spkr, 2, 5, 4))
    assert len(got) == 5                                                 # five files: two minibatches an epoch
    for files, spkrs in got:
        assert len(files) == 2 and spkrs == sorted(spkrs) and spkrs == [file_spkr[i] for i in files]
    assert len(set(np.concatenate([g[0] for g in got[:2]]).tolist())) == 4
    # a continuation: steps 3 .. 4 of the same seed are the last two of steps 0 .. 4, for files and for frames
    tail = list(pkg.recipe.utterance_minibatches(file_spkr, 2, 2, 4, start=3))
    assert [f.tolist() for f, _ in tail] == [f.tolist() for f, _ in got[3:]]
    frame_spkr = np.repeat([0, 1], [40, 30])
    whole = list(pkg.recipe.minibatches(frame_spkr, 16, 9, 2))
    rest = list(pkg.recipe.minibatches(frame_spkr, 16, 4, 2, start=5))
    assert [r[0].tolist() for r in rest] == [r[0].tolist() for r in whole[5:]]


def test_optimizer_groups(pkg):
    m = pkg.training.AcousticModel(5, [4, 3], 2, n_spkrs=3)
    for name in pkg.recipe.OPTIMIZERS:
        opt = pkg.recipe.make_optimizer(m, name, 0.5)
        assert [g["lr"] for g in opt.param_groups] == [0.5, 0.5, 0.005]
        ids = [{id(p) for p in g["params"]} for g in opt.param_groups]
        named = dict(m.named_parameters())
        assert ids[0] == {id(p) for k, p in named.items() if ".si_" in k} and len(ids[0]) == 6
        assert ids[1] == {id(p) for k, p in named.items() if ".sd_" in k} and len(ids[1]) == 2
        assert ids[2] == {id(named["variance.variances"])}
    sd = pkg.training.AcousticModel(5, [4], 2)
    assert [g["lr"] for g in pkg.recipe.make_optimizer(sd, "sgd", 0.5).param_groups] == [0.5, 0.005]
    o = pkg.recipe.make_optimizer(m, "adagrad", 0.1)
    assert o.defaults["initial_accumulator_value"] == 0.1
    o = pkg.recipe.make_optimizer(m, "rmsprop", 0.1)
    assert o.defaults["alpha"] == 0.9 and o.defaults["eps"] == 1e-10
    with pytest.raises(ValueError):
        pkg.recipe.make_optimizer(m, "lbfgs", 0.1)


def test_train_files_loop_with_a_torch_step(pkg, tmp_path, monkeypatch):
    """The loop around the library call, the call replaced by torch float32 on the CPU: the log lines, the saved model,
    --restore, and that the GPU test's learning rate does lower the cost."""
    calls, lines = [], []
    monkeypatch.setattr(pkg.recipe, "_train_cost", _torch_cost(pkg, calls))
    jobs = T.write_corpus(tmp_path, 2)
    n_in, units, n_out = T.CORPUS_NET
    var_dir = tmp_path / "var"
    for s in range(2):
        (var_dir / str(s)).mkdir(parents=True)
        np.full(n_out, 0.5 + s, dtype=np.float32).tofile(str(var_dir / str(s) / "ffo.var"))
    path = str(tmp_path / "m.npz")
    log = pkg.recipe.train_files(jobs, path, n_in, units, n_out, n_spkrs=2, variance_dir=str(var_dir), keep_prob=1.0,
                                 optimizer="sgd", learning_rate=T.CORPUS_LR, batch_size=T.CORPUS_BATCH, n_steps=T.CORPUS_STEPS,
                                 seed=5, log_interval=5, device="cpu", report=lines.append)
    assert [s for s, _ in log] == [0, 5, 10, 15, 19] and lines[0] == "Step %7d: cost = %e" % log[0]
    assert log[-1][1] < log[0][1], log
    assert [c[2] for c in calls] == list(range(T.CORPUS_STEPS)) and all(c[1] == [0, 1] and sum(c[0]) == 128 for c in calls)
    m = pkg.training.AcousticModel.load(path)
    assert m.sat and m.units == [48] and abs(float(m.variance.variances[1, 0]) - 1.5) < 0.1
    more = pkg.recipe.train_files(jobs, str(tmp_path / "m2.npz"), n_in, units, n_out, n_spkrs=2, keep_prob=1.0, optimizer="sgd",
                                  learning_rate=T.CORPUS_LR, batch_size=T.CORPUS_BATCH, n_steps=3, seed=6, log_interval=1,
                                  restore=path, device="cpu", report=lines.append)
    assert more[0][1] < log[0][1] and [s for s, _ in more] == [20, 21, 22]       # the steps go on from the file's count
    assert [c[2] for c in calls[-3:]] == [20, 21, 22] and pkg.training.AcousticModel.load(str(tmp_path / "m2.npz")).step == 23
    whole = [r[0] for r in pkg.recipe.minibatches(np.repeat([0, 1, 0, 1], T.CORPUS_LENGTHS), T.CORPUS_BATCH, 23, 5)]
    assert m.step == 20 and len(whole) == 23
    with pytest.raises(ValueError):
        pkg.recipe.train_files(jobs, path, n_in, [7], n_out, n_spkrs=2, restore=path, device="cpu", n_steps=1)

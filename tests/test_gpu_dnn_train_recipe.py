"""recipe.train_files / the `dnn-train` verb on the library's training pass: a handful of generated `.ffi` / `.ffo` files
(dnn_train_reference.write_corpus), net 37 -> 48 -> 229, 20 SGD steps at keep_prob 1.  tests/test_dnn_train_host.py
confirms on the CPU, with the torch float32 path in the library call's place, that this learning rate lowers the cost."""
import numpy as np
import pytest

import dnn_train_reference as T

pytestmark = pytest.mark.gpu


def _train(pkg, scp, model, extra=()):
    lines = []
    import contextlib
    import io
    n_in, units, n_out = T.CORPUS_NET
    argv = ["dnn-train", "--scp", scp, "--model", model, "--inputs", str(n_in), "--outputs", str(n_out), "--units"] + \
        [str(n) for n in units] + ["--keep-prob", "1", "--optimizer", "sgd", "--learning-rate", str(T.CORPUS_LR), "--batch-size",
                                   str(T.CORPUS_BATCH), "--steps", str(T.CORPUS_STEPS), "--seed", "5", "--log-interval", "5"] + list(extra)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert pkg.recipe.main(argv) == 0
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("Step")]
    return [float(ln.split("cost = ")[1]) for ln in lines], lines


def test_dnn_train_writes_a_model_that_dnn_forward_accepts(gpu, pkg, tmp_path):
    jobs = T.write_corpus(tmp_path)
    scp = str(tmp_path / "train.scp")
    with open(scp, "w") as f:
        f.write("".join("%s %s\n" % (a, b) for a, b, _ in jobs))
    first = str(tmp_path / "a.npz")
    costs, lines = _train(pkg, scp, first)
    assert len(costs) == 5 and lines[0].startswith("Step       0: cost = ")
    assert np.isfinite(costs).all() and costs[-1] < costs[0], costs
    m = pkg.training.AcousticModel.load(first)
    assert (m.n_inputs, m.units, m.n_outputs, m.sat) == (37, [48], 229, False)
    again = str(tmp_path / "b.npz")
    costs2, _ = _train(pkg, scp, again)
    assert costs2 == costs and open(again, "rb").read() == open(first, "rb").read()      # the same seed: the same bytes
    out_dir = tmp_path / "gen"
    evals = pkg.recipe.forward_files([(a, b) for a, b, _ in jobs], first, str(out_dir), report=lambda s: None)
    assert all(c is not None and np.isfinite(c) for c in evals)
    assert np.fromfile(str(out_dir / "u0.ffo"), dtype=np.float32).shape == (T.CORPUS_LENGTHS[0] * 229,)
    more = str(tmp_path / "c.npz")
    costs3, lines3 = _train(pkg, scp, more, ["--restore", first])
    assert lines3[0].startswith("Step      20: cost = ") and lines3[-1].startswith("Step      39: cost = ")
    assert costs3[0] < costs[0] and open(more, "rb").read() != open(first, "rb").read()
    assert pkg.training.AcousticModel.load(first).step == 20 and pkg.training.AcousticModel.load(more).step == 40


def test_dnn_train_sat_with_dropout(gpu, pkg, tmp_path):
    """Two speakers, keep_prob 0.5, Adam: the loop runs on the library's masks and returns finite costs."""
    jobs = T.write_corpus(tmp_path, 2)
    n_in, units, n_out = T.CORPUS_NET
    log = pkg.recipe.train_files(jobs, str(tmp_path / "sat.npz"), n_in, units, n_out, n_spkrs=2, keep_prob=0.5, optimizer="adam",
                                 learning_rate=0.01, batch_size=T.CORPUS_BATCH, n_steps=6, seed=3, log_interval=1,
                                 report=lambda s: None)
    assert len(log) == 6 and np.isfinite([c for _, c in log]).all()
    m = pkg.training.AcousticModel.load(str(tmp_path / "sat.npz"))
    assert m.sat and m.n_spkrs == 2


def test_dnn_train_trajectory_mode(gpu, pkg, tmp_path):
    """--stream: minibatches of utterances, DNNDefine.trajectory_cost on the recipe's layout (229 columns), two speakers
    with their own ffo.var and gv.var; the same seed writes the same bytes."""
    import mlpg_reference as M
    jobs = T.write_corpus(tmp_path, 2)
    n_in, units, n_out = T.CORPUS_NET
    var_dir = tmp_path / "var"
    for s in range(2):
        (var_dir / str(s)).mkdir(parents=True)
        np.full(n_out, 1.0 + s, dtype=np.float32).tofile(str(var_dir / str(s) / "ffo.var"))
        np.full(76, 2.0 + s, dtype=np.float32).tofile(str(var_dir / str(s) / "gv.var"))
    streams = [(50, M.RECIPE, False), (1, M.RECIPE, True), (25, M.RECIPE, False)]
    runs = []
    for name in ("t0.npz", "t1.npz"):
        log = pkg.recipe.train_files(jobs, str(tmp_path / name), n_in, units, n_out, n_spkrs=2, variance_dir=str(var_dir),
                                     keep_prob=0.5, optimizer="sgd", learning_rate=0.5, batch_size=3, n_steps=6, seed=9,
                                     log_interval=1, streams=streams, report=lambda s: None)
        runs.append(log)
    assert [s for s, _ in runs[0]] == list(range(6)) and np.isfinite([c for _, c in runs[0]]).all()
    assert runs[0] == runs[1] and open(str(tmp_path / "t0.npz"), "rb").read() == open(str(tmp_path / "t1.npz"), "rb").read()
    m = pkg.training.AcousticModel.load(str(tmp_path / "t0.npz"))
    assert m.step == 6 and m.sat
    fresh = pkg.training.AcousticModel(n_in, list(units), n_out, 2)
    v = m.variance.variances.detach().numpy()
    assert (v[0] != 1.0).any() and (v[1] != 2.0).any() and abs(v[1, 0] - 2.0) < 0.5        # started from ffo.var, and trained
    assert fresh.hidden0.sd_weights.shape == m.hidden0.sd_weights.shape
    with pytest.raises(ValueError):                                      # the streams must make the rows
        pkg.recipe.train_files(jobs, str(tmp_path / "x.npz"), n_in, units, n_out, n_spkrs=2, n_steps=1, batch_size=2,
                               streams=streams[:2])

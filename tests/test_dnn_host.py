"""The acoustic model's host side: tests/dnn_reference.py (numpy float64) against training.AcousticModel.double(), two
independent statements of DNNDefine.inference and DNNDefine.cost; the `.npz` interchange file; forward_files' size check
and scp parsing; and the error bound of dnn_reference on plain numpy float32 passes over every case of the GPU tests."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dnn_reference as R


def module_of(pkg, params, hidden, output):
    """training.AcousticModel holding `params` (float32 numpy, the reference's names)."""
    n = R.n_layers(params)
    units = [params["hidden%d.si_weights" % i].shape[1] for i in range(n)]
    wo = params["output.si_weights"]
    n_in = params["hidden0.si_weights"].shape[0] if n else wo.shape[0]
    m = pkg.training.AcousticModel(n_in, units, wo.shape[1], params["variance.variances"].shape[0], hidden, output,
                                   sat="hidden0.sd_weights" in params)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
    return m


def test_parameter_names_and_initialisation(pkg):
    torch.manual_seed(3)
    m = pkg.training.AcousticModel(400, [300, 200], 229, n_spkrs=4)
    names = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert names == {"hidden0.si_weights": (400, 300), "hidden0.si_biases": (300,), "hidden0.sd_weights": (4, 300),
                     "hidden1.si_weights": (300, 200), "hidden1.si_biases": (200,), "hidden1.sd_weights": (4, 200),
                     "output.si_weights": (200, 229), "output.si_biases": (229,), "variance.variances": (4, 229)}
    for name, fan in (("hidden0.si_weights", 400), ("hidden1.si_weights", 300), ("output.si_weights", 200),
                      ("hidden0.sd_weights", 4)):
        w, std = m.state_dict()[name].numpy(), 1.0 / np.sqrt(fan)
        assert np.abs(w).max() <= 2.0 * std                              # truncated at two deviations
        if w.size > 10000:                                               # a truncated normal's deviation is 0.88 std
            assert 0.8 * std < w.std() < 0.95 * std and abs(w.mean()) < 0.02 * std
    assert all((m.state_dict()[k] == 0).all() for k in names if k.endswith("si_biases"))
    assert (m.state_dict()["variance.variances"] == 1).all()
    sd = pkg.training.AcousticModel(5, [], 3)                            # one speaker: SD mode, no speaker rows
    assert set(sd.state_dict()) == {"output.si_weights", "output.si_biases", "variance.variances"}


def test_reference_agrees_with_the_module(pkg):
    """SD and SAT, every activation, n_layers 0, on every case of the GPU tests: every element within 1e-12 of the
    case's largest |output| -- relative to that scale, not per element (a linear output near zero is a cancelled sum,
    and two float64 summation orders differ there by rounding of the terms, not of the result)."""
    worst = 0.0
    for net, mode, hidden, output in R.all_cases():
        params, x, spkr, out, _ = R.cached_case(net, mode, hidden, output)
        m = module_of(pkg, params, hidden, output).double()
        rows = None if spkr is None else torch.from_numpy(R.spkr_rows(R.LENGTHS, spkr))
        with torch.no_grad():
            got = m(torch.from_numpy(np.array(x)).double(), rows).numpy()
        scale = float(np.abs(out).max())                                 # relative to the case's largest output
        assert np.abs(got - out).max() <= 1e-12 * scale, (net, mode, hidden, output)
        worst = max(worst, float(np.abs(got - out).max()) / scale)
    print("worst |module - reference| / max|reference|: %.2e" % worst)


def test_cost_agrees_with_the_module(pkg):
    params, x, spkr, out, _ = R.cached_case(0, "sat", "tanh", "linear")
    rng = np.random.default_rng(5)
    obs = (out + rng.standard_normal(out.shape)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(R.LENGTHS)])
    for u in (0, 4, 8):
        sl = slice(off[u], off[u + 1])
        var = params["variance.variances"][spkr[u]]
        c, S = R.cost(out[sl].astype(np.float32), obs[sl], var)
        t = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)).double()
        got = float(pkg.training.frame_cost(t(out[sl].astype(np.float32)), t(obs[sl]), t(var)))
        assert abs(got - c) <= 1e-12 * S


def test_npz_round_trip(pkg, tmp_path):
    params, _, _, _, _ = R.cached_case(0, "sat", "relu", "sigmoid")
    m = module_of(pkg, params, "relu", "sigmoid")
    path = str(tmp_path / "model.npz")
    m.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == set(params) | {"hidden_activation", "output_activation"}
        for k, v in params.items():
            assert z[k].dtype == np.float32 and z[k].tobytes() == v.tobytes(), k
        assert str(z["hidden_activation"]) == "relu" and str(z["output_activation"]) == "sigmoid"
    back = pkg.training.AcousticModel.load(path)
    assert (back.hidden_activation, back.output_activation, back.sat, back.n_spkrs) == ("relu", "sigmoid", True, R.N_SPKRS)
    assert (back.n_inputs, back.units, back.n_outputs) == (37, [48, 130], 229)
    for k, v in back.state_dict().items():
        assert v.numpy().tobytes() == params[k].tobytes(), k
    sd = module_of(pkg, R.cached_case(2, "sd", "linear", "linear")[0], "linear", "linear")
    sd.save(path)
    back = pkg.training.AcousticModel.load(path)
    assert (back.units, back.sat, back.n_inputs, back.n_outputs) == ([], False, 3, 33)


def test_scp_parsing(pkg, tmp_path):
    scp = tmp_path / "jobs.scp"
    scp.write_text("/a/b/x1.ffi /c/x1.ffo\n/a/b/x2.ffi\n\n/a/b/x3.ffi   /c/x3.ffo  \n")
    assert pkg.recipe.read_forward_scp(str(scp)) == [("/a/b/x1.ffi", "/c/x1.ffo"), ("/a/b/x2.ffi", None),
                                                     ("/a/b/x3.ffi", "/c/x3.ffo")]


def test_forward_files_size_check(pkg, tmp_path):
    """A file that is no whole number of rows, or targets of another length, is an error that names the file -- raised
    before any device is touched."""
    module_of(pkg, R.cached_case(2, "sd", "linear", "linear")[0], "linear", "linear").save(str(tmp_path / "m.npz"))
    bad = tmp_path / "bad.ffi"
    np.zeros(3 * 4 + 1, dtype=np.float32).tofile(str(bad))
    with pytest.raises(ValueError, match="bad.ffi"):
        pkg.recipe.forward_files([(str(bad), None)], str(tmp_path / "m.npz"), str(tmp_path / "out"))
    good, short = tmp_path / "good.ffi", tmp_path / "short.ffo"
    np.zeros(3 * 4, dtype=np.float32).tofile(str(good))
    np.zeros(33 * 3, dtype=np.float32).tofile(str(short))
    with pytest.raises(ValueError, match="short.ffo"):
        pkg.recipe.forward_files([(str(good), str(short))], str(tmp_path / "m.npz"), str(tmp_path / "out"))


def test_exact_cases_stay_in_the_integers():
    """The exact test's ranges: every partial sum below 2^24 (asserted inside exact_case), and a plain float32 pass
    reproduces the float64 integers bit for bit."""
    for net in range(len(R.NETS)):
        for mode in R.MODES:
            for hidden in ("linear", "relu"):
                p, x, spkr, out = R.exact_case(net, mode, hidden)
                rows = R.spkr_rows(R.LENGTHS, spkr if spkr is not None else [p["variance.variances"].shape[0] - 1] * len(R.LENGTHS))
                got = R.forward_f32(p, x, rows, hidden, "linear")
                assert got.tobytes() == out.astype(np.float32).tobytes()
                assert (out == np.round(out)).all() and np.abs(out).max() > 0


def test_bound_covers_a_float32_pass():
    """Every GPU case, and 65 -> 2048 -> 33 on 65 rows: |float32 pass - reference| <= e everywhere."""
    worst = 0.0
    for net, mode, hidden, output in R.all_cases():
        params, x, spkr, out, e = R.cached_case(net, mode, hidden, output)
        n_spkrs = params["variance.variances"].shape[0]
        rows = R.spkr_rows(R.LENGTHS, spkr if spkr is not None else [n_spkrs - 1] * len(R.LENGTHS))
        got = R.forward_f32(params, x, rows, hidden, output).astype(np.float64)
        ratio = float((np.abs(got - out) / e).max())
        assert ratio <= 1.0, (net, mode, hidden, output, ratio)
        worst = max(worst, ratio)
    params = R.make_model(R.SEED + 9, 65, (2048,), 33)
    x = R.make_inputs(R.SEED + 10, 65, 65)
    for hidden in R.ACTIVATIONS:
        out, e = R.forward(params, x, np.zeros(65, dtype=np.int64), hidden, "linear")
        got = R.forward_f32(params, x, np.zeros(65, dtype=np.int64), hidden, "linear").astype(np.float64)
        ratio = float((np.abs(got - out) / e).max())
        assert ratio <= 1.0, (hidden, ratio)
        worst = max(worst, ratio)
    print("worst float32 error / bound: %.3f" % worst)


def test_abi_struct_matches_the_header(pkg):
    """The ctypes mirror of WorldMi355AcousticModel: field order and the size of the C struct on this ABI."""
    D = pkg.world.AcousticModelDesc
    assert [f[0] for f in D._fields_] == ["n_layers", "n_inputs", "n_outputs", "n_spkrs", "hidden_activation",
                                          "output_activation", "units", "weights", "biases", "spkr_weights", "variances",
                                          "max_chunk_frames"]
    assert C.sizeof(D) == 6 * 4 + 5 * 8 + 8 and D.units.offset == 24 and D.max_chunk_frames.offset == 64
    assert pkg.world.ACTIVATIONS == R.ACTIVATIONS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "world_mi355.h")).read()
    assert "WorldMi355AcousticModelForward" in header and '"dnn_layer_kernel"' in header and '"dnn_cost_kernel"' in header

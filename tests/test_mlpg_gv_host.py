"""Parameter generation considering global variance: what can be checked without a GPU.  The ABI is declared, exported,
has the recipe's defaults and refuses its arguments before any device call; recipe.gv_pdf_files and the mask built from
labels are held to numpy; the numpy statement the GPU tests are held to (tests/gv_reference.py) is checked against the
dense statement of tests/mlpg_reference.py and against its own properties."""
import ctypes
import os
import re

import numpy as np
import pytest

import gv_reference as G
import mlpg_reference as M
from conftest import ROOT


def test_abi_declared_exported_with_defaults(pkg):
    text = open(os.path.join(ROOT, "include", "world_mi355.h")).read()
    assert re.search(r"\bint\s+WorldMi355ParameterGenerationGv\s*\(", text)
    assert re.search(r"\bvoid\s+WorldMi355DefaultGvOption\s*\(", text)
    assert "Training.pl:1892-1903" in text and '"mlpg_gv_kernel"' in text
    lib = pkg.load_library()
    o = pkg.world.GvOption(7, 7, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0)
    lib.WorldMi355DefaultGvOption(ctypes.byref(o))
    assert (o.max_iter, o.scale, o.epsilon, o.step_init, o.step_inc, o.step_dec, o.hmm_weight, o.gv_weight) == \
        (50, 1, 1e-4, 1.0, 1.2, 0.5, 1.0, 1.0)                                   # configure.ac:808-880
    O = pkg.world.GvOption
    assert ctypes.sizeof(O) == 56 and (O.max_iter.offset, O.scale.offset, O.epsilon.offset, O.gv_weight.offset) == (0, 4, 8, 48)
    lib.WorldMi355DefaultGvOption(None)                                          # a null option struct is left alone
    for name in ("gv_pdf_files", "gen_param_gv_files", "gv_label_mask"):
        assert hasattr(pkg.recipe, name), name
    assert hasattr(pkg.world.WorldBatch, "parameter_generation_gv")
    assert "mlpg_gv.hip" in open(os.path.join(ROOT, "hts-train-world_amd", "csrc", "Makefile")).read()


def _call(pkg, drop=(), gv_over=None, n=1):
    """A complete argument set over host memory (never dereferenced: the batch is NULL or the set is refused first)."""
    lib = pkg.load_library()
    dp = ctypes.POINTER(ctypes.c_double)
    buf = (ctypes.c_float * 64)()
    ptrs = lambda: (ctypes.c_void_p * n)(*[ctypes.addressof(buf)] * n)
    arrs = [(ctypes.c_double * len(w))(*w) for w in M.RECIPE]
    pa = (dp * 3)(*[ctypes.cast(a, dp) for a in arrs])
    sz = (ctypes.c_int * 3)(1, 3, 3)
    wptrs, sptrs = (ctypes.POINTER(dp) * n)(), (ctypes.POINTER(ctypes.c_int) * n)()
    for s in range(n):
        wptrs[s], sptrs[s] = ctypes.cast(pa, ctypes.POINTER(dp)), ctypes.cast(sz, ctypes.POINTER(ctypes.c_int))
    a = {"mean": ptrs(), "var": ptrs(), "dims": (ctypes.c_int * n)(*[2] * n), "n_windows": (ctypes.c_int * n)(*[3] * n),
         "windows": wptrs, "window_sizes": sptrs, "gv_mean": ptrs(), "gv_var": ptrs(), "out": ptrs()}
    o, g = pkg.world.MlpgOption(), pkg.world.GvOption()
    lib.WorldMi355DefaultMlpgOption(ctypes.byref(o))
    lib.WorldMi355DefaultGvOption(ctypes.byref(g))
    for k, v in (gv_over or {}).items():
        setattr(g, k, v)
    a["opt"], a["gv"] = ctypes.byref(o), ctypes.byref(g)
    for name in drop:
        a[name] = None
    return lib.WorldMi355ParameterGenerationGv(None, n, a["mean"], 6, a["var"], 0, a["dims"], a["n_windows"], a["windows"],
                                               a["window_sizes"], None, a["opt"], a["gv_mean"], a["gv_var"], None, a["gv"],
                                               a["out"], None, None)


@pytest.mark.parametrize("what", [dict(), dict(drop=("mean",)), dict(drop=("var",)), dict(drop=("gv_mean",)),
                                  dict(drop=("gv_var",)), dict(drop=("gv",)), dict(drop=("opt",)), dict(drop=("out",)),
                                  dict(drop=("windows",)), dict(gv_over=dict(max_iter=-1)), dict(gv_over=dict(scale=2)),
                                  dict(gv_over=dict(epsilon=-1e-4)), dict(gv_over=dict(step_init=0.0)),
                                  dict(gv_over=dict(step_inc=float("nan"))), dict(gv_over=dict(step_dec=float("inf"))),
                                  dict(gv_over=dict(hmm_weight=0.0)), dict(gv_over=dict(gv_weight=-1.0))],
                         ids=["null_batch", "mean", "var", "gv_mean", "gv_var", "gv_option", "mlpg_option", "out", "windows",
                              "max_iter", "scale", "epsilon", "step_init", "step_inc", "step_dec", "hmm_weight", "gv_weight"])
def test_refusals_return_bad_argument_without_a_device(pkg, what):
    assert _call(pkg, **what) == 2                                               # WM_ERR_BAD_ARG


def test_gv_pdf_files_against_numpy(pkg, tmp_path):
    rng = np.random.default_rng(3)
    x = (10.0 ** rng.uniform(-3, 1, (9, 7))).astype(np.float32)
    paths = []
    for k, row in enumerate(x):
        paths.append(str(tmp_path / ("u%d.cmp" % k)))
        with open(paths[-1], "wb") as f:
            f.write(pkg.world.htk_header(1, 48000, 240, 4 * 7, 9))
            f.write(row.tobytes())
    assert pkg.recipe.gv_pdf_files(paths, str(tmp_path / "gv")) == 9
    x64 = x.astype(np.float64)
    mean, var = np.fromfile(tmp_path / "gv" / "gv.mean", np.float32), np.fromfile(tmp_path / "gv" / "gv.var", np.float32)
    assert mean.tobytes() == x64.mean(axis=0).astype(np.float32).tobytes()
    assert var.tobytes() == x64.var(axis=0).astype(np.float32).tobytes()        # ddof 0: divides by n, as stats_files
    with open(paths[3], "ab") as f:
        f.write(b"\0\0\0\0")
    with pytest.raises(ValueError, match="holds 8 values"):
        pkg.recipe.gv_pdf_files(paths, str(tmp_path / "gv"))
    with pytest.raises(ValueError, match="no file"):
        pkg.recipe.gv_pdf_files([], str(tmp_path / "gv"))


def test_mask_from_labels(pkg):
    lines = ["0 125000 x-sil+a\n", "125000 275000 sil-a+b\n", "275000 325000 a-pau+b\n", "325000 475000 a-b+sil\n",
             "475000 600000 b-sil+x\n"]                    # boundaries at half frames of 5 ms
    mask = pkg.recipe.gv_label_mask(lines, 0.005, 12, ("x-sil+a", "a-pau+b", "b-sil+x"))
    want = np.zeros(12, dtype=np.uint8)
    want[2:6] = 1                                      # 12.5 ms .. 27.5 ms: frames 2 .. 5, both ends inclusive
    want[6:10] = 1                                     # 32.5 ms .. 47.5 ms: frames 6 .. 9
    assert mask.dtype == np.uint8 and (mask == want).all()
    rows = pkg.recipe.mspf_label_rows(lines, 0.005, 12, ("x-sil+a", "a-pau+b", "b-sil+x"))
    assert set(np.nonzero(mask)[0]) == set(rows.tolist())
    assert (pkg.recipe.gv_label_mask(lines, 0.005, 12) == np.array([1] * 12, dtype=np.uint8)).all()
    assert pkg.recipe.gv_label_mask(lines, 0.005, 9, ("sil-a+b",)).tolist() == [1, 1, 1, 0, 0, 1, 1, 1, 1]


def test_unknown_options_are_refused_on_the_host(pkg, tmp_path):
    with pytest.raises(TypeError, match="unknown option steps"):
        pkg.recipe.gen_param_gv_files([], [(1, [[1.0]], False)], "v", "m", "g", steps=3)
    with pytest.raises(ValueError, match="unknown option steps"):
        pkg.generate._Setup._gv(("gv", np.ones(2), np.ones(2), {"steps": 3}), [2])
    with pytest.raises(ValueError, match="holds 3 values"):
        pkg.generate._Setup._gv(("gv", np.ones(3), np.ones(2), None), [2])
    (kind, options), rows = pkg.generate._Setup._gv(("gv", np.arange(3.0), np.ones(3), {"max_iter": 5}), [2, 1])
    assert kind == "gv" and options == {"max_iter": 5} and rows[1][0].tolist() == [2.0] and rows[0][1].tolist() == [1.0, 1.0]
    assert pkg.generate.flagged_stage(pkg.generate.status_word([0], [0], [4], [0])[0]) is None
    assert pkg.generate.flagged_stage(pkg.generate.status_word([0], [0], [5], [0])[0]) == ("mlpg", 1)


@pytest.mark.parametrize("edge", [0, 1])
@pytest.mark.parametrize("name", ["recipe", "five", "static"])
def test_helper_bands_are_the_dense_matrix(name, edge):
    wins = M.WINDOW_SETS[name]
    B = 2 * max((len(w) - 1) // 2 for w in wins)
    for T in (1, 2, 3, 7, 33):
        for vpf in (False, True):
            mean, var = M.make_stream(T, [T], 2, wins, vpf)
            Rb, r = G.normal_bands(mean, var, wins, edge, 0, np.float64)
            W = M.window_matrix(T, wins, edge)
            prec = np.broadcast_to(M.precisions(var), mean.shape)
            for d in range(2):
                R, WtP = M.normal_matrix(W, np.ascontiguousarray(prec[:, d::2]).reshape(-1))
                dense = np.zeros((T, T))
                for j in range(-B, B + 1):
                    for t in range(max(0, -j), min(T, T - j)):
                        dense[t, t + j] = Rb[B + j, t, d]
                np.testing.assert_allclose(dense, R, rtol=1e-13, atol=1e-13 * np.abs(R).max())
                np.testing.assert_allclose(r[:, d], WtP @ mean.astype(np.float64)[:, d::2].reshape(-1), rtol=1e-12, atol=1e-12)
                x = np.random.default_rng(T).standard_normal((T, 2))
                np.testing.assert_allclose(G.band_times(Rb, x)[:, d], R @ x[:, d], rtol=1e-12, atol=1e-12 * np.abs(R).max())


def _column_case(T, seed, dtype=np.float64, **options):
    mean, var = M.make_stream(seed, [T], 3, M.RECIPE)
    c0 = M.mlpg(mean, var, M.RECIPE, want_cond=False)[0].astype(np.float32)
    member = np.arange(T) % 5 != 2
    gm = (3.0 * G.variance_over(c0, member) + 0.01).astype(np.float32)
    Rb, r = G.normal_bands(mean, var, M.RECIPE, 0, 0, dtype)
    return c0, member, G.generate(c0, Rb, r, 3, member, gm, (0.2 * gm) ** 2, dtype, **options)


@pytest.mark.parametrize("T", [3, 7, 33, 200])
def test_helper_never_loses_likelihood_over_an_accept(T):
    """f after k trials is f after k - 1 trials or larger, for every k: a rejected trial changes nothing."""
    last = None
    for k in (0, 1, 2, 5, 20, 50):
        _, _, res = _column_case(T, 40 + T, max_iter=k, epsilon=0.0)
        assert (res["trials"] == k).all() and (res["accepts"] <= k).all() and (res["f1"] >= res["f0"]).all()
        if last is not None:
            assert (res["f1"] >= last).all()
        last = res["f1"]
    assert (res["accepts"] > 0).all()
    _, _, short = _column_case(T, 40 + T, step_init=1e6, max_iter=3, epsilon=0.0)     # a step that overshoots is rejected
    assert (short["accepts"] < 3).any() and (short["f1"] >= short["f0"]).all()


def test_helper_without_trials_and_scaling_returns_the_start():
    c0, member, res = _column_case(33, 9, max_iter=0, scale=0)
    assert G.finish(res["c"], None, 0.0).tobytes() == c0.tobytes()
    voiced = np.arange(33) % 4 != 0
    out = G.finish(res["c"], voiced, -1e10)
    assert (out[~voiced] == np.float32(-1e10)).all() and (out[voiced] == c0[voiced]).all()
    _, _, scaled = _column_case(33, 9, max_iter=0, scale=1)
    assert (scaled["c"][~member] == c0[~member]).all()                           # scaling moves the GV frames alone
    gm = (3.0 * G.variance_over(c0, member) + 0.01).astype(np.float32)
    np.testing.assert_allclose(G.variance_over(scaled["c"], member), gm.astype(np.float64), rtol=1e-12)


def test_helper_status_and_double_against_long_double():
    """N < 2 and a gv_var that is not positive return the start with 4 and 1; float64 and long double agree on the
    trial counts at the stop rule on these columns."""
    mean, var = M.make_stream(2, [7], 2, M.RECIPE)
    c0 = M.mlpg(mean, var, M.RECIPE, want_cond=False)[0].astype(np.float32)
    Rb, r = G.normal_bands(mean, var, M.RECIPE, 0, 0, np.float64)
    one = np.zeros(7, dtype=bool)
    one[3] = True
    res = G.generate(c0, Rb, r, 3, one, np.ones(2), np.ones(2))
    assert (res["status"] == 4).all() and (res["trials"] == 0).all() and (res["c"] == c0).all()
    res = G.generate(c0, Rb, r, 3, np.ones(7, bool), np.ones(2), np.array([0.0, 1.0]))
    assert res["status"].tolist() == [1, 0] and (res["c"][:, 0] == c0[:, 0]).all() and (res["c"][:, 1] != c0[:, 1]).any()
    for T in (7, 33, 200):
        _, _, a = _column_case(T, 70 + T)
        _, _, b = _column_case(T, 70 + T, dtype=np.longdouble)
        assert (a["trials"] == b["trials"]).all() and (a["accepts"] == b["accepts"]).all()
        assert np.abs(a["c"] - b["c"].astype(np.float64)).max() < 1e-9 * np.abs(a["c"]).max()

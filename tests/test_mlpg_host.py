"""Parameter generation (SPTK `mlpg`, scripts/Training.pl:2755-2810): what can be checked without a GPU.  The ABI is
declared, exported, has its defaults and refuses null arguments before any device call; the dense numpy statement of
tests/mlpg_reference.py, which the GPU tests are held to, is checked against itself."""
import ctypes
import os
import re

import numpy as np
import pytest

import mlpg_reference as ref
from conftest import ROOT


def test_abi_declared_exported_with_defaults(pkg):
    text = open(os.path.join(ROOT, "include", "world_mi355.h")).read()
    assert re.search(r"\bint\s+WorldMi355ParameterGeneration\s*\(", text)
    assert re.search(r"\bvoid\s+WorldMi355DefaultMlpgOption\s*\(", text)
    assert "Training.pl:2755-2810" in text and '"mlpg_kernel"' in text
    lib = pkg.load_library()
    assert hasattr(lib, "WorldMi355ParameterGeneration") and hasattr(lib, "WorldMi355DefaultMlpgOption")
    o = pkg.world.MlpgOption(7, 7, 7, 7.0)
    lib.WorldMi355DefaultMlpgOption(ctypes.byref(o))
    assert (o.edge, o.var_per_frame, o.input_type, o.unvoiced_value) == (0, 0, 0, -1e10)
    M = pkg.world.MlpgOption
    assert ctypes.sizeof(M) == 24
    assert (M.edge.offset, M.var_per_frame.offset, M.input_type.offset, M.unvoiced_value.offset) == (0, 4, 8, 16)
    assert hasattr(pkg.world.WorldBatch, "parameter_generation") and hasattr(pkg.recipe, "gen_param_files")


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.load_library()
    o = pkg.world.MlpgOption()
    lib.WorldMi355DefaultMlpgOption(ctypes.byref(o))
    assert lib.WorldMi355ParameterGeneration(None, 1, None, 0, None, 0, None, None, None, None, None, ctypes.byref(o),
                                             None, None) == 2                   # WM_ERR_BAD_ARG
    assert lib.WorldMi355ParameterGeneration(None, 0, None, 0, None, 0, None, None, None, None, None, None, None,
                                             None) == 2
    lib.WorldMi355DefaultMlpgOption(None)                                       # a null option struct is left alone


@pytest.mark.parametrize("edge", [0, 1])
@pytest.mark.parametrize("T", [1, 2, 7])
def test_helper_static_window_returns_the_mean(T, edge):
    rng = np.random.default_rng(T)
    mean = rng.standard_normal((T, 3)).astype(np.float32)
    var = (10.0 ** rng.uniform(-3, 3, (T, 3))).astype(np.float32)
    c, cond = ref.mlpg(mean, var, ref.STATIC, edge)
    np.testing.assert_allclose(c, mean.astype(np.float64), rtol=4e-16, atol=0)
    assert (cond >= 1.0).all()


def test_helper_window_matrix_rules():
    """Row (t, i) holds w_i[k] at column t + k - h_i; beyond the ends a tap is dropped (0) or lands on the end (1)."""
    W0, W1 = ref.window_matrix(4, ref.RECIPE, 0), ref.window_matrix(4, ref.RECIPE, 1)
    assert W0.shape == W1.shape == (12, 4)
    np.testing.assert_array_equal(W0[1], [0, 0.5, 0, 0])           # t 0, delta: the -0.5 at column -1 is dropped
    np.testing.assert_array_equal(W1[1], [-0.5, 0.5, 0, 0])        # clamped onto column 0, with the 0 tap
    np.testing.assert_array_equal(W1[2], [-1, 1, 0, 0])            # t 0, delta-delta: 1 - 2 on column 0
    np.testing.assert_array_equal(W0[3 * 3 + 2], [0, 0, 1, -2])
    np.testing.assert_array_equal(W1[3 * 3 + 2], [0, 0, 1, -1])
    np.testing.assert_array_equal(W0[4:7], W1[4:7])                # an inner frame: the rules agree
    np.testing.assert_array_equal(ref.window_matrix(1, ref.RECIPE, 1)[:, 0], [1, 0, 0])


@pytest.mark.parametrize("name", ["recipe", "five", "ramp15", "zero_ends"])
@pytest.mark.parametrize("edge", [0, 1])
def test_helper_dense_agrees_with_banded_solver(name, edge):
    """np.linalg.solve on the dense R against scipy's banded Cholesky on the same R: two float64 solvers agree far
    inside the GPU tests' bound: here within its second term alone (measured: 0.03 of it at most)."""
    from scipy.linalg import solveh_banded
    wins = ref.WINDOW_SETS[name]
    half = 2 * max((len(w) - 1) // 2 for w in wins)
    worst = 0.0
    for T in (1, 2, 3, 5, 64, 257):
        mean, var = ref.make_stream(T, [T], 2, wins, var_per_frame=True)
        c, cond = ref.mlpg(mean, var, wins, edge)
        W = ref.window_matrix(T, wins, edge)
        for d in range(2):
            Rm, WtP = ref.normal_matrix(W, ref.precisions(var[:, d::2]).reshape(-1))
            np.testing.assert_allclose(Rm, Rm.T, rtol=0, atol=1e-14 * np.abs(Rm).max())
            far = np.abs(np.subtract.outer(np.arange(T), np.arange(T))) > half
            assert (Rm[far] == 0).all(), "R is banded with half-bandwidth 2 max h"
            u = min(half, T - 1)
            ab = np.zeros((u + 1, T))
            for k in range(u + 1):
                ab[u - k, k:] = np.diagonal(Rm, k)
            x = solveh_banded(ab, WtP @ mean.astype(np.float64)[:, d::2].reshape(-1))
            err = np.abs(x - c[:, d]).max()
            tol = 64.0 * cond[d] * 2.0 ** -53 * np.abs(c[:, d]).max()
            worst = max(worst, err / tol)
            assert err <= tol, (name, edge, T, d, err, tol)
    print("%s edge %d: dense against banded, worst err / (64 cond 2^-53 max|c|) = %.3g" % (name, edge, worst))


@pytest.mark.parametrize("name", ["recipe", "five", "ramp15"])
def test_helper_inverts_composition_at_edge_1(name):
    """cmp rows made from a float32 random walk by the edge-1 matrix give the walk back, at any positive variances,
    within the spacing of the walk's largest value (the rows are rounded to float32 once)."""
    wins = ref.WINDOW_SETS[name]
    for T in (1, 2, 3, 4, 5, 17, 64, 129, 257):
        rng = np.random.default_rng(1000 + T)
        x = ref.random_walk(rng, T, 3, scale=4.0)
        var = (10.0 ** rng.uniform(-3, 3, 3 * len(wins))).astype(np.float32)
        c, _ = ref.mlpg(ref.compose(x, wins, 1), var, wins, edge=1, want_cond=False)
        err = np.abs(c - x).max(axis=0)
        assert (err <= np.spacing(np.abs(x).max(axis=0))).all(), (name, T, err, np.spacing(np.abs(x).max(axis=0)))


def test_helper_bound_terms():
    c = np.array([[1.0, -300.0], [0.5, 2.0]])
    b = ref.bound(c, np.array([1.0, 1e6]))
    assert b[0] == pytest.approx(2.0 ** -23 + 64 * 2.0 ** -53)
    assert b[1] == pytest.approx(2.0 ** -15 + 64e6 * 2.0 ** -53 * 300)

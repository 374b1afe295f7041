"""The mel-cepstral postfilter (scripts/Training.pl:2642-2687, postfiltering_mcp): what can be checked without a GPU.
The ABI is declared, exported and has its defaults; the fixture tests/golden/sptk_postfilter.npz (written by
tools/gen_golden_postfilter.py from the compiled reference's freqt and fftr) is complete, every set of it was admitted
by the generator's rule, and the definition the library implements -- the energies at the warped frequencies, no
freqt, no transform -- evaluated by numpy meets the reference's delta within the tolerance the GPU test uses."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_postfilter as gen  # noqa: E402

PATH = os.path.join(GOLDEN, "sptk_postfilter.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(PATH)


def direct_delta(c, L, alpha, beta):
    """1/2 ln(sum_k v_k e^{2 (A_k + B_k)} / sum_k v_k e^{2 (A_k + beta B_k)}) over the bins k = 0 .. L/2 (v = 1 at the
    ends, 2 between), A_k = c[1] cos W_k, B_k = sum_{j >= 2} c[j] cos(j W_k), W_k the warped frequency of 2 pi k / L."""
    w = 2.0 * np.pi * np.arange(L // 2 + 1) / L
    W = w + 2.0 * np.arctan2(alpha * np.sin(w), 1.0 - alpha * np.cos(w))
    j = np.arange(len(c))
    cs = np.cos(j[:, None] * W[None, :])
    A = c[1] * cs[1]
    B = c[2:] @ cs[2:]
    v = np.full(L // 2 + 1, 2.0)
    v[0] = v[-1] = 1.0
    return 0.5 * np.log((v * np.exp(2.0 * (A + B))).sum() / (v * np.exp(2.0 * (A + beta * B))).sum())


def gain_tol(c, beta, sens):
    """The GPU test's bound on |gain - delta| for the rows of c: max(10 sens, 64 ulp of sum_{k >= 1} w_k |c_k|)."""
    w = gen.weights(c.shape[1] - 1, beta)
    return np.maximum(10.0 * sens, 64.0 * np.spacing((w[1:] * np.abs(c[:, 1:])).sum(axis=1)))


def test_abi_declared_exported_with_defaults(pkg):
    text = open(os.path.join(ROOT, "include", "world_mi355.h")).read()
    assert re.search(r"\bint\s+WorldMi355MelCepstrumPostfilter\s*\(", text)
    assert re.search(r"\bvoid\s+WorldMi355DefaultMcpfOption\s*\(", text)
    assert "Training.pl:2642-2687" in text and '"mcpf_kernel"' in text
    lib = pkg.load_library()
    assert hasattr(lib, "WorldMi355MelCepstrumPostfilter") and hasattr(lib, "WorldMi355DefaultMcpfOption")
    o = pkg.world.McpfOption()
    lib.WorldMi355DefaultMcpfOption(ctypes.byref(o))
    assert (o.alpha, o.beta, o.order, o.length) == (0.35, 1.4, 25, 4096)
    assert ctypes.sizeof(pkg.world.McpfOption) == 24 and pkg.world.McpfOption.length.offset == 20
    lib.WorldMi355DefaultMcpfOption(None)                                       # a null option struct is left alone


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.load_library()
    o = pkg.world.McpfOption()
    lib.WorldMi355DefaultMcpfOption(ctypes.byref(o))
    assert lib.WorldMi355MelCepstrumPostfilter(None, None, ctypes.byref(o), None, None, None) == 2   # WM_ERR_BAD_ARG
    assert lib.WorldMi355MelCepstrumPostfilter(None, None, None, None, None, None) == 2


def test_fixture_is_present_finite_and_complete(fx):
    assert os.path.getsize(PATH) < 1 << 20
    assert sorted(fx["keys"]) == sorted(gen.OPTIONS) and len(gen.OPTIONS) == 16
    seen = set()
    for key, (L, co, m, alpha, beta) in gen.OPTIONS.items():
        for name in ("opt", "mc", "delta", "tail", "sens", "sens_abc", "recipe_f32_gap"):
            assert key + "/" + name in fx.files, (key, name)
            assert np.isfinite(fx[key + "/" + name]).all(), (key, name)
        assert list(fx[key + "/opt"]) == [L, co, m, alpha, beta] and co < L
        rows = gen.rows_of(L)
        assert fx[key + "/mc"].shape == (rows, m + 1) and fx[key + "/delta"].shape == (rows,)
        assert (fx[key + "/mc"] == gen.inputs(L, m, alpha)).all(), key
        assert fx[key + "/sens"] == fx[key + "/sens_abc"].max() and fx[key + "/sens"] < 1e-14
        assert (fx[key + "/delta"] != 0).all() if m > 1 else (fx[key + "/delta"] == 0).all(), key
        seen.add((L, m, alpha, beta))
    # the issue's table, alpha 0 and the three betas
    assert {(512, 1, 0.55, 1.4), (512, 2, 0.55, 1.4), (512, 24, 0.42, 1.4), (512, 24, -0.42, 1.4), (512, 24, 0.55, 1.4),
            (512, 49, 0.55, 1.4), (512, 63, 0.42, 1.4), (512, 24, 0.77, 1.4), (1024, 49, 0.55, 1.4),
            (2048, 63, 0.77, 1.4), (4096, 49, 0.55, 1.4), (512, 24, 0.0, 0.7), (512, 24, 0.0, 1.4),
            (512, 24, 0.0, 2.0)} <= seen
    assert gen.OPTIONS[gen.RECIPE][:2] == (4096, 2047)


def test_every_set_was_admitted_by_the_one_rule(fx):
    """2 tail <= max(a, b): the script's truncation at co is not what limits the reference."""
    for key in gen.OPTIONS:
        a, b, c = fx[key + "/sens_abc"]
        assert c == 2.0 * float(fx[key + "/tail"]) and c <= max(a, b), (key, a, b, c)


@pytest.mark.parametrize("key", sorted(gen.OPTIONS))
def test_direct_evaluation_meets_the_reference(fx, key):
    """The co -> infinity quantity at the script's bins against the compiled chain with its co: inside the tolerance of
    the GPU test, so the reference alone stays inside it."""
    L, co, m, alpha, beta = gen.OPTIONS[key]
    c = fx[key + "/mc"]
    got = np.asarray([direct_delta(r, L, alpha, beta) for r in c])
    err = np.abs(got - fx[key + "/delta"])
    tol = gain_tol(c, beta, float(fx[key + "/sens"]))
    print("%s: worst err %.2e, worst err / tol %.3f" % (key, err.max(), (err / tol).max()))
    assert (err <= tol).all(), (key, err, tol)

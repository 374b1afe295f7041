"""Spectra from mel-generalized cepstra (SPTK's mgc2sp, test/sptkfunctions.cpp:186-219): what can be checked without a
GPU.  The ABI is declared, exported and has SPTK's defaults; the fixture tests/golden/sptk_mgc2sp_full.npz (written by
tools/gen_golden_mgc2sp.py from the compiled reference) has every option set in its shape and agrees with numpy."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_mgc2sp as gen  # noqa: E402

PATH = os.path.join(GOLDEN, "sptk_mgc2sp_full.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(PATH)


def freqt(c1, m2, a):
    """SPTK's freqt (:596-631): g_i[j] = g_{i-1}[j-1] + a (g_{i-1}[j] - g_i[j-1]) over the input coefficients from the
    last to the first, with g[0] = c + a d[0] and g[1] = (1 - a a) d[0] + a d[1]."""
    g = np.zeros(m2 + 1)
    for c in c1[::-1]:
        d = g.copy()
        g[0] = c + a * d[0]
        g[1] = (1 - a * a) * d[0] + a * d[1]
        for j in range(2, m2 + 1):
            g[j] = d[j - 1] + a * (d[j] - g[j - 1])
    return g


def test_abi_declared_exported_with_sptk_defaults(pkg):
    text = open(os.path.join(ROOT, "include", "world_mi355.h")).read()
    assert re.search(r"\bint\s+WorldMi355MelCepstrumToSpectrum\s*\(", text)
    assert re.search(r"\bvoid\s+WorldMi355DefaultMgc2spOption\s*\(", text)
    assert "sptkfunctions.cpp:186-219" in text and ":347-385" in text
    lib = pkg.load_library()
    assert hasattr(lib, "WorldMi355MelCepstrumToSpectrum") and hasattr(lib, "WorldMi355DefaultMgc2spOption")
    o = pkg.world.Mgc2spOption()
    lib.WorldMi355DefaultMgc2spOption(ctypes.byref(o))
    assert (o.alpha, o.gamma, o.order, o.out_format) == (0.35, 0.0, 25, 0)
    assert ctypes.sizeof(pkg.world.Mgc2spOption) == 24 and pkg.world.Mgc2spOption.out_format.offset == 20


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.load_library()
    o = pkg.world.Mgc2spOption()
    assert lib.WorldMi355MelCepstrumToSpectrum(None, None, ctypes.byref(o), None, None, None) == 2   # WM_ERR_BAD_ARG


def test_fixture_is_present_finite_and_complete(fx):
    assert os.path.getsize(PATH) < 1 << 20
    assert sorted(fx["keys"]) == sorted(gen.OPTIONS) and len(gen.OPTIONS) == 57
    assert float(fx["y_sign"]) == 1.0 and list(fx["round_trips"]) == list(gen.ROUND_TRIPS)
    for key in list(gen.OPTIONS) + ["S"]:
        for name in ("opt", "mc", "x", "y", "sens_x", "sens_y", "sens_ab"):
            assert key + "/" + name in fx.files, (key, name)
        if key != "S":
            assert np.isfinite(fx[key + "/mc"]).all(), key
        assert np.isfinite(fx[key + "/x"]).all() and np.isfinite(fx[key + "/y"]).all(), key
        # the larger of the two figures, both measured, both at rounding level for values of a few units
        ab = fx[key + "/sens_ab"]
        assert ab.shape == (2, 2) and (ab > 0).all() and (ab < 1e-11).all(), key
        assert fx[key + "/sens_x"] == ab[0].max() and fx[key + "/sens_y"] == ab[1].max()
        assert np.abs(fx[key + "/x"]).max() < gen.X_LIMIT
    for key in gen.ROUND_TRIPS:
        assert 0 < fx[key + "/rt_ref"] < 1e-13, key


def test_fixture_shapes_and_option_sets(fx):
    seen = set()
    for key, (F, m, alpha, gamma) in gen.OPTIONS.items():
        assert list(fx[key + "/opt"]) == [F, m, alpha, gamma]
        rows = gen.ROWS[F]
        assert fx[key + "/mc"].shape == (rows, m + 1)
        assert fx[key + "/x"].shape == fx[key + "/y"].shape == (rows, F // 2 + 1)
        assert (1.0 + gamma * fx[key + "/mc"][:, 0] > 0).all(), key
        seen.add((F, m, alpha, round(gamma * 6)))
    for m in (1, 24, 63):
        for alpha in (0.0, 0.42, 0.55, -0.3):
            for g6 in (0, -2, -3, -6):
                assert (512, m, alpha, g6) in seen
    assert {(1024, 24, 0.55, 0), (1024, 24, 0.55, -2), (1024, 49, 0.42, 0), (1024, 49, 0.42, -2), (2048, 63, 0.55, 0),
            (2048, 63, 0.55, -6), (4096, 24, 0.55, 0), (4096, 24, 0.55, -2), (512, 8, 0.42, 0)} <= seen
    assert fx["S/mc"].shape == (4, gen.STATUS_OPT[1] + 1) and fx["S/x"].shape == fx["S/y"].shape == (4, 257)


def test_inputs_at_gamma_0_are_the_generators_candidates(fx):
    for key, (F, m, alpha, gamma) in gen.OPTIONS.items():
        if gamma != 0.0:
            continue
        cand = np.concatenate(gen.candidates(F, m, alpha))
        for row in fx[key + "/mc"]:
            assert (cand == row).all(axis=1).any(), key


@pytest.mark.parametrize("key", sorted(k for k, o in gen.OPTIONS.items() if o[3] == 0.0))
def test_gamma_0_agrees_with_numpy(fx, key):
    """x + i y = rfft of freqt(mc, F/2, -alpha) zero-padded to F: pins the warp's sign, the bin order and y's sign."""
    F, m, alpha, _ = gen.OPTIONS[key]
    for row, x, y in zip(fx[key + "/mc"], fx[key + "/x"], fx[key + "/y"]):
        c = freqt(row, F // 2, -alpha) if alpha != 0 else row
        X = np.fft.rfft(c, F)
        assert np.abs(X.real - x).max() < 1e-12 and np.abs(X.imag - y).max() < 1e-12, key


def test_status_case_rows_are_what_the_generator_says(fx):
    F, m, alpha, gamma = fx["S/opt"]
    assert (F, m, alpha, gamma) == gen.STATUS_OPT and gamma < 0 and alpha != 0
    mc = fx["S/mc"]
    assert list(fx["S/status"]) == list(gen.STATUS) == [0, 1, 0, 1]
    assert np.isfinite(mc[[0, 1, 2]]).all() and np.isnan(mc[3]).sum() == 1
    # row 1: 1 + gamma c0 < 0 for the c0 the chain sees, i.e. after the frequency transformation as well
    assert 1.0 + gamma * mc[1, 0] < 0 and 1.0 + gamma * freqt(mc[1], 4, -alpha)[0] < 0
    for r in (0, 2):
        assert 1.0 + gamma * freqt(mc[r], 4, -alpha)[0] > 0
        assert np.abs(fx["S/x"][r]).max() > 0
    for r in (1, 3):
        assert (fx["S/x"][r] == 0).all() and (fx["S/y"][r] == 0).all()

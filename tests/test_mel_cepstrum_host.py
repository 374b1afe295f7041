"""Mel-cepstral analysis (SPTK's mcep, test/sptkfunctions.cpp:11-184): what can be checked without a GPU.
The ABI is declared, exported and has SPTK's defaults; the fixture tests/golden/sptk_mcep.npz (written by
tools/gen_golden_mcep.py from the compiled reference) is consistent with itself and with numpy."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_mcep as gen  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "sptk_mcep.npz"))


def test_abi_declared_exported_with_sptk_defaults(pkg):
    text = open(os.path.join(ROOT, "include", "world_mi355.h")).read()
    assert re.search(r"\bint\s+WorldMi355MelCepstrum\s*\(", text)
    assert re.search(r"\bvoid\s+WorldMi355DefaultMcepOption\s*\(", text)
    assert "sptkfunctions.cpp:11-184" in text and "theq.cpp" in text
    lib = pkg.load_library()
    assert hasattr(lib, "WorldMi355MelCepstrum") and hasattr(lib, "WorldMi355DefaultMcepOption")
    o = pkg.world.McepOption()
    lib.WorldMi355DefaultMcepOption(ctypes.byref(o))
    assert (o.alpha, o.order, o.itr1, o.itr2, o.dd, o.etype, o.e, o.f, o.itype) == \
        (0.35, 25, 2, 30, 1e-3, 0, 0.0, 1e-6, 3)
    assert ctypes.sizeof(pkg.world.McepOption) == 64 and pkg.world.McepOption.itype.offset == 56


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.load_library()
    o = pkg.world.McepOption()
    assert lib.WorldMi355MelCepstrum(None, None, ctypes.byref(o), None, None) == 2       # WM_ERR_BAD_ARG


def test_fixture_has_every_case_and_enough_robust_frames(fx):
    assert set(gen.OPTIONS) == {k.split("/")[0] for k in fx.files if k.endswith("/conv") and not k.startswith("D/")}
    assert len(gen.OPTIONS) == 14
    for key, (case, m, alpha, extra) in gen.OPTIONS.items():
        F, frames = gen.CASE_SHAPE[case]
        assert fx[key + "/fixed"].shape == (4, frames, m + 1) and fx[key + "/conv"].shape == (frames, m + 1)
        assert fx[key + "/robust"].mean() >= 0.9, key
        assert set(np.unique(fx[key + "/ret"])) <= {0, -1}
        assert fx[key + "/opt"][1] == extra.get("itr2", 30)
        if "itr2" in extra:                                 # frames that run out of steps although dd > 0, and others
            ret = fx[key + "/ret"][fx[key + "/robust"]]
            assert (ret == -1).sum() >= 4 and (ret == 0).sum() >= 4, key
        assert np.isfinite(fx[key + "/fixed"]).all() and np.isfinite(fx[key + "/conv"]).all()
        assert 0 < fx[key + "/sens_conv"] < 1e-12 and (fx[key + "/sens_fixed"] < 1e-12).all(), key
    assert list(fx["fixed_itr"]) == [0, 1, 2, 5] and float(fx["dd"]) == 1e-3
    assert list(fx["D/status"]) == [0, 2, 0, 0] and list(fx["D/status_f1e6"]) == [1, 2, 1, 1]
    assert 0 < fx["D/sens_conv"] < 1e-12 and 0 < fx["D/sens_init"] < 1e-12
    assert os.path.getsize(os.path.join(GOLDEN, "sptk_mcep.npz")) < 600 * 1024


def test_seeds_regenerate_the_inputs(fx):
    for case in ("A", "C"):
        F, frames = gen.CASE_SHAPE[case]
        assert int(fx["seed_" + case]) == gen.CASE_SEEDS[case]
        x = gen.smooth_spectra(int(fx["seed_" + case]), frames, F)
        np.testing.assert_allclose(x, fx["x_" + case], rtol=1e-14, atol=0)       # cos / exp of another libm: last bits
        db = 20 * np.log10(x.max(axis=1) / x.min(axis=1))
        assert np.allclose(db, 60.0, atol=1e-6)
    xd = fx["x_D"]
    assert xd[1, 5] == 0.0 and (np.delete(xd.ravel(), 257 + 5) > 0).all()
    b = gen.case_b_rows()
    assert b.shape == (24, 513) and (b[8:11] > 9999.0).all() and (b[11:] < 9999.0).any()   # unvoiced and voiced ap rows


def np_freqt(c, m2, a):
    """freqt (sptkfunctions.cpp:596-631) as a matrix-free recursion in numpy."""
    g = np.zeros(m2 + 1)
    b = 1 - a * a
    for v in c[::-1]:
        d = g.copy()
        g[0] = v + a * d[0]
        if m2 >= 1:
            g[1] = b * d[0] + a * d[1]
        for j in range(2, m2 + 1):
            g[j] = d[j - 1] + a * (d[j] - g[j - 1])
    return g


def test_initial_estimate_is_freqt_of_the_halved_cepstrum(fx):
    """Mode (i) with itr2 = 0 (:119-138): c = IFFT[log x], c[0] and c[F/2] halved, mc = freqt(c, F/2 -> m, a)."""
    for key, (case, m, alpha, extra) in gen.OPTIONS.items():
        F, _ = gen.CASE_SHAPE[case]
        x = gen.case_input(case) if case.startswith("B") else fx["x_" + case]
        per = (x * x if extra.get("itype", 3) == 3 else x) + (extra.get("e", 0.0) if extra.get("etype", 0) == 1 else 0.0)
        c = np.fft.irfft(np.log(per), n=F, axis=1)[:, :F // 2 + 1]
        c[:, 0] /= 2
        c[:, F // 2] /= 2
        want = np.stack([np_freqt(row, m, alpha) for row in c[:4]])
        np.testing.assert_allclose(fx[key + "/fixed"][0][:4], want, rtol=0, atol=1e-12, err_msg=key)


def test_more_steps_fit_better(fx):
    """The Newton steps do what they are for: the unbiased log-spectral criterion's proxy, the distance to the converged
    row, shrinks with the step count."""
    for key in ("A_m1_a42", "B_cli", "B_m49"):
        f, conv = fx[key + "/fixed"], fx[key + "/conv"]
        err = [np.abs(f[k] - conv).max() for k in range(4)]
        assert err[0] > 1e-6 and err[0] > err[1] > err[3], (key, err)


def test_mel_cepstrum_matches_the_decoders_conventions(fx):
    """What test_gpu_mel_cepstrum.py feeds to WorldMi355RecipeDecode, on the CPU restatement of the decoder: exp of the
    mel-cepstral log spectrum at the warped frequency is what mgc2sp (sptkfunctions.cpp:186-219) yields from the row."""
    from oracle.bindings import Oracle
    mc = fx["B_cli/conv"][8:]
    bap = mc.astype(np.float32)
    bap[:, 0] = (mc[:, 0] - 9.210340).astype(np.float32)
    lf0 = np.zeros(len(bap), dtype=np.float32)
    mgc = np.zeros((len(bap), 50), dtype=np.float32)
    _, _, ap = Oracle().recipe_decode(lf0, mgc, bap, 16000, 1024)
    np.testing.assert_allclose(ap[:, :24], expected_decoded_ap(bap, 1024, 0.55), rtol=1e-11, atol=0)


def expected_decoded_ap(bap, F, alpha):
    c = bap.astype(np.float64)
    c[:, 0] += 9.210340
    w = 2 * np.pi * np.arange(24) / F
    wt = w + 2 * np.arctan2(alpha * np.sin(w), 1 - alpha * np.cos(w))
    return np.exp(c @ np.cos(np.outer(np.arange(c.shape[1]), wt))) / 1e4

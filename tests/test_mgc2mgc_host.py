"""Conversion between mel-generalized cepstra (SPTK's mgc2mgc; the core is test/sptkfunctions.cpp:221-254): what can be
checked without a GPU.  The numpy restatement (tests/mgc2mgc_reference.py) and, where it is built, the compiled reference
against the fixture tests/golden/sptk_mgc2mgc.npz (tools/gen_golden_mgc2mgc.py); the algebra of the four flags; the ABI,
its defaults, its layout and its refusals, all of which happen on the host."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

import mgc2mgc_reference as R

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_mgc2mgc as gen  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return np.load(gen.PATH)


def check_rows(got, want, sens, what):
    err = np.abs(got - want).max(axis=1)
    tol = R.row_tol(want, sens)
    print("%s: max err %.3e, worst err / tol %.3f" % (what, err.max(), (err / tol).max()))
    assert np.isfinite(got).all(), what
    assert (err <= tol).all(), (what, float(err.max()), float(tol.min()))


def test_fixture_is_present_finite_and_complete(fx):
    assert os.path.getsize(gen.PATH) < 1 << 20
    assert sorted(fx["keys"]) == sorted(gen.OPTIONS) and len(gen.OPTIONS) == 23
    for key, (opt, rows) in gen.OPTIONS.items():
        assert tuple(fx[key + "/opt"]) == opt, key
        m1, g1, m2 = opt[0], opt[2], opt[5]
        assert fx[key + "/in"].shape == (rows, m1 + 1) and fx[key + "/out"].shape == (rows, m2 + 1), key
        assert np.isfinite(fx[key + "/in"]).all() and np.isfinite(fx[key + "/out"]).all(), key
        ab = fx[key + "/sens_ab"]
        assert ab.shape == (rows, 2) and (ab[:, 0] > 0).all() and (ab < 1e-11).all(), key
        assert (fx[key + "/sens"] == ab.max(axis=1)).all(), key
        plain = np.stack([R.plain_input(r, opt) for r in fx[key + "/in"]])
        assert (1.0 + g1 * plain[:, 0] > 0).all(), key
    assert rows_of("c24_g2_to_m2047_a0_g1p") == rows_of("c34_g3_to_m4095_a0_g1p") == 2
    assert list(fx["S/status"]) == list(gen.STATUS) == [0, 1, 0, 1] and tuple(fx["S/opt"]) == gen.STATUS_OPT
    s_in, s_out = fx["S/in"], fx["S/out"]
    assert 1.0 + gen.STATUS_OPT[2] * s_in[1, 0] < 0 and np.isnan(s_in[3]).sum() == 1 and np.isfinite(s_in[:3]).all()
    assert (s_out[[1, 3]] == 0).all() and np.abs(s_out[[0, 2]]).max() > 0 and np.isfinite(s_out).all()


def rows_of(key):
    return gen.OPTIONS[key][1]


def test_option_sets_reach_every_branch_and_boundary():
    opts = [o for o, _ in gen.OPTIONS.values()]
    warps = [R.warp(o[1], o[6]) for o in opts]
    assert any(a == 0 for a in warps) and any(a != 0 for a in warps)
    assert {o[5] for o in opts} >= {1, 8, 24, 63, 64, 65, 127, 128, 200, 2047, 4095}
    assert {o[0] for o in opts} >= {1, 8, 24, 49, 63, 127, 2047}
    assert any(o[0] > 63 and a != 0 for o, a in zip(opts, warps))                 # the lane-per-output freqt
    assert any(o[2] == 0 and o[7] == 0 and a != 0 for o, a in zip(opts, warps))   # gamma 0 to gamma 0: freqt alone
    assert any(o[7] == 1 for o in opts) and any(o[2] == -1 for o in opts)
    flags = {(o[3], o[4], o[8], o[9]) for o in opts}
    assert flags == {(0, 0, 0, 0), (1, 1, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 1, 1), (0, 0, 0, 1)}
    for o in opts:
        assert min(o[0], o[5]) <= 63


def test_inputs_are_the_generators_candidates(fx):
    """At gamma 1 == 0 without flags the stored rows are the seeded candidates themselves, all of them in order."""
    for key, (opt, rows) in gen.OPTIONS.items():
        if opt[2] == 0.0 and not (opt[3] or opt[4]):
            assert (fx[key + "/in"] == gen.candidates(opt, rows)).all(), key


@pytest.mark.parametrize("key", sorted(gen.OPTIONS))
def test_numpy_restatement_matches_the_fixture(fx, key):
    opt, _ = gen.OPTIONS[key]
    check_rows(R.convert_rows(fx[key + "/in"], opt), fx[key + "/out"], fx[key + "/sens"], key)


def test_numpy_restatement_on_the_status_rows(fx):
    good = np.asarray(gen.STATUS) == 0
    check_rows(R.convert_rows(fx["S/in"][good], gen.STATUS_OPT), fx["S/out"][good], fx["S/sens"][good], "S")
    bad = R.convert_rows(fx["S/in"][~good], gen.STATUS_OPT)
    assert not np.isfinite(bad[0]).all() and not np.isfinite(bad[1]).all()      # what the reference makes of them


def test_compiled_reference_reproduces_the_fixture_bit_for_bit(fx):
    if not os.path.exists(gen.LIB):
        pytest.skip("oracle/_ref/libsptk_ref.so not built (needs the reference tree)")
    for key in sorted(gen.OPTIONS):
        opt, rows = gen.OPTIONS[key]
        r = gen.run_child(opt, rows_in=fx[key + "/in"])            # a process of its own per option set
        assert r["out"].tobytes() == fx[key + "/out"].tobytes(), key


def test_flag_algebra(fx):
    """Each output flag undone by the input flag of the same letter returns the plain result, and each flagged input is
    the plain one behind its flag, within the rule's bound (sens of the plain set)."""
    plain_key = "c24_g3_to_m63"                                      # rows at (24, .55, -1/3), no flag
    rows = fx[plain_key + "/in"]
    m, a, g = 24, .55, gen.G3
    sens = np.maximum.reduce([fx[k + "/sens"] for k in ("f_N", "f_NU", "f_U")])
    want = R.convert_rows(rows, R.option(m, a, g, m, a, g))
    for n, u in ((1, 0), (0, 1), (1, 1)):
        out = R.convert_rows(rows, R.option(m, a, g, m, a, g, N=n, U=u))
        back = R.convert_rows(out, R.option(m, a, g, m, a, g, n=n, u=u))
        check_rows(back, want, sens, "-N%d -U%d fed back with -n%d -u%d" % (n, u, n, u))
    # -U alone is c[0] g + 1 and c[k] g; -N leaves gnorm's gain in c[0]
    out = R.convert_rows(rows, R.option(m, a, g, m, a, g, U=1))
    assert np.abs(out[:, 0] - (want[:, 0] * g + 1)).max() < 1e-14 and np.abs(out[:, 1:] - want[:, 1:] * g).max() < 1e-14
    out = R.convert_rows(rows, R.option(m, a, g, m, a, g, N=1))
    k = 1 + g * want[:, 0]
    assert np.abs(out[:, 0] / k ** (1 / g) - 1).max() < 1e-14 and np.abs(out[:, 1:] - want[:, 1:] / k[:, None]).max() < 1e-13
    # the fixture's flagged inputs are flagged forms of one set of plain rows
    plain = np.stack([R.plain_input(r, gen.OPTIONS["f_nu"][0]) for r in fx["f_nu/in"]])
    plain_u = np.stack([R.plain_input(r, gen.OPTIONS["f_u"][0]) for r in fx["f_u/in"]])
    assert np.abs(plain - fx["f_U/in"]).max() < 1e-14 and np.abs(plain_u - fx["f_U/in"]).max() < 1e-14


def test_abi_declared_exported_with_sptk_defaults_and_layout(pkg):
    text = open(os.path.join(ROOT, "include", "world_mi355.h")).read()
    assert re.search(r"\bint\s+WorldMi355MelGeneralizedCepstrumConvert\s*\(", text)
    assert re.search(r"\bvoid\s+WorldMi355DefaultMgcConvertOption\s*\(", text)
    assert "sptkfunctions.cpp:221-254" in text and '"mgc2mgc_kernel"' in text
    assert "FLAG SEMANTICS UNPINNED AGAINST" in text
    body = re.search(r"typedef struct \{([^}]*)\} WorldMi355MgcConvertOption;", text).group(1)
    fields = re.findall(r"\b(int|double)\s+(\w+);", body)
    assert [f for _, f in fields] == list(R.FIELDS)
    O = pkg.world.MgcConvertOption
    assert [(n, {ctypes.c_int: "int", ctypes.c_double: "double"}[t]) for n, t in O._fields_] == [(f, t) for t, f in fields]
    assert ctypes.sizeof(O) == 64 and O.in_alpha.offset == 8 and O.in_multiplied.offset == 28
    assert O.out_order.offset == 32 and O.out_alpha.offset == 40 and O.out_multiplied.offset == 60
    lib = pkg.load_library()
    assert hasattr(lib, "WorldMi355MelGeneralizedCepstrumConvert") and hasattr(lib, "WorldMi355DefaultMgcConvertOption")
    o = O()
    lib.WorldMi355DefaultMgcConvertOption(ctypes.byref(o))
    assert tuple(getattr(o, f) for f in R.FIELDS) == (25, 0.0, 0.0, 0, 0, 25, 0.0, 0.0, 0, 0)
    lib.WorldMi355DefaultMgcConvertOption(None)                      # a null option struct is left alone
    assert pkg.MgcConvertOption is O
    assert "mgc2mgc.hip" in open(os.path.join(ROOT, "hts-train-world_amd", "csrc", "Makefile")).read()


def test_every_refusal_without_a_device(pkg):
    """No context, no batch, no device memory: the answer is WM_ERR_BAD_ARG (2) from the host alone.  The pointers that
    stand for device memory are never followed."""
    lib = pkg.load_library()
    O = pkg.world.MgcConvertOption
    fake, other = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)
    good = R.option(24, .42, gen.G3, 24, .42, 0)

    def call(opt=good, src=fake, dst=other):
        o = None if opt is None else ctypes.byref(O(*opt))
        return lib.WorldMi355MelGeneralizedCepstrumConvert(None, src, o, dst, None)

    nan = float("nan")
    for opt in (None,
                R.option(0, .42, 0, 24, .42, 0), R.option(24, .42, 0, 0, .42, 0), R.option(-1, .42, 0, 24, .42, 0),
                R.option(4096, 0, 0, 24, 0, 0), R.option(24, 0, 0, 4096, 0, 0),
                R.option(64, 0, 0, 64, 0, 0), R.option(200, 0, 0, 2047, .1, 0),          # min(m1, m2) > 63
                R.option(24, 1.0, 0, 24, .42, 0), R.option(24, .42, 0, 24, -1.0, 0), R.option(24, nan, 0, 24, 0, 0),
                R.option(24, 0, 0, 24, nan, 0),
                R.option(24, .42, -1.5, 24, .42, 0), R.option(24, .42, 1.5, 24, .42, 0), R.option(24, .42, 0, 24, .42, 1.01),
                R.option(24, .42, 0, 24, .42, -1.01), R.option(24, .42, nan, 24, .42, 0), R.option(24, .42, 0, 24, .42, nan),
                R.option(24, .42, 0, 24, .42, -.5, u=1),                                 # -u at gamma 1 == 0
                R.option(24, .42, 0, 24, .42, -.5, n=1, u=1),
                R.option(24, .42, -.5, 24, .42, 0, U=1),                                 # -U at gamma 2 == 0
                R.option(24, .42, -.5, 24, .42, 0, N=1, U=1)):
        assert call(opt=opt) == 2, opt
    assert call(src=None) == 2 and call(dst=None) == 2
    # sound arguments get as far as the missing batch
    assert call() == 2
    for opt in (R.option(1, 0, -1, 4095, .3, 1), R.option(4095, 0, 1, 1, -.99, -1), R.option(63, 0, 0, 63, 0, 0, n=1, N=1),
                R.option(24, .42, -.5, 24, .42, .5, n=1, u=1, N=1, U=1)):
        assert call(opt=opt) == 2



def test_bad_tensors_are_refused_before_the_library(pkg):
    """The checks tests/test_world_arguments_host.py owes every tensor argument of a WorldBatch method, for this one at
    another order than that file's row, on the method WorldBatch itself defines."""
    import torch
    import test_world_arguments_host as A
    W = pkg.world
    pkg.load_library()
    assert "convert_mel_generalized_cepstrum" in vars(W.WorldBatch)
    b = W.WorldBatch.__new__(W.WorldBatch)                          # a batch made by hand, as that file makes its own
    b.handle, b.ctx, b.total_frames, b.device = None, None, A.TF, torch.device("cpu")
    kwargs = dict(mc=A.z(A.F64, A.TF, 25), alpha=0.42, gamma=-0.5, out_order=30, out_alpha=0.0, out_gamma=1.0)
    n = A.refusals(b.convert_mel_generalized_cepstrum, "convert_mel_generalized_cepstrum", kwargs, [A.arg("mc", free=(1,))])
    assert n >= 4

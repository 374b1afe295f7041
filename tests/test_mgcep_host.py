"""The host side of `frame | window | mgcep`: the frame rule and the window table of the library (no device needed)
against tests/mgcep_reference.py, that reference against tests/mspf_reference.py where the two rules meet, the fixture
tests/golden/sptk_mgcep.npz against what tools/gen_golden_mgcep.py makes today, and the argument checks of
`recipe.py mgcep`."""
import importlib
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import mgcep_reference as ref
import mspf_reference as mspf

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_mgcep as gen  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "sptk_mgcep.npz"))


@pytest.fixture(scope="module")
def W(pkg):
    pkg.load_library()
    return pkg.world


def test_frame_rule_is_the_modulation_spectrum_one_where_they_meet():
    """L odd, P = (L - 1) / 2: the counts and the frames of tests/mspf_reference.py (which also applies its window)."""
    rs = np.random.RandomState(3)
    for L in (3, 5, 25, 401):
        P = (L - 1) // 2
        for T in (0, 1, 2, P - 1, P, P + 1, L, 3 * L + 1, 1000):
            if T < 0:
                continue
            assert ref.n_frames(T, L, P) == mspf.n_frames(T, L), (L, T)
            if T:
                y = rs.randn(T)
                np.testing.assert_array_equal(ref.frames(y, L, P) * mspf.bartlett(L)[None, :], mspf.frames(y, L))


def test_frames_hold_what_the_definition_says():
    x = np.arange(1.0, 12.0)                                           # T = 11
    z = ref.frames(x, 6, 4)                                            # J = ceil((11 + 3) / 4) = 4
    assert z.shape == (4, 6)
    np.testing.assert_array_equal(z[0], [0, 0, 0, 1, 2, 3])            # frame 0 is centred on sample 0
    np.testing.assert_array_equal(z[1], [2, 3, 4, 5, 6, 7])
    np.testing.assert_array_equal(z[3], [10, 11, 0, 0, 0, 0])          # the last frame still holds a sample
    assert ref.n_frames(9, 6, 4) == 3 and ref.n_frames(10, 6, 4) == 4  # sample 9 lies under frame 3's first slot


def test_library_frame_count(W):
    for L in (2, 3, 400, 401, 512, 1200):
        for P in sorted({1, 2, 80, 240, L // 2, L} - {0}):
            if P > L:
                continue
            for T in (0, 1, L // 2, L // 2 + 1, L, 12345, 2 ** 31 + 7):
                assert W.sptk_frames(T, L, P) == ref.n_frames(T, L, P), (T, L, P)
    for T, L, P in ((10, 400, 0), (10, 400, 401), (-1, 400, 80), (10, 0, 0)):
        with pytest.raises(RuntimeError, match="bad argument"):
            W.sptk_frames(T, L, P)


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_library_window_table(W):
    """Within 4 ulp of the reference table (libm's cos, exact sums); the normalised tables sum to 1 within 1e-15."""
    for L in (3, 4, 400, 401, 512, 1200, 4096):
        for kind in (0, 1, 2, 5):
            for norm in (0, 1, 2):
                w, want = W.sptk_window(kind, norm, L), ref.window(kind, norm, L)
                assert w.shape == (L,) and w.dtype == np.float64
                worst = ulps(w, want)[want != 0].max() if (want != 0).any() else 0.0
                assert (w[want == 0] == 0).all() and worst <= 4.0, (L, kind, norm, worst)
                if norm == 1:
                    assert abs(float(np.sum(w.astype(np.longdouble) ** 2)) - 1.0) <= 1e-15, (L, kind)
                if norm == 2:
                    assert abs(float(np.sum(w.astype(np.longdouble))) - 1.0) <= 1e-15, (L, kind)
    for kind in (3, 4):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            W.sptk_window(kind, 0, 400)
    for kind, norm, L in ((-1, 0, 400), (6, 0, 400), (1, 3, 400), (1, -1, 400), (1, 1, 1), (2, 1, 2)):
        with pytest.raises(RuntimeError, match="bad argument"):
            W.sptk_window(kind, norm, L)


def test_fixture_is_data_of_todays_generator(fx, W):
    """The waveforms are the generator's, integer-valued; the frame counts are the library's; every option set of the
    generator is in the file; the robust share of every stop-rule run meets the cap on the reference alone."""
    assert os.path.getsize(os.path.join(GOLDEN, "sptk_mgcep.npz")) < 1_000_000
    for group, Ts in gen.UTTERANCES.items():
        assert fx["x_" + group].dtype == np.int16 and list(fx["T_" + group]) == list(Ts)
        np.testing.assert_array_equal(fx["x_" + group].astype(np.float64), np.concatenate(gen.waves(group)))
    for key, (group, F, L, P, kind, norm, f32, m, alpha, extra) in gen.SETS.items():
        counts = [W.sptk_frames(T, L, P) for T in gen.UTTERANCES[group]]
        assert list(fx[key + "/counts"]) == counts
        assert fx[key + "/fixed"].shape == (4, sum(counts), m + 1) and fx[key + "/conv"].shape == (sum(counts), m + 1)
        taken = ~fx[key + "/exits"]
        assert fx[key + "/robust"][taken].mean() >= 0.9, key
        assert not fx[key + "/robust"][~taken].any()
    # the sets cover what the GPU tests are asked to cover
    waves = [v for k, v in gen.SETS.items() if v[0] == "wave"]
    assert {v[2] for v in waves} == {400, 401, 512} and {v[3] == v[2] for v in waves} == {False, True}
    assert {v[3] for v in waves if v[3] != v[2]} == {80}
    assert {v[4] for v in waves} == {0, 1, 2, 5} and {v[5] for v in waves} == {0, 1, 2} and {v[6] for v in waves} == {False, True}
    rows = [v for k, v in gen.SETS.items() if v[0] == "rows"]
    assert {v[7] for v in rows} == {12, 49, 63} and {v[8] for v in rows} == {0.0, 0.42, 0.55}
    assert {v[9].get("etype", 0) for v in rows} == {0, 1, 2}
    assert any(fx[k + "/exits"].any() for k in gen.SETS)              # a frame the reference exits on is among them


@pytest.mark.parametrize("key", ["R_m49_a42_e2", "W_L401_P80_w2_n2_f1", "W_L512_P512_w0_n1_f1"])
def test_fixture_against_a_fresh_run_of_the_compiled_reference(fx, key):
    if not os.path.exists(gen.LIB):
        pytest.skip("oracle/_ref/libsptk_ref.so not built (needs the reference tree)")
    rows, counts = gen.set_frames(key)
    r = gen.reference_of(key, rows)
    for name, v in r.items():
        np.testing.assert_array_equal(fx[key + "/" + name], v, err_msg=key + "/" + name)


def test_recipe_command_checks_its_arguments_before_it_opens_anything(pkg, tmp_path, monkeypatch, capsys):
    recipe = importlib.import_module("hts-train-world_amd.recipe")

    def no_context():
        raise AssertionError("a context was opened")
    monkeypatch.setattr(recipe, "_own_context", no_context)
    scp = tmp_path / "jobs.scp"
    scp.write_text("%s %s\n" % (tmp_path / "a.raw", tmp_path / "a.mgc"))
    for args in (["--frame-shift", "0"], ["--frame-shift", "1201"], ["--frame-length", "2049"], ["--frame-length", "1"],
                 ["--fft-length", "1000"], ["--window", "3"], ["--window", "6"], ["--normalize", "3"], ["--order", "0"],
                 ["--order", "64"], ["--alpha", "1.0"], ["--eps", "-1"], ["--max-batch-frames", "0"]):
        with pytest.raises(SystemExit) as e:
            recipe.main(["mgcep", "--scp", str(scp)] + args)
        assert e.value.code == 2, args
        assert "mgcep" in capsys.readouterr().err
    with pytest.raises(ValueError):
        recipe.mgcep_files([], frame_shift=0)
    with pytest.raises(ValueError):
        recipe.mgcep_files([], frame_length=4097, fft_length=4096)
    recipe.mgcep_check(1200, 240, 2048, 1, 1, 0.55, 49, 1e-8)          # the command's defaults pass

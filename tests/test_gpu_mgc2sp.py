"""WorldBatch.spectrum_from_mel_cepstrum (mgc2sp_kernel) against the compiled reference's mgc2sp
(test/sptkfunctions.cpp:186-219) as recorded in tests/golden/sptk_mgc2sp_full.npz by tools/gen_golden_mgc2sp.py.

Tolerance per row: max(10 * sens, 64 ulp of the row's largest |value|), sens being per option set the larger of the
reference's response to a last-bit perturbation of its input and its own distance from the chain in long double."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_mgc2sp as gen  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "sptk_mgc2sp_full.npz"))


def uneven(frames):
    """Utterance lengths that add up to `frames`, the first of a single frame."""
    return [1, frames - 1] if frames > 1 else [1]


def run(gpu, mc, F, lengths, alpha, gamma, out_format=0):
    torch, W, ctx = gpu
    b = W.WorldBatch(ctx, W.default_params(16000, 5.0, fft_size=F), f0_lengths=list(lengths))
    try:
        sp, ph, st = b.spectrum_from_mel_cepstrum(torch.from_numpy(np.ascontiguousarray(mc)).cuda(), alpha, gamma,
                                                  out_format, phase=True)
        return sp.cpu().numpy(), ph.cpu().numpy(), st.cpu().numpy()
    finally:
        b.close()


def row_tol(want, sens):
    return np.maximum(10.0 * sens, 64.0 * np.spacing(np.abs(want).max(axis=1)))


def check_rows(got, want, sens, what):
    err = np.abs(got - want).max(axis=1)
    tol = row_tol(want, sens)
    print("%s: max err %.3e  (10 sens %.3e, least row tol %.3e, worst err / tol %.3f)" % (
        what, err.max(), 10 * sens, tol.min(), (err / tol).max()))
    assert np.isfinite(got).all(), what
    assert (err <= tol).all(), (what, float(err.max()), float(tol.min()))


def check_key(fx, key, x, y, rows=slice(None), what=None):
    what = what or key
    check_rows(x, fx[key + "/x"][rows], float(fx[key + "/sens_x"]), what + " x")
    check_rows(y, fx[key + "/y"][rows], float(fx[key + "/sens_y"]), what + " y")


@pytest.mark.parametrize("key", sorted(gen.OPTIONS))
def test_parity_against_reference(gpu, fx, key):
    F, m, alpha, gamma = gen.OPTIONS[key]
    mc = fx[key + "/mc"]
    x, y, st = run(gpu, mc, F, uneven(len(mc)), alpha, gamma)
    assert (st == 0).all()
    check_key(fx, key, x, y)


@pytest.mark.parametrize("key", ["F512_m24_a42_g3", "F512_m1_a00_g1", "F1024_m24_a55_g0", "F2048_m63_a55_g1",
                                 "F4096_m24_a55_g3"])
def test_amplitude_and_power_formats(gpu, fx, key):
    """|H| = exp(x), |H|^2 = exp(2 x): the relative deviation is the derivative of exp times the deviation of k x, plus
    the roundings of k x_ref -> exp here and in numpy (8 * 2^-52 covers a 1-ulp exp on both sides); y is untouched."""
    F, m, alpha, gamma = gen.OPTIONS[key]
    mc, want = fx[key + "/mc"], fx[key + "/x"]
    tol_x = row_tol(want, float(fx[key + "/sens_x"]))
    for fmt, k in ((3, 1.0), (4, 2.0)):
        sp, y, st = run(gpu, mc, F, uneven(len(mc)), alpha, gamma, fmt)
        assert (st == 0).all() and np.isfinite(sp).all() and (sp > 0).all()
        ref = np.exp(k * want)
        rel = np.abs(sp - ref) / ref
        bound = k * tol_x + 8.0 * 2.0 ** -52
        print("%s format %d: worst relative deviation %.3e, worst / bound %.3f" % (
            key, fmt, rel.max(), (rel.max(axis=1) / bound).max()))
        assert (rel.max(axis=1) <= bound).all(), (key, fmt)
        check_rows(y, fx[key + "/y"], float(fx[key + "/sens_y"]), "%s format %d y" % (key, fmt))


def test_status_rows(gpu, fx):
    """1 + gamma c0 <= 0 and a NaN coefficient are status 1 and rows of zeros; their neighbours are what they are in a
    batch of their own."""
    F, m, alpha, gamma = fx["S/opt"]
    F = int(F)
    mc = fx["S/mc"]
    x, y, st = run(gpu, mc, F, (4,), alpha, gamma)
    assert list(st) == list(fx["S/status"]) == [0, 1, 0, 1]
    assert (x[[1, 3]] == 0).all() and (y[[1, 3]] == 0).all()
    good = np.array([0, 2])
    check_key(fx, "S", x[good], y[good], rows=good)
    for i in good:
        x1, y1, st1 = run(gpu, mc[i:i + 1], F, (1,), alpha, gamma)
        assert st1[0] == 0 and (x1[0] == x[i]).all() and (y1[0] == y[i]).all()
    for fmt in (3, 4):                                                 # zeros whatever the format
        sp, y, st = run(gpu, mc, F, (4,), alpha, gamma, fmt)
        assert list(st) == [0, 1, 0, 1] and (sp[[1, 3]] == 0).all() and (y[[1, 3]] == 0).all()


def test_bad_options_are_refused_before_any_launch(gpu, fx):
    torch, W, ctx = gpu
    F = 512
    b = W.WorldBatch(ctx, W.default_params(16000, 5.0, fft_size=F), f0_lengths=[4])
    rows = lambda cols: torch.zeros(4, cols, dtype=torch.float64, device="cuda")
    ctx.timing_enable(True)
    try:
        for cols, alpha, gamma, fmt, msg in ((1, 0.42, 0.0, 0, "bad argument"),          # order 0
                                             (65, 0.42, 0.0, 0, "bad argument"),         # order 64
                                             (F // 2 + 2, 0.42, 0.0, 0, "bad argument"),  # order > fft_size / 2
                                             (25, 1.0, 0.0, 0, "bad argument"),
                                             (25, 0.42, 0.5, 0, "bad argument"),
                                             (25, 0.42, -1.5, 0, "bad argument"),
                                             (25, 0.42, 0.0, 1, "unsupported configuration")):
            with pytest.raises(RuntimeError, match=msg):
                b.spectrum_from_mel_cepstrum(rows(cols), alpha, gamma, fmt)
        assert ctx.timing_query("mgc2sp_kernel")[1] == 0
        sp, st = b.spectrum_from_mel_cepstrum(rows(25), 0.42, -0.5)
        assert ctx.timing_query("mgc2sp_kernel")[1] == 1
        assert (st.cpu().numpy() == 0).all() and (sp.cpu().numpy() == 0).all()     # mgc2sp of zeros: ln 1
    finally:
        ctx.timing_enable(False)
        b.close()


def test_grid_stride_walk_and_independence_from_placement(gpu, fx):
    """About 6 000 frames (more than one pass of the persistent grid), uneven utterances, one of a single frame: every
    copy of a row is bit-identical to the first, the first copies meet parity, and a second run repeats the first."""
    key = "F512_m24_a42_g3"
    F, m, alpha, gamma = gen.OPTIONS[key]
    rows = len(fx[key + "/mc"])
    reps = 6000 // rows
    mc = np.tile(fx[key + "/mc"], (reps, 1))
    total = len(mc)
    lengths = [1, 7, 333, 1024, 2, 1999]
    lengths.append(total - sum(lengths))
    assert 5900 <= total <= 6000 and min(lengths) == 1 and lengths[-1] > 0
    x, y, st = run(gpu, mc, F, lengths, alpha, gamma)
    x2, y2, st2 = run(gpu, mc, F, lengths, alpha, gamma)
    assert (x == x2).all() and (y == y2).all() and (st == st2).all() and (st == 0).all()
    bins = F // 2 + 1
    assert (x.reshape(reps, rows, bins) == x[:rows]).all() and (y.reshape(reps, rows, bins) == y[:rows]).all()
    check_key(fx, key, x[:rows], y[:rows], what="tiled " + key)


def test_agrees_with_the_existing_bap_decoder(gpu, fx):
    """Conventions (c0, alpha, scaling) agree with codec_bap_decode_kernel: at fft 1024, m 24, alpha 0.55, gamma 0 the
    rows rounded to float32 as `bap` with c0 - 9.210340 go through WorldMi355RecipeDecode, and the same float32 values
    with that entry point's offset put back (synth.cpp:241) through this one: exp(x) / 1e4 on the first 24 bins, with
    test_recipe_decode_against_oracle's tolerance for that entry point."""
    torch, W, ctx = gpu
    key = "F1024_m24_a55_g0"
    F, m, alpha, gamma = gen.OPTIONS[key]
    c = fx[key + "/mc"]
    bap = c.astype(np.float32)
    bap[:, 0] = (c[:, 0] - 9.210340).astype(np.float32)
    mc = bap.astype(np.float64)
    mc[:, 0] += 9.210340
    x, _, st = run(gpu, mc, F, (len(mc),), alpha, gamma)
    assert (st == 0).all()
    b = W.WorldBatch(ctx, W.default_params(16000, 5.0, fft_size=F), f0_lengths=[len(mc)])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    try:
        _, _, ap = b.recipe_decode(dev(np.zeros(len(mc), dtype=np.float32)),
                                   dev(np.zeros((len(mc), 50), dtype=np.float32)), dev(bap))
        ap = ap.cpu().numpy()
    finally:
        b.close()
    got = np.exp(x[:, :24]) / 1e4
    print("bap decoder: worst relative difference %.3e" % (np.abs(got - ap[:, :24]) / ap[:, :24]).max())
    np.testing.assert_allclose(got, ap[:, :24], rtol=1e-11, atol=0)


@pytest.mark.parametrize("key", gen.ROUND_TRIPS)
def test_round_trip_with_the_encoder(gpu, fx, key):
    """mc -> |H| (out_format 3) -> mel_cepstrum(itr2 100, dd 1e-10) returns mc to within what the reference's own round
    trip leaves (rt_ref) times ten, or 64 ulp of the row's largest coefficient."""
    torch, W, ctx = gpu
    F, m, alpha, gamma = gen.OPTIONS[key]
    mc = fx[key + "/mc"]
    b = W.WorldBatch(ctx, W.default_params(16000, 5.0, fft_size=F), f0_lengths=uneven(len(mc)))
    try:
        sp, st = b.spectrum_from_mel_cepstrum(torch.from_numpy(np.ascontiguousarray(mc)).cuda(), alpha, gamma, 3)
        back, st2 = b.mel_cepstrum(sp, m, alpha, itr2=100, dd=1e-10)
        back, st, st2 = back.cpu().numpy(), st.cpu().numpy(), st2.cpu().numpy()
    finally:
        b.close()
    assert (st == 0).all() and (st2 == 0).all()
    check_rows(back, mc, float(fx[key + "/rt_ref"]), key + " round trip")

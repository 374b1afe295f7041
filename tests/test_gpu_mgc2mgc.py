"""WorldBatch.convert_mel_generalized_cepstrum (mgc2mgc_kernel) against the compiled reference's mgc2mgc, gnorm and ignorm
(test/sptkfunctions.cpp:221-254, :313-345) as recorded in tests/golden/sptk_mgc2mgc.npz by tools/gen_golden_mgc2mgc.py.

Tolerance per row: max(10 * sens, 64 ulp of the row's largest |value|), the project's rule for mgc2sp_kernel:
sens is per row the larger of the reference's response to a last-bit perturbation of its input and its own distance from
the chain in long double."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import mgc2mgc_reference as R

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_mgc2mgc as gen  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return np.load(gen.PATH)


def uneven(frames):
    """Utterance lengths that add up to `frames`, the first of a single frame."""
    return [1, frames - 1] if frames > 1 else [1]


def run(gpu, rows, opt, lengths=None, ctx=None):
    torch, W, ctx0 = gpu
    m1, a1, g1, n, u, m2, a2, g2, N, U = opt
    b = W.WorldBatch(ctx or ctx0, W.default_params(48000, 5.0), f0_lengths=list(lengths or uneven(len(rows))))
    try:
        out, st = b.convert_mel_generalized_cepstrum(torch.from_numpy(np.ascontiguousarray(rows)).cuda(), a1, g1, m2, a2,
                                                     g2, bool(n), bool(u), bool(N), bool(U))
        return out.cpu().numpy(), st.cpu().numpy()
    finally:
        b.close()


def check_rows(got, want, sens, what):
    err = np.abs(got - want).max(axis=1)
    tol = R.row_tol(want, sens)
    print("%s: max err %.3e  (least row tol %.3e, worst err / tol %.3f)" % (what, err.max(), tol.min(), (err / tol).max()))
    assert np.isfinite(got).all(), what
    assert (err <= tol).all(), (what, float(err.max()), float(tol.min()))


def same_bits(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("key", sorted(gen.OPTIONS))
def test_parity_against_reference(gpu, fx, key):
    opt, _ = gen.OPTIONS[key]
    out, st = run(gpu, fx[key + "/in"], opt)
    assert (st == 0).all()
    check_rows(out, fx[key + "/out"], fx[key + "/sens"], key)


@pytest.mark.parametrize("key", sorted(k for k, (o, _) in gen.OPTIONS.items() if o[2] == 0 and o[7] == 0 and not any(o[3:5] + o[8:])))
def test_gamma_0_to_gamma_0_is_the_references_bits(gpu, fx, key):
    """freqt, or the copy, alone: coefficients 1 .. m2 are the reference's expression in its order."""
    opt, _ = gen.OPTIONS[key]
    out, st = run(gpu, fx[key + "/in"], opt)
    assert (st == 0).all() and same_bits(out[:, 1:], fx[key + "/out"][:, 1:])


def test_flag_steps_are_the_restatements_bits(gpu, fx):
    """gen_wave's call, -n -u towards the same (alpha, gamma): coefficients k >= 1 bit for bit the numpy restatement's.
    Between the same (alpha, gamma) the reference's gc2gc is no copy -- c2[i] = ca[i] + (g ss2 - g ss1) / i with two sums
    that cancel only in exact arithmetic -- so this holds the flag steps, gnorm's division, ignorm's product AND the order
    of gc2gc's sums to the reference: towards m2 <= 64 the kernel keeps that order (csrc/mgc2mgc.hip).  It also rests on
    the device library's pow agreeing with numpy's on these twelve gains, which it does."""
    opt, _ = gen.OPTIONS[gen.GEN_WAVE]
    rows = fx[gen.GEN_WAVE + "/in"]
    out, st = run(gpu, rows, opt)
    want = R.convert_rows(rows, opt)
    differ = out[:, 1:] != want[:, 1:]
    ulps = np.abs(out[:, 1:] - want[:, 1:]) / np.spacing(np.abs(want[:, 1:]))
    print("-n -u: %d of %d coefficients differ from the restatement, by at most %.1f ulp; column 1: %d of %d" % (
        differ.sum(), differ.size, ulps.max(), differ[:, 0].sum(), len(rows)))
    assert (st == 0).all() and same_bits(out[:, 1:], want[:, 1:])


@pytest.mark.parametrize("key", ["f_nu", "f_u", "f_N", "f_NU", "f_U", "c24_g3_to_g0", "c8_g0_to_g1p"])
def test_elementwise_steps_are_the_restatements_bits_where_gc2gc_adds_nothing(gpu, fx, key):
    """a == 0 and i = 1: gc2gc's sums are empty, c2[1] = ca[1], so coefficient 1 is the flag steps, gnorm's division and
    ignorm's product alone, each the reference's expression without contraction, around pow / exp / log results that
    agree with numpy's on these rows.  (Towards m2 <= 64 the sums themselves are in the reference's order too: the test
    above.  This one does not depend on that.)"""
    opt, _ = gen.OPTIONS[key]
    assert R.warp(opt[1], opt[6]) == 0
    rows = fx[key + "/in"]
    out, st = run(gpu, rows, opt)
    assert (st == 0).all() and same_bits(out[:, 1], R.convert_rows(rows, opt)[:, 1])


def test_flagged_input_is_the_plain_input_of_the_restatement(gpu, fx):
    """-n -u, -u alone and -n alone: the rows the kernel makes of a flagged input are bit for bit the restatement's plain
    rows -- the same conversion of those plain rows, without input flags, returns the same bits in every coefficient."""
    for key, n, u in (("f_nu", 1, 1), ("f_u", 0, 1), ("f_nu_to_m127_a0_g1p", 1, 1), ("f_N", 1, 0)):
        opt, _ = gen.OPTIONS[key]
        m1, g1 = opt[0], opt[2]
        rows = fx[key + "/in"] if (opt[3], opt[4]) == (n, u) else R.convert_rows(
            fx[key + "/in"], R.option(m1, opt[1], g1, m1, opt[1], g1, N=1))          # -n alone: gain-normalized rows
        flagged = opt[:3] + (n, u) + opt[5:8] + (0, 0)
        plain_opt = opt[:3] + (0, 0) + opt[5:8] + (0, 0)
        plain = np.stack([R.plain_input(r, flagged) for r in rows])
        got, st = run(gpu, rows, flagged)
        want, st2 = run(gpu, plain, plain_opt)
        assert (st == 0).all() and (st2 == 0).all() and same_bits(got, want), key


def test_status_rows(gpu, fx):
    """A gain that is not positive and a NaN coefficient are status 1 and rows of zeros; their neighbours are what they
    are in a batch of their own.  A result that overflows is status 2."""
    opt = tuple(fx["S/opt"])
    rows = fx["S/in"]
    out, st = run(gpu, rows, gen.STATUS_OPT, (4,))
    assert opt == gen.STATUS_OPT and list(st) == list(fx["S/status"]) == [0, 1, 0, 1]
    assert (out[[1, 3]] == 0).all()
    good = np.array([0, 2])
    check_rows(out[good], fx["S/out"][good], fx["S/sens"][good], "S")
    for i in good:
        o1, s1 = run(gpu, rows[i:i + 1], gen.STATUS_OPT, (1,))
        assert s1[0] == 0 and same_bits(o1[0], out[i])
    # under -n the gain is c[0] itself
    key = "f_nu"
    nrows = fx[key + "/in"][:3].copy()
    nrows[1, 0] = -nrows[1, 0]
    out, st = run(gpu, nrows, gen.OPTIONS[key][0], (3,))
    assert list(st) == [0, 1, 0] and (out[1] == 0).all()
    check_rows(out[[0, 2]], fx[key + "/out"][[0, 2]], fx[key + "/sens"][[0, 2]], "-n, rows beside a negative gain")
    # gamma 0 -> 1 of c0 = 800: exp overflows, the result is not finite
    big = np.zeros((2, 9))
    big[0, 0] = 800.0
    out, st = run(gpu, big, R.option(8, 0, 0, 8, 0, 1), (2,))
    assert list(st) == [2, 0] and (out == 0).all()


def test_bits_do_not_depend_on_utterances_and_batches(gpu, fx):
    for key in ("c24_g3_to_m65_a0", "c2047_g0_to_m24_a55_g3", "f_nu_to_m127_a0_g1p"):
        opt, _ = gen.OPTIONS[key]
        rows = fx[key + "/in"]
        whole, st = run(gpu, rows, opt, (len(rows),))
        split, st2 = run(gpu, rows, opt, (1, 2, 4, len(rows) - 7))
        parts = [run(gpu, rows[a:b], opt, (b - a,))[0] for a, b in ((0, 5), (5, 6), (6, len(rows)))]
        assert (st == 0).all() and (st2 == 0).all()
        assert same_bits(whole, split) and same_bits(whole, np.concatenate(parts)), key


def test_rows_below_and_above_the_persistent_grid(gpu, fx):
    """A few rows, and more rows than the persistent grid holds workgroups (256 compute units x 8 waves x the context's
    oversubscription of 6 = 12 288 at the smallest class): every copy of a row is bit-identical to the first."""
    key = "c8_g0_to_g1p"
    opt, _ = gen.OPTIONS[key]
    rows = fx[key + "/in"]
    few, st = run(gpu, rows[:3], opt, (3,))
    reps = 30000 // len(rows)
    many, st2 = run(gpu, np.tile(rows, (reps, 1)), opt, (1, 7, 333, 12000, reps * len(rows) - 12341))
    assert (st == 0).all() and (st2 == 0).all()
    assert same_bits(many.reshape(reps, len(rows), -1), np.broadcast_to(many[:len(rows)], (reps,) + many[:len(rows)].shape))
    assert same_bits(few, many[:3])
    check_rows(many[:len(rows)], fx[key + "/out"], fx[key + "/sens"], "tiled " + key)


def test_bad_options_are_refused_before_any_launch(gpu):
    torch, W, ctx = gpu
    b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=[4])
    rows = lambda cols: torch.zeros(4, cols, dtype=torch.float64, device="cuda")
    ctx.timing_enable(True)
    try:
        for cols, args, kw in ((25, (1.0, 0.0, 24, 0.42, 0.0), {}), (25, (0.42, 0.0, 24, -1.0, 0.0), {}),
                               (25, (0.42, -1.5, 24, 0.42, 0.0), {}), (25, (0.42, 0.0, 24, 0.42, 1.5), {}),
                               (25, (0.42, 0.0, 0, 0.42, 0.0), {}), (25, (0.42, 0.0, 4096, 0.42, 0.0), {}),
                               (65, (0.42, 0.0, 64, 0.42, 0.0), {}), (4097, (0.0, 0.0, 24, 0.42, 0.0), {}),
                               (25, (0.42, 0.0, 24, 0.42, -0.5), dict(multiplied=True)),
                               (25, (0.42, -0.5, 24, 0.42, 0.0), dict(out_multiplied=True))):
            with pytest.raises(RuntimeError, match="bad argument"):
                b.convert_mel_generalized_cepstrum(rows(cols), *args, **kw)
        assert ctx.timing_query("mgc2mgc_kernel")[1] == 0
        out, st = b.convert_mel_generalized_cepstrum(rows(25), 0.42, -0.5, 30, 0.1, 1.0)
        assert ctx.timing_query("mgc2mgc_kernel")[1] == 1
        assert out.shape == (4, 31) and (st.cpu().numpy() == 0).all() and (out.cpu().numpy() == 0).all()
    finally:
        ctx.timing_enable(False)
        b.close()


def test_agrees_with_spectrum_from_mel_cepstrum(gpu):
    """Tie to mgc2sp_kernel: on sptk_mgc2sp_full.npz's F512_m24_a42_g3 rows the real part of the transform of
    convert(-> 256, 0, 0), zero-padded to 512, is spectrum_from_mel_cepstrum of the same rows.  Both kernels are held to
    the reference's mgc2mgc(-> 256, 0, 0) per coefficient by the rule's bound; a bin is a sum of 257 coefficients with
    weights of modulus 1, so the bins differ by at most the sum of the per-coefficient bounds, plus that key's sens_x
    for the other kernel's side."""
    torch, W, ctx = gpu
    g = np.load(os.path.join(GOLDEN, "sptk_mgc2sp_full.npz"))
    key = "F512_m24_a42_g3"
    F, m, alpha, gamma = g[key + "/opt"]
    F, m = int(F), int(m)
    mc = g[key + "/mc"]
    c, st = run(gpu, mc, R.option(m, alpha, gamma, F // 2, 0, 0))
    b = W.WorldBatch(ctx, W.default_params(16000, 5.0, fft_size=F), f0_lengths=[len(mc)])
    try:
        sp, st2 = b.spectrum_from_mel_cepstrum(torch.from_numpy(np.ascontiguousarray(mc)).cuda(), alpha, gamma)
        sp = sp.cpu().numpy()
    finally:
        b.close()
    assert (st == 0).all() and (st2.cpu().numpy() == 0).all()
    x = np.fft.rfft(c, F, axis=1).real
    sens_x = float(g[key + "/sens_x"])
    per_coefficient = np.maximum(10.0 * sens_x, 64.0 * np.spacing(np.abs(c).max(axis=1)))
    tol = (F // 2 + 1) * per_coefficient + sens_x
    err = np.abs(x - sp).max(axis=1)
    print("mgc2sp_kernel: max difference %.3e, worst / tol %.3e" % (err.max(), (err / tol).max()))
    assert (err <= tol).all()
    # and the compiled reference's ln |H| itself, by the same bound
    assert (np.abs(x - g[key + "/x"]).max(axis=1) <= tol).all()

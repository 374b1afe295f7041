"""WorldBatch.mel_cepstrum (mcep_kernel) against the compiled reference's mcep (test/sptkfunctions.cpp:11-184) as
recorded in tests/golden/sptk_mcep.npz by tools/gen_golden_mcep.py.

Tolerance per row: max(10 * sens, 64 ulp of max |mc| of the row), sens being the reference's own response to a
last-bit perturbation of its input (stored per option set and mode).  Convergence runs compare the frames the
generator found robust against a 1 % change of dd, and their share is asserted, so no case is skipped quietly."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_mcep as gen  # noqa: E402
from test_mel_cepstrum_host import expected_decoded_ap  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "sptk_mcep.npz"))


def case_rows(fx, case):
    return gen.case_input(case) if case.startswith("B") else fx["x_" + case]


def run(gpu, x, F, lengths, m, alpha, **opt):
    torch, W, ctx = gpu
    b = W.WorldBatch(ctx, W.default_params(16000, 5.0, fft_size=F), f0_lengths=list(lengths))
    try:
        mc, st = b.mel_cepstrum(torch.from_numpy(np.ascontiguousarray(x)).cuda(), m, alpha, **opt)
        return mc.cpu().numpy(), st.cpu().numpy()
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


def lengths_of(case, frames):
    return tuple(gen.A_UTTERANCES) if case == "A" else (frames,)


@pytest.mark.parametrize("key", sorted(gen.OPTIONS))
def test_fixed_iterations_against_reference(gpu, fx, key):
    """dd = 0: exactly itr2 = 0, 1, 2, 5 Newton steps on every frame; mcep then returns -1."""
    case, m, alpha, extra = gen.OPTIONS[key]
    F, frames = gen.CASE_SHAPE[case]
    x = case_rows(fx, case)
    opt = {k: v for k, v in extra.items() if k != "itr2"}             # itr2 belongs to the convergence run alone
    for k, itr2 in enumerate(fx["fixed_itr"]):
        mc, st = run(gpu, x, F, lengths_of(case, frames), m, alpha, itr1=2, itr2=int(itr2), dd=0.0, **opt)
        assert (st == -1).all()
        check_rows(mc, fx[key + "/fixed"][k], float(fx[key + "/sens_fixed"][k]), "%s itr2=%d" % (key, itr2))


@pytest.mark.parametrize("key", sorted(gen.OPTIONS))
def test_convergence_against_reference(gpu, fx, key):
    """SPTK's defaults itr1 2, itr2 30, dd 1e-3 on the frames whose stop decision is robust.  The `_short` option set
    has itr2 = 4 instead: there dd > 0 decides which frames stop (0) and which run out of steps (-1)."""
    case, m, alpha, extra = gen.OPTIONS[key]
    F, frames = gen.CASE_SHAPE[case]
    robust = fx[key + "/robust"]
    assert robust.mean() >= 0.9
    mc, st = run(gpu, case_rows(fx, case), F, lengths_of(case, frames), m, alpha, **extra)
    assert (st[robust] == fx[key + "/ret"][robust]).all()
    if "itr2" in extra:
        assert (st[robust] == -1).sum() >= 4 and (st[robust] == 0).sum() >= 4
    check_rows(mc[robust], fx[key + "/conv"][robust], float(fx[key + "/sens_conv"]), key + " conv")


def test_rows_the_reference_exits_on(gpu, fx):
    """Case D: an exact 0 in the periodogram is status 2; with f = 1e6 theq's first pivot is singular on every other
    frame (status 1) and the row keeps the initial estimate.  The neighbours of such rows are what they are alone."""
    x = fx["x_D"]
    mc, st = run(gpu, x, 512, (4,), 8, 0.42)
    assert list(st) == list(fx["D/status"]) == [0, 2, 0, 0]
    assert np.isfinite(mc).all() and (mc[1] == 0).all()
    ok = np.array([0, 2, 3])
    check_rows(mc[ok], fx["D/conv"][ok], float(fx["D/sens_conv"]), "D conv")
    for i in ok:                                                       # the same row in a batch of its own
        alone, st1 = run(gpu, x[i:i + 1], 512, (1,), 8, 0.42)
        assert st1[0] == 0 and (alone[0] == mc[i]).all()
    mc, st = run(gpu, x, 512, (4,), 8, 0.42, f=1e6)
    assert list(st) == list(fx["D/status_f1e6"]) == [1, 2, 1, 1]
    assert np.isfinite(mc).all() and (mc[1] == 0).all()
    check_rows(mc[ok], fx["D/init"][ok], float(fx["D/sens_init"]), "D singular: the initial estimate")


def test_bad_options_are_refused_before_any_launch(gpu, fx):
    torch, W, ctx = gpu
    b = W.WorldBatch(ctx, W.default_params(16000, 5.0, fft_size=512), f0_lengths=[4])
    x = torch.from_numpy(np.ascontiguousarray(fx["x_D"])).cuda()
    ctx.timing_enable(True)
    try:
        for m, alpha, opt, msg in ((0, 0.42, {}, "bad argument"), (64, 0.42, {}, "bad argument"),
                                   (8, 1.0, {}, "bad argument"), (8, -1.5, {}, "bad argument"),
                                   (8, 0.42, {"itr2": 1001}, "bad argument"), (8, 0.42, {"itr1": -1}, "bad argument"),
                                   (8, 0.42, {"etype": 2, "e": -60.0}, "unsupported configuration"),
                                   (8, 0.42, {"itype": 0}, "unsupported configuration"),
                                   (8, 0.42, {"itype": 2}, "unsupported configuration")):
            with pytest.raises(RuntimeError, match=msg):
                b.mel_cepstrum(x, m, alpha, **opt)
        assert ctx.timing_query("mcep_kernel")[1] == 0
        b.mel_cepstrum(x, 8, 0.42)
        assert ctx.timing_query("mcep_kernel")[1] == 1
    finally:
        ctx.timing_enable(False)
        b.close()


def test_grid_stride_walk_and_independence_from_placement(gpu, fx):
    """About 6 000 frames (more than one pass of the persistent grid), uneven utterances, one of a single frame: every
    copy of a row is bit-identical to the first, the first copies meet parity, and a second run repeats the first."""
    key = "A_m8_a42"
    reps = 250
    x = np.tile(fx["x_A"], (reps, 1))
    total = len(x)
    lengths = [1, 7, 333, 1024, 2, 1999]
    lengths.append(total - sum(lengths))
    assert total == 6000 and min(lengths) == 1 and lengths[-1] > 0
    mc, st = run(gpu, x, 512, lengths, 8, 0.42)
    mc2, st2 = run(gpu, x, 512, lengths, 8, 0.42)
    assert (mc == mc2).all() and (st == st2).all()
    assert (mc.reshape(reps, 24, 9) == mc[:24]).all() and (st.reshape(reps, 24) == st[:24]).all()
    robust = fx[key + "/robust"]
    assert robust.mean() >= 0.9 and (st[:24][robust] == fx[key + "/ret"][robust]).all()
    check_rows(mc[:24][robust], fx[key + "/conv"][robust], float(fx[key + "/sens_conv"]), "tiled A")


def test_decoder_inverts_the_encoder(gpu, fx):
    """Conventions (c0, alpha, scaling) agree with the existing decoder: the 1e4 * ap rows of case B at m = 24, rounded to
    float32 as `bap` with c0 - 9.210340, through WorldMi355RecipeDecode; expected from the FIXTURE's mc in numpy, with
    test_recipe_decode_against_oracle's tolerance for that entry point."""
    torch, W, ctx = gpu
    key = "B_cli"
    case, m, alpha, extra = gen.OPTIONS[key]
    x = case_rows(fx, case)[8:]
    mc, st = run(gpu, x, 1024, (len(x),), m, alpha, **extra)
    robust = fx[key + "/robust"][8:]
    want = fx[key + "/conv"][8:]
    check_rows(mc[robust], want[robust], float(fx[key + "/sens_conv"]), "B ap rows")

    def as_bap(c):
        bap = c.astype(np.float32)
        bap[:, 0] = (c[:, 0] - 9.210340).astype(np.float32)
        return bap
    bap = as_bap(mc)
    assert (bap[robust] == as_bap(want)[robust]).mean() > 0.99          # float32 hides the last bits
    b = W.WorldBatch(ctx, W.default_params(16000, 5.0, fft_size=1024), f0_lengths=[len(x)])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _, _, ap = b.recipe_decode(dev(np.zeros(len(x), dtype=np.float32)), dev(np.zeros((len(x), 50), dtype=np.float32)),
                               dev(bap))
    b.close()
    ap = ap.cpu().numpy()
    np.testing.assert_allclose(ap[robust, :24], expected_decoded_ap(as_bap(want), 1024, 0.55)[robust], rtol=1e-11, atol=0)

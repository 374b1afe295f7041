"""WorldBatch.mel_cepstrum_of_frames / mel_cepstrum_of_waveform (mgcep_kernel) against the compiled reference's mcep with
itype 0 (test/sptkfunctions.cpp:11-184) on tests/mgcep_reference.py's frames, as recorded in tests/golden/sptk_mgcep.npz
by tools/gen_golden_mgcep.py.

Tolerance per row: test_gpu_mel_cepstrum.py's, max(10 * sens, 64 ulp of max |mc| of the row), sens being the reference's
own response to a last-bit perturbation of the windowed frame (stored per option set and mode).  Fixed step counts are
compared on every frame the reference takes, the stop rule on the frames the generator found robust against a 1 % change
of dd, whose share is asserted.  A frame the reference exits on is status 2 and a row of zeros."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import mgcep_reference as ref

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_mgcep as gen  # noqa: E402
from test_gpu_mel_cepstrum import check_rows  # noqa: E402

pytestmark = pytest.mark.gpu

ROW_KEYS = sorted(k for k, v in gen.SETS.items() if v[0] == "rows")
WAVE_KEYS = sorted(k for k, v in gen.SETS.items() if v[0] != "rows")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "sptk_mgcep.npz"))


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_rows(gpu, rows, F, counts, m, alpha, ctx=None, **opt):
    torch, W, ctx0 = gpu
    b = W.WorldBatch(ctx or ctx0, W.default_params(16000, 5.0, fft_size=F), f0_lengths=list(counts))
    try:
        mc, st = b.mel_cepstrum_of_frames(dev(torch, rows), m, alpha, **opt)
        return mc.cpu().numpy(), st.cpu().numpy()
    finally:
        b.close()


def wave_batch(gpu, xs, F, L, P, ctx=None, counts=None):
    torch, W, ctx0 = gpu
    counts = [W.sptk_frames(len(x), L, P) for x in xs] if counts is None else counts
    return W.WorldBatch(ctx or ctx0, W.default_params(16000, 5.0, fft_size=F), x_lengths=[len(x) for x in xs],
                        f0_lengths=counts)


def run_wave(gpu, xs, F, L, P, table, f32, m, alpha, ctx=None, **opt):
    torch = gpu[0]
    b = wave_batch(gpu, xs, F, L, P, ctx)
    try:
        mc, st = b.mel_cepstrum_of_waveform(dev(torch, np.concatenate(xs)), table, L, P, m, alpha, f32, **opt)
        return mc.cpu().numpy(), st.cpu().numpy()
    finally:
        b.close()


def utterances(fx, group):
    x, at = fx["x_" + group].astype(np.float64), np.concatenate([[0], np.cumsum(fx["T_" + group])])
    return [x[at[k]:at[k + 1]] for k in range(len(at) - 1)]


def against_reference(fx, key, call):
    """call(**options) -> (mc, status) of the option set's batch: fixed step counts on every frame, then the stop rule."""
    extra = gen.SETS[key][9]
    exits = fx[key + "/exits"]
    taken = ~exits
    for k, itr2 in enumerate(fx["fixed_itr"]):
        mc, st = call(itr1=2, itr2=int(itr2), dd=0.0, **extra)
        assert (st[taken] == -1).all() and (st[exits] == 2).all() and (mc[exits] == 0).all()
        check_rows(mc[taken], fx[key + "/fixed"][k][taken], float(fx[key + "/sens_fixed"][k]), "%s itr2=%d" % (key, itr2))
    robust = fx[key + "/robust"]
    assert robust[taken].mean() >= 0.9
    mc, st = call(**extra)
    assert (st[robust] == fx[key + "/ret"][robust]).all() and (st[exits] == 2).all() and (mc[exits] == 0).all()
    assert np.isfinite(mc).all()
    check_rows(mc[robust], fx[key + "/conv"][robust], float(fx[key + "/sens_conv"]), key + " conv")
    return mc, st


@pytest.mark.parametrize("key", ROW_KEYS)
def test_rows_mode_against_reference(gpu, fx, key):
    """Orders 12, 49 (2 m + 1 > 64) and 63, alpha 0, 0.42 and 0.55, etype 0, 1 and 2 (e = -60) at F = 512."""
    group, F, L, P, kind, norm, f32, m, alpha, extra = gen.SETS[key]
    rows, counts = gen.set_frames(key)
    against_reference(fx, key, lambda **o: run_rows(gpu, rows, F, counts, m, alpha, **o))


@pytest.mark.parametrize("key", WAVE_KEYS)
def test_waveform_mode_against_reference_and_rows_mode(gpu, fx, key):
    """The seven utterances of 1 to 1203 samples in one batch, every frame length, shift, window, normalisation and pipe
    mode of the fixture, and the recipe's shape (F 2048, L 1200, P 240, m 49); then the same windowed frames through the
    rows mode: the same bits, only the gather differs."""
    W = gpu[1]
    group, F, L, P, kind, norm, f32, m, alpha, extra = gen.SETS[key]
    xs = utterances(fx, group)
    table = W.sptk_window(kind, norm, L)
    mc, st = against_reference(fx, key, lambda **o: run_wave(gpu, xs, F, L, P, table, f32, m, alpha, **o))
    rows, counts = ref.windowed_batch(xs, table, P, F, f32)
    assert counts == list(fx[key + "/counts"])
    mc_r, st_r = run_rows(gpu, rows, F, counts, m, alpha, **extra)
    assert (st == st_r).all() and (mc == mc_r).all()


def test_independent_of_batch_composition_and_stream(gpu, fx):
    """An utterance alone, in a batch of three and on a caller's non-blocking stream: the same bits."""
    torch, W, ctx = gpu
    xs = utterances(fx, "wave")
    F, L, P, m, alpha = 512, 400, 80, 12, 0.42
    table = W.sptk_window(1, 1, L)
    three = [xs[3], xs[5], xs[6]]
    mc3, st3 = run_wave(gpu, three, F, L, P, table, True, m, alpha)
    n0 = W.sptk_frames(len(three[0]), L, P)
    n1 = W.sptk_frames(len(three[1]), L, P)
    alone, st1 = run_wave(gpu, [three[1]], F, L, P, table, True, m, alpha)
    assert len(alone) == n1 and (alone == mc3[n0:n0 + n1]).all() and (st1 == st3[n0:n0 + n1]).all()
    side = torch.cuda.Stream()                                         # torch's own streams do not wait for stream 0
    ctx2 = W.Context(stream_ptr=side.cuda_stream)
    try:
        with torch.cuda.stream(side):
            other, st2 = run_wave(gpu, [three[1]], F, L, P, table, True, m, alpha, ctx=ctx2)
        side.synchronize()
    finally:
        ctx2.close()
    assert (other == alone).all() and (st2 == st1).all()


def test_rows_the_reference_exits_on(gpu, fx):
    """A stretch of digital zero longer than the frame: at etype 0 the frames inside it are status 2 and zeros, and every
    other frame is what it is in a batch without them; with eps 1e-8 all frames are analysed.  An all-zero row at etype 2:
    the floor of a zero maximum is zero, status 2."""
    torch, W, ctx = gpu
    F, L, P, m, alpha = 512, 400, 80, 12, 0.42
    x = utterances(fx, "rows")[0].copy()
    x[600:1300] = 0.0
    table = W.sptk_window(1, 1, L)
    rows, counts = ref.windowed_batch([x], table, P, F, False)
    silent = ~rows.any(axis=1)
    assert list(np.nonzero(silent)[0]) == [10, 11, 12, 13]            # 80 j - 200 in [600, 900]
    mc, st = run_wave(gpu, [x], F, L, P, table, False, m, alpha)
    assert (st[silent] == 2).all() and (mc[silent] == 0).all()
    assert np.isin(st[~silent], (-1, 0)).all() and np.isfinite(mc).all()
    mc_n, st_n = run_rows(gpu, rows[~silent], F, [int((~silent).sum())], m, alpha)
    assert (mc[~silent] == mc_n).all() and (st[~silent] == st_n).all()
    mc, st = run_wave(gpu, [x], F, L, P, table, False, m, alpha, etype=1, e=1e-8)
    assert (st >= -1).all() and (st != 2).all() and np.isfinite(mc).all()
    assert (mc[~silent] != 0).any(axis=1).all() and (mc[silent] != 0).any(axis=1).all()
    mc, st = run_rows(gpu, rows, F, counts, m, alpha, etype=2, e=-60.0)
    assert (st[silent] == 2).all() and (mc[silent] == 0).all() and np.isin(st[~silent], (-1, 0)).all()


def test_bad_calls_are_refused_before_any_launch(gpu, fx):
    torch, W, ctx = gpu
    F, L, P = 512, 400, 80
    x = utterances(fx, "wave")[5]
    xd = dev(torch, x)
    table = W.sptk_window(1, 1, L)
    b = wave_batch(gpu, [x], F, L, P)
    rows = dev(torch, ref.windowed(x, table, P, F))
    off = wave_batch(gpu, [x], F, L, P, counts=[W.sptk_frames(len(x), L, P) + 1])
    off_mc = None
    ctx.timing_enable(True)
    try:
        for opt in ({"itype": 3}, {"itype": 4}, {"itype": 1}, {"etype": 2, "e": 0.0}, {"etype": 2, "e": 3.0},
                    {"etype": 1, "e": -1.0}, {"etype": 3}, {"itr2": 1001}):
            with pytest.raises(RuntimeError, match="bad argument"):
                b.mel_cepstrum_of_frames(rows, 12, 0.42, **opt)
            with pytest.raises(RuntimeError, match="bad argument"):
                b.mel_cepstrum_of_waveform(xd, table, L, P, 12, 0.42, **opt)
        for m, alpha in ((0, 0.42), (64, 0.42), (12, 1.0)):
            with pytest.raises(RuntimeError, match="bad argument"):
                b.mel_cepstrum_of_frames(rows, m, alpha)
        for Lx, Px in ((F + 1, 80), (L, 0), (L, L + 1)):
            with pytest.raises(RuntimeError, match="bad argument"):
                b.mel_cepstrum_of_waveform(xd, np.ones(Lx), Lx, Px, 12, 0.42)
        with pytest.raises(RuntimeError, match="bad argument"):         # f0_lengths off by one
            off_mc = off.mel_cepstrum_of_waveform(xd, table, L, P, 12, 0.42)
        assert off_mc is None and ctx.timing_query("mgcep_kernel")[1] == 0
        b.mel_cepstrum_of_waveform(xd, table, L, P, 12, 0.42)
        b.mel_cepstrum_of_frames(rows, 12, 0.42)
        assert ctx.timing_query("mgcep_kernel")[1] == 2 and ctx.timing_query("mcep_kernel")[1] == 0
    finally:
        ctx.timing_enable(False)
        b.close()
        off.close()
    # what mel_cepstrum refuses is what it refused
    b = W.WorldBatch(ctx, W.default_params(16000, 5.0, fft_size=F), f0_lengths=[4])
    try:
        sp = torch.ones(4, F // 2 + 1, dtype=torch.float64, device="cuda")
        for opt in ({"itype": 0}, {"etype": 2, "e": -60.0}):
            with pytest.raises(RuntimeError, match="unsupported configuration"):
                b.mel_cepstrum(sp, 8, 0.42, **opt)
    finally:
        b.close()

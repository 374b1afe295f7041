"""The f0 estimator of the one-call forms (WorldMi355BatchSetF0Estimator): Harvest or Dio, with StoneMask or without.

The chain's definition is the composition of the reference's functions, so it is held to two things: bit for bit to the
library's own stages called one by one (plain and forked order, cold and warm), and to the oracle's
harvest -> [stonemask] -> cheaptrick -> d4c -> synthesis within the bounds test_gpu_parity.py defines, with the
voiced / unvoiced decision identical on every frame.  Shapes: the two utterances (0.3 s, 0.5 s at 16 kHz, 5 ms) on which
test_gpu_caller_stream.py already holds Harvest to the oracle, and one utterance at 48 kHz."""
import importlib

import numpy as np
import pytest

from test_gpu_caller_stream import DelayedBatch, env  # noqa: F401 -- `env` is a fixture (its own instance for this module)
from test_gpu_parity import AP_TOL, F0_TOL, Y_TOL, cat, sp_close

pytestmark = pytest.mark.gpu
sd = importlib.import_module("hts-train-world_amd.synth_data")

FS = 16000
SETTINGS = [("harvest", False), ("harvest", True), ("dio", False), ("dio", True)]


def host(t):
    return t.cpu().numpy()


class Case:
    """Utterances at one rate on the device, and what is computed once for them: the stages one by one per setting (on a
    batch of their own) and the oracle's chain per setting."""

    def __init__(self, gpu, oracle, fs, xs):
        self.torch, self.W, self.ctx = gpu
        self.oracle, self.fs, self.xs = oracle, fs, xs
        self.lens = [len(x) for x in xs]
        self.x = self.torch.from_numpy(np.concatenate(xs)).cuda()
        self.params = self.W.default_params(fs, 5.0)
        self._staged, self._oracle = {}, {}

    def batch(self, estimator="dio", refine=True):
        return self.W.WorldBatch(self.ctx, self.params, x_lengths=self.lens, f0_estimator=estimator, refine=refine)

    def staged(self, estimator, refine):
        key = (estimator, refine)
        if key not in self._staged:
            b = self.batch()                                   # a batch of its own, at a new batch's setting
            t, f0 = b.harvest(self.x) if estimator == "harvest" else b.dio(self.x)
            if refine:
                f0 = b.stonemask(self.x, t, f0)
            sp = b.cheaptrick(self.x, t, f0)
            ap = b.d4c(self.x, t, f0)
            y = b.synthesize(f0, sp, ap)
            self.torch.cuda.synchronize()
            b.close()
            self._staged[key] = (t, f0, sp, ap, y)
        return self._staged[key]

    def reference(self, refine):
        """oracle.harvest -> [stonemask] -> cheaptrick -> d4c -> synthesis per utterance."""
        if refine not in self._oracle:
            o, fs, rs = self.oracle, self.fs, []
            F = o.cheaptrick_fft_size(fs)
            for x in self.xs:
                t, f0 = o.harvest(x, fs, 5.0)
                if refine:
                    f0 = o.stonemask(x, fs, t, f0)
                sp = o.cheaptrick(x, fs, t, f0, -0.15, F)
                ap = o.d4c(x, fs, t, f0, F, 0.0)
                rs.append(dict(t=t, f0=f0, sp=sp, ap=ap, y=o.synthesis(f0, sp, ap, F, 5.0, fs)))
            self._oracle[refine] = rs
        return self._oracle[refine]


@pytest.fixture(scope="module")
def case16(gpu, oracle):
    return Case(gpu, oracle, FS, [sd.make_utterance(200, FS, duration=0.3), sd.make_utterance(202, FS, duration=0.5)])


@pytest.fixture(scope="module")
def case48(gpu, oracle):
    return Case(gpu, oracle, 48000, [sd.make_utterance(4, 48000, duration=0.8)])


def same_bits(torch, got, want, what):
    for name, g, w in zip(("t", "f0", "sp", "ap", "y"), got, want):
        assert g.shape == w.shape and torch.equal(g, w), "%s: %s differs from the stages called one by one" % (what, name)


def chain_is_its_stages(case, estimator, refine):
    torch = case.torch
    want = case.staged(estimator, refine)
    b = case.batch(estimator, refine)
    same_bits(torch, b.analyze(case.x), want[:4], "analyze, plain order")
    same_bits(torch, b.analyze(case.x), want[:4], "analyze, forked order")
    b.close()
    b = case.batch(estimator, refine)
    same_bits(torch, b.analyze_synthesize(case.x), want, "analyze_synthesize, cold")
    same_bits(torch, b.analyze_synthesize(case.x), want, "analyze_synthesize, warm")
    same_bits(torch, b.analyze(case.x), want[:4], "analyze after analyze_synthesize")
    b.close()


def meets_the_oracle(got, rs):
    t, f0, sp, ap, y = (host(v) for v in got)
    np.testing.assert_array_equal(t, cat(rs, "t"))
    ref = cat(rs, "f0")
    assert (ref > 0).any() and (ref == 0).any()                    # both decisions occur
    assert ((f0 > 0) == (ref > 0)).all()                           # V/UV on every frame, none left out
    print("max|df0| %.3e  max rel sp %.3e  max|dap| %.3e  max|dy| %.3e" % (
        np.abs(f0 - ref).max(), np.abs(sp / cat(rs, "sp") - 1).max(), np.abs(ap - cat(rs, "ap")).max(),
        np.abs(y - cat(rs, "y")).max()))
    np.testing.assert_allclose(f0, ref, atol=F0_TOL, rtol=0)
    sp_close(sp, cat(rs, "sp"))
    np.testing.assert_allclose(ap, cat(rs, "ap"), atol=AP_TOL, rtol=0)
    np.testing.assert_allclose(y, cat(rs, "y"), atol=Y_TOL, rtol=0)


@pytest.mark.parametrize("estimator,refine", SETTINGS)
def test_the_chain_is_its_stages_bit_for_bit(case16, estimator, refine):
    chain_is_its_stages(case16, estimator, refine)


def test_a_new_batch_is_dio_with_stonemask_and_the_setter_checks_its_arguments(case16):
    import ctypes as C
    W = case16.W
    L = W.load_library()
    b = case16.batch()
    est, ref = C.c_int(-1), C.c_int(-1)
    assert L.WorldMi355BatchGetF0Estimator(b.handle, C.byref(est), C.byref(ref)) == 0 and (est.value, ref.value) == (0, 1)
    assert (b.f0_estimator, b.refine) == ("dio", True)
    for bad in ((2, 1), (-1, 1), (1, 2), (0, -1)):
        assert L.WorldMi355BatchSetF0Estimator(b.handle, *bad) == 2
    assert L.WorldMi355BatchGetF0Estimator(b.handle, C.byref(est), C.byref(ref)) == 0 and (est.value, ref.value) == (0, 1)
    with pytest.raises(ValueError):
        b.set_f0_estimator("yin")
    b.set_f0_estimator("harvest", False)
    assert L.WorldMi355BatchGetF0Estimator(b.handle, C.byref(est), C.byref(ref)) == 0 and (est.value, ref.value) == (1, 0)
    b.close()
    # a batch made without x_lengths has nothing to estimate f0 from
    s = W.WorldBatch(case16.ctx, case16.params, f0_lengths=[20, 30])
    assert L.WorldMi355BatchSetF0Estimator(s.handle, 1, 1) == 2
    with pytest.raises(RuntimeError, match="bad argument"):
        s.set_f0_estimator("harvest")
    s.close()
    with pytest.raises(RuntimeError, match="bad argument"):
        W.WorldBatch(case16.ctx, case16.params, f0_lengths=[20, 30], f0_estimator="harvest")


def test_switching_estimators_on_one_batch(case16):
    torch = case16.torch
    b = case16.batch()
    for estimator, refine in (("dio", True), ("harvest", True), ("dio", True), ("harvest", False), ("dio", False)):
        b.set_f0_estimator(estimator, refine)
        same_bits(torch, b.analyze(case16.x), case16.staged(estimator, refine)[:4], "%s, refine %d" % (estimator, refine))
    b.set_f0_estimator("harvest", True)
    same_bits(torch, b.analyze_synthesize(case16.x), case16.staged("harvest", True), "cold, harvest")
    b.set_f0_estimator("dio", True)
    same_bits(torch, b.analyze_synthesize(case16.x), case16.staged("dio", True), "warm, dio")
    b.set_f0_estimator("harvest", False)
    same_bits(torch, b.analyze_synthesize(case16.x), case16.staged("harvest", False), "warm, harvest alone")
    b.close()


@pytest.mark.parametrize("refine", [False, True])
def test_harvest_chain_against_the_oracle(case16, refine):
    b = case16.batch("harvest", refine)
    meets_the_oracle(b.analyze_synthesize(case16.x), case16.reference(refine))
    meets_the_oracle(b.analyze_synthesize(case16.x), case16.reference(refine))       # warm: the forked order
    b.close()


def test_harvest_chain_at_48_khz(case48):
    """Harvest's pick from its 1 ms contour at a 5 ms hop feeding CheapTrick at fft_size 2048 and D4C at 4096."""
    chain_is_its_stages(case48, "harvest", False)
    b = case48.batch("harvest", False)
    assert b.fft_size == 2048
    meets_the_oracle(b.analyze_synthesize(case48.x), case48.reference(False))
    b.close()


def test_harvest_chain_on_a_callers_non_blocking_stream(env, case16):  # noqa: F811
    """The method of test_gpu_caller_stream.py: the call is issued behind a delay kernel and ahead of its input on a
    non-blocking stream; it returns while the delay still runs, and what is cloned on that stream meets the oracle."""
    torch = env.torch
    stale = [sd.make_utterance(202, FS, duration=0.3), sd.make_utterance(200, FS, duration=0.5)]
    assert [len(x) for x in stale] == case16.lens
    rs = case16.reference(False)
    with torch.cuda.stream(env.U):
        b = DelayedBatch(env, env.ctx, case16.params, x_lengths=case16.lens)
        for w in (b._b, b._twin):
            w.set_f0_estimator("harvest", False)
        fresh_x = torch.from_numpy(np.concatenate(case16.xs)).cuda()
        stale_x = torch.from_numpy(np.concatenate(stale)).cuda()
        env.U.synchronize()
        for order in ("forked (the warm-up took the plain order)", "forked again"):
            t, f0, sp, ap = b.analyze(fresh_x, _stale=[stale_x])
            assert env.pending["analyze"][-1], order
            np.testing.assert_array_equal(host(t), cat(rs, "t"))
            ref = cat(rs, "f0")
            assert ((host(f0) > 0) == (ref > 0)).all()
            np.testing.assert_allclose(host(f0), ref, atol=F0_TOL, rtol=0)
            sp_close(host(sp), cat(rs, "sp"))
            np.testing.assert_allclose(host(ap), cat(rs, "ap"), atol=AP_TOL, rtol=0)
        b.close()
    env.U.synchronize()
    differed, env.mismatches[:] = list(env.mismatches), []
    assert not differed, "other bits on a caller's stream than on the stream-0 context: %s" % differed


def test_host_pipeline_takes_the_estimator(case16):
    """pipeline.HostPipeline(f0_estimator=, refine=): the float32 features of a step are those of an in-memory batch with
    the same setting on the same int16 samples, and not Dio's."""
    torch = case16.torch
    pipeline = importlib.import_module("hts-train-world_amd.pipeline")
    pcm = pipeline.to_int16(np.concatenate(case16.xs))
    xq = torch.from_numpy(pcm.astype(np.float64) / 32768.0).cuda()
    got = {}
    for estimator, refine in (("harvest", False), ("dio", True)):
        pl = pipeline.HostPipeline(case16.ctx, case16.params, case16.lens, synthesis=True, f0_estimator=estimator,
                                   refine=refine)
        assert (pl.batch.f0_estimator, pl.batch.refine) == (estimator, refine)
        for _ in range(2):                                         # cold, then the overlapped order
            pl.input_buffer()[:] = pcm
            pl.feed()
            f0, sp, ap, y = (v.copy() for v in pl.result(pl.submit()))
        pl.close()
        b = case16.batch(estimator, refine)
        t, f0w, spw, apw, yw = b.analyze_synthesize(xq)
        assert torch.equal(torch.from_numpy(f0), f0w.float().cpu()) and torch.equal(torch.from_numpy(sp), spw.float().cpu())
        assert torch.equal(torch.from_numpy(ap), apw.float().cpu())
        assert torch.equal(torch.from_numpy(y), b.samples_to_pcm16(yw).cpu())
        b.close()
        got[estimator] = f0
    assert (got["harvest"] != got["dio"]).any()


def test_too_short_is_dios_rule(gpu):
    """0.3 s and 0.03 s: seven frames are no more than Dio's voice_range_minimum (dio.cpp:263-266), and Harvest has no
    such rule.  The flag depends on the frame count alone: nothing is analysed here."""
    torch, W, ctx = gpu
    xs = [sd.make_utterance(200, FS, duration=0.3), sd.make_utterance(202, FS, duration=0.03)]
    b = W.WorldBatch(ctx, W.default_params(FS, 5.0), x_lengths=[len(v) for v in xs])
    assert np.diff(b.frame_offsets).tolist() == [61, 7]
    x = torch.from_numpy(np.concatenate(xs)).cuda()
    zeros = torch.zeros(b.total_frames, dtype=torch.float64, device="cuda")
    assert b.utterance_status(x, f0=zeros).tolist() == [0, 2]
    b.set_f0_estimator("harvest", True)
    assert b.utterance_status(x, f0=zeros).tolist() == [0, 0]
    b.set_f0_estimator("dio", False)
    assert b.utterance_status(x, f0=zeros).tolist() == [0, 2]
    b.close()

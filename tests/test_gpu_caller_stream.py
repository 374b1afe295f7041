"""Every entry point that queues device work, on a caller's own NON-BLOCKING stream, against the references and bounds
the suite already holds it to on stream 0.

The rest of the suite runs the library on HIP's legacy default stream, which orders with every blocking stream and with
every synchronous copy: a launch that lost its stream argument, a side stream that was never forked from the caller's
or never joined back, a synchronous copy into a block that queued work still reads -- none of them can show there.
Here the context sits on a torch side stream U (non-blocking), and every call is made like this:

  1  two valid inputs of one shape: `fresh`, whose reference is known, and `stale` (another utterance, or the same rows
     shifted by a frame: real data either way; `stale` never holds NaN or garbage -- a kernel that reads too early
     computes a legitimate, different result.  `fresh` holds a NaN in two places only, each the documented input of
     its entry point and never an index: the sample that samples_to_pcm16 writes as 0 (test_pcm16_conversions, reused)
     and the sample that utterance_status flags);
  2  one warm-up call on `stale` (tables, workspaces, function attributes, the randn table), then U.synchronize();
  3  on U: a delay kernel of about 50 ms, an event, the copy of `fresh` over `stale` -- and the library call at once;
  4  right after the call returns the event must NOT have completed (entry points of caller_stream_table.py's
     ASYNC: the call was issued ahead of its input); the results are cloned on U, U alone is synchronised, and the
     clones meet the reference.

Work on stream 0, or on a side stream not forked from U, reads `stale`; work not joined back into U leaves the clone
with the warm-up's result.  Either way the reference of `fresh` is missed.  Secondary: the clones equal, bit for bit, the
same call on the session's stream-0 context.

The entry points' own tests are reused as they are (their references, their bounds, their shapes): they are called with
a `gpu` triple whose WorldBatch is DelayedBatch below, which makes every covered method go through steps 2-4.  WORLD's
stages are held to the oracle on two utterances of 0.3 s and 0.5 s directly.
"""
import functools
import importlib
import os

import numpy as np
import pytest

from caller_stream_table import ASYNC, COVERED, SYNCHRONISES
from conftest import GOLDEN

import dnn_reference as DR
import dnn_train_reference as DT
import dtw_cases as K_DTW
import gv_cases as K_GV
import mlpg_reference as M
import mlsa_reference as R_MLSA
import modify_reference as mr
import optimizer_reference as O
import test_gpu_dnn as T_DNN
import test_gpu_dnn_train as T_TRAIN
import test_gpu_ffo as T_FFO
import test_gpu_label_features as T_LABEL
import test_gpu_mel_cepstrum as T_MCEP
import test_gpu_mgc2mgc as T_MGC2MGC
import test_gpu_mgc2sp as T_MGC2SP
import test_gpu_mgcep as T_MGCEP
import test_gpu_mlpg as T_MLPG
import test_gpu_mlpg_gv as T_GV
import test_gpu_mlsa as T_MLSA
import test_gpu_modify as T_MOD
import test_gpu_mspf as T_MSPF
import test_gpu_parity as T_WORLD
import test_gpu_postfilter as T_MCPF
import test_gpu_trj as T_TRJ
import test_vibrato as T_VIB
import label_features_reference as LR
import trj_reference as TR
from test_gpu_parity import AP_TOL, F0_TOL, Y_TOL, cat, oracle_chain, sp_close

pytestmark = pytest.mark.gpu
sd = importlib.import_module("hts-train-world_amd.synth_data")

def _walk(obj, torch, f):
    """obj with f applied to every tensor in it (lists, tuples and dicts are walked; the rest is kept)."""
    if torch.is_tensor(obj):
        return f(obj)
    if isinstance(obj, (list, tuple)):
        return type(obj)(_walk(o, torch, f) for o in obj)
    if isinstance(obj, dict):
        return {k: _walk(v, torch, f) for k, v in obj.items()}
    return obj


def _same_bits(a, b, torch):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and \
            a.contiguous().cpu().numpy().tobytes() == b.contiguous().cpu().numpy().tobytes()
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same_bits(x, y, torch) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same_bits(a[k], b[k], torch) for k in a)
    return a == b


class Env:
    """The streams, the context on U, the delay, and the record of which call was still ahead of its input."""

    def __init__(self, torch, W, ctx0):
        self.torch, self.W, self.ctx0 = torch, W, ctx0
        self.U, self.V = torch.cuda.Stream(), torch.cuda.Stream()
        assert self.U.cuda_stream != 0 and self.V.cuda_stream not in (0, self.U.cuda_stream)
        self.ctx = W.Context(stream_ptr=self.U.cuda_stream)
        self.default = torch.cuda.default_stream()
        self.pending = {}                                  # entry point -> [the delay was still running at its return]
        self.mismatches = []                               # entry points whose bits differed from the stream-0 context's
        self.tests_run = set()                             # the test functions of this file that have started
        self.proxy = WProxy(self)
        self.gpu = (torch, self.proxy, self.ctx)           # what the entry points' own tests take as `gpu`
        self._calibrate()

    def _timed(self, stream, work):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            work()
            b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b)

    def _calibrate(self):
        """A delay of about 50 ms on one stream, measured with two events: torch.cuda._sleep where there is one, else
        a chain of matrix products.  Bounded: one kernel (or a fixed number of them) of known length."""
        torch = self.torch
        if hasattr(torch.cuda, "_sleep"):
            unit, spin, self.delay_kind = 2_000_000, (lambda n: torch.cuda._sleep(int(n))), "torch.cuda._sleep"
        else:
            m = torch.randn(2048, 2048, device="cuda")
            unit, self.delay_kind = 8, "matmul chain"

            def spin(n):
                acc = m
                for _ in range(int(n)):
                    acc = (acc @ m) * 1e-2
        self._timed(self.U, lambda: spin(unit))             # the first launch pays for loading the kernel
        ms = self._timed(self.U, lambda: spin(unit))
        for _ in range(3):                                  # too short to measure: a longer probe, three times at most
            if ms >= 0.5:
                break
            unit *= 10
            ms = self._timed(self.U, lambda: spin(unit))
        assert ms >= 0.5, ms
        n = max(1, int(unit * 50.0 / ms))
        ms = self._timed(self.U, lambda: spin(n))
        if not 30.0 <= ms <= 100.0:                          # clocks settle: scale once more
            n = max(1, int(n * 50.0 / ms))
            ms = self._timed(self.U, lambda: spin(n))
        self.delay_ms, self._spin = ms, functools.partial(spin, n)
        print("caller-stream delay: %s(%d) measured %.1f ms" % (self.delay_kind, n, ms))
        assert 20.0 <= ms <= 200.0, ms

    def delay(self):
        """Queue the delay on the current stream (U, or V where a test says so); the event that follows it."""
        torch = self.torch
        self._spin()
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        return ev

    def note(self, name, pending):
        self.pending.setdefault(name, []).append(bool(pending))
        if name in ASYNC:
            assert pending, "%s returned after the %.0f ms delay queued ahead of it: it waits for the stream " \
                            "somewhere (find the line, move it to SYNCHRONISES)" % (name, self.delay_ms)

    def behind_delay(self, tensors, fresh, call):
        """Step 3: `tensors` hold stale data; queue the delay, the event and the copies of `fresh`, then call at once.
        Returns (what the call returned, the event, whether the event was still pending at the call's return)."""
        done = self.delay()
        for t, f in zip(tensors, fresh):
            t.copy_(f)
        out = call()
        return out, done, not done.query()

    def pending_call(self, name, real, twin, args, kwargs, twin_args, stale=None):
        torch = self.torch
        seen, tensors = set(), []

        def collect(t):
            key = (t.data_ptr(), tuple(t.shape), tuple(t.stride()))
            if t.is_cuda and t.numel() and key not in seen:
                seen.add(key)
                tensors.append(t)
            return t
        _walk((args, kwargs), torch, collect)
        fresh = [t.clone() for t in tensors]
        if stale is None:                                   # the same rows one frame on: real data of the same kind
            stale = [torch.roll(t, 1, 0) for t in tensors]  # (a NaN that a reused test feeds on purpose becomes 0 here)
            stale = [torch.nan_to_num(t, nan=0.0) if t.is_floating_point() else t for t in stale]
        assert len(stale) == len(tensors) and all(s.shape == t.shape and s.dtype == t.dtype for s, t in zip(stale, tensors))
        for t, s in zip(tensors, stale):
            t.copy_(s)
        real(*args, **kwargs)                               # step 2: the warm-up, on stale
        self.U.synchronize()
        out, done, pending = self.behind_delay(tensors, fresh, lambda: real(*args, **kwargs))
        got = _walk(out, torch, lambda t: t.clone())        # step 4: read through U only
        self.U.synchronize()
        assert done.query()
        self.note(name, pending)
        if twin is not None:                                # the same call on the stream-0 context: the same bits
            with torch.cuda.stream(self.default):
                want = twin(*twin_args, **kwargs)
                torch.cuda.synchronize()
            if not _same_bits(got, want, torch):              # asserted when the test ends: its reference check comes first
                self.mismatches.append(name)
        return got


class DelayedBatch:
    """A WorldBatch on the caller's-stream context whose covered methods go through Env.pending_call, and its twin on
    the session's stream-0 context.  `_stale=[...]` names the stale data of the call's tensors, in argument order."""

    def __init__(self, env, ctx, params, x_lengths=None, f0_lengths=None, y_lengths=None):
        self._env = env
        self._b = env.W.WorldBatch(ctx, params, x_lengths, f0_lengths, y_lengths)
        with env.torch.cuda.stream(env.default):
            self._twin = env.W.WorldBatch(env.ctx0, params, x_lengths, f0_lengths, y_lengths)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        attr = getattr(self._b, name)
        if name not in COVERED:
            return attr

        def call(*args, _stale=None, **kwargs):
            twin_args = tuple(a._twin if isinstance(a, DelayedFeatureSet) else a for a in args)
            real_args = tuple(a._set if isinstance(a, DelayedFeatureSet) else a for a in args)
            return self._env.pending_call(name, attr, getattr(self._twin, name), real_args, kwargs, twin_args, _stale)
        return call

    def close(self):
        self._b.close()
        self._twin.close()


class DelayedFeatureSet:
    def __init__(self, env, ctx, features):
        self._set = env.W.LabelFeatureSet(ctx, features)
        self._twin = env.W.LabelFeatureSet(env.ctx0, features)
        self.n_features = self._set.n_features

    def close(self):
        self._set.close()
        self._twin.close()


class WProxy:
    """The world module with WorldBatch and LabelFeatureSet replaced by the delayed ones."""

    def __init__(self, env):
        self._env = env

    def __getattr__(self, name):
        return getattr(self._env.W, name)

    def WorldBatch(self, ctx, params, x_lengths=None, f0_lengths=None, y_lengths=None):
        return DelayedBatch(self._env, ctx, params, x_lengths, f0_lengths, y_lengths)

    def LabelFeatureSet(self, ctx, features):
        return DelayedFeatureSet(self._env, ctx, features)


@pytest.fixture(scope="module")
def env(gpu):
    torch, W, ctx0 = gpu
    e = Env(torch, W, ctx0)
    yield e
    with torch.cuda.stream(e.U):
        e.ctx.close()
    torch.cuda.synchronize()


@pytest.fixture(autouse=True)
def on_the_callers_stream(env, request):
    """Everything in this module runs with U as torch's current stream: the tensors the wrapper allocates are U's."""
    env.tests_run.add(request.node.originalname)
    with env.torch.cuda.stream(env.U):
        yield
    env.U.synchronize()
    differed, env.mismatches[:] = list(env.mismatches), []
    assert not differed, "other bits on a caller's stream than on the stream-0 context: %s" % differed


FS = 16000


@pytest.fixture(scope="module")
def world(env, oracle):
    """Two utterances of 0.3 s and 0.5 s, their oracle results, and two other utterances of the same lengths (stale)."""
    torch = env.torch
    fresh = [sd.make_utterance(200, FS, duration=0.3), sd.make_utterance(202, FS, duration=0.5)]
    stale = [sd.make_utterance(202, FS, duration=0.3), sd.make_utterance(200, FS, duration=0.5)]
    rs, ss = [oracle_chain(oracle, x, FS) for x in fresh], [oracle_chain(oracle, x, FS) for x in stale]
    f0 = cat(rs, "f0")
    assert (f0 > 0).any() and (f0 == 0).any() and (cat(ss, "f0") > 0).any() and (cat(ss, "f0") == 0).any()
    with torch.cuda.stream(env.U):
        b = DelayedBatch(env, env.ctx, env.W.default_params(FS, 5.0), x_lengths=[len(x) for x in fresh])
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        fd = {k: dev(cat(rs, k)) for k in ("t", "f0d", "f0", "sp", "ap")}
        st = {k: dev(cat(ss, k)) for k in ("t", "f0d", "f0", "sp", "ap")}
        fd["x"], st["x"] = dev(np.concatenate(fresh)), dev(np.concatenate(stale))
        env.U.synchronize()
    yield b, rs, fd, st, fresh
    with torch.cuda.stream(env.U):
        b.close()


def host(t):
    return t.cpu().numpy()


def test_the_context_is_on_a_non_blocking_stream_of_its_own(env):
    assert env.U.cuda_stream != 0 and env.torch.cuda.current_stream() == env.U
    print("delay %.1f ms (%s)" % (env.delay_ms, env.delay_kind))


def test_f0_stages(env, world, oracle):
    b, rs, fd, st, fresh = world
    t, f0d = b.dio(fd["x"], _stale=[st["x"]])
    np.testing.assert_array_equal(host(t), cat(rs, "t"))
    assert ((host(f0d) > 0) == (cat(rs, "f0d") > 0)).all()
    np.testing.assert_allclose(host(f0d), cat(rs, "f0d"), atol=F0_TOL, rtol=0)
    f0 = b.stonemask(fd["x"], fd["t"], fd["f0d"], _stale=[st["x"], st["t"], st["f0d"]])
    np.testing.assert_allclose(host(f0), cat(rs, "f0"), atol=F0_TOL, rtol=0)
    t, fh = b.harvest(fd["x"], _stale=[st["x"]])
    ro = [oracle.harvest(x, FS, 5.0) for x in fresh]
    fo = np.concatenate([r[1] for r in ro])
    np.testing.assert_array_equal(host(t), np.concatenate([r[0] for r in ro]))
    assert ((host(fh) > 0) == (fo > 0)).all()
    np.testing.assert_allclose(host(fh), fo, atol=F0_TOL, rtol=0)


def test_spectral_stages(env, world):
    b, rs, fd, st, _ = world
    three = lambda d: [d["x"], d["t"], d["f0"]]
    sp = b.cheaptrick(*three(fd), _stale=three(st))
    sp_close(host(sp), cat(rs, "sp"))
    ap = b.d4c(*three(fd), _stale=three(st))
    np.testing.assert_allclose(host(ap), cat(rs, "ap"), atol=AP_TOL, rtol=0)


def check_analysis(got, rs):
    t, f0, sp, ap = (host(v) for v in got[:4])
    np.testing.assert_array_equal(t, cat(rs, "t"))
    assert ((f0 > 0) == (cat(rs, "f0") > 0)).all() and np.abs(f0 - cat(rs, "f0")).max() < F0_TOL
    sp_close(sp, cat(rs, "sp"))
    np.testing.assert_allclose(ap, cat(rs, "ap"), atol=AP_TOL, rtol=0)


def test_one_call_forms_and_synthesis(env, world):
    """Analyze (D4C's preparation on the second stream, its rare frames on the third), AnalyzeSynthesize (Synthesis's
    preparation on the second stream, the overlap-adds beside the pulse kernel) and Synthesis alone."""
    b, rs, fd, st, _ = world
    check_analysis(b.analyze(fd["x"], _stale=[st["x"]]), rs)          # the warm-up took the plain order, this one forks
    check_analysis(b.analyze(fd["x"], _stale=[st["x"]]), rs)
    for _ in range(2):                                                # cold (inside: the warm-up), then overlapped
        got = b.analyze_synthesize(fd["x"], _stale=[st["x"]])
        check_analysis(got, rs)
        np.testing.assert_allclose(host(got[4]), cat(rs, "y"), atol=Y_TOL, rtol=0)
    three = lambda d: [d["f0"], d["sp"], d["ap"]]
    y = b.synthesize(*three(fd), _stale=three(st))
    np.testing.assert_allclose(host(y), cat(rs, "y"), atol=Y_TOL, rtol=0)


def test_codec_and_recipe_features(env, world, oracle):
    """The bounds of test_codec_against_oracle and test_recipe_decode_against_oracle."""
    from test_golden import recipe_pack
    torch = env.torch
    b, rs, fd, st, _ = world
    F, nd = rs[0]["F"], 50
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    sp, ap, f0 = cat(rs, "sp"), cat(rs, "ap"), cat(rs, "f0")
    ref_csp = oracle.code_spectral_envelope(sp, FS, F, nd)
    np.testing.assert_allclose(host(b.code_spectral_envelope(fd["sp"], nd, _stale=[st["sp"]])), ref_csp, atol=1e-11, rtol=0)
    np.testing.assert_allclose(host(b.decode_spectral_envelope(dev(ref_csp))),
                               oracle.decode_spectral_envelope(ref_csp, FS, F), rtol=1e-10)
    ref_cap = oracle.code_aperiodicity(ap, FS, F)
    np.testing.assert_allclose(host(b.code_aperiodicity(fd["ap"], _stale=[st["ap"]])), ref_cap, atol=1e-10, rtol=0)
    mix = ref_cap.copy()
    mix[::3] = -0.1                                             # CheckVUV keeps the default row
    np.testing.assert_allclose(host(b.decode_aperiodicity(dev(mix))), oracle.decode_aperiodicity(mix, FS, F),
                               atol=1e-12, rtol=0)
    three = lambda d: [d["f0"], d["sp"], d["ap"]]
    lf0, mgc, bap = b.recipe_features(*three(fd), nd, 25, _stale=three(st))
    rl, rm, rb = recipe_pack(oracle, f0, sp, ap, FS, F, nd)
    np.testing.assert_allclose(host(lf0), rl, atol=1e-6, rtol=0)
    np.testing.assert_allclose(host(mgc), rm, atol=2e-6, rtol=0)
    np.testing.assert_allclose(host(bap), rb, atol=2e-6, rtol=0)
    sl, sm, sb = recipe_pack(oracle, host(st["f0"]), host(st["sp"]), host(st["ap"]), FS, F, nd)
    g_f0, g_sp, g_ap = (host(v) for v in b.recipe_decode(dev(rl), dev(rm), dev(rb), _stale=[dev(sl), dev(sm), dev(sb)]))
    o_f0, o_sp, o_ap = oracle.recipe_decode(rl, rm, rb, FS, F)
    assert ((g_f0 > 0) == (o_f0 > 0)).all()
    np.testing.assert_allclose(g_f0, o_f0, rtol=1e-14, atol=0)
    np.testing.assert_allclose(g_sp, o_sp, rtol=1e-10, atol=0)
    np.testing.assert_allclose(g_ap[:, :24], o_ap[:, :24], rtol=1e-11, atol=0)
    assert (g_ap[:, 24:] == 0).all()


def test_sample_formats_and_status(env, world):
    T_WORLD.test_pcm16_conversions(env.gpu)
    b, rs, fd, st, _ = world
    bad = fd["x"].clone()
    bad[int(b.sample_offsets[1]) + 1000] = float("nan")          # the flag's documented input; the stale one is clean
    status = b.utterance_status(bad, _stale=[st["x"]])
    assert list(host(status)) == [0, 1]
    assert list(host(b.utterance_status(fd["x"], fd["f0"], fd["sp"], fd["ap"]))) == [0, 0]


def test_synthesis_in_two_parts(env):
    """test_synthesis_split_with_a_short_pulse_list's route to the split form (16 or more utterances, 4 Mi output
    samples, few pulses): its third stream, its two host round trips, the device-wide wait before the third piece.
    Every utterance must come out as from a batch of its own (made on the stream-0 context), bit for bit: that is the
    reference the suite has for the split form (there is no oracle run of 100 s of 48 kHz audio in it), another path of
    the library and not an independent one.  A read of the stale features, or a piece not joined, still gives other
    bits, so the ordering is checked; the arithmetic of Synthesis is held to the oracle in the test above."""
    torch, W = env.torch, env.W
    fs, fp, n_utt = 48000, 5.0, 18
    p = W.default_params(fs, fp)
    rng = np.random.default_rng(5)
    T = [int(rng.integers(1000, 1300)) for _ in range(n_utt)]
    Y = [int((t - 1) * fp / 1000.0 * fs) + 1 for t in T]
    assert sum(Y) >= 4 << 20
    bs = DelayedBatch(env, env.ctx, p, f0_lengths=T, y_lengths=Y)
    H = bs.fft_size // 2 + 1
    nt = sum(T)

    def features(seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        f0 = 70.0 + 25.0 * torch.rand(nt, dtype=torch.float64, device="cuda", generator=g)
        k = torch.arange(H, dtype=torch.float64, device="cuda")
        sp = (1e-3 * torch.exp(-k / 300.0))[None, :] * (0.5 + torch.rand(nt, H, dtype=torch.float64, device="cuda", generator=g))
        ap = 0.05 + 0.9 * torch.rand(nt, H, dtype=torch.float64, device="cuda", generator=g) * (k / H)[None, :]
        return [f0, sp, ap]
    fresh, stale = features(11), features(12)
    y = bs.synthesize(*fresh, _stale=stale)
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    env.U.synchronize()
    fo, yo = np.concatenate([[0], np.cumsum(T)]), np.concatenate([[0], np.cumsum(Y)])
    with torch.cuda.stream(env.default):
        for u in range(n_utt):
            b1 = W.WorldBatch(env.ctx0, p, f0_lengths=[T[u]], y_lengths=[Y[u]])
            fr = slice(int(fo[u]), int(fo[u + 1]))
            y1 = b1.synthesize(*[v[fr].contiguous() for v in fresh])
            torch.cuda.synchronize()
            assert torch.equal(y1, y[int(yo[u]):int(yo[u + 1])]), u
            b1.close()
    bs.close()


# ---- the recipe's stages: their own tests, on the caller's stream ---------------------------------------------------

def load(name):
    return np.load(os.path.join(GOLDEN, name))


def test_cmp_and_ffo_rows_gaps_and_moments(env, pkg, oracle):
    T_WORLD.test_cmp_composition(env.gpu, pkg, oracle)
    fx = load("recipe_ffo.npz")
    T_FFO.test_interpolation_has_the_scripts_bits(env.gpu, fx, 2)
    T_FFO.test_ffo_rows_have_the_scripts_bits(env.gpu, fx)
    rng = np.random.default_rng(5)
    lengths = (5, 64, 33)
    x = (rng.standard_normal((sum(lengths), 25)) * rng.uniform(0.1, 10, 25) + rng.uniform(-3, 3, 25)).astype(np.float32)
    got = T_FFO.moments(env.gpu, lengths, env.torch.from_numpy(x).cuda())
    print("moments: worst error / bound %.3f" % T_FFO.check_moments(x, lengths, got))


def test_mel_cepstra_both_ways_and_their_postfilter(env):
    T_MCEP.test_convergence_against_reference(env.gpu, load("sptk_mcep.npz"), "A_m8_a42_short")
    T_MGC2SP.test_parity_against_reference(env.gpu, load("sptk_mgc2sp_full.npz"), "F512_m24_a42_g3")
    T_MCPF.test_parity_against_reference(env.gpu, load("sptk_postfilter.npz"), T_MCPF.KEY24)


def test_modulation_spectrum_postfilter_and_statistics(env):
    fx = load("sptk_mspf.npz")
    T_MSPF.test_parity_against_the_long_double_reference(env.gpu, fx, "l15n16d65e10")
    T_MSPF.test_statistics_against_the_long_double_reference(env.gpu, fx, "l15n16d65e10")     # utterance_means too


def test_parameter_generation_and_trajectory_cost(env, pkg):
    T_MLPG.test_against_dense_reference(env.gpu, T_MLPG.CALL_B, False, 0)
    T_TRJ.test_weights(env.gpu, pkg, (10.0, 10.0))


LENGTHS = (5, 64, 33)
NET = 1                                                     # 1 -> 1 -> 1, the smallest net the DNN tests use


def test_acoustic_model_passes(env):
    """Forward with its cost, the training forward with dropout and the cost gradients, the backward pass: the bounds
    of test_gpu_dnn.py and test_gpu_dnn_train.py on the smallest net, SAT mode, lengths 5, 64 and 33."""
    hidden, output = "tanh", "linear"
    params, x, spkr, ref, e = DR.cached_case(NET, "sat", hidden, output, LENGTHS)
    out, _, status = T_DNN.run(env.gpu, LENGTHS, params, x, spkr, hidden, output)
    assert (status == 0).all() and (np.abs(out.astype(np.float64) - ref) <= e).all()
    obs = T_DNN.make_obs(ref)
    out, cost, status = T_DNN.run(env.gpu, LENGTHS, params, x, spkr, hidden, output, obs=obs)
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    for u in range(len(LENGTHS)):
        sl = slice(off[u], off[u + 1])
        want, S = DR.cost(out[sl], obs[sl], params["variance.variances"][spkr[u]])
        assert abs(cost[u] - want) <= 64.0 * 2.0 ** -53 * S
    sr = DR.spkr_rows(LENGTHS, spkr)
    G = DT.random_G(DR.SEED + 900 + NET, int(off[-1]), DR.NETS[NET][2])
    p = 0.8
    fw = DT.train_forward(params, x, sr, hidden, output, p, T_TRAIN.SEED, T_TRAIN.OFFSET)
    want, bound = DT.backward(params, fw, G, sr, hidden, output)
    got = T_TRAIN.run(env.gpu, params, x, spkr, hidden, output, p, G, obs=obs, lengths=LENGTHS)
    assert (got["status"] == 0).all() and (got["bstatus"] == 0).all()
    assert (np.abs(got["out"].astype(np.float64) - fw["out"]) <= fw["e_out"]).all()
    for k in want:
        err = np.abs(got["grads"][k].astype(np.float64) - want[k])
        assert (err <= bound[k]).all(), k
    for u, Tn in enumerate(LENGTHS):                                  # the cost gradients, as test_cost_gradients
        sl = slice(off[u], off[u + 1])
        var = params["variance.variances"][spkr[u]].astype(np.float64)
        D = ref.shape[1]
        go = (fw["out"][sl] - obs[sl].astype(np.float64)) / (var[None, :] * Tn * D)
        tol = fw["e_out"][sl] / (var[None, :] * Tn * D) + 2.0 * DR.U * np.abs(go)
        assert (np.abs(got["grad_out"][sl] - go) <= tol).all()
        _, gv, S = DT.cost_grads(got["out"][sl], obs[sl], params["variance.variances"][spkr[u]])
        assert (np.abs(got["grad_var"][u] - gv) <= 64.0 * 2.0 ** -53 * S).all()


@pytest.mark.parametrize("rule", ["momentum", "adam"])
def test_optimizer_step(env, rule):
    """One step of two rules (one and two slots) on tensors of 5, 64 and 33 elements: step32's bits."""
    torch, W = env.torch, env.W
    sizes = (5, 64, 33)
    params, grads = O.inputs(sizes=sizes, steps=2)
    rates = O.rates(len(sizes))
    powers = O.initial_powers(np.float32)
    slots = [[np.full(p.shape, v, dtype=np.float32) for p in params] for v in O.SLOT_INIT[rule]]
    dev = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)).cuda()
    want_p, want_s = [], [[] for _ in slots]
    for k, n in enumerate(sizes):
        p2, s2 = O.step32(rule, params[k], grads[0][k], [s[k] for s in slots], rates[k], powers)
        want_p.append(p2)
        for j, s in enumerate(s2):
            want_s[j].append(s)
    o = W.default_optimizer_option(rule, beta1_power=float(powers[0]), beta2_power=float(powers[1]))

    def state():
        return [dev(p) for p in params], [[dev(s) for s in sl] for sl in slots]
    wp, ws = state()
    env.ctx.optimizer_step(o, wp, [dev(g) for g in grads[1]], rates, *ws)          # the warm-up, on other gradients
    env.U.synchronize()
    ps, ss = state()
    g = [dev(a) for a in grads[1]]                                                   # stale: the other step's gradients
    fresh = [dev(a) for a in grads[0]]
    _, done, pending = env.behind_delay(g, fresh, lambda: env.ctx.optimizer_step(o, ps, g, rates, *ss))
    got = [t.clone() for t in ps], [[t.clone() for t in sl] for sl in ss]
    env.U.synchronize()
    env.note("optimizer_step", pending)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
    for k in range(len(sizes)):
        assert (bits(host(got[0][k])) == bits(want_p[k])).all(), (rule, k)
        for j in range(len(slots)):
            assert (bits(host(got[1][j][k])) == bits(want_s[j][k])).all(), (rule, j, k)
    with torch.cuda.stream(env.default):                                             # the same bits on stream 0
        p0, s0 = state()
        env.ctx0.optimizer_step(o, p0, fresh, rates, *s0)
        torch.cuda.synchronize()
    assert _same_bits((p0, s0), got, torch)


def test_label_features_and_vibrato(env, pkg, oracle):
    T_LABEL.test_fixture_as_one_batch_and_utterance_by_utterance(env.gpu, load("label_features.npz"), pkg, "recipe")
    T_VIB.test_vibrato_on_gpu_against_the_restatement(env.gpu, oracle)


# ---- calls back to back on one batch: the reuse paths that rest on "synchronise the caller's stream first" ----------

def raw_frames_batch(env, lengths, fs=48000, **params):
    return env.W.WorldBatch(env.ctx, env.W.default_params(fs, 5.0, **params), f0_lengths=list(lengths))


def test_parameter_generation_regrows_its_workspace_behind_a_pending_call(env):
    """A narrow band pending behind the delay, then the 15-tap set at once on the same batch: launch_mlpg must wait for
    the caller's stream before it lets go of the smaller workspace (mlpg.hip, the regrowth), so the second call may
    return only after the delay -- asserted here and in the tests below, because a wrong number cannot show a missing
    wait: the block let go stays intact in the block cache, and a stage workspace is scratch its kernel writes before
    it reads.  (Synthesis's response scratch, Context::ensure_scratch, has no such assertion: the call before it waits
    for the stream itself.)"""
    torch = env.torch
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    lengths = T_MLPG.LENGTHS
    m1, v1, c1, k1 = M.cached_reference(11, lengths, 1, "recipe", False, 0, 0)
    m2, v2, c2, k2 = M.cached_reference(32, lengths, 65, "ramp15", False, 0, 0)
    b = raw_frames_batch(env, lengths)
    mean1, fresh1 = dev(np.roll(m1, 1, axis=0)), dev(m1)
    s2 = [(dev(m2), dev(v2), M.WINDOW_SETS["ramp15"], None)]
    env.U.synchronize()
    var1 = dev(v1)
    (o1, st1), done, pending = env.behind_delay(
        [mean1], [fresh1], lambda: b.parameter_generation([(mean1, var1, M.WINDOW_SETS["recipe"], None)]))
    o2, st2 = b.parameter_generation(s2)                      # grows the workspace: waits for call 1 inside
    waited = done.query()
    g1, g2 = o1[0].clone(), o2[0].clone()
    env.U.synchronize()
    assert pending and waited
    T_MLPG.check(host(g1), c1, k1, lengths, "pending narrow band")
    T_MLPG.check(host(g2), c2, k2, lengths, "15 taps at once")
    assert (host(st1) == 0).all() and (host(st2) == 0).all()
    b.close()


def test_acoustic_model_regrows_its_workspace_behind_a_pending_call(env):
    """max_chunk_frames 16 pending, then 64 at once: the hidden activations' buffers are replaced by larger ones."""
    torch = env.torch
    hidden, output = "tanh", "linear"
    params, x, spkr, ref, e = DR.cached_case(3, "sd", hidden, output, LENGTHS)         # 65 -> 129 -> 31
    model = T_DNN.model_dict(torch, params, hidden, output)
    b = raw_frames_batch(env, LENGTHS)
    xd, fresh = torch.from_numpy(np.roll(x, 1, axis=0).copy()).cuda(), torch.from_numpy(np.array(x)).cuda()
    x2 = fresh.clone()
    env.U.synchronize()
    (o1, _, s1), done, pending = env.behind_delay([xd], [fresh], lambda: b.acoustic_model_forward(model, xd, spkr, None, 16))
    o2, _, s2 = b.acoustic_model_forward(model, x2, spkr, None, 64)
    waited = done.query()
    g1, g2 = o1.clone(), o2.clone()
    env.U.synchronize()
    assert pending and waited
    for g in (g1, g2):
        assert (np.abs(host(g).astype(np.float64) - ref) <= e).all()
    assert (host(s1) == 0).all() and (host(s2) == 0).all()
    b.close()


def test_training_pass_replaces_the_forward_workspace_behind_a_pending_call(env):
    """A forward pass (max_chunk_frames 16) pending, then a training forward pass at keep_prob 1 at once on the same batch:
    the forward pass's workspace is replaced by the training pass's larger one (dnn_train.hip, dnn_train_ws), which must
    wait for the pending kernels first.  The same utterances (LENGTHS) and 3-layer SD case (65 -> 129 -> 31 units) as the
    test above; the forward pass within test_gpu_dnn.py's bound, the training pass within test_gpu_dnn_train.py's."""
    torch = env.torch
    hidden, output = "tanh", "linear"
    params, x, spkr, ref, e = DR.cached_case(3, "sd", hidden, output, LENGTHS)
    last = params["variance.variances"].shape[0] - 1                 # spkr None: every utterance is the last speaker's
    sr = DR.spkr_rows(LENGTHS, spkr if spkr is not None else [last] * len(LENGTHS))
    fw = DT.train_forward(params, x, sr, hidden, output, 1.0, T_TRAIN.SEED, T_TRAIN.OFFSET)
    model = T_DNN.model_dict(torch, params, hidden, output)
    b = raw_frames_batch(env, LENGTHS)
    xd, fresh = torch.from_numpy(np.roll(x, 1, axis=0).copy()).cuda(), torch.from_numpy(np.array(x)).cuda()
    x2 = fresh.clone()
    env.U.synchronize()
    (o1, _, s1), done, pending = env.behind_delay([xd], [fresh], lambda: b.acoustic_model_forward(model, xd, spkr, None, 16))
    o2, _, s2 = b.acoustic_model_train_forward(model, x2, spkr, None, 1.0, T_TRAIN.SEED, T_TRAIN.OFFSET)
    waited = done.query()
    g1, g2 = o1.clone(), o2.clone()
    env.U.synchronize()
    assert pending and waited
    assert (np.abs(host(g1).astype(np.float64) - ref) <= e).all()
    assert (np.abs(host(g2).astype(np.float64) - fw["out"]) <= fw["e_out"]).all()
    assert (host(s1) == 0).all() and (host(s2) == 0).all()
    b.close()


def test_vibrato_twice_with_other_pitches(env, oracle):
    torch = env.torch
    l, segs = T_VIB.synth_lf0(700, 4, T_VIB.NOTES)
    segs2 = [(a, e, p * 2.0 ** (2.0 / 12.0) if p > 0 else p) for a, e, p in segs]
    b = raw_frames_batch(env, [len(l)])
    lf0 = torch.from_numpy(np.roll(l, 1).copy()).cuda()
    fresh = torch.from_numpy(np.array(l)).cuda()
    b.vibrato(fresh, [segs])                                    # the warm-up
    env.U.synchronize()
    (v1, l1, n1), done, _ = env.behind_delay([lf0], [fresh], lambda: b.vibrato(lf0, [segs]))
    v2, l2, n2 = b.vibrato(lf0, [segs2])
    got = [t.clone() for t in (v1, l1, v2, l2)]
    env.U.synchronize()
    assert done.query() and n1 == 0 and n2 == 0
    for (gv, gl), sg in (((got[0], got[1]), segs), ((got[2], got[3]), segs2)):
        wv, wl, _ = oracle.vibrato(l, sg)
        np.testing.assert_allclose(host(gl), wl, rtol=1e-6, atol=0)
        np.testing.assert_allclose(host(gv), wv, rtol=2e-6, atol=0)
    b.close()


def test_cheaptrick_pending_while_a_larger_batch_grows_the_randn_table(env, world, oracle):
    """A context of its own on U: CheapTrick of the small batch is pending behind the delay when a batch with a longer
    utterance makes Context::ensure_rng replace the table the pending kernels read: the growing call may return only
    after the delay (it waits for the caller's stream before it lets go of the old table), and both spectra meet the
    oracle."""
    torch, W = env.torch, env.W
    _, rs, fd, st, fresh_x = world
    long_x = sd.make_utterance(203, FS, duration=1.2)
    rl = oracle_chain(oracle, long_x, FS)
    ctx = W.Context(stream_ptr=env.U.cuda_stream)
    p = W.default_params(FS, 5.0)
    small = W.WorldBatch(ctx, p, x_lengths=[len(x) for x in fresh_x])
    big = W.WorldBatch(ctx, p, x_lengths=[len(long_x)])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x, lx, lt, lf0 = st["x"].clone(), dev(long_x), dev(rl["t"]), dev(rl["f0"])
    small.cheaptrick(x, fd["t"], fd["f0"])                          # the warm-up sizes the table for the small batch
    env.U.synchronize()
    sp1, done, pending = env.behind_delay([x], [fd["x"]], lambda: small.cheaptrick(x, fd["t"], fd["f0"]))
    sp2 = big.cheaptrick(lx, lt, lf0)                               # grows the table: must wait for sp1's kernels
    waited = done.query()
    g1, g2 = sp1.clone(), sp2.clone()
    env.U.synchronize()
    assert pending
    sp_close(host(g1), cat(rs, "sp"))
    sp_close(host(g2), rl["sp"])
    assert waited, "the table was replaced while the caller's stream still had the delay ahead of its kernels"
    small.close()
    big.close()
    ctx.close()


def other_names(text):
    """The label file `text` with every line's name taken from another line of the file: five lines on in a state-level
    file (the state suffixes stay where they are), the next line in a phoneme-level one.  Times and line count stay."""
    lines = [l.split(" ") for l in text.split("\n") if l]
    state = "[" in lines[0][2]
    step = 5 if state and len(lines) % 5 == 0 else 1
    names = [l[2].rsplit("[", 1) if state else [l[2]] for l in lines]
    out = []
    for i, l in enumerate(lines):
        base = names[(i + step) % len(lines)][0]
        out.append(" ".join(l[:2] + [base + ("[" + names[i][1] if state else "")]))
    return "\n".join(out) + "\n"


def test_label_features_twice_with_other_names(env, pkg):
    """The first call of a batch pending behind the delay, the second at once with other names of the same lines: it
    reuses the upload image and the device block, so it must wait for the first (ffi.hip).  Both meet makefeature.pl's
    rows: the fixture's, and label_features_reference's for the changed names."""
    torch, W = env.torch, env.W
    fx = load("label_features.npz")
    config, features, labels, outs, bits = T_LABEL.block(fx, pkg, "recipe")
    labels, outs, bits = labels[:3], outs[:3], bits[:3]               # the three state-level files
    shift = int(fx["recipe/frame_shift"])
    texts2 = [other_names(str(fx["recipe/label%d" % i])) for i in range(len(labels))]
    labels2 = [pkg.recipe.parse_label(t, shift) for t in texts2]
    rows2 = [LR.rows(config, t, shift) for t in texts2]
    want2 = [r[0] for r in rows2]
    bits2 = [(1 if r[1][0] > 0 else 0) | (2 if r[1][1] > 0 else 0) for r in rows2]
    assert [T_LABEL.frames_of(l) for l in labels2] == [T_LABEL.frames_of(l) for l in labels]
    assert any(not T_LABEL.same_bits(a, b) for a, b in zip(want2, outs))
    fset = W.LabelFeatureSet(env.ctx, features)
    b = T_LABEL.batch_of(W, env.ctx, labels)
    done = env.delay()
    r1, s1 = b.label_features(fset, labels)
    pending = not done.query()
    r2, s2 = b.label_features(fset, labels2)
    waited = done.query()                                          # call 2 returned only after call 1's delay
    g1, g2 = r1.clone(), r2.clone()
    env.U.synchronize()
    assert pending, "the first label_features call of a batch waited for the stream: call 2 had nothing to wait for"
    assert waited, "the second call reused the image and the block while the first was still queued"
    env.pending.setdefault("label_features (a batch's first call)", []).append(pending)
    assert T_LABEL.same_bits(host(g1), np.concatenate(outs)) and list(host(s1)) == bits
    assert T_LABEL.same_bits(host(g2), np.concatenate(want2)) and list(host(s2)) == bits2
    b.close()
    fset.close()


def test_trajectory_cost_regrows_its_workspace_behind_a_pending_call(env, pkg):
    torch = env.torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lengths = T_TRJ.W_LENGTHS
    narrow = ((1, "recipe", True),)
    cases = [(st, TR.cached_case(TR.SEED + 100, lengths, st)) for st in (narrow, TR.STREAMS)]
    b = raw_frames_batch(env, lengths)
    calls = []
    for st, (pred, obs, var, gv_var, refs) in cases:
        pd = dev(pred)
        calls.append((pd, pkg.training.stream_views(pd, dev(obs), TR.named(st)), dev(var), dev(gv_var)))
    pd1, fresh1 = calls[0][0], calls[0][0].clone()
    pd1.copy_(torch.roll(fresh1, 1, 0))
    env.U.synchronize()
    out1, done, pending = env.behind_delay([pd1], [fresh1], lambda: b.trajectory_cost(*calls[0][1:]))
    out2 = b.trajectory_cost(*calls[1][1:])                       # more streams and dims: a larger workspace
    waited = done.query()
    got = [_walk(o, torch, lambda t: t.clone()) for o in (out1, out2)]
    env.U.synchronize()
    assert pending and waited
    for g, (st, case), what in zip(got, cases, ("pending narrow call", "wide call at once")):
        T_TRJ.check(_walk(g, torch, host), lengths, st, case[4], what)
    b.close()


def test_modulation_spectrum_postfilter_regrows_its_workspace_behind_a_pending_call(env):
    torch = env.torch
    fx = load("sptk_mspf.npz")
    keys = ("l25n64d1e05", "l25n64d50e10")                       # one column, then fifty, on the same utterances
    lengths = fx[keys[0] + "/lengths"]
    assert list(lengths) == list(fx[keys[1] + "/lengths"])
    b = T_MSPF.batch_of((torch, env.W, env.ctx), lengths)
    xs = [torch.from_numpy(fx[k + "/x"].astype(np.float64)).cuda() for k in keys]
    opts = [T_MSPF.gen.OPTIONS[k] for k in keys]
    call = lambda i, x: b.postfilter_modulation_spectrum(x, *T_MSPF.tables_of(fx, keys[i]), emphasis=opts[i][3],
                                                         frame_length=opts[i][0], fft_length=opts[i][1])
    x1, fresh1 = torch.roll(xs[0], 1, 0), xs[0]
    env.U.synchronize()
    (o1, s1), done, pending = env.behind_delay([x1], [fresh1], lambda: call(0, x1))
    o2, s2 = call(1, xs[1])
    waited = done.query()
    g = [o1.clone(), o2.clone()]
    env.U.synchronize()
    assert pending and waited and (host(s1) == 0).all() and (host(s2) == 0).all()
    for k, out in zip(keys, g):                                   # test_parity_against_the_long_double_reference's bound
        x = fx[k + "/x"].astype(np.float64)
        err = np.abs(host(out) - fx[k + "/out"]).max(axis=0)
        tol = np.maximum(10.0 * fx[k + "/sens"], 64.0 * np.spacing(np.abs(x).max(axis=0)))
        assert (err <= tol).all(), (k, (err / tol).max())
    b.close()


def test_synthesis_outgrows_the_pulse_scratch_behind_a_pending_render(env, world, oracle):
    """A context of its own: the small batch's Synthesis (its render queued when the call returns) is followed at once by
    a longer utterance's, whose pulse list needs a larger response scratch (Context::ensure_scratch)."""
    torch, W = env.torch, env.W
    _, rs, fd, st, fresh_x = world
    long_x = sd.make_utterance(203, FS, duration=1.2)
    rl = oracle_chain(oracle, long_x, FS)
    assert (rl["f0"] > 0).sum() > (cat(rs, "f0") > 0).sum()
    ctx = W.Context(stream_ptr=env.U.cuda_stream)
    p = W.default_params(FS, 5.0)
    small = W.WorldBatch(ctx, p, x_lengths=[len(x) for x in fresh_x])
    big = W.WorldBatch(ctx, p, x_lengths=[len(long_x)])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lf0, lsp, lap = dev(rl["f0"]), dev(rl["sp"]), dev(rl["ap"])
    three = [st[k].clone() for k in ("f0", "sp", "ap")]
    env.U.synchronize()
    y1, done, _ = env.behind_delay(three, [fd[k] for k in ("f0", "sp", "ap")], lambda: small.synthesize(*three))
    y2 = big.synthesize(lf0, lsp, lap)
    g1, g2 = y1.clone(), y2.clone()
    env.U.synchronize()
    assert done.query()
    np.testing.assert_allclose(host(g1), cat(rs, "y"), atol=Y_TOL, rtol=0)
    np.testing.assert_allclose(host(g2), rl["y"], atol=Y_TOL, rtol=0)
    for o in (small, big, ctx):
        o.close()


# ---- lifetime with pending work ------------------------------------------------------------------------------------

def test_close_waits_for_pending_work_and_the_blocks_are_reused(env, world):
    """batch.close() issued with CheapTrick pending behind the delay, ctx.close() with an optimiser step (a call of the
    context, no batch) pending and no other close before it: each returns only after the delay, the pending result
    meets its reference, and a new batch and context of the same sizes (which take the cached blocks) do too."""
    torch, W = env.torch, env.W
    _, rs, fd, st, fresh_x = world
    lens = [len(x) for x in fresh_x]
    p = W.default_params(FS, 5.0)
    ctx = W.Context(stream_ptr=env.U.cuda_stream)
    b = W.WorldBatch(ctx, p, x_lengths=lens)
    x = st["x"].clone()
    b.cheaptrick(x, fd["t"], fd["f0"])
    env.U.synchronize()
    sp, done, pending = env.behind_delay([x], [fd["x"]], lambda: b.cheaptrick(x, fd["t"], fd["f0"]))
    b.close()
    assert pending and done.query(), "DestroyBatch returned while the batch's kernels were still queued"
    b2 = W.WorldBatch(ctx, p, x_lengths=lens)                       # the arena of b, from the block cache
    sp2 = b2.cheaptrick(fd["x"], fd["t"], fd["f0"])
    g1, g2 = sp.clone(), sp2.clone()
    env.U.synchronize()
    sp_close(host(g1), cat(rs, "sp"))
    sp_close(host(g2), cat(rs, "sp"))
    b2.close()
    # the context itself: a call that needs no batch (the optimiser step) pending, and no batch close in between
    sizes = (5, 64, 33)
    params, grads = O.inputs(sizes=sizes, steps=2)
    rates = O.rates(len(sizes))
    dev = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)).cuda()
    want = [O.step32("sgd", params[k], grads[0][k], [], rates[k])[0] for k in range(len(sizes))]
    ps, g, fresh = [dev(a) for a in params], [dev(a) for a in grads[1]], [dev(a) for a in grads[0]]
    o = W.default_optimizer_option("sgd")
    ctx.optimizer_step(o, [dev(a) for a in params], g, rates)       # the warm-up
    env.U.synchronize()
    _, done, pending = env.behind_delay(g, fresh, lambda: ctx.optimizer_step(o, ps, g, rates))
    ctx.close()
    assert pending and done.query(), "DestroyContext returned while a call of the context was still queued"
    got = [t.clone() for t in ps]
    env.U.synchronize()
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
    for k in range(len(sizes)):
        assert (bits(host(got[k])) == bits(want[k])).all(), k
    ctx = W.Context(stream_ptr=env.U.cuda_stream)                   # the randn table and the arena, cached, once more
    b3 = W.WorldBatch(ctx, p, x_lengths=lens)
    g = b3.d4c(fd["x"], fd["t"], fd["f0"]).clone()
    env.U.synchronize()
    np.testing.assert_allclose(host(g), cat(rs, "ap"), atol=AP_TOL, rtol=0)
    b3.close()
    ctx.close()


def test_label_feature_set_close_waits_for_pending_rows(env, pkg):
    torch, W = env.torch, env.W
    fx = load("label_features.npz")
    config, features, labels, outs, bits = T_LABEL.block(fx, pkg, "recipe")
    fset = W.LabelFeatureSet(env.ctx, features)
    b = T_LABEL.batch_of(W, env.ctx, labels)
    done = env.delay()
    rows, status = b.label_features(fset, labels)                  # the batch's first call: no wait inside
    pending = not done.query()
    fset.close()
    assert pending, "the first label_features call of a batch waited for the stream: the close had nothing pending"
    assert done.query(), "DestroyLabelFeatureSet returned while the rows' kernels were still queued"
    g, s = rows.clone(), status.clone()
    env.U.synchronize()
    env.pending.setdefault("label_features (a batch's first call)", []).append(pending)
    assert T_LABEL.same_bits(host(g), np.concatenate(outs)) and list(host(s)) == bits
    b.close()


def test_two_contexts_on_two_streams(env, world):
    """Interleaved calls of two contexts, one on U and one on V, U's pending behind a delay: both results equal the
    oracle's, and the bits of a single-context run."""
    torch, W = env.torch, env.W
    _, rs, fd, st, fresh_x = world
    lens = [len(x) for x in fresh_x]
    p = W.default_params(FS, 5.0)
    cu, cv = W.Context(stream_ptr=env.U.cuda_stream), W.Context(stream_ptr=env.V.cuda_stream)
    bu, bv = W.WorldBatch(cu, p, x_lengths=lens), W.WorldBatch(cv, p, x_lengths=lens)
    single = [v.clone() for v in bu.analyze(fd["x"])]
    env.U.synchronize()
    x = st["x"].clone()
    env.U.synchronize()
    out_u, done, pending = env.behind_delay([x], [fd["x"]], lambda: bu.analyze(x))
    with torch.cuda.stream(env.V):
        out_v = [v.clone() for v in bv.analyze(fd["x"])]
        ahead = not done.query()                                    # V's call did not wait for U's delay
    got_u = [v.clone() for v in out_u]
    env.U.synchronize()
    env.V.synchronize()
    assert pending and ahead
    for got in (got_u, out_v):
        check_analysis(got, rs)
        assert _same_bits(got, single, torch)
    for o in (bu, bv, cu, cv):
        o.close()


# ---- Context.set_stream ---------------------------------------------------------------------------------------------

def test_set_stream(env, world):
    torch, W = env.torch, env.W
    _, rs, fd, st, fresh_x = world
    p = W.default_params(FS, 5.0)
    ctx = W.Context(stream_ptr=env.U.cuda_stream)
    b = W.WorldBatch(ctx, p, x_lengths=[len(x) for x in fresh_x])
    b.analyze(st["x"])
    env.U.synchronize()
    # (a), (b): analysis pending on U; set_stream(V) returns only after it; Synthesis on V from its outputs
    x = st["x"].clone()
    (t, f0, sp, ap), done, pending = env.behind_delay([x], [fd["x"]], lambda: b.analyze(x))
    ctx.set_stream(env.V.cuda_stream)
    assert pending and done.query(), "SetStream returned while work on the stream it leaves was still queued"
    with torch.cuda.stream(env.V):
        y = b.synthesize(f0, sp, ap).clone()
        env.V.synchronize()
        np.testing.assert_allclose(host(y), cat(rs, "y"), atol=Y_TOL, rtol=0)
        check_analysis((t, f0, sp, ap), rs)
        # (c): a call behind a delay on V; synchronize() returns after it; the timing records count the launch
        ctx.timing_enable(True)
        x.copy_(st["x"])
        env.V.synchronize()
        spv, done, pending = env.behind_delay([x], [fd["x"]], lambda: b.cheaptrick(x, fd["t"], fd["f0"]))
        ctx.synchronize()
        assert pending and done.query(), "Synchronize did not wait for the context's new stream"
        sp_close(host(spv), cat(rs, "sp"))
        ms, n = ctx.timing_query("cheaptrick_kernel")
        assert n >= 1 and ms > 0.0
        ctx.timing_enable(False)
        env.V.synchronize()
    # (d): back to stream 0
    ctx.set_stream(None)
    with torch.cuda.stream(env.default):
        ap0 = b.d4c(fd["x"], fd["t"], fd["f0"])
        torch.cuda.synchronize()
        np.testing.assert_allclose(host(ap0), cat(rs, "ap"), atol=AP_TOL, rtol=0)
    b.close()
    ctx.close()


def test_host_pipeline_on_the_callers_stream(env, pkg):
    """test_host_pipeline_gives_the_device_results with the pipeline made and driven under U, on U's context: it takes
    torch's current stream as its compute stream.  The resident results it is compared with come from stream 0."""
    torch, W = env.torch, env.W
    pl = pkg.pipeline
    sets = [[sd.make_utterance(120 + 3 * k + j, FS, duration=d) for j, d in enumerate((0.5, 0.9, 0.7))] for k in range(3)]
    lens = [len(x) for x in sets[0]]
    want = []
    env.U.synchronize()
    with torch.cuda.stream(env.default):
        b = W.WorldBatch(env.ctx0, W.default_params(FS, 5.0), x_lengths=lens)
        for xs in sets:
            t, f0, sp, ap, y = b.analyze_synthesize(torch.from_numpy(np.concatenate(xs)).cuda())
            y16 = np.clip(np.trunc(y.cpu().numpy() * 32767.0), -32768, 32767).astype(np.int16)
            want.append((f0.float().cpu().numpy(), sp.float().cpu().numpy(), ap.float().cpu().numpy(), y16))
        b.close()
        torch.cuda.synchronize()
    pipe = pl.HostPipeline(env.ctx, W.default_params(FS, 5.0), lens, synthesis=True)
    assert pipe.compute == env.U
    got, prev = [], None
    pipe.input_buffer()[:] = pl.to_int16(np.concatenate(sets[0]))
    pipe.feed()
    for k in range(len(sets)):
        if k + 1 < len(sets):
            pipe.input_buffer()[:] = pl.to_int16(np.concatenate(sets[k + 1]))
            pipe.feed()
        slot = pipe.submit()
        if prev is not None:
            got.append(tuple(a.copy() for a in pipe.result(prev)))
        prev = slot
    got.append(tuple(a.copy() for a in pipe.result(prev)))
    for g, w in zip(got, want):
        for a, c in zip(g, w):
            np.testing.assert_array_equal(a, c)
    pipe.close()


# ---- the later stages: evaluation, MLSA synthesis, GV, cepstrum conversion, voice modification -------------------

def frames_batch(env, lengths, fs=48000, y_lengths=None, **params):
    return env.proxy.WorldBatch(env.ctx, env.W.default_params(fs, 5.0, **params), f0_lengths=list(lengths),
                                y_lengths=y_lengths)


def test_dtw_align_and_feature_distortion(env):
    """Three ragged pairs: the path, its length and cost against dtw_cases.reference, the distortion along that path."""
    torch = env.torch
    pairs = ((65, 130), (7, 1), (129, 64))
    a, b = K_DTW.batch_rows(pairs, **K_DTW.RAGGED_SHAPE)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    b_len = [tb for _, tb in pairs]
    batch = frames_batch(env, [ta for ta, _ in pairs])
    path, n, cost, status = batch.dtw_align(da, db, b_len, 1, 5)
    out = batch.feature_distortion([(da, db, 1, 5, 0)], b_len, path, n,
                                   _stale=[da.clone(), db.clone(), path.clone(), n.clone()])
    path, n, cost, status, out = [host(t) for t in (path, n, cost, status, out)]
    batch.close()
    at = 0
    for u, (ta, tb) in enumerate(pairs):
        ref_path, ref_cost, _ = K_DTW.reference(ta, tb, 5)
        assert status[u] == 0 and n[u] == len(ref_path)
        assert np.array_equal(path[at:at + n[u]], ref_path) and (path[at + n[u]:at + ta + tb - 1] == -1).all()
        assert abs(cost[u] - float(ref_cost)) <= K_DTW.cost_bound(ta, tb, 5, ref_cost)
        assert out[u, 0, 2] == n[u] and out[u, 0, 0] > 0.0
        at += ta + tb - 1


def test_mlsa_synthesis_while_the_noise_table_grows(env):
    """Ahead of every other MLSA call of the file's context: 195 samples at the most, then a batch with 5520 -- past the
    first noise table's 4096 spare values, so that the table grows between the calls."""
    torch = env.torch
    order, alpha, pd = 12, 0.42, 4
    rounds = [(5, [("voiced", 9), ("alternate", 40), ("unvoiced", 3)]), (80, [("alternate", 70), ("voiced", 3)])]
    for k, (P, parts) in enumerate(rounds):
        pitches, mcs = T_MLSA.synthesis_inputs(81 + k, parts, order)
        Ts = [len(m) for m in mcs]
        b = frames_batch(env, Ts, 16000, [R_MLSA.samples(t, P) for t in Ts])
        y, status = b.mlsa_synthesis(T_MLSA.dev(torch, np.concatenate(pitches), np.float32),
                                     T_MLSA.dev(torch, np.concatenate(mcs), np.float32), T_MLSA.LP16, T_MLSA.HP16,
                                     alpha=alpha, pade_order=pd, frame_shift=P)
        y, status = host(y), host(status)
        b.close()
        assert (status == 0).all()
        es = T_MLSA.run_excitation(env.gpu, pitches, T_MLSA.LP16, T_MLSA.HP16, P)
        for u, p in enumerate(pitches):
            x = R_MLSA.excite(p, P)[0]
            g = R_MLSA.noise(len(x))
            want = R_MLSA.fir(T_MLSA.LP16, x) + R_MLSA.fir(T_MLSA.HP16, g)
            bound = 64.0 * np.spacing(np.abs(T_MLSA.LP16).sum() * max(np.abs(x).max(), 1e-300)
                                      + np.abs(T_MLSA.HP16).sum() * np.abs(g).max())
            assert np.abs(es[u] - want).max() <= bound
        T_MLSA.check_filter("on the caller's stream, round %d" % k, T_MLSA.split(y, Ts, P), es, mcs, alpha,
                            R_MLSA.pade(pd), P)


def test_mlsa_excitation_and_filter(env):
    T_MLSA.test_synthesis_is_the_two_calls(env.gpu, False)


def test_parameter_generation_considering_global_variance(env):
    torch = env.torch
    lengths = (3, 33, 200)
    data, voiced = K_GV.inputs(lengths, False)
    streams, gm, gv = T_GV.device_streams(torch, data, voiced)
    mask = torch.from_numpy(K_GV.holes(lengths)).cuda()
    b = frames_batch(env, lengths)
    outs, status, info = b.parameter_generation_gv(streams, gm, gv, gv_mask=mask, want_info=True,
                                                   unvoiced_value=T_GV.UNVOICED, max_iter=5, epsilon=0.0)
    c0, _ = b.parameter_generation([(m, v, w, None) for m, v, w, _ in streams])
    c0s, outs, status = [host(o) for o in c0], [host(o) for o in outs], host(status)
    b.close()
    opts = dict(max_iter=5, epsilon=0.0)
    r64 = K_GV.reference(lengths, data, voiced, c0s, K_GV.holes(lengths), 0, np.float64, **opts)
    rld = K_GV.reference(lengths, data, voiced, c0s, K_GV.holes(lengths), 0, np.longdouble, **opts)
    T_GV.compare(lengths, voiced, outs, status, c0s, r64, rld, "on the caller's stream")


def test_mel_generalized_cepstrum_conversion(env):
    """The parity case (24, .42, -1/3 -> 65, 0, -1/3) of test_gpu_mgc2mgc.py on uneven utterance lengths."""
    fx = np.load(T_MGC2MGC.gen.PATH)
    key = T_MGC2MGC.gen.PARITY_STREAM
    m1, a1, g1, n, u, m2, a2, g2, N, U = T_MGC2MGC.gen.OPTIONS[key][0]
    assert (m1, m2, a2) == (24, 65, 0.0)
    rows = fx[key + "/in"]
    b = frames_batch(env, T_MGC2MGC.uneven(len(rows)))
    mc = env.torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    out, st = b.convert_mel_generalized_cepstrum(mc, a1, g1, m2, a2, g2)
    out, st = host(out), host(st)
    b.close()
    assert (st == 0).all()
    T_MGC2MGC.check_rows(out, fx[key + "/out"], fx[key + "/sens"], key + " on a caller's stream")


def test_mel_cepstra_of_frames_and_waveforms(env):
    fx = load("sptk_mgcep.npz")
    fewest = lambda keys: min(keys, key=lambda k: len(fx[k + "/exits"]))
    T_MGCEP.test_rows_mode_against_reference(env.gpu, fx, fewest(T_MGCEP.ROW_KEYS))
    T_MGCEP.test_waveform_mode_against_reference_and_rows_mode(env.gpu, fx, fewest(T_MGCEP.WAVE_KEYS))


def test_modify_features(env):
    """test_gpu_modify.py's 64 speech rows as utterances of 7 and 57 frames, a factor pair each: f0 with numpy's bits,
    the envelope within modify_reference.bound."""
    FS, F = T_MOD.FS, T_MOD.F
    lengths, rs, shifts = [7, 57], [0.75, 1.2], [1.37, 0.5]
    speech64, f0h = T_MOD.speech_rows(), mr.f0_contour(64)
    b = frames_batch(env, lengths, FS, fft_size=F)
    got = b.modify_features(T_MOD.dev(env.torch, f0h), T_MOD.dev(env.torch, speech64), f0_scale=shifts, formant_ratio=rs)
    f0_out, sp_out = (host(t) for t in got)
    b.close()
    want = np.concatenate([mr.modify_f0(f0h[:7], shifts[0]), mr.modify_f0(f0h[7:], shifts[1])])
    assert f0_out.tobytes() == want.tobytes()
    want = np.concatenate([mr.modify_sp(speech64[:7], rs[0], FS, F), mr.modify_sp(speech64[7:], rs[1], FS, F)])
    err = np.abs(sp_out - want) / want
    assert (err.max(axis=1) <= [mr.bound(r) for r in speech64]).all()


def test_the_table_of_asynchronous_entry_points(env, request):
    """Last in the file: every covered entry point was called behind the delay, the asynchronous ones all returned
    ahead of it (asserted where they were called), and what the synchronising ones did is printed.  With only a
    selection of the file's tests run, what they called is printed and nothing is asked about the rest."""
    print("delay %.1f ms by %s" % (env.delay_ms, env.delay_kind))
    for name in sorted(env.pending):
        flags = env.pending[name]
        print("%-40s %3d calls, %3d returned ahead of their input%s" % (
            name, len(flags), sum(flags), "" if name in ASYNC else "   (" + SYNCHRONISES.get(name, "see its test") + ")"))
    assert all(all(env.pending[n]) for n in ASYNC if n in env.pending)
    if env.tests_run >= {name for name in vars(request.module) if name.startswith("test_")}:
        missing = [n for n in ASYNC + tuple(SYNCHRONISES) if n not in env.pending]
        assert not missing, missing

"""WorldMi355ModifyFeatures (modify_sp_kernel, csrc/modify.hip) against tests/modify_reference.py, the restatement of
test.cpp:201-238 that tests/test_modify_host.py pins to the compiled reference's interp1.

Finite rows are held to bound = 8 (1 + L) 2^-52, L = max |ln sp| of the input row (modify_reference.bound: derived from
the two logarithms', the interpolation's and the two exponentials' roundings, not measured); rows with zeros, a NaN or an
infinity must have every NaN, +-inf and 0 where the reference has it, and their other bins within the bound; the fill
region of a ratio below 1 has the bits of the GPU's own bin c - 1; f0 has numpy's bits.

Observed on an MI355X, worst error over the bound per family, the same at every ratio of the list to the digits shown
(printed by the test):
    8000 / 512 and 16000 / 1024:   speech, zeros, nan, inf 0.007 - 0.008; wide and flat 0.000
    48000 / 2048 and 96000 / 4096: speech, zeros, nan, inf 0.007;         wide and flat 0.000
that is about one unit in the last place of the result: on these rows wm_log gave numpy's logarithm bit for bit, and what
is left is the exponential's rounding.  convert's waveform: max |dy| 4.5e-12 against the bound 1e-8.
"""
import ctypes as C
import importlib
import types

import numpy as np
import pytest

import modify_reference as mr

pytestmark = pytest.mark.gpu
sd = importlib.import_module("hts-train-world_amd.synth_data")

FS, F = 16000, 1024                                     # the layout tests' shape
BINS = F // 2 + 1


def dev(torch, a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def bits(t):
    return t.contiguous().cpu().numpy().tobytes()


def batch_of(gpu, fs, fft_size, lengths):
    torch, W, ctx = gpu
    return W.WorldBatch(ctx, W.default_params(fs, 5.0, fft_size=fft_size), f0_lengths=list(lengths))


def run_sp(gpu, pkg, fs, fft_size, rows, ratio, lengths=None, **kw):
    """rows [T][bins] as one batch of `lengths` (default: one utterance); ratio a number or one per utterance."""
    torch = gpu[0]
    b = batch_of(gpu, fs, fft_size, lengths or [len(rows)])
    try:
        out = pkg.modify.modify_features(b, sp=dev(torch, rows), formant_ratio=ratio, **kw)[1]
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        b.close()


def speech_rows():
    return np.concatenate([mr.rows("speech", F, seed=s) for s in range(22)])[:64]


@pytest.fixture(scope="module")
def speech64():
    return speech_rows()


@pytest.fixture(scope="module")
def base64(gpu, pkg, speech64):
    """The 64 speech rows at ratio 0.8 as one utterance: what the layout tests compare bits with."""
    return run_sp(gpu, pkg, FS, F, speech64, 0.8)


@pytest.mark.parametrize("fs, fft_size", mr.SHAPES)
def test_every_family_at_every_ratio(gpu, pkg, fs, fft_size):
    """One call per family: an utterance of ROWS frames per ratio of the list."""
    rs = mr.ratios(fft_size)
    worst_all = 0.0
    for family in mr.FAMILIES:
        rows = mr.rows(family, fft_size)
        got = run_sp(gpu, pkg, fs, fft_size, np.tile(rows, (len(rs), 1)), rs, [mr.ROWS] * len(rs))
        worst = 0.0
        for u, ratio in enumerate(rs):
            mine = got[u * mr.ROWS:(u + 1) * mr.ROWS]
            want = mr.modify_sp(rows, ratio, fs, fft_size)
            assert mr.same_class(mine, want).all(), (family, ratio, np.argwhere(~mr.same_class(mine, want))[:4])
            if family in mr.FINITE_FAMILIES:
                assert np.isfinite(want).all() and (want > 0).all(), (family, ratio)
            for t in range(mr.ROWS):
                ok = np.isfinite(want[t]) & (want[t] != 0)
                if ok.any():
                    err = np.abs(mine[t][ok] - want[t][ok]) / np.abs(want[t][ok])
                    worst = max(worst, float(err.max() / mr.bound(rows[t])))
            c = mr.fill_start(ratio, fft_size)
            if ratio < 1.0:                                    # the GPU's own bin c - 1, bit for bit (NaN included)
                assert c >= 1
                assert (mine[:, c:].view(np.int64) == mine[:, c - 1:c].view(np.int64)).all(), (family, ratio)
        print("fs %d fft %d %-6s worst error / bound %.3f" % (fs, fft_size, family, worst))
        assert worst <= 1.0, (family, worst)
        worst_all = max(worst_all, worst)
    print("fs %d fft %d: worst error / bound over all families %.3f" % (fs, fft_size, worst_all))


def test_tie_patterns(gpu, pkg):
    """The reference's NaN places for zeros at bins 7 and 10 (tests/test_modify_host.py reads them off the golden file)."""
    rows = mr.rows("zeros", F)
    half = run_sp(gpu, pkg, FS, F, rows, 0.5)
    assert np.flatnonzero(np.isnan(half[0])).tolist() == [3, 5]
    one = run_sp(gpu, pkg, FS, F, rows, 1.0)
    assert np.flatnonzero(np.isnan(one[0])).tolist() == [6, 7, 9, 10]
    assert np.flatnonzero(np.isnan(one[1])).tolist() == [0, F // 2 - 1] and one[1][F // 2] == 0.0


def test_f0_scaling_has_numpys_bits(gpu, pkg):
    torch = gpu[0]
    lengths = [1, 2, 7, 64, 300]
    for shift in mr.F0_SCALES:
        f0 = np.concatenate([mr.f0_contour(max(T, 2), seed=k)[:T] for k, T in enumerate(lengths)])
        b = batch_of(gpu, FS, F, lengths)
        out = pkg.modify.modify_features(b, f0=dev(torch, f0), f0_scale=shift)[0]
        assert bits(out) == mr.modify_f0(f0, shift).tobytes()
        assert (out.cpu().numpy()[f0 == 0] == 0).all()
        b.close()
    per = [0.5, 1.0, 1.37, 2.0, 3.0]                           # one per utterance
    b = batch_of(gpu, FS, F, lengths)
    out = pkg.modify.modify_features(b, f0=dev(torch, f0), f0_scale=per)[0]
    want = np.concatenate([mr.modify_f0(f0[a:e], s) for a, e, s in zip(b.frame_offsets[:-1], b.frame_offsets[1:], per)])
    assert bits(out) == want.tobytes()
    g = dev(torch, f0)                                         # in place
    assert pkg.modify.modify_features(b, f0=g, f0_scale=per, out=(g, None))[0] is g and bits(g) == want.tobytes()
    b.close()


@pytest.mark.parametrize("T", [1, 2, 7])
def test_short_batches(gpu, pkg, speech64, base64, T):
    assert run_sp(gpu, pkg, FS, F, speech64[:T], 0.8).tobytes() == base64[:T].tobytes()


def test_twenty_thousand_rows_tiled_from_64(gpu, pkg, speech64, base64):
    """More rows than the grid has workgroups: frame i has the bits of frame i mod 64."""
    torch = gpu[0]
    n = 20000
    b = batch_of(gpu, FS, F, [n])
    sp = dev(torch, speech64).repeat(n // 64 + 1, 1)[:n].contiguous()
    out = pkg.modify.modify_features(b, sp=sp, formant_ratio=0.8)[1]
    want = dev(torch, base64).repeat(n // 64 + 1, 1)[:n]
    assert torch.equal(out.view(torch.int64), want.view(torch.int64))
    b.close()


def test_ragged_batch_with_a_factor_pair_per_utterance(gpu, pkg, speech64):
    torch = gpu[0]
    lengths, rs, shifts = [1, 7, 2, 64], [0.75, 1.2, 1.0 / 3.0, 2.0], [0.5, 1.37, 2.0, 1.0]
    rows = np.concatenate([speech64[:T] for T in lengths])
    f0 = np.concatenate([mr.f0_contour(64, seed=k)[:T] for k, T in enumerate(lengths)])
    b = batch_of(gpu, FS, F, lengths)
    f0_out, sp_out = pkg.modify.modify_features(b, dev(torch, f0), dev(torch, rows), shifts, rs)
    fo = b.frame_offsets
    for k, T in enumerate(lengths):
        alone = batch_of(gpu, FS, F, [T])
        a, e = int(fo[k]), int(fo[k + 1])
        f1, s1 = pkg.modify.modify_features(alone, dev(torch, f0[a:e]), dev(torch, rows[a:e]), shifts[k], rs[k])
        assert bits(f0_out[a:e]) == bits(f1) and bits(sp_out[a:e]) == bits(s1), k
        alone.close()
    b.close()


def test_a_nan_row_leaves_its_neighbours_alone(gpu, pkg, speech64, base64):
    rows = speech64.copy()
    rows[5, 100] = np.nan
    got = run_sp(gpu, pkg, FS, F, rows, 0.8)
    keep = np.arange(64) != 5
    assert got[keep].tobytes() == base64[keep].tobytes()
    assert np.isnan(got[5]).any() and not np.isnan(got[keep]).any()


def test_in_place_and_unaligned_rows(gpu, pkg, speech64, base64):
    """sp_out == sp gives the out-of-place bits; so does a block that starts 8 bytes past a 16-byte boundary, where
    the rows' 16-byte loads begin one element later."""
    torch = gpu[0]
    b = batch_of(gpu, FS, F, [64])
    sp = dev(torch, speech64)
    out = pkg.modify.modify_features(b, sp=sp, formant_ratio=0.8, out=(None, sp))[1]
    assert out is sp and bits(sp) == base64.tobytes()
    for shift in (1, 2, 3):
        block = torch.zeros(64 * BINS + 4, dtype=torch.float64, device="cuda")
        view = block[shift:shift + 64 * BINS].view(64, BINS)
        view.copy_(dev(torch, speech64))
        dst = torch.zeros(64 * BINS + 4, dtype=torch.float64, device="cuda")
        dview = dst[3 - shift:3 - shift + 64 * BINS].view(64, BINS)
        assert pkg.modify.modify_features(b, sp=view, formant_ratio=0.8, out=(None, dview))[1] is dview
        assert bits(dview) == base64.tobytes(), shift
        assert float(dst[:3 - shift].abs().sum()) == 0.0 and float(dst[3 - shift + 64 * BINS:].abs().sum()) == 0.0
    b.close()


def call(lib, b, shift, ratio, f0, sp, f0_out, sp_out):
    dp = C.POINTER(C.c_double)
    arr = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    s, r = arr(shift), arr(ratio)
    ptr = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())
    return lib.WorldMi355ModifyFeatures(b.handle, None if s is None else s.ctypes.data_as(dp),
                                        None if r is None else r.ctypes.data_as(dp), ptr(f0), ptr(sp), ptr(f0_out), ptr(sp_out))


def test_one_factor_leaves_the_other_array_untouched(gpu, pkg, speech64, base64):
    torch, W, ctx = gpu
    lib = W.load_library()
    b = batch_of(gpu, FS, F, [64])
    f0 = dev(torch, mr.f0_contour(64))
    sp = dev(torch, speech64)
    f0_out, sp_out = torch.full_like(f0, -7.0), torch.full_like(sp, -7.0)
    assert call(lib, b, [2.0], None, f0, sp, f0_out, sp_out) == 0
    torch.cuda.synchronize()
    assert bits(f0_out) == mr.modify_f0(f0.cpu().numpy(), 2.0).tobytes() and bool((sp_out == -7.0).all())
    assert call(lib, b, [2.0], None, f0, None, f0_out, None) == 0          # the other part's pointers are not read
    f0_out.fill_(-7.0)
    assert call(lib, b, None, [0.8], f0, sp, f0_out, sp_out) == 0
    torch.cuda.synchronize()
    assert bits(sp_out) == base64.tobytes() and bool((f0_out == -7.0).all())
    assert call(lib, b, None, [0.8], None, sp, None, sp_out) == 0
    torch.cuda.synchronize()
    b.close()


def test_refusals_queue_nothing(gpu, pkg, speech64):
    torch, W, ctx = gpu
    lib = W.load_library()
    b = batch_of(gpu, FS, F, [32, 32])
    f0 = dev(torch, mr.f0_contour(64))
    sp = dev(torch, speech64)
    f0_out, sp_out = torch.full_like(f0, -7.0), torch.full_like(sp, -7.0)
    big = torch.zeros(2 * 64 * BINS, dtype=torch.float64, device="cuda")
    ctx.timing_enable(True)
    try:
        bad = 2                                                # WM_ERR_BAD_ARG
        for r in mr.refused_ratios(F) + [float("inf")]:
            assert call(lib, b, None, [1.0, r], f0, sp, f0_out, sp_out) == bad, r
            assert call(lib, b, [1.0, 1.0], [r, 1.0], f0, sp, f0_out, sp_out) == bad, r
        for s in (0.0, float("inf"), -1.0, float("nan")):
            assert call(lib, b, [1.0, s], None, f0, sp, f0_out, sp_out) == bad, s
            assert call(lib, b, [s, 1.0], [1.0, 1.0], f0, sp, f0_out, sp_out) == bad, s
        assert call(lib, b, None, None, f0, sp, f0_out, sp_out) == bad
        assert call(lib, b, [1.0, 1.0], None, None, sp, f0_out, sp_out) == bad
        assert call(lib, b, [1.0, 1.0], None, f0, sp, None, sp_out) == bad
        assert call(lib, b, None, [1.0, 1.0], f0, None, f0_out, sp_out) == bad
        assert call(lib, b, None, [1.0, 1.0], f0, sp, f0_out, None) == bad
        assert call(lib, types.SimpleNamespace(handle=None), [1.0, 1.0], None, f0, sp, f0_out, sp_out) == bad
        src = big[:64 * BINS]
        for off in (1, BINS, 64 * BINS - 1):                   # partial overlap, either way round
            assert call(lib, b, None, [1.0, 1.0], None, src, None, src.data_ptr() + 8 * off) == bad
            assert call(lib, b, None, [1.0, 1.0], None, src.data_ptr() + 8 * off, None, src) == bad
        assert call(lib, b, None, [2.0 / F, float(F)], None, src, None, big[64 * BINS:]) == 0   # adjacent: no overlap
        torch.cuda.synchronize()
        assert ctx.timing_query("modify_kernel")[1] == 1       # the accepted call's launch and no other
        assert bool((f0_out == -7.0).all()) and bool((sp_out == -7.0).all())
    finally:
        ctx.timing_enable(False)
        b.close()


def test_convert_chain(gpu, pkg, oracle):
    """modify.convert on two short utterances at 16 kHz, shift 1.2, ratio 0.9, against the oracle's analysis ->
    modify_reference -> the oracle's synthesis, y within test_gpu_parity.py's Y_TOL; and bit for bit the three calls."""
    from test_gpu_parity import Y_TOL, oracle_chain
    torch, W, ctx = gpu
    shift, ratio = 1.2, 0.9
    xs = [sd.make_utterance(200, FS, duration=0.3), sd.make_utterance(202, FS, duration=0.5)]
    want = []
    for x in xs:
        r = oracle_chain(oracle, x, FS)
        want.append(oracle.synthesis(mr.modify_f0(r["f0"], shift), mr.modify_sp(r["sp"], ratio, FS, r["F"]), r["ap"],
                                     r["F"], 5.0, FS))
    b = W.WorldBatch(ctx, W.default_params(FS, 5.0), x_lengths=[len(x) for x in xs])
    x = dev(torch, np.concatenate(xs))
    y = pkg.modify.convert(b, x, shift, ratio)
    diff = float(np.abs(y.cpu().numpy() - np.concatenate(want)).max())
    print("convert: max |dy| %.3e (bound %.0e)" % (diff, Y_TOL))
    assert diff <= Y_TOL
    t, f0, sp, ap = b.analyze(x)
    f0m, spm = pkg.modify.modify_features(b, f0, sp, shift, ratio)
    assert f0m is not f0 and spm is not sp
    assert torch.equal(b.synthesize(f0m, spm, ap), y)
    assert torch.equal(pkg.modify.convert(b, x), b.synthesize(f0, sp, ap))       # no factor: the features as analysed
    b.close()

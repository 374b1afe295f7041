"""WorldBatch.postfilter_mel_cepstrum (mcpf_kernel, csrc/mcpf.hip) against the recipe's postfiltering_mcp
(scripts/Training.pl:2642-2687) composed from the compiled reference's freqt and fftr, as recorded in
tests/golden/sptk_postfilter.npz by tools/gen_golden_postfilter.py.

Tolerance on the gain per row: max(10 sens, 64 ulp of sum_{k >= 1} w_k |c_k|), sens being per option set the largest of
the reference's response to a last-bit perturbation of its input, its distance from the same chain in long double and
twice its truncation tail.  Everything else about a row is exact: out[0] = c[0] + gain, out[k] = w[k] c[k]."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_postfilter as gen  # noqa: E402
import mlpg_reference  # noqa: E402

pytestmark = pytest.mark.gpu

KEY24 = "L512_m24_a42_b14"


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "sptk_postfilter.npz"))


def uneven(frames):
    return [1, frames - 1] if frames > 1 else [1]


def batch_of(W, ctx, lengths, fft_size=512):
    return W.WorldBatch(ctx, W.default_params(16000, 5.0, fft_size=fft_size), f0_lengths=list(lengths))


def run(gpu, mc, lengths, alpha, beta, length):
    torch, W, ctx = gpu
    b = batch_of(W, ctx, lengths)
    try:
        out, g, st = b.postfilter_mel_cepstrum(torch.from_numpy(np.ascontiguousarray(mc)).cuda(), alpha, beta, length,
                                               gain=True)
        return out.cpu().numpy(), g.cpu().numpy(), st.cpu().numpy()
    finally:
        b.close()


def gain_tol(c, beta, sens):
    w = gen.weights(c.shape[1] - 1, beta)
    return np.maximum(10.0 * sens, 64.0 * np.spacing((w[1:] * np.abs(c[:, 1:])).sum(axis=1)))


def same_bits(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.int64) == np.ascontiguousarray(b).view(np.int64)).all()


def check_exact_rows(out, g, c, beta):
    w = gen.weights(c.shape[1] - 1, beta)
    assert (out[:, 0] == c[:, 0] + g).all()
    assert (out[:, 1:] == w[1:] * c[:, 1:]).all() and same_bits(out[:, 1], c[:, 1])


@pytest.mark.parametrize("key", sorted(gen.OPTIONS))
def test_parity_against_reference(gpu, fx, key):
    L, co, m, alpha, beta = gen.OPTIONS[key]
    c = fx[key + "/mc"]
    out, g, st = run(gpu, c, uneven(len(c)), alpha, beta, L)
    assert (st == 0).all() and np.isfinite(out).all()
    err = np.abs(g - fx[key + "/delta"])
    tol = gain_tol(c, beta, float(fx[key + "/sens"]))
    print("%s: max err %.3e, 10 sens %.3e, least tol %.3e, worst err / tol %.3f" % (
        key, err.max(), 10 * float(fx[key + "/sens"]), tol.min(), (err / tol).max()))
    assert (err <= tol).all(), (key, err, tol)
    check_exact_rows(out, g, c, beta)


def test_identity_at_order_1_and_beta_1(gpu, fx):
    c1 = fx["L512_m1_a55_b14/mc"]
    c24 = fx[KEY24 + "/mc"]
    for c, alpha, beta in ((c1, 0.55, 1.4), (c24, 0.42, 1.0), (c1, 0.55, 1.0)):
        out, g, st = run(gpu, c, uneven(len(c)), alpha, beta, 512)
        assert same_bits(out, c) and same_bits(g, np.zeros(len(c))) and (st == 0).all()


def raw_call(gpu, b, mc, out, gain, status, alpha, beta, order, length, opt=True):
    """The C entry point itself on tensors (or None) that the caller owns."""
    torch, W, ctx = gpu
    o = W.McpfOption()
    o.alpha, o.beta, o.order, o.length = alpha, beta, order, length
    ptr = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    return W.load_library().WorldMi355MelCepstrumPostfilter(b.handle, ptr(mc), C.byref(o) if opt else None, ptr(out),
                                                            ptr(gain), ptr(status))


def test_in_place_equals_out_of_place(gpu, fx):
    torch, W, ctx = gpu
    L, co, m, alpha, beta = gen.OPTIONS[KEY24]
    c = fx[KEY24 + "/mc"]
    want, wg, wst = run(gpu, c, [len(c)], alpha, beta, L)
    b = batch_of(W, ctx, [len(c)])
    try:
        t = torch.from_numpy(c.copy()).cuda()
        g = torch.empty(len(c), dtype=torch.float64, device="cuda")
        assert raw_call(gpu, b, t, t, g, None, alpha, beta, m, L) == 0            # no status array either
        ctx.synchronize()
        assert same_bits(t.cpu().numpy(), want) and same_bits(g.cpu().numpy(), wg)
        assert raw_call(gpu, b, t, t, None, None, alpha, 1.0, m, L) == 0          # the identity in place: nothing moves
        ctx.synchronize()
        assert same_bits(t.cpu().numpy(), want)
    finally:
        b.close()


def test_more_frames_than_the_grid_has_waves(gpu, fx):
    """12 000 frames: the device holds at most 256 x 32 = 8192 waves, so the grid-stride walk runs whatever the
    occupancy.  Every copy of a row is bit-identical to the row in a batch of its own."""
    L, co, m, alpha, beta = gen.OPTIONS[KEY24]
    four = np.concatenate([fx[KEY24 + "/mc"], fx["L512_m24_a55_b14/mc"][:1]])
    assert four.shape == (4, 25)
    alone = [run(gpu, four[i:i + 1], [1], alpha, beta, L) for i in range(4)]
    reps = 3000
    c = np.tile(four, (reps, 1))
    lengths = [1, 7, 333, 4096, 2, 1999]
    lengths.append(len(c) - sum(lengths))
    out, g, st = run(gpu, c, lengths, alpha, beta, L)
    assert (st == 0).all()
    for i in range(4):
        o1, g1, s1 = alone[i]
        assert s1[0] == 0
        assert same_bits(out[i::4], np.tile(o1, (reps, 1))) and same_bits(g[i::4], np.tile(g1, reps))
    err = np.abs(g[:3] - fx[KEY24 + "/delta"])
    assert (err <= gain_tol(four[:3], beta, float(fx[KEY24 + "/sens"]))).all()


def test_status_rows(gpu, fx):
    L, co, m, alpha, beta = gen.OPTIONS[KEY24]
    good = fx[KEY24 + "/mc"]
    nan_row, big_row = good[0].copy(), good[1].copy()
    nan_row[5] = np.nan
    big_row[2] = 1.0e4                                                           # exp overflows
    c = np.stack([good[0], nan_row, good[1], big_row, good[2]])
    out, g, st = run(gpu, c, [2, 3], alpha, beta, L)
    assert list(st) == [0, 1, 0, 2, 0]
    assert (out[[1, 3]] == 0).all() and (g[[1, 3]] == 0).all()
    out3, g3, st3 = run(gpu, good, [3], alpha, beta, L)
    assert (st3 == 0).all() and same_bits(out[[0, 2, 4]], out3) and same_bits(g[[0, 2, 4]], g3)
    # c0 does not enter the gain
    rows = np.stack([good[0]] * 3)
    rows[:, 0] = (0.0, 700.0, -700.0)
    o, gg, s = run(gpu, rows, [3], alpha, beta, L)
    assert (s == 0).all() and same_bits(gg, np.full(3, gg[0])) and gg[0] != 0
    check_exact_rows(o, gg, rows, beta)


def test_bad_arguments_are_refused_before_any_launch(gpu, fx):
    torch, W, ctx = gpu
    b = batch_of(W, ctx, [4])
    mc = torch.zeros(4, 64, dtype=torch.float64, device="cuda")
    out = torch.full((4, 64), 7.0, dtype=torch.float64, device="cuda")
    gain = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    status = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    inf, nan = float("inf"), float("nan")
    ctx.timing_enable(True)
    try:
        for alpha, beta, order, length in ((0.42, 1.4, 0, 512), (0.42, 1.4, 64, 512), (0.42, 1.4, -1, 512),
                                           (1.0, 1.4, 24, 512), (-1.0, 1.4, 24, 512), (nan, 1.4, 24, 512),
                                           (0.42, inf, 24, 512), (0.42, nan, 24, 512), (0.42, -inf, 24, 512),
                                           (0.42, 1.4, 24, 32), (0.42, 1.4, 24, 16384), (0.42, 1.4, 24, 500),
                                           (0.42, 1.4, 24, 0), (0.42, 1.4, 24, -512),
                                           (0.42, 1.0, 0, 512), (0.42, 1.0, 24, 100)):     # the identity checks too
            assert raw_call(gpu, b, mc, out, gain, status, alpha, beta, order, length) == 2, (alpha, beta, order, length)
        assert raw_call(gpu, b, None, out, gain, status, 0.42, 1.4, 24, 512) == 2
        assert raw_call(gpu, b, mc, None, gain, status, 0.42, 1.4, 24, 512) == 2
        assert raw_call(gpu, b, mc, out, gain, status, 0.42, 1.4, 24, 512, opt=False) == 2
        with pytest.raises(RuntimeError, match="bad argument"):
            b.postfilter_mel_cepstrum(mc[:, :25].contiguous(), 0.42, 1.4, 100)
        with pytest.raises(ValueError):
            b.postfilter_mel_cepstrum(mc[:, :25].contiguous().float())
        ctx.synchronize()
        assert ctx.timing_query("mcpf_kernel")[1] == 0
        assert (out == 7.0).all() and (gain == 7.0).all() and (status == 7).all()
        for length in (64, 128, 8192):                                           # the ends of the range are served
            assert raw_call(gpu, b, mc, out, gain, status, 0.42, 1.4, 24, length) == 0
        assert ctx.timing_query("mcpf_kernel")[1] == 3
        flat = out.flatten()                                                     # rows of 25 at the front of the buffer
        assert (flat[:100] == 0).all() and (flat[100:] == 7.0).all()
        assert (gain == 0).all() and (status == 0).all()                         # zeros in: equal energies, gain ln 1
    finally:
        ctx.timing_enable(False)
        b.close()


@pytest.mark.parametrize("length", [64, 128, 256, 8192])
def test_lengths_without_a_fixture_agree_with_numpy(gpu, fx, length):
    """The kernel forms that no option set of the fixture reaches (64 and 128 share one, with 32 and 64 bins in a
    wave; 256; 8192), against the definition in numpy: tests/test_postfilter_host.py holds that evaluation to the
    compiled reference.  Bound: the spacing term of the parity rule plus the same for numpy's own sum."""
    import test_postfilter_host as host
    L, co, m, alpha, beta = gen.OPTIONS[KEY24]
    c = fx[KEY24 + "/mc"]
    out, g, st = run(gpu, c, [len(c)], alpha, beta, length)
    want = np.asarray([host.direct_delta(r, length, alpha, beta) for r in c])
    tol = 2.0 * gain_tol(c, beta, 0.0)
    print("length %d: worst err / tol %.3f" % (length, (np.abs(g - want) / tol).max()))
    assert (st == 0).all() and (np.abs(g - want) <= tol).all()
    check_exact_rows(out, g, c, beta)


def test_chain_generation_postfilter_spectrum(gpu, fx):
    """parameter_generation -> postfilter_mel_cepstrum -> spectrum_from_mel_cepstrum(|H|^2) at fft_size = length = 512,
    m 24, alpha 0.42: the postfilter keeps the mean of |H|^2 over the 512 bins (the ends once, the others twice), which
    is what its gain term is for, and changes the spectrum itself.  Relative bound: twice the gain tolerance (the mean
    scales with e^{2 c0}) plus the 8 * 2^-52 that test_gpu_mgc2sp.py allows for the exponential on both sides."""
    torch, W, ctx = gpu
    L, co, m, alpha, beta = gen.OPTIONS[KEY24]
    T = 40
    base = fx[KEY24 + "/mc"]
    t = np.linspace(0.0, 1.0, T)[:, None]
    traj = ((1 - t) * base[0] + t * base[1] + 0.1 * np.sin(2 * np.pi * t) * base[2]).astype(np.float32)
    b = batch_of(W, ctx, [T], fft_size=L)
    try:
        rows = b.compose_cmp([(torch.from_numpy(traj).cuda(), mlpg_reference.RECIPE)])
        var = torch.ones(rows.shape[1], dtype=torch.float32, device="cuda")
        (c32,), status = b.parameter_generation([(rows, var, mlpg_reference.RECIPE, None)], edge=1)
        assert int(status[0]) == 0
        c = c32.double().contiguous()
        out, g, st = b.postfilter_mel_cepstrum(c, alpha, beta, L, gain=True)
        p0, s0 = b.spectrum_from_mel_cepstrum(c, alpha, 0.0, 4)
        p1, s1 = b.spectrum_from_mel_cepstrum(out, alpha, 0.0, 4)
        c, g, p0, p1 = c.cpu().numpy(), g.cpu().numpy(), p0.cpu().numpy(), p1.cpu().numpy()
        assert (st.cpu().numpy() == 0).all() and (s0.cpu().numpy() == 0).all() and (s1.cpu().numpy() == 0).all()
    finally:
        b.close()
    assert np.abs(c - traj).max() < 1e-3 and np.abs(g).min() > 1e-3
    v = np.full(L // 2 + 1, 2.0)
    v[0] = v[-1] = 1.0
    e0, e1 = (p0 * v).sum(axis=1) / L, (p1 * v).sum(axis=1) / L
    rel = np.abs(e1 / e0 - 1.0)
    tol = 2.0 * gain_tol(c, beta, 0.0) + 8.0 * 2.0 ** -52
    print("chain: worst relative change of the mean power %.3e, worst / bound %.3f" % (rel.max(), (rel / tol).max()))
    assert (rel <= tol).all()
    assert (np.abs(p1 / p0 - 1.0).max(axis=1) > 1e-3).all()                     # not a no-op

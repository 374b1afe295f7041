"""The modulation-spectrum postfilter and its statistics on the device (scripts/Training.pl:2950-3038, :3133-3221)
against the definition written out in tests/mspf_reference.py: every set of tests/golden/sptk_mspf.npz (long double),
the statistics, the identity with equal tables, a time-segment boundary, bit-exactness under every regrouping of the
batch, the status bits, zero frames and the raw entry points' refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_mspf as gen  # noqa: E402
import mspf_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "sptk_mspf.npz"))


def tables_of(fx, key):
    return tuple(fx[key + "/" + n] for n in ("mean_gen", "std_gen", "mean_nat", "std_nat"))


def batch_of(gpu, lengths):
    """A batch of the utterances that have frames: CreateBatch refuses an utterance of zero frames (test_zero_frames),
    so the fixture's T = S - 1 = 0 at frame_length 3 has no rows in, none out and no place in the batch."""
    torch, W, ctx = gpu
    return W.WorldBatch(ctx, W.default_params(16000, 5.0), f0_lengths=[int(n) for n in lengths if int(n) > 0])


def run(gpu, lengths, x, tabs, e, Lw, N):
    """(out [total][dim], status [n_utt]) of one call on a fresh batch."""
    torch, W, ctx = gpu
    b = batch_of(gpu, lengths)
    try:
        out, st = b.postfilter_modulation_spectrum(torch.from_numpy(np.ascontiguousarray(x, np.float64)).cuda(), *tabs,
                                                   emphasis=e, frame_length=Lw, fft_length=N)
        return out.cpu().numpy(), st.cpu().numpy()
    finally:
        b.close()


def run_stats(gpu, lengths, x, Lw, N, mean=None):
    torch, W, ctx = gpu
    b = batch_of(gpu, lengths)
    try:
        m = None if mean is None else torch.from_numpy(np.ascontiguousarray(mean, np.float64)).cuda()
        s1, s2, n = b.modulation_spectrum_stats(torch.from_numpy(np.ascontiguousarray(x, np.float64)).cuda(), Lw, N, m)
        return s1.cpu().numpy(), s2.cpu().numpy(), n
    finally:
        b.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and (a.view(np.uint64) == b.view(np.uint64)).all()


def split(x, lengths):
    off = np.concatenate([[0], np.cumsum(lengths)])
    return [x[off[i]:off[i + 1]] for i in range(len(lengths))]


@pytest.mark.parametrize("key", sorted(gen.OPTIONS))
def test_parity_against_the_long_double_reference(gpu, fx, key):
    """|out - golden| <= max(10 sens, 64 spacing(max|x|)) per column: the 10 covers the difference between the kernel's
    transform order and the reference's direct sums."""
    Lw, N, dim, e = gen.OPTIONS[key]
    x = fx[key + "/x"].astype(np.float64)
    out, st = run(gpu, fx[key + "/lengths"], x, tables_of(fx, key), e, Lw, N)
    err = np.abs(out - fx[key + "/out"]).max(axis=0)
    tol = np.maximum(10.0 * fx[key + "/sens"], 64.0 * np.spacing(np.abs(x).max(axis=0)))
    print("%s: worst err %.2e, worst err / tol %.3f" % (key, err.max(), (err / tol).max()))
    assert (st == 0).all()
    assert (err <= tol).all(), (key, (err / tol).max())


@pytest.mark.parametrize("key", ["l25n64d50e10", "l3n16d65e05", "l15n16d65e10", "l31n32d50e05"])
def test_statistics_against_the_long_double_reference(gpu, fx, key):
    """Sums within 64 ulp n_frames max|m| (max m^2 for the squares).  The finalised mean within the same bound over n;
    the standard deviation within what the two bounds allow sqrt(q / n - mean^2): (dq / n + 2 |mean| ds / n) / (2 std),
    plus 64 ulp of its own value."""
    torch, W, ctx = gpu
    Lw, N, dim, _ = gen.OPTIONS[key]
    lengths = fx[key + "/lengths"]
    x = fx[key + "/x"].astype(np.float64)
    seqs = [s for s in split(x, lengths) if len(s)]                             # as batch_of() makes the batch
    r1, r2, rn = R.stats(seqs, Lw, N, np.longdouble)
    mmax = max(np.abs(R.forward(s[:, d], Lw, N)[3]).max() for s in seqs if len(s) for d in range(dim))
    s1, s2, n = run_stats(gpu, lengths, x, Lw, N)
    assert n == rn == sum(R.n_frames(int(t), Lw) for t in lengths)
    b1, b2 = 64.0 * EPS * n * mmax, 64.0 * EPS * n * mmax * mmax
    e1, e2 = np.abs(s1 - r1).astype(np.float64).max(), np.abs(s2 - r2).astype(np.float64).max()
    print("%s: sum err / bound %.3f, sumsq err / bound %.3f (n %d, max|m| %.1f)" % (key, e1 / b1, e2 / b2, n, mmax))
    assert e1 <= b1 and e2 <= b2
    mean, std = W.mspf_finalize(s1, s2, n)
    rmean, rstd = R.finalize(r1, r2, np.longdouble(rn))
    assert (np.abs(mean - rmean) <= b1 / n).all()
    bstd = ((b2 / n + 2.0 * np.abs(rmean) * b1 / n) / (2.0 * rstd) + 64.0 * EPS * rstd).astype(np.float64)
    assert (rstd > 0).all() and (np.abs(std - rstd) <= bstd).all()
    # the same sums with the means handed in, and the means themselves
    b = batch_of(gpu, lengths)
    try:
        mu = b.utterance_means(torch.from_numpy(x).cuda()).cpu().numpy()
    finally:
        b.close()
    for k, s in enumerate(seqs):
        want = s.astype(np.longdouble).mean(axis=0)
        # blocks of 32 frames, the blocks of a wave in turn, two more additions, one division: each rounds by 2^-53 of a
        # partial sum that is at most T max|x|
        depth = 31 + (len(s) + 127) // 128 + 3
        assert (np.abs(mu[k] - want) <= depth * 0.5 * EPS * np.abs(s).max(axis=0)).all()
    t1, t2, tn = run_stats(gpu, lengths, x, Lw, N, mean=mu)
    assert tn == n and same_bits(t1, s1) and same_bits(t2, s2)


@pytest.mark.parametrize("key", ["l25n64d50e10", "l3n16d64e10", "l15n16d65e10", "l31n32d1e10"])
def test_identity_with_equal_tables(gpu, fx, key):
    """gen == nat returns the input: to 64 ulp of max|x| plus the 1e-15 K that the 1e-30 under the logarithm of step 4
    puts on an amplitude."""
    Lw, N, dim, e = gen.OPTIONS[key]
    mg, sg = fx[key + "/mean_gen"], fx[key + "/std_gen"]
    x = fx[key + "/x"].astype(np.float64)
    out, st = run(gpu, fx[key + "/lengths"], x, (mg, sg, mg, sg), 1.0, Lw, N)
    tol = 64.0 * np.spacing(np.abs(x).max(axis=0)) + 1e-15 * (N // 2 + 1)
    err = np.abs(out - x).max(axis=0)
    print("%s: identity worst err / tol %.3f" % (key, (err / tol).max()))
    assert (st == 0).all() and (err <= tol).all()


@pytest.mark.parametrize("key", ["l25n64d50e10", "l3n16d65e05"])
def test_time_segment_boundaries(gpu, pkg, fx, key):
    """One utterance of 2 segments + 5 frames (three time segments) against the reference, by the parity test's rule
    with `sens` worked out here the way the fixture's is."""
    Lw, N, _, e = gen.OPTIONS[key]
    dim, T = 3, 2 * pkg.world.mspf_segment_frames() + 5
    tabs = tuple(t[:dim] for t in tables_of(fx, key))
    rng = np.random.default_rng(11)
    x = gen.smooth(gen.ar1(rng, T + 4, dim)).astype(np.float32).astype(np.float64)
    xp = x * (1.0 + 4.0 * EPS * rng.choice([-1.0, 1.0], size=x.shape))
    ld = R.postfilter(x, *tabs, Lw, N, e, np.longdouble)
    d = R.postfilter(x, *tabs, Lw, N, e, np.float64)
    dp = R.postfilter(xp, *tabs, Lw, N, e, np.float64)
    sens = np.maximum(np.abs(dp - d).max(axis=0), np.abs(d - ld).astype(np.float64).max(axis=0))
    out, st = run(gpu, [T], x, tabs, e, Lw, N)
    err = np.abs(out - ld).astype(np.float64).max(axis=0)
    tol = np.maximum(10.0 * sens, 64.0 * np.spacing(np.abs(x).max(axis=0)))
    print("%s: T %d worst err / tol %.3f" % (key, T, (err / tol).max()))
    assert (st == 0).all() and (err <= tol).all()
    assert np.abs(out - x).max() > 0.1                                            # the tables differ: the values move


def test_bits_do_not_depend_on_the_batch(gpu, pkg, fx):
    key = "l15n16d65e10"
    Lw, N, dim, e = gen.OPTIONS[key]
    tabs = tables_of(fx, key)
    rng = np.random.default_rng(5)
    Ta, Tb = 2 * pkg.world.mspf_segment_frames() + 3, 41                          # A spans three time segments
    A = gen.smooth(gen.ar1(rng, Ta + 4, dim))
    B = gen.smooth(gen.ar1(rng, Tb + 4, dim))
    alone, _ = run(gpu, [Ta], A, tabs, e, Lw, N)
    first, _ = run(gpu, [Ta, Tb], np.concatenate([A, B]), tabs, e, Lw, N)
    last, _ = run(gpu, [Tb, Ta], np.concatenate([B, A]), tabs, e, Lw, N)
    assert same_bits(first[:Ta], alone) and same_bits(last[Tb:], alone)
    again, _ = run(gpu, [Ta, Tb], np.concatenate([A, B]), tabs, e, Lw, N)
    assert same_bits(again, first)
    # another neighbour, another column: everything else keeps its bits
    B2 = B + 1.0
    other, _ = run(gpu, [Ta, Tb], np.concatenate([A, B2]), tabs, e, Lw, N)
    assert same_bits(other[:Ta], alone) and not same_bits(other[Ta:], first[Ta:])
    A2 = A.copy()
    A2[:, 7] += 0.5
    col, _ = run(gpu, [Ta], A2, tabs, e, Lw, N)
    keep = np.arange(dim) != 7
    assert same_bits(col[:, keep], alone[:, keep]) and not same_bits(col[:, 7], alone[:, 7])
    # a narrower block of the same columns: a column does not know its neighbours
    narrow, _ = run(gpu, [Ta], A[:, :5], tuple(t[:5] for t in tabs), e, Lw, N)
    assert same_bits(narrow, alone[:, :5])
    # the statistics: the same bits again, and an utterance's sums do not depend on its batch -- the utterances are
    # added in index order from zero, so a batch of two is the one double addition of the two batches of one
    s = run_stats(gpu, [Ta, Tb], np.concatenate([A, B]), Lw, N)
    s_again = run_stats(gpu, [Ta, Tb], np.concatenate([A, B]), Lw, N)
    sa, sb = run_stats(gpu, [Ta], A, Lw, N), run_stats(gpu, [Tb], B, Lw, N)
    assert same_bits(s[0], s_again[0]) and same_bits(s[1], s_again[1]) and s[2] == s_again[2]
    assert same_bits(s[0], sa[0] + sb[0]) and same_bits(s[1], sa[1] + sb[1]) and s[2] == sa[2] + sb[2]


def test_status_bits(gpu, pkg, fx):
    key = "l25n64d50e10"
    Lw, N, dim, e = gen.OPTIONS[key]
    tabs = tables_of(fx, key)
    rng = np.random.default_rng(9)
    lengths = [5, pkg.world.mspf_segment_frames() + 40, 17]                       # the middle one has two time segments
    x = gen.smooth(gen.ar1(rng, sum(lengths) + 4, dim))
    clean, st = run(gpu, lengths, x, tabs, e, Lw, N)
    assert (st == 0).all() and np.isfinite(clean).all()
    # a NaN in the second segment of utterance 1, column 3
    bad = x.copy()
    bad[lengths[0] + lengths[1] - 2, 3] = np.nan
    out, st = run(gpu, lengths, bad, tabs, e, Lw, N)
    assert list(st) == [0, 1, 0]
    rows = slice(lengths[0], lengths[0] + lengths[1])
    assert (out[rows, 3] == 0).all()
    want = clean.copy()
    want[rows, 3] = 0.0
    assert same_bits(out, want)
    # a natural mean of 1e4 in column 6: exp overflows there, in every utterance
    mn = tabs[2].copy()
    mn[6] = 1.0e4
    out, st = run(gpu, lengths, x, (tabs[0], tabs[1], mn, tabs[3]), e, Lw, N)
    assert list(st) == [2, 2, 2]
    want = clean.copy()
    want[:, 6] = 0.0
    assert same_bits(out, want)


def test_zero_frames(gpu, fx):
    """The entry points return WM_OK on a batch without frames and skip an utterance without frames, but no such
    batch exists: CreateBatch has always refused an utterance of zero frames (and a batch of no utterances), and every
    other stage relies on it.  What is checked is that refusal, and that the shortest utterance there is, one frame,
    goes through both calls beside longer ones."""
    torch, W, ctx = gpu
    for lengths in ([7, 0, 9], [0], []):
        with pytest.raises((RuntimeError, ValueError, TypeError)):
            W.WorldBatch(ctx, W.default_params(16000, 5.0), f0_lengths=lengths)
    key = "l15n16d1e05"
    Lw, N, dim, e = gen.OPTIONS[key]
    tabs = tables_of(fx, key)
    rng = np.random.default_rng(2)
    x = gen.smooth(gen.ar1(rng, 21, dim))
    out, st = run(gpu, [7, 1, 9], x, tabs, e, Lw, N)
    one, _ = run(gpu, [1], x[7:8], tabs, e, Lw, N)
    assert list(st) == [0, 0, 0] and same_bits(out[7:8], one)
    want = R.postfilter(x[7:8], *tabs, Lw, N, e, np.longdouble)
    assert np.abs(one - want).max() <= 64.0 * np.spacing(np.abs(x[7:8]).max())
    s1, s2, n = run_stats(gpu, [7, 1, 9], x, Lw, N)
    assert n == sum(R.n_frames(t, Lw) for t in (7, 1, 9))


def test_refusals_leave_the_output_untouched(gpu, fx):
    torch, W, ctx = gpu
    key = "l15n16d1e05"
    Lw, N, dim, e = gen.OPTIONS[key]
    tabs = [np.ascontiguousarray(t) for t in tables_of(fx, key)]
    L = W.load_library()
    b = batch_of(gpu, [6])
    x = torch.ones(6, dim, dtype=torch.float64, device="cuda")
    out = torch.full((6, dim), 7.0, dtype=torch.float64, device="cuda")
    st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    K = N // 2 + 1
    s1 = torch.full((dim, K), 7.0, dtype=torch.float64, device="cuda")
    s2 = torch.full((dim, K), 7.0, dtype=torch.float64, device="cuda")
    mu = torch.full((1, dim), 7.0, dtype=torch.float64, device="cuda")
    n = C.c_int64(-1)

    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def h(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def post(x_=x, dim_=dim, opt=(Lw, N, e), t=tabs, out_=out):
        o = None if opt is None else C.byref(W.MspfOption(*opt))
        return L.WorldMi355ModulationSpectrumPostfilter(b.handle, p(x_), dim_, o, h(t[0]), h(t[1]), h(t[2]), h(t[3]),
                                                        p(out_), p(st))

    def stats(x_=x, dim_=dim, opt=(Lw, N, e), s1_=s1, s2_=s2, n_=n):
        o = None if opt is None else C.byref(W.MspfOption(*opt))
        return L.WorldMi355ModulationSpectrumStats(b.handle, p(x_), dim_, o, None, p(s1_), p(s2_),
                                                   None if n_ is None else C.byref(n_))

    def poisoned(i, v):
        t = [a.copy() for a in tabs]
        t[i][0, 1] = v
        return t

    ctx.timing_enable(True)
    try:
        bad_opts = [None, (Lw, 8, e), (Lw, 128, e), (Lw, 48, e), (14, N, e), (1, N, e), (N + 1, N, e), (N + 3, N, e),
                    (Lw, N, float("nan")), (Lw, N, float("inf"))]
        for opt in bad_opts:
            assert post(opt=opt) == 2, opt
            assert stats(opt=opt) == 2, opt
        assert post(x_=None) == 2 and post(out_=None) == 2 and post(dim_=0) == 2 and post(out_=x) == 2
        for i in range(4):
            assert post(t=[a if k != i else None for k, a in enumerate(tabs)]) == 2, i
            assert post(t=poisoned(i, float("nan"))) == 2 and post(t=poisoned(i, float("inf"))) == 2, i
        assert post(t=poisoned(1, 0.0)) == 2 and post(t=poisoned(1, -1.0)) == 2
        assert stats(x_=None) == 2 and stats(s1_=None) == 2 and stats(s2_=None) == 2 and stats(n_=None) == 2
        assert stats(dim_=0) == 2
        assert L.WorldMi355ColumnMeans(b.handle, None, dim, p(mu)) == 2
        assert L.WorldMi355ColumnMeans(b.handle, p(x), dim, None) == 2
        assert L.WorldMi355ColumnMeans(b.handle, p(x), 0, p(mu)) == 2
        torch.cuda.synchronize()
        assert ctx.timing_query("mspf_kernel")[1] == 0 and ctx.timing_query("mspf_stats_kernel")[1] == 0
        assert (out == 7.0).all() and (st == 7).all() and (s1 == 7.0).all() and (s2 == 7.0).all() and (mu == 7.0).all()
        assert n.value == -1
        # and the same arguments, sound, go through
        assert post() == 0 and stats() == 0 and L.WorldMi355ColumnMeans(b.handle, p(x), dim, p(mu)) == 0
        torch.cuda.synchronize()
        assert (st == 0).all() and (mu == 1.0).all() and n.value == R.n_frames(6, Lw)
        assert torch.isfinite(out).all() and (out != 7.0).all()
        assert ctx.timing_query("mspf_kernel")[1] == 1 and ctx.timing_query("mspf_stats_kernel")[1] == 1
    finally:
        ctx.timing_enable(False)
        b.close()

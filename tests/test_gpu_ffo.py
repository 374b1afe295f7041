"""Gap interpolation, `ffo` rows and per-utterance column moments on the device (csrc/ffo.hip) against
tests/golden/recipe_ffo.npz, which the reference's own Perl scripts wrote, bit for bit, and against the long-double
moments of tests/ffo_reference.py within bounds derived from the summation, not measured."""
import ctypes as C
import os

import numpy as np
import pytest

import ffo_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
LENGTHS = (1, 2, 3, 5, 63, 64, 65, 130, 257)
MAGIC = np.float32(-1.0e10)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "recipe_ffo.npz"))


def batch_of(gpu, lengths):
    torch, W, ctx = gpu
    return W.WorldBatch(ctx, W.default_params(16000, 5.0), f0_lengths=[int(n) for n in lengths])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and (bits(a) == bits(b)).all()


def interpolate(gpu, lengths, x, ignore=-1e10):
    torch, W, ctx = gpu
    b = batch_of(gpu, lengths)
    try:
        out, voiced, status = b.interpolate_gaps(torch.from_numpy(np.ascontiguousarray(x)).cuda(), ignore)
        return out.cpu().numpy(), voiced.cpu().numpy(), status.cpu().numpy()
    finally:
        b.close()


@pytest.mark.parametrize("dim", [1, 2])
def test_interpolation_has_the_scripts_bits(gpu, fx, dim):
    """Every case of the golden in one batch, then each utterance alone: the script's bits both times."""
    x = np.concatenate([fx["ip/d%d_T%d/x" % (dim, T)] for T in LENGTHS])
    want = np.concatenate([fx["ip/d%d_T%d/out" % (dim, T)] for T in LENGTHS])
    out, voiced, status = interpolate(gpu, LENGTHS, x)
    assert (status == 0).all()
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    for u, T in enumerate(LENGTHS):
        assert same_bits(out[off[u]:off[u + 1]], want[off[u]:off[u + 1]]), (dim, T)
    assert (voiced == (x[:, 0] != MAGIC)).all()
    for u, T in enumerate(LENGTHS):
        one, v1, st = interpolate(gpu, [T], x[off[u]:off[u + 1]])
        assert same_bits(one, want[off[u]:off[u + 1]]) and list(st) == [0], (dim, T)
        assert (v1 == voiced[off[u]:off[u + 1]]).all()


def test_column_without_a_valid_value(gpu, fx):
    """Status 1 and zeros in that column; the other column of the utterance and the neighbours keep their bits."""
    lengths = (65, 130, 257)
    x = np.concatenate([fx["ip/d2_T%d/x" % T] for T in lengths])
    want = np.concatenate([fx["ip/d2_T%d/out" % T] for T in lengths])
    x[65:195, 1] = MAGIC
    out, voiced, status = interpolate(gpu, lengths, x)
    assert list(status) == [0, 1, 0]
    assert (out[65:195, 1] == 0).all()
    keep = np.ones(out.shape, bool)
    keep[65:195, 1] = False
    assert (bits(out)[keep] == bits(want)[keep]).all()
    x[65:195, 0] = MAGIC                                               # and column 0: no frame of it is voiced
    out, voiced, status = interpolate(gpu, lengths, x)
    assert list(status) == [0, 1, 0] and (out[65:195] == 0).all() and (voiced[65:195] == 0).all()
    assert same_bits(out[:65], want[:65]) and same_bits(out[195:], want[195:])
    # more columns than the block has waves
    rng = np.random.default_rng(1)
    y = rng.standard_normal((70, 7)).astype(np.float32)
    y[rng.random(y.shape) < 0.5] = MAGIC
    y[:, 5] = MAGIC
    y[3, :5] = 1.0
    y[3, 6] = 1.0
    out, _, status = interpolate(gpu, [70], y)
    ref, _, st = R.interpolate(y)
    assert list(status) == [1] and st == 1 and same_bits(out, ref)


@pytest.mark.parametrize("ignore", [0.0, 1e-8])
def test_other_gap_markers(gpu, fx, ignore):
    """This fork's own files mark unvoiced frames by 0 (the analysis CLI) or 1e-8 (Extract.py)."""
    lengths = (5, 64, 130, 257)
    x = np.concatenate([fx["ip/d2_T%d/x" % T] for T in lengths])
    x[x == MAGIC] = np.float32(ignore)
    x[7, 1] = np.nan                                                   # a value, not a gap
    out, voiced, status = interpolate(gpu, lengths, x, ignore)
    off = np.concatenate([[0], np.cumsum(lengths)])
    for u in range(len(lengths)):
        ref, v, st = R.interpolate(x[off[u]:off[u + 1]], ignore)
        got = out[off[u]:off[u + 1]]
        assert st == status[u] == 0
        nan = np.isnan(ref)                                            # NaN propagates; its payload is not compared
        assert (np.isnan(got) == nan).all() and (bits(got)[~nan] == bits(ref)[~nan]).all()
        assert (voiced[off[u]:off[u + 1]] == v).all()
    assert np.isnan(out[:, 1]).any() and not np.isnan(out[:, 0]).any()


def ffo_case(fx):
    names = [str(n) for n in fx["ffo/names"]]
    streams = [(int(d), [list(fx["ffo/%s_win%d" % (n, i)]) for i in (1, 2, 3)], bool(m))
               for n, d, m in zip(names, fx["ffo/dims"], fx["ffo/msd"])]
    return [fx["ffo/" + n] for n in names], streams


def compose(gpu, lengths, feats, streams):
    torch, W, ctx = gpu
    b = batch_of(gpu, lengths)
    try:
        args = []
        for x, (dim, wins, msd) in zip(feats, streams):
            t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
            if msd:
                t, voiced, status = b.interpolate_gaps(t)
                assert (status == 0).all()
                args.append((t, wins, voiced))
            else:
                args.append((t, wins, None))
        return b.compose_ffo(args).cpu().numpy()
    finally:
        b.close()


def test_ffo_rows_have_the_scripts_bits(gpu, fx):
    """The golden's block alone, then between two other utterances (whose rows are the helper's)."""
    feats, streams = ffo_case(fx)
    want = fx["ffo/rows"]
    T = len(want)
    assert same_bits(compose(gpu, [T], feats, streams), want)
    rng = np.random.default_rng(2)
    others = []
    for Tn in (3, 66):
        fs = [rng.standard_normal((Tn, d)).astype(np.float32) for d, _, _ in streams]
        fs[1][rng.random((Tn, 1)) < 0.5] = MAGIC
        fs[1][1] = 4.0
        others.append(fs)
    cat = [np.concatenate([others[0][s], feats[s], others[1][s]]) for s in range(len(streams))]
    rows = compose(gpu, [3, T, 66], cat, streams)
    assert same_bits(rows[3:3 + T], want)
    assert same_bits(rows[:3], R.ffo_rows(others[0], streams)[0])
    assert same_bits(rows[3 + T:], R.ffo_rows(others[1], streams)[0])
    # no msd at all: compose_cmp's rows
    torch, W, ctx = gpu
    b = batch_of(gpu, [T])
    dev = [(torch.from_numpy(f).cuda(), w) for f, (_, w, _) in zip(feats, streams)]
    assert torch.equal(b.compose_ffo([(t, w, None) for t, w in dev]), b.compose_cmp(dev))
    b.close()


def moments(gpu, lengths, x, width=None, ignore=None):
    torch, W, ctx = gpu
    b = batch_of(gpu, lengths)
    try:
        return tuple(t.cpu().numpy() for t in b.column_moments(x, width, ignore))
    finally:
        b.close()


def check_moments(x, lengths, got, ignore=None, what=""):
    """|mean - ref| <= eps_mean = T 2^-52 mean|x| and |m2 - ref| <= (T + 4) 2^-52 ref + T eps_mean^2, T the kept count:
    the first is a sum of T terms and one division, each rounding at most 2^-53 of the running sum of |x|; the second
    adds the two roundings of (x - mean)^2 and what the error of the mean moves m2 by.  Returns the worst error/bound."""
    cnt, mean, m2 = got
    off = np.concatenate([[0], np.cumsum(lengths)])
    worst = 0.0
    for u in range(len(lengths)):
        seg = x[off[u]:off[u + 1]]
        rc, rm, r2 = R.moments(seg, ignore)
        assert (cnt[u] == rc).all(), (what, u)
        for c in range(seg.shape[1]):
            col = seg[:, c]
            if ignore is not None:
                col = col[~(col == np.float32(ignore))]
            T = len(col)
            if T == 0:
                assert mean[u, c] == 0.0 and m2[u, c] == 0.0, (what, u, c)
                continue
            eps_mean = R.LD(T) * 2.0 ** -52 * np.abs(col.astype(R.LD)).mean()
            e1 = abs(R.LD(mean[u, c]) - rm[c])
            bound2 = R.LD(T + 4) * 2.0 ** -52 * r2[c] + T * eps_mean ** 2
            e2 = abs(R.LD(m2[u, c]) - r2[c])
            assert e1 <= eps_mean, (what, u, c, float(e1), float(eps_mean))
            assert e2 <= bound2, (what, u, c, float(e2), float(bound2))
            worst = max(worst, float(e1 / eps_mean) if eps_mean > 0 else 0.0, float(e2 / bound2) if bound2 > 0 else 0.0)
    return worst


M_LENGTHS = (1, 2, 31, 32, 33, 127, 128, 129, 300)


@pytest.fixture(scope="module")
def moment_rows():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((sum(M_LENGTHS), 165)) * rng.uniform(0.1, 10, 165) + rng.uniform(-3, 3, 165)).astype(np.float32)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("width", [1, 64, 65, 165])
def test_moments_against_long_double(gpu, moment_rows, width):
    torch = gpu[0]
    x = np.array(moment_rows[:, :width])
    got = moments(gpu, M_LENGTHS, torch.from_numpy(x).cuda())
    assert got[0].dtype == np.int64 and got[1].dtype == got[2].dtype == np.float64
    assert got[0].shape == (len(M_LENGTHS), width)
    print("width %d: worst error / bound %.3f" % (width, check_moments(x, M_LENGTHS, got, what="width %d" % width)))


def test_moments_of_a_strided_view(gpu, moment_rows):
    """Columns 40 .. 140 of a 165-column matrix, NaN everywhere else: the view is read by its row stride."""
    torch = gpu[0]
    full = np.full(moment_rows.shape, np.nan, dtype=np.float32)
    full[:, 40:140] = moment_rows[:, 40:140]
    dev = torch.from_numpy(full).cuda()
    got = moments(gpu, M_LENGTHS, dev[:, 40:140])
    assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    x = np.ascontiguousarray(moment_rows[:, 40:140])
    print("strided: worst error / bound %.3f" % check_moments(x, M_LENGTHS, got, what="strided"))
    alone = moments(gpu, M_LENGTHS, torch.from_numpy(x).cuda())
    assert all(same_bits(a, b) for a, b in zip(got, alone))
    # the first `width` columns of a wider tensor
    part = moments(gpu, M_LENGTHS, dev[:, 40:], width=100)
    assert all(same_bits(a, b) for a, b in zip(got, part))


def test_moments_do_not_come_from_a_sum_of_squares(gpu):
    """x = 1e4 + 1e-2 noise, T = 300: sum x^2 - (sum x)^2 / T in double misses m2 by about 1e-5 relative (asserted by
    the helper that makes the case); the bound here is about 1e-13."""
    torch = gpu[0]
    x = R.large_offset_case()
    got = moments(gpu, [len(x)], torch.from_numpy(x).cuda())
    worst = check_moments(x, [len(x)], got, what="large offset")
    ref = R.moments(x)[2][0]
    print("large offset: worst error / bound %.3f, relative error of m2 %.2e, relative bound %.2e" % (
        worst, float(abs(R.LD(got[2][0, 0]) - ref) / ref), (len(x) + 4) * 2.0 ** -52))


def test_moments_with_an_ignored_value(gpu, moment_rows):
    torch = gpu[0]
    lengths = (33, 129, 300)
    x = np.array(moment_rows[:sum(lengths), :66])
    plain = moments(gpu, lengths, torch.from_numpy(x).cuda(), ignore=-1e10)           # nothing to ignore
    assert all(same_bits(a, b) for a, b in zip(plain, moments(gpu, lengths, torch.from_numpy(x).cuda())))
    rng = np.random.default_rng(9)
    y = x.copy()
    y[:, :3][rng.random((len(y), 3)) < 0.5] = MAGIC                     # columns 0-2: about half dropped
    y[33:162, 65] = MAGIC                                              # one column of one utterance: all dropped
    got = moments(gpu, lengths, torch.from_numpy(y).cuda(), ignore=-1e10)
    assert got[0][1, 65] == 0 and got[1][1, 65] == 0.0 and got[2][1, 65] == 0.0
    print("ignored: worst error / bound %.3f" % check_moments(y, lengths, got, ignore=-1e10, what="ignored"))
    untouched = np.ones(got[0].shape, bool)
    untouched[:, :3] = False
    untouched[1, 65] = False
    for a, b in zip(got, plain):
        assert (bits(a)[untouched] == bits(b)[untouched]).all()
    # without ignore_value the magic number is a value like any other
    assert (moments(gpu, lengths, torch.from_numpy(y).cuda())[0] == np.array(lengths)[:, None]).all()


def test_moment_bits_do_not_depend_on_the_batch(gpu, moment_rows):
    torch = gpu[0]
    x = np.ascontiguousarray(moment_rows[:, :70])
    got = moments(gpu, M_LENGTHS, torch.from_numpy(x).cuda())
    off = np.concatenate([[0], np.cumsum(M_LENGTHS)])
    for u, T in enumerate(M_LENGTHS):
        one = moments(gpu, [T], torch.from_numpy(np.ascontiguousarray(x[off[u]:off[u + 1]])).cuda())
        assert all(same_bits(a[u:u + 1], b) for a, b in zip(got, one)), T
    order = [8, 0, 4]                                                  # other neighbours, another order
    rows = np.concatenate([x[off[u]:off[u + 1]] for u in order])
    again = moments(gpu, [M_LENGTHS[u] for u in order], torch.from_numpy(rows).cuda())
    assert all(same_bits(a[order], b) for a, b in zip(got, again))


def test_python_wrappers_refuse(gpu):
    torch, W, ctx = gpu
    b = batch_of(gpu, [6])
    x = torch.ones(6, 2, dtype=torch.float32, device="cuda")
    v = torch.ones(6, dtype=torch.float32, device="cuda")
    try:
        for bad in (x.double(), x[:5], x.cpu(), x.reshape(-1), x.t().contiguous().t(), torch.ones(6, 4, device="cuda")[:, ::2]):
            with pytest.raises(ValueError):
                b.interpolate_gaps(bad)
            with pytest.raises(ValueError):
                b.compose_ffo([(bad, [[1.0]], None)])
            with pytest.raises(ValueError):
                b.column_moments(bad)
        with pytest.raises(ValueError):
            b.interpolate_gaps(torch.ones(6, 4, device="cuda")[:, :2])           # a view: the call takes no stride
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError):
                b.interpolate_gaps(x, bad)
            with pytest.raises(ValueError):
                b.column_moments(x, ignore_value=bad)
        for width in (0, 3, -1):
            with pytest.raises(ValueError):
                b.column_moments(x, width=width)
        for msd in (v.double(), v[:5], v.cpu(), x[:, 0]):
            with pytest.raises(ValueError):
                b.compose_ffo([(x, [[1.0]], msd)])
        with pytest.raises(ValueError):
            b.compose_ffo([])
        with pytest.raises(ValueError):
            b.compose_ffo([(x, [], None)])
        with pytest.raises(RuntimeError):                                        # the library's own limits, as ComposeCmp
            b.compose_ffo([(x, [[1.0, 2.0]], None)])
        with pytest.raises(RuntimeError):
            b.compose_ffo([(x, [[1.0]], None)] * 5)
    finally:
        b.close()


def test_raw_calls_refuse_and_timing_names(gpu):
    """WM_ERR_BAD_ARG before any device call: no kernel is recorded and the outputs keep their contents.  Then the
    same arguments, sound, go through, each under its kernel's name."""
    torch, W, ctx = gpu
    L = W.load_library()
    b = batch_of(gpu, [6])
    x = torch.ones(6, 2, dtype=torch.float32, device="cuda")
    out = torch.full((6, 2), 7.0, dtype=torch.float32, device="cuda")
    voiced = torch.full((6,), 7.0, dtype=torch.float32, device="cuda")
    st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    rows = torch.full((6, 3), 7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((1, 2), 7, dtype=torch.int64, device="cuda")
    mean = torch.full((1, 2), 7.0, dtype=torch.float64, device="cuda")
    m2 = torch.full((1, 2), 7.0, dtype=torch.float64, device="cuda")
    names = ("interpolate_gaps_kernel", "ffo_compose_kernel", "column_moments_kernel")

    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def gaps(x_=x, dim=2, ig=-1e10, out_=out):
        return L.WorldMi355InterpolateGaps(b.handle, p(x_), dim, ig, p(out_), p(voiced), p(st))

    def mom(x_=x, ld=2, width=2, ig=None, c=cnt, m=mean, s=m2):
        return L.WorldMi355ColumnMoments(b.handle, p(x_), ld, width, None if ig is None else C.byref(C.c_double(ig)),
                                         p(c), p(m), p(s))

    dp = C.POINTER(C.c_double)
    taps = (C.c_double * 1)(1.0)
    wins = (dp * 1)(C.cast(taps, dp))
    sizes = (C.c_int * 1)(1)

    def ffo(data=x, dim=2, nwin=1, size=1, n=1, out_=rows, wp=True, sp=True, msd=voiced):
        sizes[0] = size
        return L.WorldMi355ComposeFfo(
            b.handle, n, (C.c_void_p * 1)(p(data)), (C.c_int * 1)(dim), (C.c_int * 1)(nwin),
            (C.POINTER(dp) * 1)(C.cast(wins, C.POINTER(dp))) if wp else None,
            (C.POINTER(C.c_int) * 1)(C.cast(sizes, C.POINTER(C.c_int))) if sp else None,
            (C.c_void_p * 1)(p(msd)), p(out_))

    ctx.timing_enable(True)
    try:
        assert gaps(x_=None) == 2 and gaps(out_=None) == 2 and gaps(out_=x) == 2 and gaps(dim=0) == 2
        assert gaps(ig=float("nan")) == 2 and gaps(ig=float("inf")) == 2
        assert mom(x_=None) == 2 and mom(c=None) == 2 and mom(m=None) == 2 and mom(s=None) == 2
        assert mom(width=0) == 2 and mom(ld=1) == 2 and mom(ig=float("nan")) == 2 and mom(ig=float("-inf")) == 2
        assert ffo(data=None) == 2 and ffo(out_=None) == 2 and ffo(wp=False) == 2 and ffo(sp=False) == 2
        assert ffo(dim=0) == 2 and ffo(nwin=0) == 2 and ffo(nwin=5) == 2 and ffo(size=2) == 2 and ffo(size=17) == 2
        assert ffo(n=0) == 2 and ffo(n=5) == 2
        torch.cuda.synchronize()
        assert all(ctx.timing_query(n)[1] == 0 for n in names)
        for t in (out, voiced, rows, mean, m2):
            assert (t == 7.0).all()
        assert (st == 7).all() and (cnt == 7).all()
        assert gaps() == 0 and ffo() == 0 and mom() == 0 and mom(ig=-1e10) == 0
        torch.cuda.synchronize()
        assert (out == 1.0).all() and (voiced == 1.0).all() and (st == 0).all() and (rows == 1.0).all()
        assert (cnt == 6).all() and (mean == 1.0).all() and (m2 == 0.0).all()
        assert [ctx.timing_query(n)[1] for n in names] == [1, 1, 2]
        assert all(ctx.timing_query(n)[0] > 0.0 for n in names)
    finally:
        ctx.timing_enable(False)
        b.close()

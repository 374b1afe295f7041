"""WorldBatch.dtw_align / feature_distortion (csrc/dtw.hip) against tests/dtw_reference.py, the numpy statement of the
definition in include/world_mi355.h.  Paths are compared exactly: tests/dtw_cases.py draws inputs whose float64 and long
double reference paths agree with a margin far above rounding (asserted here again).  Costs within
2 (T_a + T_b - 1 + count + 2) 2^-53 cost: the rounding of a recursive sum of that many positive terms, each a count-term
root, doubled because the library may fuse multiply-adds.  Distortion sums within max(10 |float64 - long double of the
reference|, 2 (path_len + count + 4) 2^-53 |sum|); counts exactly."""
import ctypes as C

import numpy as np
import pytest

import dtw_cases as K
import dtw_reference as R

pytestmark = pytest.mark.gpu


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(torch, W, ctx, pairs, a, b, first, count):
    batch = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=[ta for ta, _ in pairs])
    try:
        out = batch.dtw_align(dev(torch, a), dev(torch, b), [tb for _, tb in pairs], first, count)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in out]
    finally:
        batch.close()


def starts(pairs):
    at, out = 0, []
    for ta, tb in pairs:
        out.append(at)
        at += max(ta + tb - 1, 0)
    return out + [at]


def check_pair(what, ta, tb, count, path, n, cost, status, ref_path, ref_cost, exact=False):
    assert status == 0, (what, status)
    assert n == len(ref_path), (what, n, len(ref_path))
    assert np.array_equal(path[:n], ref_path), (what, "path")
    assert (path[n:] == -1).all() and len(path) == ta + tb - 1, (what, "unused capacity")
    err, tol = abs(cost - float(ref_cost)), 0.0 if exact else K.cost_bound(ta, tb, count, ref_cost)
    print("%s: path_len %d cost %.17g |err| %.3e bound %.3e" % (what, n, cost, err, tol))
    assert err <= tol, (what, cost, float(ref_cost), err, tol)


@pytest.fixture(scope="module")
def ragged(gpu):
    torch, W, ctx = gpu
    a, b = K.batch_rows(K.RAGGED, **K.RAGGED_SHAPE)
    return a, b, run(torch, W, ctx, K.RAGGED, a, b, K.RAGGED_SHAPE["first"], K.RAGGED_SHAPE["count"])


@pytest.mark.parametrize("pairs,shape", [(K.RAGGED, K.RAGGED_SHAPE), (K.WIDE, K.WIDE_SHAPE)], ids=["ragged", "wide"])
def test_paths_and_costs(gpu, ragged, pairs, shape):
    torch, W, ctx = gpu
    if pairs is K.RAGGED:
        path, n, cost, status = ragged[2]
    else:
        a, b = K.batch_rows(pairs, **shape)
        path, n, cost, status = run(torch, W, ctx, pairs, a, b, shape["first"], shape["count"])
    at = starts(pairs)
    assert path.shape == (at[-1], 2) and path.dtype == np.int32
    for u, (ta, tb) in enumerate(pairs):
        p64, c64, m64 = K.reference(ta, tb, shape["count"])
        pld, _, _ = K.reference(ta, tb, shape["count"], True)
        assert np.array_equal(p64, pld) and (min(ta, tb) == 1 or m64 >= K.MIN_MARGIN), (ta, tb, m64)
        check_pair("(%d, %d) count %d" % (ta, tb, shape["count"]), ta, tb, shape["count"], path[at[u]:at[u + 1]], n[u],
                   cost[u], status[u], p64, c64)


@pytest.mark.parametrize("count", K.COUNTS)
def test_every_padded_count(gpu, count):
    torch, W, ctx = gpu
    ta, tb = K.COUNTS_PAIR
    first, ld_a, ld_b = 2, count + 3, count + 2
    a, b = K.batch_rows([K.COUNTS_PAIR], first, count, ld_a, ld_b)
    path, n, cost, status = run(torch, W, ctx, [K.COUNTS_PAIR], a, b, first, count)
    p64, c64, m64 = K.reference(ta, tb, count)
    assert np.array_equal(p64, K.reference(ta, tb, count, True)[0]) and m64 >= K.MIN_MARGIN, (count, m64)
    check_pair("(%d, %d) count %d" % (ta, tb, count), ta, tb, count, path, n[0], cost[0], status[0], p64, c64)


def test_tie_rule_bit_for_bit(gpu):
    torch, W, ctx = gpu
    ramp = np.arange(40, dtype=np.float32)[:, None]
    cases = [(np.full((ta, 1), 3.0, np.float32), np.full((tb, 1), 3.0, np.float32)) for ta, tb in ((3, 5), (5, 3), (64, 65))]
    cases += [(np.full((64, 1), 3.0, np.float32), np.full((65, 1), 5.0, np.float32)),       # every d equal and not zero
              (ramp, np.repeat(ramp, 2, axis=0)), (np.repeat(ramp, 2, axis=0), ramp)]
    pairs = [(len(a), len(b)) for a, b in cases]
    path, n, cost, status = run(torch, W, ctx, pairs, np.concatenate([a for a, _ in cases]),
                                np.concatenate([b for _, b in cases]), 0, 1)
    at = starts(pairs)
    for u, (a, b) in enumerate(cases):
        ref_path, ref_cost, _ = R.dtw(a, b)
        check_pair("tie case %d %s" % (u, pairs[u]), len(a), len(b), 1, path[at[u]:at[u + 1]], n[u], cost[u], status[u],
                   ref_path, ref_cost, exact=True)


def test_alone_as_in_the_batch(gpu, ragged):
    torch, W, ctx = gpu
    u = K.RAGGED.index((65, 130))
    a, b = K.batch_rows([(65, 130)], **K.RAGGED_SHAPE)
    path, n, cost, status = run(torch, W, ctx, [(65, 130)], a, b, 1, 5)
    at = starts(K.RAGGED)
    assert np.array_equal(path, ragged[2][0][at[u]:at[u + 1]]) and n[0] == ragged[2][1][u] and status[0] == 0
    assert cost[0].tobytes() == ragged[2][2][u].tobytes()


def test_flagged_utterances_leave_their_neighbours_alone(gpu):
    torch, W, ctx = gpu
    pairs = [(64, 3), (63, 65), (65, 0), (7, 1), (65, 130)]
    shape = K.RAGGED_SHAPE
    cols = [K.pair(ta, tb, 5) if tb else (K.pair(ta, 9, 5)[0], np.zeros((0, 5), np.float32)) for ta, tb in pairs]
    a = np.concatenate([K.embed(x, 1, 7, 1e30) for x, _ in cols])
    b = np.concatenate([K.embed(y, 1, 9, -1e30) for _, y in cols])
    good = run(torch, W, ctx, pairs, a, b, 1, 5)
    assert good[3].tolist() == [0, 0, 2, 0, 0] and good[1][2] == 0 and good[2][2] == 0.0
    a2, b2 = a.copy(), b.copy()
    a2[64 + 10, 0] = np.nan                     # unused columns of utterance 1: nothing changes
    b2[3 + 40, 6:] = np.inf
    same = run(torch, W, ctx, pairs, a2, b2, 1, 5)
    for x, y in zip(good, same):
        assert x.tobytes() == y.tobytes()
    b2[3 + 40, 3] = np.nan                      # a used column of utterance 1's B; -inf in utterance 3's A
    a2[64 + 63 + 65 + 2, 5] = -np.inf
    path, n, cost, status = run(torch, W, ctx, pairs, a2, b2, 1, 5)
    assert status.tolist() == [0, 1, 2, 1, 0] and n[1] == n[2] == n[3] == 0
    assert np.isnan(cost[1]) and np.isnan(cost[3]) and cost[2] == 0.0
    at = starts(pairs)
    for u in (1, 2, 3):
        assert (path[at[u]:at[u + 1]] == -1).all()
    for u in (0, 4):
        assert np.array_equal(path[at[u]:at[u + 1]], good[0][at[u]:at[u + 1]]) and n[u] == good[1][u]
        assert cost[u].tobytes() == good[2][u].tobytes()
        assert np.array_equal(path[at[u]:at[u] + n[u]], K.reference(*pairs[u], 5)[0])


def test_refused_arguments(gpu):
    torch, W, ctx = gpu
    batch = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=[4, 3])
    big = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=[32768])
    try:
        a, b = torch.zeros(7, 70, device="cuda"), torch.zeros(9, 66, device="cuda")

        def refused(call, *args, **kw):
            with pytest.raises(RuntimeError, match="bad argument"):
                call(*args, **kw)
        refused(batch.dtw_align, a, b, [4, 5], 0, 0)                     # count 1 .. 64
        refused(batch.dtw_align, a, b, [4, 5], 0, 65)
        refused(batch.dtw_align, a, b, [4, 5], -1, 4)                    # first < 0
        refused(batch.dtw_align, a, b, [4, 5], 8, 60)                    # beyond ld_b = 66
        refused(batch.dtw_align, a[:, :40].contiguous(), b, [4, 5], 1, 40)   # beyond ld_a = 40
        refused(big.dtw_align, torch.zeros(32768, 1, device="cuda"), torch.zeros(1, 1, device="cuda"), [1])   # T_a
        refused(batch.dtw_align, a, torch.zeros(32770, 66, device="cuda"), [32768, 2], 0, 4)                  # T_b
        L, vp = W.load_library(), C.c_void_p
        off = lambda *v: (C.c_int64 * len(v))(*v)
        path = torch.empty(14, 2, dtype=torch.int32, device="cuda")
        n = torch.empty(2, dtype=torch.int32, device="cuda")
        cost = torch.empty(2, dtype=torch.float64, device="cuda")
        ptr = lambda t: vp(t.data_ptr())
        ok = (batch.handle, ptr(a), 70, ptr(b), 66, off(0, 4, 9), 0, 4, ptr(path), ptr(n), ptr(cost), None)
        assert L.WorldMi355DtwAlign(*ok) == 0                            # status may be NULL
        for k in (1, 3, 5, 8, 9, 10):                                    # a required pointer is NULL
            args = list(ok)
            args[k] = None
            assert L.WorldMi355DtwAlign(*args) == 2, k
        for bad in (off(1, 4, 9), off(0, 5, 4)):                         # b_off starts at 0 and never decreases
            args = list(ok)
            args[5] = bad
            assert L.WorldMi355DtwAlign(*args) == 2
        torch.cuda.synchronize()
        fd = batch.feature_distortion
        refused(fd, [], [4, 5])
        refused(fd, [(a, b, 0, 4, 0)] * 9, [4, 5])
        refused(fd, [(a, b, 0, 4, 2)], [4, 5])
        refused(fd, [(a, b, 0, 2, 1)], [4, 5])                           # log f0 is one column
        refused(fd, [(a, b, 0, 65, 0)], [4, 5])
        refused(fd, [(a, b, 3, 64, 0)], [4, 5])                          # beyond ld_b
        refused(fd, [(a, b, -1, 4, 0)], [4, 5])
        refused(fd, [(a, b, 0, 4, 0)], [4, 5], voiced_above=float("nan"))
        with pytest.raises(ValueError):
            fd([(a, b, 0, 4, 0)], [4, 5], path=path)                     # path without path_len
        torch.cuda.synchronize()
    finally:
        batch.close()
        big.close()


def lf0_column(rng, t, runs):
    x = (5.0 + 0.3 * rng.standard_normal(t)).astype(np.float32)
    for lo, hi in runs:
        x[lo:hi] = -1.0e10
    return x[:, None]


def distortion_case():
    """Three utterances with T_a != T_b: an mgc-like stream of 6 columns (scored without column 0), an lf0 stream with
    unvoiced runs on both sides and a mask with holes on the natural side."""
    pairs = [(65, 130), (40, 33), (7, 20)]
    rng = np.random.default_rng(77)
    mgc = [K.pair(ta, tb, 5) for ta, tb in pairs]
    mgc_a = np.concatenate([K.embed(x, 1, 6, 9.0) for x, _ in mgc])
    mgc_b = np.concatenate([K.embed(y, 1, 6, -7.0) for _, y in mgc])
    lf0_a = np.concatenate([lf0_column(rng, ta, ((0, 3), (ta // 2, ta // 2 + 4))) for ta, _ in pairs])
    lf0_b = np.concatenate([lf0_column(rng, tb, ((1, 5), (tb // 2 + 2, tb // 2 + 9), (tb - 2, tb))) for _, tb in pairs])
    mask = np.ones(sum(tb for _, tb in pairs), dtype=np.uint8)
    mask[[0, 5, 6, 7, 60, 131, 140, 141, 165, 170]] = 0
    return pairs, mgc_a, mgc_b, lf0_a, lf0_b, mask


def check_distortion(what, pairs, out, paths, mgc_a, mgc_b, lf0_a, lf0_b, mask):
    fa = np.concatenate([[0], np.cumsum([ta for ta, _ in pairs])])
    fb = np.concatenate([[0], np.cumsum([tb for _, tb in pairs])])
    seen = np.zeros(4, dtype=np.int64)
    for u in range(len(pairs)):
        m = None if mask is None else mask[fb[u]:fb[u + 1]]
        for g, (xa, xb, kind, count) in enumerate(((mgc_a[:, 1:6], mgc_b[:, 1:6], 0, 5), (lf0_a, lf0_b, 1, 1))):
            args = (xa[fa[u]:fa[u + 1]], xb[fb[u]:fb[u + 1]], paths[u], kind, m)
            r64, rld = R.distortion(*args), R.distortion(*args, dtype=np.longdouble)
            got = out[u, g]
            sums = (0, 1) if kind == 0 else (0,)
            for k in range(4):
                if k in sums:
                    tol = max(10.0 * abs(float(rld[k]) - r64[k]), 2.0 * (len(paths[u]) + count + 4) * 2.0 ** -53 * abs(r64[k]))
                    print("%s utterance %d group %d slot %d: %.17g |err| %.3e bound %.3e"
                          % (what, u, g, k, got[k], abs(got[k] - r64[k]), tol))
                    assert abs(got[k] - r64[k]) <= tol, (what, u, g, k, got[k], r64[k], tol)
                else:
                    assert got[k] == r64[k], (what, u, g, k, got[k], r64[k])
            if kind == 1:
                pa, pb = paths[u][:, 0], paths[u][:, 1]
                keep = np.ones(len(pa), bool) if m is None else m[pb] != 0
                va, vb = xa[fa[u]:fa[u + 1]][pa, 0] > -1e9, xb[fb[u]:fb[u + 1]][pb, 0] > -1e9
                for c, sel in enumerate((va & vb, va & ~vb, ~va & vb, ~va & ~vb)):
                    seen[c] += int((sel & keep).sum())
    assert (seen > 0).all(), ("the four voicing combinations", seen)


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
def test_distortion_along_the_path_and_by_truncation(gpu, with_mask):
    torch, W, ctx = gpu
    pairs, mgc_a, mgc_b, lf0_a, lf0_b, mask = distortion_case()
    b_len = [tb for _, tb in pairs]
    batch = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=[ta for ta, _ in pairs])
    try:
        d = [dev(torch, x) for x in (mgc_a, mgc_b, lf0_a, lf0_b)]
        dm = dev(torch, mask) if with_mask else None
        groups = [(d[0], d[1], 1, 5, 0), (d[2], d[3], 0, 1, 1)]
        trunc = batch.feature_distortion(groups, b_len, b_mask=dm).cpu().numpy()         # before any alignment on the batch
        path, n, cost, status = batch.dtw_align(d[0], d[1], b_len, 1, 5)
        along = batch.feature_distortion(groups, b_len, path, n, dm).cpu().numpy()
        again = batch.feature_distortion(groups, b_len, b_mask=dm).cpu().numpy()
        path, n = path.cpu().numpy(), n.cpu().numpy()
    finally:
        batch.close()
    assert trunc.tobytes() == again.tobytes()
    at = starts(pairs)
    paths = [path[at[u]:at[u] + n[u]] for u in range(len(pairs))]
    for u, (ta, tb) in enumerate(pairs):
        assert np.array_equal(paths[u], K.reference(ta, tb, 5)[0])
    m = mask if with_mask else None
    check_distortion("along the path", pairs, along, paths, mgc_a, mgc_b, lf0_a, lf0_b, m)
    check_distortion("truncated", pairs, trunc, [R.truncation(ta, tb) for ta, tb in pairs], mgc_a, mgc_b, lf0_a, lf0_b, m)
    assert along[0, 0, 0] != trunc[0, 0, 0]


def test_flagged_utterance_scores_zero(gpu):
    torch, W, ctx = gpu
    pairs = [(7, 20), (7, 1)]
    a = np.concatenate([K.pair(7, 20, 5)[0], K.pair(7, 1, 5)[0]])
    b = np.concatenate([K.pair(7, 20, 5)[1], K.pair(7, 1, 5)[1]])
    b[3, 2] = np.nan
    batch = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=[7, 7])
    try:
        da, db = dev(torch, a), dev(torch, b)
        path, n, cost, status = batch.dtw_align(da, db, [20, 1])
        out = batch.feature_distortion([(da, db, 0, 5, 0)], [20, 1], path, n).cpu().numpy()
    finally:
        batch.close()
    assert status.cpu().tolist() == [1, 0] and (out[0] == 0).all() and out[1, 0, 2] == 7

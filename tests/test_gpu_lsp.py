"""lsp.lsp_to_lpc / lsp_to_mel_generalized_cepstrum / postfilter_lsp (lsp_kernel, mgc2mgc_kernel's energy form) against
the numpy restatement tests/lsp_reference.py, which is the definition (parity with SPTK's lspcheck and lsp2lpc is
unpinned: the commands are not in the reference tree).

Bit for bit: the checked LSPs, the filtered LSPs, the status, gains that are raised or kept.  Under the project's rule,
max(10 * sens, 64 ulp of the row's largest |value|): LPC rows, MGC rows and energies, sens being per row the larger of the
restatement's response to a last-bit change of its input and its distance from the same chain in np.longdouble
(lsp_reference.sens).  Every batch of 130 rows holds a reflected, a swapped, a too-close, a low-gain and a NaN row."""
import functools
import importlib
import math

import numpy as np
import pytest

import lsp_reference as L
import mgc2mgc_reference as M

pytestmark = pytest.mark.gpu

ORDERS = (1, 2, 3, 34, 35, 63)
G3 = -1.0 / 3.0


@pytest.fixture(scope="module")
def lsp(pkg):
    return importlib.import_module(pkg.__name__ + ".lsp")


def uneven(n):
    return [1, n - 1] if n > 1 else [1]


def on_gpu(gpu, rows, fn, ctx=None):
    """fn(batch, rows on the device) -> tensors, as numpy."""
    torch, W, ctx0 = gpu
    b = W.WorldBatch(ctx or ctx0, W.default_params(48000, 5.0), f0_lengths=uneven(len(rows)))
    try:
        out = fn(b, torch.from_numpy(np.array(rows)).cuda())             # a copy: the shared rows stay read-only
        return tuple(t.cpu().numpy() for t in out)
    finally:
        b.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def batch_rows(m, n, log_gain):
    x, where = L.rows(m, n, 1000 * m + n + int(log_gain), log_gain)
    x.setflags(write=False)
    return x, where


@functools.lru_cache(maxsize=None)
def lpc_reference(m, n, log_gain):
    """Per row of batch_rows: (lpc, checked, status, bound of the LPC row)."""
    x, _ = batch_rows(m, n, log_gain)
    out = []
    for row in x:
        lpc, chk, st = L.to_lpc(row, log_gain=log_gain)
        bound = 0.0
        if not st & 12:
            s = L.sens(lambda c, K, dt: L.lpc_of_checked(c, K, dt), chk, lpc[0])
            bound = L.tol(lpc, s)
        out.append((lpc, chk, st, bound))
    return out


def worst(name, err, bound):
    ratio = max((e / b for e, b in zip(err, bound) if b > 0), default=0.0)
    print("%s: worst error / bound %.3f (largest error %.3e)" % (name, ratio, max(err, default=0.0)))
    return ratio


@pytest.mark.parametrize("n", [1, 130])
@pytest.mark.parametrize("log_gain", [False, True])
@pytest.mark.parametrize("m", ORDERS)
def test_lsp_to_lpc(gpu, lsp, m, log_gain, n):
    x, where = batch_rows(m, n, log_gain)
    ref = lpc_reference(m, n, log_gain)
    lpc, chk, st = on_gpu(gpu, x, lambda b, r: lsp.lsp_to_lpc(b, r, log_gain=log_gain, checked=True))
    want_st = np.array([r[2] for r in ref], dtype=np.int32)
    assert same_bits(st, want_st), (st, want_st)
    assert same_bits(chk, np.stack([r[1] for r in ref]))               # checked LSPs, raised and kept gains
    if n == 130:
        assert want_st[where["nan"]] == 4 and (lpc[where["nan"]] == 0).all() and (chk[where["nan"]] == 0).all()
        assert want_st[where["low_gain"]] & 2 and lpc[where["low_gain"], 0] == 1e-10
        assert chk[where["low_gain"], 0] == (math.log(1e-10) if log_gain else 1e-10)
        if m >= 2:
            assert want_st[where["reflected"]] & 1 and want_st[where["swapped"]] & 1 and want_st[where["close"]] & 1
        kept = want_st & 6 == 0
        assert kept.sum() >= 120 and same_bits(chk[kept, 0], x[kept, 0])
    assert np.isfinite(lpc).all()
    err = [float(np.abs(g - r[0]).max()) for g, r in zip(lpc, ref)]
    bound = [r[3] for r in ref]
    assert worst("lsp_to_lpc m %d log_gain %d n %d" % (m, log_gain, n), err, bound) <= 1.0
    # without the optional outputs: the same rows
    only, st2 = on_gpu(gpu, x, lambda b, r: lsp.lsp_to_lpc(b, r, log_gain=log_gain))
    assert same_bits(only, lpc) and same_bits(st2, st)


@pytest.mark.parametrize("case", [(34, 0.55, G3, None, None, None), (24, 0.42, -1.0, 30, 0.0, -0.5)])
@pytest.mark.parametrize("log_gain", [False, True])
def test_lsp_to_mgc(gpu, lsp, case, log_gain):
    """gen_wave's call (the same alpha, gamma and order on both sides) and a call towards another set: against the
    restatement chained with mgc2mgc_reference.convert_rows, and bit for bit lsp_to_lpc followed by
    WorldBatch.convert_mel_generalized_cepstrum(normalized=True, multiplied=True)."""
    m, a1, g1, m2, a2, g2 = case
    n = 130
    x, where = batch_rows(m, n, log_gain)
    out, st = on_gpu(gpu, x, lambda b, r: lsp.lsp_to_mel_generalized_cepstrum(b, r, a1, g1, m2, a2, g2, log_gain))
    m2, a2, g2 = (m if m2 is None else m2), (a1 if a2 is None else a2), (g1 if g2 is None else g2)
    assert out.shape == (n, m2 + 1)

    def chain(c, K, dt):
        return L.lpc_to_mgc(L.lpc_of_checked(c, K, dt), a1, g1, m2, a2, g2, dt)

    err, bound = [], []
    for i, row in enumerate(x):
        lpc, chk, want_st = L.to_lpc(row, log_gain=log_gain)
        assert st[i] == want_st, (i, st[i], want_st)
        if want_st & 12:
            assert (out[i] == 0).all()
            continue
        want = chain(chk, lpc[0], L.F64)
        err.append(float(np.abs(out[i] - want).max()))
        bound.append(L.tol(want, L.sens(chain, chk, lpc[0])))
    assert st[where["nan"]] == 4 and len(err) == n - 1 and np.isfinite(out).all()
    assert worst("lsp_to_mgc %s log_gain %d" % (case, log_gain), err, bound) <= 1.0

    def two_calls(b, r):
        lpc, st1 = lsp.lsp_to_lpc(b, r, a1, g1, log_gain)
        mgc, st2 = b.convert_mel_generalized_cepstrum(lpc, a1, g1, m2, a2, g2, normalized=True, multiplied=True)
        return mgc, st1, st2
    mgc, st1, st2 = on_gpu(gpu, x, two_calls)
    assert same_bits(mgc, out) and same_bits(st1, st) and (st2 != 0).sum() == 1 and st2[where["nan"]] == 1


def test_a_row_the_conversion_refuses_is_bit_8(gpu, lsp):
    """K = 1e300 at gamma -1: K^gamma = 1e-300 vanishes beside 1, the plain row's 1 + gamma c0 is 0 and the conversion
    refuses the row (its status 1), as the restatement's division by that 0 shows."""
    x, _ = batch_rows(34, 130, False)
    x = x[:8].copy()
    x[np.isnan(x)] = 1.0
    x[3, 0] = 1e300
    out, st = on_gpu(gpu, x, lambda b, r: lsp.lsp_to_mel_generalized_cepstrum(b, r, 0.0, -1.0, 63, 0.0, 1.0))
    want = M.convert_rows(L.to_lpc(x[3])[0][None], M.option(34, 0.0, -1.0, 63, 0.0, 1.0, n=1, u=1))
    assert not np.isfinite(want).all()
    assert st[3] & 8 and (out[3] == 0).all() and not (st[[0, 1, 2, 4]] & 12).any() and np.abs(out[[0, 1, 2, 4]]).max() > 0


@functools.lru_cache(maxsize=None)
def energy_reference(m, n, alpha, gamma, beta, length, log_gain, both=True):
    """Per row of batch_rows, None for a row with a non-finite value, else ([(ene, bound)] of the raw row and, with
    `both`, of [gain, p]; the status of the checks made; the filtered row)."""
    x, _ = batch_rows(m, n, log_gain)

    def fn(c, K, dt):
        return L.energy(L.lpc_of_checked(c, K, dt), alpha, gamma, length, dt)

    out = []
    for row in x:
        if not np.isfinite(row).all():
            out.append(None)
            continue
        p = L.filter_row(row, beta)
        st, figures = 0, []
        for src in ((row, p) if both else (row,)):
            lpc, chk, s = L.to_lpc(src, log_gain=log_gain)
            st |= s
            e = fn(chk, lpc[0], L.F64)
            figures.append((float(e), L.tol(e, L.sens(fn, chk, lpc[0]))))
        out.append((figures, st, p))
    return out


@pytest.mark.parametrize("length,alpha,n,second", [(64, 0.55, 40, True), (256, 0.55, 40, True), (4096, 0.0, 12, True),
                                                   (4096, 0.55, 2, False)])
def test_energies(gpu, lsp, length, alpha, n, second):
    """ene1 and ene2 against the restatement's math.fsum, and against the sum over the storing form's own output.  At
    4096 the restatement costs 0.4 s a row and precision where alpha != 0 (freqt and gc2gc in Python loops): twelve rows
    at alpha 0, and two rows' ene1 at the recipe's 0.55."""
    m, gamma, beta = 34, G3, 0.7
    x, _ = batch_rows(m, n, True)
    ref = energy_reference(m, n, alpha, gamma, beta, length, True, second)
    out, e1, e2, st = on_gpu(gpu, x, lambda b, r: lsp.postfilter_lsp(b, r, alpha, gamma, beta, length, log_gain=True,
                                                                     energies=True))
    c2, st3 = on_gpu(gpu, x, lambda b, r: lsp.lsp_to_mel_generalized_cepstrum(b, r, alpha, gamma, length - 1, 0.0, 1.0,
                                                                              True))
    err, bound, err_own = [], [], []
    for i, r in enumerate(ref):
        if r is None:
            assert st[i] & 12 and e1[i] == 0 and e2[i] == 0 and (out[i] == 0).all()
            continue
        bounds, want_st, p = r
        assert not want_st & 12 and (st[i] == want_st or not second)
        assert same_bits(out[i], p)                                      # compensation 0: the gain's bits, p's bits
        for got, (want, tol) in zip((e1[i], e2[i]), bounds):
            err.append(abs(float(got) - want))
            bound.append(tol)
        own = 0.5 * math.log(math.fsum(float(v) * float(v) for v in c2[i]))
        err_own.append(abs(float(e1[i]) - own))
    assert len(err) >= (2 if second else 1) * (n - 1) and np.isfinite(e1).all() and np.isfinite(e2).all()
    assert worst("energy L %d alpha %.2f" % (length, alpha), err, bound) <= 1.0
    assert worst("energy form against the storing form's own sum, L %d" % length, err_own, bound[::2 if second else 1]) <= 1.0


def test_energy_bits_do_not_depend_on_the_batch(gpu, lsp):
    x, where = batch_rows(34, 130, True)
    call = lambda b, r: lsp.postfilter_lsp(b, r, 0.55, G3, 0.7, 256, True, True, energies=True)
    out, e1, e2, st = on_gpu(gpu, x, call)
    for i in (0, 77, where["close"], where["low_gain"], 129):
        o1, a1, a2, s1 = on_gpu(gpu, x[i:i + 1], call)
        assert same_bits(o1[0], out[i]) and a1[0] == e1[i] and a2[0] == e2[i] and s1[0] == st[i]


@pytest.mark.parametrize("log_gain", [False, True])
def test_postfilter(gpu, lsp, log_gain):
    m, alpha, gamma, beta, length, n = 34, 0.55, G3, 0.7, 64, 130
    x, where = batch_rows(m, n, log_gain)
    ref = energy_reference(m, n, alpha, gamma, beta, length, log_gain)
    assert all(r is None or not r[1] & 12 for r in ref)
    # compensation 0, no energy asked for: one launch, gain bits untouched, LSPs filtered from the raw row, unchecked
    out, st = on_gpu(gpu, x, lambda b, r: lsp.postfilter_lsp(b, r, alpha, gamma, beta, length, log_gain=log_gain))
    for i, row in enumerate(x):
        if np.isfinite(row).all():
            assert st[i] == 0 and same_bits(out[i], L.filter_row(row, beta)), i
            assert same_bits(out[i, [0, 1, m]], row[[0, 1, m]])
        else:
            assert st[i] == 4 and (out[i] == 0).all()
    i = where["swapped"]
    assert out[i, 1] == x[i, 1] > out[i, m] == x[i, m]                   # not sorted: the script merges the file as written
    assert st[where["nan"] - 1] == 0 and st[where["nan"] + 1] == 0
    # compensation 1
    comp, e1, e2, st1 = on_gpu(gpu, x, lambda b, r: lsp.postfilter_lsp(b, r, alpha, gamma, beta, length, True, log_gain,
                                                                       energies=True))
    err, bound = [], []
    for i, r in enumerate(ref):
        if r is None:
            assert st1[i] & 12 and (comp[i] == 0).all() and e1[i] == 0 and e2[i] == 0
            continue
        ((w1, t1), (w2, t2)), want_st, p = r
        assert st1[i] == want_st and same_bits(comp[i, 1:], p[1:]) and same_bits(comp[i, 1:], out[i, 1:])
        if log_gain:
            want = x[i, 0] + (w1 - w2)
            tol = t1 + t2 + 4 * np.spacing(abs(want))
        else:
            want = x[i, 0] * math.exp(w1 - w2)
            tol = abs(want) * (t1 + t2) + 8 * np.spacing(abs(want))
        # the gain as the call's own energies give it, exactly where the expression has no library function in it
        if log_gain:
            assert comp[i, 0] == x[i, 0] + (e1[i] - e2[i])
        err.append(abs(float(comp[i, 0]) - want))
        bound.append(tol)
    assert len(err) == n - 1 and worst("compensated gain, log_gain %d" % log_gain, err, bound) <= 1.0
    assert np.abs(comp[:, 0] - out[:, 0]).max() > 1e-3                   # and it does something
    # in place
    def in_place(b, r):
        buf = r.clone()
        got, a1, a2, s = lsp.postfilter_lsp(b, buf, alpha, gamma, beta, length, True, log_gain, energies=True, out=buf)
        return got, a1, a2, s, buf
    got, a1, a2, s, buf = on_gpu(gpu, x, in_place)
    assert same_bits(got, comp) and same_bits(buf, comp) and same_bits(a1, e1) and same_bits(a2, e2) and same_bits(s, st1)
    plain_in_place = on_gpu(gpu, x, lambda b, r: lsp.postfilter_lsp(b, r, alpha, gamma, beta, length, log_gain=log_gain, out=r))
    assert same_bits(plain_in_place[0], out)


def test_postfilter_identities(gpu, lsp):
    for m, beta in ((34, 1.0), (2, 0.7), (1, 0.7)):
        x, _ = batch_rows(m, 130, False)
        out, e1, e2, st = on_gpu(gpu, x, lambda b, r: lsp.postfilter_lsp(b, r, 0.55, G3, beta, 256, True, energies=True))
        assert same_bits(out, x) and (st == 0).all() and (e1 == 0).all() and (e2 == 0).all()     # NaN and all: a copy
    x, _ = batch_rows(3, 130, False)                                      # the least order with a filtered LSP
    out, st = on_gpu(gpu, x, lambda b, r: lsp.postfilter_lsp(b, r, 0.55, G3, 0.7, 256))
    good = np.isfinite(x).all(axis=1)
    assert same_bits(out[good], np.stack([L.filter_row(r, 0.7) for r in x[good]])) and (out[good, 2] != x[good, 2]).any()


def test_bad_options_are_refused_before_any_launch(gpu, lsp):
    torch, W, ctx = gpu
    b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=[4])
    rows = lambda cols: torch.full((4, cols), 0.5, dtype=torch.float64, device="cuda")
    ctx.timing_enable(True)
    try:
        for call in (lambda: lsp.lsp_to_lpc(b, rows(65)), lambda: lsp.lsp_to_lpc(b, rows(35), gamma=0.0),
                     lambda: lsp.lsp_to_lpc(b, rows(35), min_distance=1.5), lambda: lsp.lsp_to_lpc(b, rows(35), min_gain=0.0),
                     lambda: lsp.lsp_to_mel_generalized_cepstrum(b, rows(35), 1.0, -0.5),
                     lambda: lsp.lsp_to_mel_generalized_cepstrum(b, rows(35), 0.5, -0.5, out_order=4096),
                     lambda: lsp.postfilter_lsp(b, rows(35), 0.55, -0.5, length=100),
                     lambda: lsp.postfilter_lsp(b, rows(35), 0.55, -0.5, beta=float("nan")),
                     lambda: lsp.postfilter_lsp(b, rows(35), 0.55, 0.5)):
            with pytest.raises(RuntimeError, match="bad argument"):
                call()
        big = torch.full((6, 35), 0.5, dtype=torch.float64, device="cuda")
        with pytest.raises(RuntimeError, match="bad argument"):            # a shifted view of the input is no in-place call
            lsp.postfilter_lsp(b, big[:4], 0.55, -0.5, out=big[2:])
        assert ctx.timing_query("lsp_kernel")[1] == 0 and ctx.timing_query("mgc2mgc_kernel")[1] == 0
        lsp.lsp_to_lpc(b, rows(35))
        assert ctx.timing_query("lsp_kernel")[1] == 1
    finally:
        ctx.timing_enable(False)
        b.close()


def test_on_a_callers_own_stream(gpu, lsp):
    """In the manner of tests/test_gpu_caller_stream.py, with its Env: the context sits on a non-blocking stream U; after
    a warm-up on stale rows, a delay of about 50 ms, an event and the copy of the fresh rows are queued on U and the
    calls made at once.  They return while the delay still runs, and what they leave on U is the fresh rows' result,
    bit for bit the stream-0 context's."""
    import test_gpu_caller_stream as CS
    torch, W, ctx0 = gpu
    env = CS.Env(torch, W, ctx0)
    x, _ = batch_rows(34, 130, True)
    fresh = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    stale = torch.nan_to_num(torch.roll(fresh, 1, 0), nan=0.5)
    calls = (lambda b, r: lsp.lsp_to_lpc(b, r, log_gain=True, checked=True),
             lambda b, r: lsp.lsp_to_mel_generalized_cepstrum(b, r, 0.55, G3, log_gain=True),
             lambda b, r: lsp.postfilter_lsp(b, r, 0.55, G3, 0.7, 256, True, True, energies=True))
    want = [on_gpu(gpu, x, call) for call in calls]
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(env.U):
            b = W.WorldBatch(env.ctx, W.default_params(48000, 5.0), f0_lengths=uneven(len(x)))
            try:
                for call, w in zip(calls, want):
                    buf = stale.clone()
                    call(b, buf)                                         # the warm-up: workspaces, function attributes
                    env.U.synchronize()
                    out, done, pending = env.behind_delay([buf], [fresh], lambda: call(b, buf))
                    got = [t.clone() for t in out]
                    env.U.synchronize()
                    assert done.query() and pending, "the call waited for its stream"
                    for g, v in zip(got, w):
                        assert same_bits(g.cpu().numpy(), v)
            finally:
                env.U.synchronize()
                b.close()
    finally:
        env.ctx.close()

"""The feature codec's kernels (csrc/codec.hip) against the oracle on rows that no analysis produces
(tests/codec_features.py).

Every other comparison of the codec feeds it what this library's own analysis gave: smooth envelopes, aperiodicities
inside (0, 1), four fs / fft_size / ndim shapes, aperiodicity band counts 1 and 5, ap_dim 25, 24, 9 and 41.  Here the
envelopes are rough, spiked, flat, denormal, zero and overflowing; the aperiodicities sit at their ends and on both sides
of both ends of the interval (0, 1e-4) in which the recipe sets bap's coefficient 0 to 0; the coded rows decode to
1e-250 ... 1e250; the band rows sit on CheckVUV's gate, one unit in the last place below and above it; ndim, the decoded
width and ap_dim take the values at which a kernel changes its path (1, 2, the 64-lane boundary, the coder's limit
F/4 + 1, the decoder's F/2, the bap decoder's switch between two frames per wavefront and one at order 31 / 32, its
largest order 62) at every fft_size, the float32 instantiations included; the frame counts are 1, 2, 7, and 20 000.
Every value of every row is compared, and every case prints its worst error over its bound ("codec-handmade ...",
under pytest -s).  The oracle itself is pinned to the compiled reference on the same grid (tests/test_oracle_vs_ref.py,
tests/test_golden.py: no grid entry on which the two put their non-finite values in different places).

Bounds: coding 1e-11 x max(1, max |coded|) (test_codec_against_oracle's bar, which analysis-made coefficients of order
10 meet as it stands; the rows here reach 50); envelope decoding rtol 1e-10; aperiodicity coding 1e-10 x max(1, max
|coded|) and decoding 1e-12 x max(1, max |ap|); the recipe's float32 files within one float32 spacing, at most 1 % of a
case's entries different at all, the rows whose bap coefficient 0 is exactly 0 the oracle's; recipe_decode f0 rtol
1e-14, sp rtol 1e-10, ap rtol 1e-11 x max(1, max |x|) with x the exponent of mgc2sp, bins from the order on exactly 0.

Found with these cases: nothing.  Every case passes on an MI355X, far inside its bound (below), so csrc/codec.hip is
unchanged.  What the cases add is that a defect can no longer hide: with CodeOpts::c0_snap ignored, or its threshold
at 1e-5, test_recipe_features fails on the snap rows (and on the 1 - 1e-12 rows, and test_many_frames); with zero_value
ignored it fails on the zeros envelopes; with the bap decoder's two-frames-per-wavefront kernel chosen at order 32,
test_recipe_decode fails at ap_dim 32 and 33 at every fft_size; with CheckVUV's gate at mean >= -0.5,
test_aperiodicity_bands fails at every rate.  Striding the bap decoder's frame loop by gridDim.x instead of
gridDim.x x 2 is no defect of value: every frame is still computed, some twice, to the same bits, and all tests pass.

Largest error / bound per entry point and fft_size on an MI355X (one run; "codec-handmade" lines under pytest -s):

    fft_size                          512       1024      2048      4096
    code_spectral_envelope            1.9e-5    1.9e-5    9.7e-6    2.0e-5
    decode_spectral_envelope          2.9e-3    3.6e-3    3.4e-3    4.6e-3
    code_aperiodicity                 -         1.7e-6    1.5e-6    7.1e-7
    decode_aperiodicity               -         4.4e-4    4.4e-4    5.0e-4
    recipe_features, in spacings      0         0         0         0       (no entry differs from the oracle's at all)
    recipe_decode f0                  0         0         0         0
    recipe_decode sp                  2.9e-4    2.9e-4    3.5e-4    2.9e-4
    recipe_decode ap                  4.3e-5    5.5e-5    4.5e-5    6.9e-5
    C ABI at 1024: CodeSpectralEnvelope 1.9e-5, DecodeSpectralEnvelope 3.4e-3
"""
import functools

import numpy as np
import pytest

import codec_features as cf

pytestmark = pytest.mark.gpu

FOUR = cf.INSTANTIATIONS[:4]
MANY = 20000                                                    # more frames than any grid: the kernels are persistent
DEFAULT_ROW = 1.0 - 1e-12                                       # InitializeAperiodicity, codec.cpp:20-25


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.bindings import Oracle
    return Oracle()


@functools.lru_cache(maxsize=None)
def want(case):
    """The oracle's outputs on a grid entry, computed once and left unchanged."""
    out = cf.outputs(_oracle(), case)
    for a in out:
        a.setflags(write=False)
    return out


def batch(gpu, fs, F, lengths=(cf.NF,)):
    torch, W, ctx = gpu
    b = W.WorldBatch(ctx, W.default_params(fs, 5.0, fft_size=F), f0_lengths=list(lengths))
    assert b.fft_size == F and b.total_frames == sum(lengths)
    return b


def dev(gpu, a):
    return gpu[0].from_numpy(np.ascontiguousarray(a)).cuda()


def host(*tensors):
    out = tuple(t.cpu().numpy() for t in tensors)
    return out if len(out) > 1 else out[0]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def report(entry, F, what, ratio):
    print("codec-handmade %s F=%d %s err/bound=%.3e" % (entry, F, what, ratio))


def atol_ratio(got, ref, factor):
    """Worst |got - ref| over factor x max(1, max |ref|); every value finite."""
    assert got.shape == ref.shape and np.isfinite(ref).all() and np.isfinite(got).all()
    if not ref.size:
        return 0.0
    return float(np.abs(got - ref).max() / (factor * max(1.0, np.abs(ref).max())))


def rtol_ratio(got, ref, rtol):
    assert got.shape == ref.shape and np.isfinite(ref).all() and np.isfinite(got).all() and (ref != 0).all()
    return float((np.abs(got - ref) / np.abs(ref)).max() / rtol)


def refused(call, how="bad argument"):
    with pytest.raises(RuntimeError, match=how):
        call()


# ---- code_spectral_envelope / decode_spectral_envelope (double) ----------------------------------------------------
@pytest.mark.parametrize("inst", cf.INSTANTIATIONS, ids=lambda i: "%d-%d" % i)
@pytest.mark.parametrize("name", ["rough", "spike", "flat", "denormal"])
def test_code_spectral_envelope(gpu, name, inst):
    fs, F = inst
    b = batch(gpu, fs, F)
    sp = dev(gpu, cf.envelope(name, fs, F))
    worst = 0.0
    for ndim in cf.code_ndims(F):
        ref, = want(("code_sp", name, fs, F, (ndim,)))
        got = host(b.code_spectral_envelope(sp, ndim))
        r = atol_ratio(got, ref, 1e-11)
        report("code_sp", F, "%s fs=%d ndim=%d max|c|=%.1f" % (name, fs, ndim, np.abs(ref).max()), r)
        worst = max(worst, r)
    b.close()
    assert worst <= 1.0


@pytest.mark.parametrize("inst", cf.INSTANTIATIONS, ids=lambda i: "%d-%d" % i)
@pytest.mark.parametrize("name", cf.DECODE_FAMILIES)
def test_decode_spectral_envelope(gpu, name, inst):
    fs, F = inst
    b = batch(gpu, fs, F)
    worst = 0.0
    for width in cf.decode_widths(F):
        ref, = want(("decode_sp", name, fs, F, (width,)))
        assert np.isfinite(ref).all() and (np.abs(ref) >= 2.2250738585072014e-308).all(), "normal finite doubles"
        if name == "wide" and width > 1:
            assert ref.min() < 1e-245 and ref.max() > 1e245
        got = host(b.decode_spectral_envelope(dev(gpu, cf.coded_sp(name, fs, F, width))))
        r = rtol_ratio(got, ref, 1e-10)
        report("decode_sp", F, "%s fs=%d width=%d" % (name, fs, width), r)
        worst = max(worst, r)
    b.close()
    assert worst <= 1.0


@pytest.mark.parametrize("inst", cf.INSTANTIATIONS, ids=lambda i: "%d-%d" % i)
def test_widths_outside_the_limits_are_refused(gpu, inst):
    torch, W, ctx = gpu
    fs, F = inst
    b = batch(gpu, fs, F)
    sp = dev(gpu, cf.envelope("rough", fs, F))
    for ndim in (0, F // 4 + 2):
        refused(lambda: b.code_spectral_envelope(sp, ndim))
    coded = torch.zeros(cf.NF, F // 2 + 1, dtype=torch.float64, device="cuda")
    refused(lambda: b.decode_spectral_envelope(coded))
    b.close()


# ---- code_aperiodicity / decode_aperiodicity -----------------------------------------------------------------------
@pytest.mark.parametrize("rate", cf.AP_RATES, ids=lambda i: "%d-%d" % i)
def test_aperiodicity_bands(gpu, rate):
    """1 to 5 bands.  Rows on the gate of CheckVUV take the oracle's side of it exactly: the default row, or not."""
    torch, W, ctx = gpu
    fs, F = rate
    nap = cf.n_bands(fs)
    assert W.load_library().WorldMi355GetNumberOfAperiodicities(fs) == nap == _oracle().num_aperiodicities(fs)
    b = batch(gpu, fs, F)
    worst_c = worst_d = 0.0
    for name in ("mid", "one", "tiny", "ends"):
        ref, = want(("code_ap", name, fs, F, ()))
        assert ref.shape == (cf.NF, nap)
        if name == "tiny":
            np.testing.assert_allclose(ref, -6000.0, rtol=1e-12)
        r = atol_ratio(host(b.code_aperiodicity(dev(gpu, cf.aperiodicity(name, fs, F)))), ref, 1e-10)
        report("code_ap", F, "%s fs=%d bands=%d" % (name, fs, nap), r)
        worst_c = max(worst_c, r)
    for name in cf.CODED_AP:
        ref, = want(("decode_ap", name, fs, F, ()))
        default = (ref == DEFAULT_ROW).all(axis=1)
        if name in ("gate", "below", "plus5"):
            assert not default.any(), "decoded: the gate is mean > -0.5"
        if name in ("above", "mean0"):
            assert default.all()
        if name == "plus5" and nap > 1:
            assert ref.max() > 1.5
        got = host(b.decode_aperiodicity(dev(gpu, cf.coded_ap(name, fs))))
        assert np.array_equal((got == DEFAULT_ROW).all(axis=1), default), name
        assert np.array_equal(got[default], ref[default])
        r = atol_ratio(got, ref, 1e-12)
        report("decode_ap", F, "%s fs=%d bands=%d" % (name, fs, nap), r)
        worst_d = max(worst_d, r)
    b.close()
    assert worst_c <= 1.0 and worst_d <= 1.0


def test_no_bands_at_8000_hz(gpu, pkg):
    """GetNumberOfAperiodicities(8000) is 0: coding gives rows of no columns, through the batch and through the drop-in
    C ABI; decoding is refused by the batch ("unsupported configuration").  The drop-in DecodeAperiodicity ends the
    process on a refused call, as every drop-in entry point does without an error handler, so it is not called here."""
    torch, W, ctx = gpu
    fs, F = 8000, 512
    assert W.load_library().WorldMi355GetNumberOfAperiodicities(fs) == 0 == _oracle().num_aperiodicities(fs)
    assert pkg.capi.get_number_of_aperiodicities(fs) == 0 == cf.n_bands(fs)
    ap = cf.aperiodicity("mid", fs, F)
    b = batch(gpu, fs, F)
    coded = b.code_aperiodicity(dev(gpu, ap))
    assert tuple(coded.shape) == (cf.NF, 0) and coded.dtype == torch.float64
    refused(lambda: b.decode_aperiodicity(coded), "unsupported configuration")
    b.close()
    assert pkg.capi.code_aperiodicity(ap, fs, F).shape == (cf.NF, 0)


# ---- recipe_features (float32) -------------------------------------------------------------------------------------
def f32_case(gots, refs):
    """The recipe's float32 files of one case against the oracle's: every finite entry within one float32 spacing;
    returns (entries different at all / 1 % of the entries, worst difference in spacings)."""
    differ = total = 0
    worst = 0.0
    for g, r in zip(gots, refs):
        assert g.dtype == np.float32 == r.dtype and g.shape == r.shape
        fin = np.isfinite(r)
        assert np.array_equal(np.isfinite(g), fin)
        g, r = g[fin], r[fin]
        if r.size:
            worst = max(worst, float((np.abs(g.astype(np.float64) - r) / np.spacing(np.abs(r))).max()))
        differ += int((g != r).sum())
        total += r.size
    return differ / (0.01 * total), worst


@pytest.mark.parametrize("inst", FOUR, ids=lambda i: "%d-%d" % i)
@pytest.mark.parametrize("pair", cf.RECIPE_PAIRS + (("huge", "mid"),), ids=lambda p: "%s-%s" % p)
def test_recipe_features(gpu, pair, inst):
    """The float32 instantiations of the coder at every fft_size, spec_dim 1 / 50 / 65 and ap_dim 2 / 25 / 64 / 65.
    zeros: the recipe's zero_value path, mgc finite everywhere.  snap, one: the rows whose bap coefficient 0 is exactly
    0.0f are the oracle's (analysis.cpp:350-353).  huge: mgc non-finite in the oracle's rows."""
    fs, F = inst
    e, a = pair
    name = e + ":" + a
    b = batch(gpu, fs, F)
    f0, sp, ap = (dev(gpu, v) for v in cf.inputs(("recipe_features", name, fs, F, (50, 25))))
    worst = (0.0, 0.0)
    for dims in (((50, 25),) if e == "huge" else cf.RECIPE_DIMS):
        refs = want(("recipe_features", name, fs, F, dims))
        gots = host(*b.recipe_features(f0, sp, ap, *dims))
        assert gots[1].shape == (cf.NF, dims[0]) and gots[2].shape == (cf.NF, dims[1])
        zero = refs[2][:, 0] == 0.0
        if a in ("snap", "one+mid"):
            assert zero.any() and not zero.all(), "some rows are set to 0 and some are not"
        if a == "snap":
            d = np.array(cf.SNAP_D)
            assert np.array_equal(zero, (d > 0) & (d < 1e-4)) and np.abs(refs[2][~zero, 0] - d[~zero]).max() < 1e-9
            # every d clear of both ends by 3e-7 or more: eight orders above the coder's error, so the side is certain
            assert np.abs(d - 1e-4).min() > 9e-6 and np.abs(d).min() >= 3e-7
        assert np.array_equal(gots[2][:, 0] == 0.0, zero), "rows whose bap c0 is exactly 0"
        if e == "zeros":
            assert np.isfinite(refs[1]).all() and np.isfinite(gots[1]).all()
        if e == "huge":
            bad = ~np.isfinite(refs[1]).all(axis=1)
            assert bad[cf.HUGE_ROW] and bad.sum() == 1
            assert np.array_equal(~np.isfinite(gots[1]).all(axis=1), bad)
        r = f32_case(gots, refs)
        report("recipe_features", F, "%s fs=%d dims=%s differ/1%%=%.3f" % (name, fs, dims, r[0]), r[1])
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    b.close()
    assert worst[1] <= 1.0, "within one float32 spacing"
    assert worst[0] <= 1.0, "at most 1 % of a case's entries differ at all"


# ---- recipe_decode ---------------------------------------------------------------------------------------------------
def decode_ratios(gots, refs, x_scale, order):
    g_f0, g_sp, g_ap = gots
    o_f0, o_sp, o_ap = refs
    assert np.array_equal(g_f0 == 0, o_f0 == 0), "identical zeros"
    nz = o_f0 != 0
    r_f0 = rtol_ratio(g_f0[nz], o_f0[nz], 1e-14) if nz.any() else 0.0
    r_sp = rtol_ratio(g_sp, o_sp, 1e-10)
    r_ap = rtol_ratio(g_ap[:, :order], o_ap[:, :order], 1e-11 * max(1.0, x_scale))
    assert not g_ap[:, order:].any() and not o_ap[:, order:].any(), "bins from the order on are exactly 0"
    return r_f0, r_sp, r_ap


def _dims(fs, F):
    return sorted({c[2] for c in cf.recipe_decode_cases() if c[:2] == (fs, F)})


@pytest.mark.parametrize("fs,F,ap_dim", [(fs, F, d) for fs, F in FOUR for d in _dims(fs, F)])
def test_recipe_decode(gpu, fs, F, ap_dim):
    """ap_dim 25 and 33 at every fft_size: the eight instantiations of the bap kernel; at 1024 also the smallest orders,
    the orders on either side of its switch between two frames per wavefront and one, and the largest.  1, 2 and 7
    frames: an odd count leaves the second half of a two-frame wavefront without a frame."""
    order = cf.bap_order(ap_dim)
    worst = (0.0, 0.0, 0.0)
    for _, _, _, sigma, nf in [c for c in cf.recipe_decode_cases() if c[:3] == (fs, F, ap_dim)]:
        case = ("recipe_decode", "files", fs, F, (ap_dim, sigma, nf))
        lf0, mgc, bap = cf.inputs(case)
        o_f0, o_sp, x = want(case)
        refs = _oracle().recipe_decode(lf0, mgc, bap, fs, F)
        assert np.array_equal(refs[0], o_f0) and np.array_equal(refs[1], o_sp)
        b = batch(gpu, fs, F, (nf,))
        gots = host(*b.recipe_decode(dev(gpu, lf0), dev(gpu, mgc), dev(gpu, bap)))
        b.close()
        r = decode_ratios(gots, refs, float(np.abs(x).max()), order)
        report("recipe_decode", F, "fs=%d ap_dim=%d sigma=%g nf=%d max|x|=%.1f f0 %.3e sp %.3e ap"
               % (fs, ap_dim, sigma, nf, np.abs(x).max(), r[0], r[1]), r[2])
        worst = tuple(max(p, q) for p, q in zip(worst, r))
    assert max(worst) <= 1.0, worst


def test_ap_dims_outside_the_limits_are_refused(gpu):
    fs, F = 16000, 1024
    b = batch(gpu, fs, F)
    for ap_dim in (1, 64, 65):
        lf0, mgc, bap = cf.recipe_files(fs, F, ap_dim, 0.3)
        refused(lambda: b.recipe_decode(dev(gpu, lf0), dev(gpu, mgc), dev(gpu, bap)))
    b.close()


# ---- row isolation ---------------------------------------------------------------------------------------------------
def tiled(rows, n):
    return np.ascontiguousarray(np.tile(rows, (-(-n // len(rows)), 1))[:n])


SPECIAL = {"zeros": cf.ZERO_ROWS, "huge": (cf.HUGE_ROW,), "nan": (cf.NAN_ROW,)}


@pytest.mark.parametrize("fs,F,nf", [cf.ISOLATION[0] + (cf.NF,), cf.ISOLATION[1] + (cf.NF,), cf.ISOLATION[0] + (MANY,)])
@pytest.mark.parametrize("kind,name", [("code_sp", "zeros"), ("code_sp", "huge"), ("recipe_features", "huge"),
                                       ("decode_sp", "nan")])
def test_a_bad_row_leaves_its_neighbours_alone(gpu, kind, name, fs, F, nf):
    """Rows that turn non-finite (zeros under the plain coder's log, 1e305 under the recipe's x 1e4, a NaN coefficient)
    share the persistent kernels' LDS image with the rows their wavefront handles next: every other row keeps the bits
    it has in the same batch with those rows replaced by clean ones, and values are non-finite where the oracle's are.
    With 20 000 frames (the 7 rows tiled) a wavefront handles several rows.  The plain coder keeps the row holding
    1e305 finite, as the oracle does: only the recipe's x 1e4 takes it to infinity."""
    case = {"code_sp": ("code_sp", name, fs, F, (65,)), "decode_sp": ("decode_sp", name, fs, F, (65,)),
            "recipe_features": ("recipe_features", "huge:mid", fs, F, (50, 25))}[kind]
    which = 1 if kind == "recipe_features" else 0
    ref, rows = want(case)[which], cf.inputs(case)[which]
    special = np.isin(np.arange(cf.NF), SPECIAL[name])
    bad = ~np.isfinite(ref).all(axis=1)
    assert np.array_equal(bad, special & ((kind, name) != ("code_sp", "huge")))
    assert np.array_equal(~np.isfinite(ref).any(axis=1), bad), "a bad row is non-finite throughout"
    clean = cf.coded_sp("c0", fs, F, 65) if kind == "decode_sp" else cf.envelope("rough", fs, F)
    mended = np.where(special[:, None], clean, rows)
    b = batch(gpu, fs, F, (nf,))

    def run(r):
        r = dev(gpu, tiled(r, nf))
        if kind == "code_sp":
            return host(b.code_spectral_envelope(r, 65))
        if kind == "decode_sp":
            return host(b.decode_spectral_envelope(r))
        f0, ap = dev(gpu, tiled(np.array(cf.F0)[:, None], nf)[:, 0]), dev(gpu, tiled(cf.aperiodicity("mid", fs, F), nf))
        return host(b.recipe_features(f0, r, ap, 50, 25)[1])
    got, other = run(rows), run(mended)
    b.close()
    keep = ~tiled(special[:, None], nf)[:, 0]
    assert np.isfinite(other).all() and np.isfinite(got[keep]).all() and keep.sum() >= nf // 2
    assert np.array_equal(bits(got[keep]), bits(other[keep])), "the other rows keep their bits"
    assert np.array_equal(np.isfinite(got), tiled(np.isfinite(ref), nf)), "non-finite where the oracle's are"


# ---- more frames than the grid ---------------------------------------------------------------------------------------
def test_many_frames(gpu):
    """20 000 frames at 8000 / 512, 64 distinct rows tiled: frame i has the bits of frame i mod 64, and frames 0 ... 63
    are within the bounds.  The oracle sees 64 rows."""
    fs, F, o = 8000, 512, _oracle()
    sp64, ap64 = cf.envelope("rough", fs, F, 64), cf.aperiodicity("one+mid", fs, F, 64)
    f064 = tiled(np.array(cf.F0)[:, None], 64)[:, 0]
    lf0, mgc, bap = cf.recipe_files(fs, F, 25, 1.5, 64)
    b = batch(gpu, fs, F, (MANY,))
    sp, ap, f0 = dev(gpu, tiled(sp64, MANY)), dev(gpu, tiled(ap64, MANY)), dev(gpu, tiled(f064[:, None], MANY)[:, 0])

    def same_as_first_64(a):
        assert np.array_equal(bits(a), bits(tiled(a[:64].reshape(64, -1), MANY).reshape(a.shape))), "frame i mod 64"
        return a[:64]
    got = same_as_first_64(host(b.code_spectral_envelope(sp, 65)))
    r = atol_ratio(got, o.code_spectral_envelope(sp64, fs, F, 65), 1e-11)
    report("code_sp", F, "many frames", r)
    assert r <= 1.0
    from test_golden import recipe_pack
    gots = [same_as_first_64(g) for g in host(*b.recipe_features(f0, sp, ap, 50, 25))]
    refs = recipe_pack(o, f064, sp64, ap64, fs, F, 50, 25)
    assert np.array_equal(gots[2][:, 0] == 0.0, refs[2][:, 0] == 0.0) and 0 < (refs[2][:, 0] == 0.0).sum() < 64
    r = f32_case(gots, refs)
    report("recipe_features", F, "many frames differ/1%%=%.3f" % r[0], r[1])
    assert max(r) <= 1.0
    gots = [same_as_first_64(g) for g in
            host(*b.recipe_decode(dev(gpu, tiled(lf0[:, None], MANY)[:, 0]), dev(gpu, tiled(mgc, MANY)), dev(gpu, tiled(bap, MANY))))]
    b.close()
    x = np.stack([o.mgc2sp(row, 0.55, F, 24) for row in cf.bap_rows(bap)])
    r = decode_ratios(gots, o.recipe_decode(lf0, mgc, bap, fs, F), float(np.abs(x).max()), 24)
    report("recipe_decode", F, "many frames f0 %.3e sp %.3e ap" % r[:2], r[2])
    assert max(r) <= 1.0


# ---- one ragged batch --------------------------------------------------------------------------------------------------
def test_ragged_batch(gpu):
    """Utterances of 1, 7, 2 and 64 frames of different families in one batch: each has the bits of the same utterance
    run alone, through every entry point."""
    fs, F, lens = 16000, 1024, (1, 7, 2, 64)
    env = [cf.envelope(n, fs, F, nf) for n, nf in zip(("spike", "zeros", "flat", "rough"), lens)]
    aps = [cf.aperiodicity(n, fs, F, nf) for n, nf in zip(("one", "snap", "ends", "one+mid"), lens)]
    f0s = [tiled(np.array(cf.F0)[:, None], nf)[:, 0] for nf in lens]
    cod = [cf.coded_sp(n, fs, F, 65, nf) for n, nf in zip(("wide", "c-60", "c40", "c0"), lens)]
    cap = [cf.coded_ap(n, fs, nf) for n, nf in zip(("gate", "random", "above", "below"), lens)]
    files = [cf.recipe_files(fs, F, 25, s, nf) for s, nf in zip((0.3, 1.5, 0.3, 1.5), lens)]

    def run(b, u):
        pick = (lambda parts: dev(gpu, np.concatenate(parts))) if u is None else (lambda parts: dev(gpu, parts[u]))
        sp, ap = pick(env), pick(aps)
        outs = [b.code_spectral_envelope(sp, 65), b.decode_spectral_envelope(pick(cod)), b.code_aperiodicity(ap),
                b.decode_aperiodicity(pick(cap)), *b.recipe_features(pick(f0s), sp, ap, 50, 25),
                *b.recipe_decode(*(pick([f[k] for f in files]) for k in range(3)))]
        return [host(t) for t in outs]
    b = batch(gpu, fs, F, lens)
    whole = [b.split_frames(a) for a in run(b, None)]
    b.close()
    for u, nf in enumerate(lens):
        b1 = batch(gpu, fs, F, (nf,))
        for k, alone in enumerate(run(b1, u)):
            assert alone.shape[0] == nf and np.array_equal(bits(alone), bits(whole[k][u])), (u, k)
        b1.close()


# ---- the drop-in C ABI -------------------------------------------------------------------------------------------------
def test_drop_in_c_abi(gpu, pkg):
    fs, F = 16000, 1024
    ref, = want(("code_sp", "rough", fs, F, (65,)))
    r = atol_ratio(pkg.capi.code_spectral_envelope(cf.envelope("rough", fs, F), fs, F, 65), ref, 1e-11)
    report("capi.code_sp", F, "rough", r)
    ref, = want(("decode_sp", "wide", fs, F, (65,)))
    assert ref.min() < 1e-245 and ref.max() > 1e245
    r2 = rtol_ratio(pkg.capi.decode_spectral_envelope(cf.coded_sp("wide", fs, F, 65), fs, F), ref, 1e-10)
    report("capi.decode_sp", F, "wide", r2)
    assert r <= 1.0 and r2 <= 1.0

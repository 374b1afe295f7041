"""The Synthesis kernels against the oracle on feature sets that no analysis produces (tests/synth_features.py).

Every other comparison of csrc/synthesis.hip feeds it what this library's own analysis gave: a smooth f0 contour of
65-330 Hz, voiced stretches of 0.3 s or more, smooth envelopes.  The recipe calls Synthesis on model-generated
lf0 / mgc / bap, so here the contours are arbitrary (voicing that flips per frame, 10 Hz to 0.3 fs, values on the
lowest_f0 gate, periods of a whole number of samples that put every pulse on a phase-wrap tie and on the edges of the
pulse search's tiles), the envelopes rough, the aperiodicities at their clamps, and the outputs shorter and longer than
the frames cover.  Every sample of every case is compared; the tolerance is the project's bar for y, 1e-8
(test_gpu_parity.Y_TOL), times max(1, max|y_oracle|) for the cases whose output exceeds 1.

Found with these cases: wrap_two_pi returned the remainder in [0, 2 pi) where fmod keeps the sign of the accumulated
phase.  A y_length far enough beyond the frames of a contour that ends on a fall extrapolates f0 below zero until the
phase itself turns negative ("jumps:smooth:mid:lenfar"); every pulse from there on had another time shift than the
reference's.  The defect was found by reading the kernel beside the reference; the size of its effect on y has not
been measured on a GPU.  Fixed in synthesis.hip.

Largest max|y - y_oracle| / max(1, max|y_oracle|) per instantiation (fs / fft_size), against 1e-8: NOT MEASURED YET.
No run of this file on an MI355X has been recorded; test_case_against_oracle prints the figure of every case
("handmade <case> ... dev/scale=") under pytest -s, and the maxima per instantiation belong here.
"""
import numpy as np
import pytest

import synth_features as sf
from test_gpu_parity import Y_TOL

pytestmark = pytest.mark.gpu

# At most one pulse, the last, whose noise_size is 0: the reference's y is all zeros at these lengths.  Any kernel that
# writes zeros passes them: what they pin is that no pulse is rendered and that nothing is written outside y.
SILENT = ("len=1", "len=2", "len=100")
MIXED = ("alternating", "singles", "random", "gate", "negative")      # contours with voiced and unvoiced pulses


def tolerance(yo):
    return Y_TOL * max(1.0, float(np.abs(yo).max()) if len(yo) else 0.0)


def non_degenerate(oracle, case, f0, sp, ap, n, yo):
    """The case is what its name says, judged on the oracle's side alone."""
    name, fs, F, fp = case
    contour, length = name.split(":")[0], name.split(":")[-1]
    idx, voiced, total = sf.time_base(f0, fs, F, fp, n)
    assert np.isfinite(yo).all()
    if length in SILENT:
        assert len(idx) <= 1 and not yo.any()
        return idx
    assert np.abs(yo).max() > 0
    if contour in MIXED:
        assert voiced.any() and (~voiced).any(), "voiced and unvoiced pulses"
    else:
        assert voiced.all() and len(idx) > 0
    if contour.startswith("fs"):                          # a pulse on or next to every multiple of 2048 inside y
        edges = np.arange(2048, n - 1, 2048)
        assert all(np.abs(idx - e).min() <= 2 for e in edges), "a pulse at each tile edge"
        assert len(edges) > 0 or n <= 2049
    if length == "lenfar" and contour == "jumps":
        assert total.min() < -2.0 * np.pi, "the accumulated phase turns negative"
    if length in ("lenlong", "lenfar"):
        assert idx.max() / fs > len(f0) * fp / 1000.0, "pulses beyond the last knot"
    # the spectra matter: the neighbouring frame's rows give another waveform
    rolled = oracle.synthesis(f0, np.roll(sp, 1, axis=0), np.roll(ap, 1, axis=0), F, fp, fs, n)
    assert np.abs(rolled - yo).max() > 1000.0 * tolerance(yo)
    return idx


def gpu_synthesis(gpu, case_arrays, fs, F, fp):
    """One WorldBatch over the given (f0, sp, ap, y_length) sets; returns (batch, y) with y on the device."""
    torch, W, ctx = gpu
    b = W.WorldBatch(ctx, W.default_params(fs, fp, fft_size=F), f0_lengths=[len(c[0]) for c in case_arrays],
                     y_lengths=[c[3] for c in case_arrays])
    assert b.fft_size == F
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    f0, sp, ap = (dev(np.concatenate([c[k] for c in case_arrays])) for k in range(3))
    return b, (f0, sp, ap), b.synthesize(f0, sp, ap)


@pytest.mark.parametrize("case", sf.grid(), ids=sf.case_id)
def test_case_against_oracle(gpu, oracle, case):
    name, fs, F, fp = case
    f0, sp, ap, n = sf.case(*case)
    yo = oracle.synthesis(f0, sp, ap, F, fp, fs, n)
    idx = non_degenerate(oracle, case, f0, sp, ap, n, yo)
    b, _, y = gpu_synthesis(gpu, [(f0, sp, ap, n)], fs, F, fp)
    y = y.cpu().numpy()
    b.close()
    dev = float(np.abs(y - yo).max())
    print("handmade %s pulses=%d max|y|=%.3e dev=%.3e dev/scale=%.3e" % (sf.case_id(case), len(idx), np.abs(yo).max(), dev,
                                                                       dev / max(1.0, np.abs(yo).max())))
    assert np.isfinite(y).all()
    np.testing.assert_allclose(y, yo, atol=tolerance(yo), rtol=0)


def all_unvoiced(fs, F, fp, nf=50):
    _, sp, ap, _ = sf.case("random", fs, F, fp)
    return np.zeros(nf), sp[:nf].copy(), ap[:nf].copy(), sf.recipe_length(nf, fs, fp)


def two_frames(fs, F, fp):
    _, sp, ap, _ = sf.case("jumps", fs, F, fp)
    return np.array([900.0, 700.0]), sp[:2].copy(), ap[:2].copy(), sf.recipe_length(2, fs, fp)


def test_ragged_batch(gpu, oracle, monkeypatch):
    """Utterances of different contour kinds and lengths in one WorldBatch: each equals the oracle, each is bit-identical
    to the same utterance synthesised alone, and the batch is bit-identical whatever the size of the response scratch."""
    torch, W, ctx = gpu
    fs, F, fp = 16000, 1024, 5.0
    names = ["random", "alternating:rough", "jumps:smooth:mid:lenlong", "const03fs", "singles:smooth:ap0bin",
             "fs32:smooth:mid:len=4097", "gate:smooth:ap1", "const41", "negative:rough:apneg", "jumps:smooth:mid:lenfar"]
    sets = [sf.case(nm, fs, F, fp) for nm in names]
    sets.insert(2, all_unvoiced(fs, F, fp))
    sets.insert(5, two_frames(fs, F, fp))
    assert len(sets) >= 8 and len({len(s[0]) for s in sets}) >= 6 and len({s[3] for s in sets}) >= 8
    assert sets[3][3] > sf.recipe_length(len(sets[3][0]), fs, fp)                 # a y_length beyond its frames
    b, (f0, sp, ap), y = gpu_synthesis(gpu, sets, fs, F, fp)
    y = y.clone()
    ys = b.split_out(y.cpu().numpy())
    for u, s in enumerate(sets):
        yo = oracle.synthesis(s[0], s[1], s[2], F, fp, fs, s[3])
        assert np.abs(yo).max() > 0, u
        print("ragged %d frames=%d samples=%d dev=%.3e" % (u, len(s[0]), s[3], np.abs(ys[u] - yo).max()))
        np.testing.assert_allclose(ys[u], yo, atol=tolerance(yo), rtol=0)
        b1, _, y1 = gpu_synthesis(gpu, [s], fs, F, fp)
        assert np.array_equal(y1.cpu().numpy(), ys[u]), u
        b1.close()
    for mb in ("1", "3"):                                   # 64 and 192 pulses per piece
        monkeypatch.setenv("WORLD_MI355_SCRATCH_MB", mb)
        assert torch.equal(b.synthesize(f0, sp, ap), y), mb
    b.close()


def test_two_part_split_with_dense_and_sparse_pulse_lists(gpu, oracle):
    """16 or more utterances and 4 Mi output samples: Synthesis alone prepares and renders the batch in two parts.
    Dense contours (1000 Hz, 0.3 fs: up to 89 000 pulses in an utterance, the whole list beyond the response scratch's cap)
    beside sparse ones (41 Hz).  Every utterance against itself synthesised alone, bit for bit.  Against the oracle: one
    utterance of the densest kind (0.3 fs) and one of the sparsest (41 Hz), the two shortest of the batch (36 000 and
    350 pulses), because the oracle takes 11 s on the longest 0.3 fs utterance (89 000 pulses) and 5 s on this one.
    So the longest lists are held to the kernels' own result on one utterance, not to the oracle: an error that the
    batched and the single call share, and that needs more than 36 000 pulses in an utterance to show, passes here."""
    torch, W, ctx = gpu
    fs, F, fp, bins = 16000, 1024, 5.0, 513
    kinds = [0.3 * fs, 41.0, 1000.0] * 6
    T = [2400 + 131 * ((7 * u) % 11) for u in range(len(kinds))]
    T[0], T[1] = 1500, 1700                                   # the two that go through the oracle: the cheapest
    sets = []
    for u, (hz, nf) in enumerate(zip(kinds, T)):
        seed = 7000 + u
        sets.append((np.full(nf, hz), sf.envelope("smooth", nf, bins, seed), sf.aperiodicity("mid", nf, bins, seed),
                     sf.recipe_length(nf, fs, fp)))
    assert len(sets) >= 16 and sum(s[3] for s in sets) >= 4 << 20
    b, _, y = gpu_synthesis(gpu, sets, fs, F, fp)
    assert bool(torch.isfinite(y).all())
    ys = b.split_out(y.cpu().numpy())
    b.close()
    for u in (0, 1):
        s = sets[u]
        yo = oracle.synthesis(s[0], s[1], s[2], F, fp, fs, s[3])
        idx, voiced, _ = sf.time_base(s[0], fs, F, fp, s[3])
        assert voiced.all() and np.abs(yo).max() > 0
        print("split %d f0=%g pulses=%d dev=%.3e" % (u, s[0][0], len(idx), np.abs(ys[u] - yo).max()))
        np.testing.assert_allclose(ys[u], yo, atol=tolerance(yo), rtol=0)
    for u, s in enumerate(sets):
        b1, _, y1 = gpu_synthesis(gpu, [s], fs, F, fp)
        assert np.array_equal(y1.cpu().numpy(), ys[u]), u
        b1.close()


@pytest.mark.parametrize("case", [("random", 8000, 512, 5.0), ("alternating:rough", 16000, 1024, 5.0),
                                  ("jumps:smooth:mid:lenfar", 16000, 1024, 5.0), ("gate", 16000, 2048, 5.0),
                                  ("fs32:smooth:mid:len=4097", 48000, 2048, 5.0), ("const03fs", 96000, 4096, 5.0),
                                  ("singles", 22050, 1024, 2.5), ("random:smooth:mid:len=2", 16000, 1024, 5.0)],
                         ids=sf.case_id)
def test_drop_in_synthesis_gives_the_batched_bits(gpu, pkg, case):
    """The reference's own entry point (host double*, double** rows) on hand-made sets: the bits of the batched call."""
    name, fs, F, fp = case
    f0, sp, ap, n = sf.case(*case)
    b, _, y = gpu_synthesis(gpu, [(f0, sp, ap, n)], fs, F, fp)
    y = y.cpu().numpy()
    b.close()
    y_c = pkg.capi.synthesis(f0, sp, ap, F, fp, fs, n)
    assert np.array_equal(y_c, y)


def test_recipe_files_of_a_hand_made_set(gpu, oracle):
    """A hand-made contour and envelope as the recipe's float32 lf0 / mgc / bap files (unvoiced frames marked -1e10),
    decoded and synthesised: against the oracle's decode and synthesis at the tolerances of
    test_gpu_parity.test_recipe_decode_against_oracle."""
    torch, W, ctx = gpu
    from test_golden import recipe_pack
    fs, F, fp = 16000, 1024, 5.0
    f0, sp, ap, n = sf.case("random", fs, F, fp)
    lf0, mgc, bap = recipe_pack(oracle, f0, sp, ap, fs, F, 50, 25)
    lf0[f0 == 0] = -1.0e10
    assert (f0 == 0).sum() > 10 and (f0 > 0).sum() > 10
    b = W.WorldBatch(ctx, W.default_params(fs, fp), f0_lengths=[len(f0)], y_lengths=[n])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g_f0, g_sp, g_ap = (v.cpu().numpy() for v in b.recipe_decode(dev(lf0), dev(mgc), dev(bap)))
    o_f0, o_sp, o_ap = oracle.recipe_decode(lf0, mgc, bap, fs, F)
    assert ((o_f0 > 0) == (f0 > 0)).all() and ((g_f0 > 0) == (o_f0 > 0)).all()
    np.testing.assert_allclose(g_f0, o_f0, rtol=1e-14, atol=0)
    np.testing.assert_allclose(g_sp, o_sp, rtol=1e-10, atol=0)
    np.testing.assert_allclose(g_ap[:, :24], o_ap[:, :24], rtol=1e-11, atol=0)
    assert (g_ap[:, 24:] == 0).all() and (o_ap[:, 24:] == 0).all()
    y = b.synthesize(dev(g_f0), dev(g_sp), dev(g_ap)).cpu().numpy()
    yo = oracle.synthesis(o_f0, o_sp, o_ap, F, fp, fs, n)
    idx, voiced, _ = sf.time_base(o_f0, fs, F, fp, n)
    assert voiced.any() and (~voiced).any() and np.abs(yo).max() > 0
    print("recipe dev=%.3e max|y|=%.3e" % (np.abs(y - yo).max(), np.abs(yo).max()))
    np.testing.assert_allclose(y, yo, atol=1e-8, rtol=0)
    b.close()

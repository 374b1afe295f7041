"""WorldBatch.mlsa_excitation / mlsa_filter / mlsa_synthesis (csrc/mlsa.hip) against tests/mlsa_reference.py, the float64
statement of the definition in include/world_mi355.h.  SPTK is not in the reference tree: parity with it is unpinned, and
the reference-free anchor (the impulse response at constant coefficients against the mel-log spectrum in closed form) is
run on the device too, with the host test's bounds.

Tolerances.  Excitation: 64 ulp of sum |lowpass| max |x| + sum |highpass| max |g| (the summation order is free); with the
taps [1] and [0] e is excite's output itself, so pulse positions and amplitudes are compared exactly.  Filter, per
utterance: max(10 sens, 64 ulp of max |y|), sens being the reference's own change when e and every b move by one ulp with
random signs.  Shapes are small on purpose: the reference is a Python loop."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import mlsa_reference as R

pytestmark = pytest.mark.gpu

TAPS = np.load(os.path.join(GOLDEN, "makefilter.npz"))
LP16, HP16 = TAPS["taps_16000_0"], TAPS["taps_16000_1"]
LP48, HP48 = TAPS["taps_48000_0"], TAPS["taps_48000_1"]
ONE, ZERO = np.array([1.0]), np.array([0.0])


def make_batch(gpu, Ts, P, ctx=None):
    torch, W, ctx0 = gpu
    return W.WorldBatch(ctx or ctx0, W.default_params(16000, 5.0), f0_lengths=list(Ts),
                        y_lengths=[R.samples(T, P) for T in Ts])


def dev(torch, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()


def split(a, Ts, P):
    at = np.concatenate([[0], np.cumsum([R.samples(T, P) for T in Ts])])
    return [a[at[k]:at[k + 1]] for k in range(len(Ts))]


def run_excitation(gpu, pitches, lp, hp, P, f32=False):
    torch = gpu[0]
    Ts = [len(p) for p in pitches]
    b = make_batch(gpu, Ts, P)
    try:
        e = b.mlsa_excitation(dev(torch, np.concatenate(pitches), np.float32), lp, hp, frame_shift=P, pipe_float32=f32)
        return split(e.cpu().numpy(), Ts, P)
    finally:
        b.close()


def run_filter(gpu, es, mcs, alpha, pd, P, f32=False, pade=None):
    torch = gpu[0]
    Ts = [len(m) for m in mcs]
    b = make_batch(gpu, Ts, P)
    try:
        y, st = b.mlsa_filter(dev(torch, np.concatenate(es), np.float64), dev(torch, np.concatenate(mcs), np.float32),
                              alpha=alpha, pade_order=pd, frame_shift=P, pipe_float32=f32, pade=pade)
        return split(y.cpu().numpy(), Ts, P), st.cpu().numpy()
    finally:
        b.close()


def run_synthesis(gpu, pitches, mcs, lp, hp, alpha, pd, P, f32=False, ctx=None):
    torch = gpu[0]
    Ts = [len(m) for m in mcs]
    b = make_batch(gpu, Ts, P, ctx)
    try:
        y, st = b.mlsa_synthesis(dev(torch, np.concatenate(pitches), np.float32),
                                 dev(torch, np.concatenate(mcs), np.float32), lp, hp, alpha=alpha, pade_order=pd,
                                 frame_shift=P, pipe_float32=f32)
        return split(y.cpu().numpy(), Ts, P), st.cpu().numpy()
    finally:
        b.close()


def pitch_of(kind, T, rng):
    if kind == "voiced":
        return (20.0 + 15.0 * rng.random(T)).astype(np.float32)
    if kind == "unvoiced":
        return np.zeros(T, dtype=np.float32)
    if kind == "alternate":                                  # one-frame runs on both sides
        p = (18.0 + 10.0 * rng.random(T)).astype(np.float32)
        p[1::2] = 0.0
        if T > 6:
            p[4:6] = 0.0
        return p
    if kind == "tiny":                                       # a period below one sample: a pulse at every sample
        return np.full(T, 0.5, dtype=np.float32)
    if kind == "huge":                                       # a period above the utterance's length
        return np.full(T, 5000.0, dtype=np.float32)
    raise KeyError(kind)


def mel_cepstra(T, order, rng, scale=0.3):
    """Smoothly varying float32 rows: c0 around -0.5, c[k] ~ scale / (k + 1)."""
    a = rng.normal(size=order + 1) * scale / (1.0 + np.arange(order + 1))
    z = rng.normal(size=order + 1) * scale / (1.0 + np.arange(order + 1))
    t = np.linspace(0.0, 1.0, T)[:, None]
    mc = a[None, :] * (1.0 - t) + z[None, :] * t
    mc[:, 0] -= 0.5
    return mc.astype(np.float32)


# (name, frame shift, [(kind, T)], lowpass, highpass)
EXCITATION_CASES = [
    ("voiced P5", 5, [("voiced", 9), ("voiced", 40), ("voiced", 2)], LP16, HP16),
    ("unvoiced P5", 5, [("unvoiced", 2), ("unvoiced", 3), ("unvoiced", 9)], LP16, HP16),
    ("alternate P5", 5, [("alternate", 9), ("alternate", 40), ("alternate", 3)], LP48, HP48),
    ("tiny and huge P5", 5, [("tiny", 9), ("huge", 9), ("tiny", 2)], LP16, HP16),
    ("P1", 1, [("voiced", 40), ("alternate", 9), ("unvoiced", 3), ("voiced", 2)], LP48, HP48),
    ("P80", 80, [("voiced", 3), ("alternate", 9), ("huge", 3), ("unvoiced", 2)], LP16, HP16),
    ("one tap", 5, [("voiced", 9), ("alternate", 40)], np.array([0.75]), np.array([-1.5])),
    ("256 taps", 80, [("voiced", 9), ("alternate", 3)], None, None),
]


@pytest.mark.parametrize("case", EXCITATION_CASES, ids=[c[0] for c in EXCITATION_CASES])
def test_excitation(gpu, case):
    name, P, parts, lp, hp = case
    rng = np.random.default_rng(11)
    if lp is None:
        lp, hp = rng.normal(size=256) / 16.0, rng.normal(size=256) / 16.0
    pitches = [pitch_of(kind, T, rng) for kind, T in parts]
    got = run_excitation(gpu, pitches, lp, hp, P)
    raw = run_excitation(gpu, pitches, ONE, ZERO, P)
    worst = 0.0
    for u, p in enumerate(pitches):
        x, pos, amp, used = R.excite(p, P)
        assert np.array_equal(raw[u], x), "%s utterance %d: excite's output (pulse positions, amplitudes, noise)" % (name, u)
        g = R.noise(len(x))
        want = R.fir(lp, x) + R.fir(hp, g)
        bound = 64.0 * np.spacing(np.abs(lp).sum() * max(np.abs(x).max(), 1e-300) + np.abs(hp).sum() * np.abs(g).max())
        err = float(np.abs(got[u] - want).max())
        worst = max(worst, err / bound)
        assert err <= bound, "%s utterance %d: |e - reference| = %.3e > %.3e" % (name, u, err, bound)
    print("excitation %s: worst error / bound %.3f" % (name, worst))


def test_excitation_of_the_walk_in_the_definition(gpu):
    pitch = np.array([20, 20, 25, 0, 0, 30, 30], dtype=np.float32)
    (x,) = run_excitation(gpu, [pitch], ONE, ZERO, 10)
    g = R.noise(30)
    assert len(x) == 60
    assert x[0] == np.sqrt(20.0) and x[50] == np.sqrt(30.0)
    assert np.array_equal(x[20:50], g)
    assert np.count_nonzero(x[:20]) == 1 and np.count_nonzero(x[50:]) == 1


def test_excitation_of_seventy_utterances(gpu):
    """Past one wave of per-utterance threads."""
    rng = np.random.default_rng(12)
    kinds = ("voiced", "alternate", "unvoiced")
    pitches = [pitch_of(kinds[u % 3], 2 + u % 4, rng) for u in range(70)]
    got = run_excitation(gpu, pitches, LP16, HP16, 5)
    for u, p in enumerate(pitches):
        x = R.excite(p, 5)[0]
        g = R.noise(len(x))
        want = R.fir(LP16, x) + R.fir(HP16, g)
        bound = 64.0 * np.spacing(np.abs(LP16).sum() * max(np.abs(x).max(), 1e-300) + np.abs(HP16).sum() * np.abs(g).max())
        assert np.abs(got[u] - want).max() <= bound, u


# (order, pade order, alpha, frame shift, frames per utterance, a caller's row or None)
FILTER_CASES = [
    (1, 1, 0.0, 1, (2, 3, 9), None),
    (2, 4, 0.42, 5, (2, 9, 40), None),
    (12, 5, -0.3, 80, (3, 40), None),
    (12, 6, 0.77, 5, (9, 40), None),
    (12, 7, 0.42, 80, (2, 40), None),
    (24, 4, 0.42, 5, (9, 40), None),
    (49, 5, 0.77, 5, (40, 3), None),
    (62, 7, -0.3, 1, (40, 9), None),
    (62, 4, 0.42, 80, (3,), (1.0, 0.5, 0.11, 0.012, 0.0006)),
]


def check_filter(label, got, es, mcs, alpha, pp, P, f32=False):
    """With f32 the reference rounds its output as the pipe does, and one float32 spacing of max |y| is added to the
    bound; sens is the double filter's either way."""
    worst = 0.0
    for u, mc in enumerate(mcs):
        B = R.mc2b(mc, alpha)
        want, sens = R.sensitivity(es[u], B, alpha, P, pp, 100 + u)
        bound = R.tolerance(want, sens)
        if f32:
            want = R.filter_b(es[u], B, alpha, P, pp, True)
            bound += float(np.spacing(np.float32(np.abs(want).max())))
        err = float(np.abs(got[u] - want).max())
        worst = max(worst, err / bound)
        assert err <= bound, "%s utterance %d: |y - reference| = %.3e > %.3e (sens %.3e)" % (label, u, err, bound, sens)
    print("filter %s: worst error / bound %.3f" % (label, worst))
    return worst


@pytest.mark.parametrize("case", FILTER_CASES, ids=["m%d pd%d a%g P%d" % c[:4] for c in FILTER_CASES])
def test_filter(gpu, case):
    order, pd, alpha, P, Ts, row = case
    rng = np.random.default_rng(21)
    mcs = [mel_cepstra(T, order, rng) for T in Ts]
    es = [rng.normal(size=R.samples(T, P)) for T in Ts]
    got, st = run_filter(gpu, es, mcs, alpha, pd, P, pade=row)
    assert (st == 0).all()
    check_filter("m%d pd%d a%g P%d" % case[:4], got, es, mcs, alpha, row or R.pade(pd), P)


@pytest.mark.parametrize("pd", sorted(R.ANCHOR_BOUNDS))
def test_anchor_on_the_device(gpu, pd):
    """The host test's anchor: the closed form is taken at the float32 coefficients the call is given."""
    P = 64
    mc, e = R.anchor_frames(P)
    mc32 = mc.astype(np.float32)
    (y,), st = run_filter(gpu, [e], [mc32], R.ANCHOR_ALPHA, pd, P)
    assert st[0] == 0
    err = R.anchor_error(y, mc32[0].astype(np.float64))
    print("anchor on the device, Pade order %d: %.3e (bound %.0e)" % (pd, err, R.ANCHOR_BOUNDS[pd]))
    assert err <= R.ANCHOR_BOUNDS[pd]


def synthesis_inputs(seed, parts, order):
    rng = np.random.default_rng(seed)
    pitches = [pitch_of(kind, T, rng) for kind, T in parts]
    mcs = [mel_cepstra(T, order, rng) for _, T in parts]
    return pitches, mcs


@pytest.mark.parametrize("f32", [False, True])
def test_synthesis_is_the_two_calls(gpu, f32):
    P, order, alpha, pd = 80, 24, 0.42, 5
    pitches, mcs = synthesis_inputs(31, [("voiced", 9), ("alternate", 40), ("unvoiced", 3), ("voiced", 2)], order)
    es = run_excitation(gpu, pitches, LP16, HP16, P, f32)
    y2, st2 = run_filter(gpu, es, mcs, alpha, pd, P, f32)
    y1, st1 = run_synthesis(gpu, pitches, mcs, LP16, HP16, alpha, pd, P, f32)
    assert (st1 == 0).all() and (st2 == 0).all()
    for u in range(len(mcs)):
        assert np.array_equal(y1[u], y2[u]), "utterance %d: other bits than the two calls" % u


def test_float32_pipes(gpu):
    P, order, alpha, pd = 5, 12, 0.42, 5
    pitches, mcs = synthesis_inputs(41, [("voiced", 40), ("alternate", 40), ("unvoiced", 9)], order)
    es = run_excitation(gpu, pitches, LP16, HP16, P, True)
    for u, p in enumerate(pitches):
        want = R.excitation(p, LP16, HP16, P, True)
        assert np.array_equal(es[u], es[u].astype(np.float32).astype(np.float64)), "e is not float32 values"
        gap = np.abs(es[u] - want)
        assert (gap <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)).all(), \
            "utterance %d: e beyond one float32 spacing of the reference's (%.3e)" % (u, gap.max())
    got, st = run_synthesis(gpu, pitches, mcs, LP16, HP16, alpha, pd, P, True)
    assert (st == 0).all()
    for u in range(len(mcs)):
        assert np.array_equal(got[u], got[u].astype(np.float32).astype(np.float64)), "y is not float32 values"
    # the reference filter on the library's own e: a flipped rounding in e does not pass for a filter error
    check_filter("float32 pipes", got, es, mcs, alpha, R.pade(pd), P, True)


def test_batch_independence(gpu):
    P, order, alpha, pd = 5, 12, 0.42, 4
    parts = [("voiced", 9), ("alternate", 40), ("unvoiced", 3), ("voiced", 40), ("alternate", 2)]
    pitches, mcs = synthesis_inputs(51, parts, order)
    inside, st = run_synthesis(gpu, pitches, mcs, LP48, HP48, alpha, pd, P)
    assert (st == 0).all()
    for u in (1, 3, 4):
        (alone,), _ = run_synthesis(gpu, [pitches[u]], [mcs[u]], LP48, HP48, alpha, pd, P)
        assert np.array_equal(alone, inside[u]), "utterance %d: its bits depend on the batch" % u


def test_status_codes(gpu):
    P, order, alpha, pd = 5, 12, 0.42, 5
    parts = [("voiced", 9), ("voiced", 9), ("alternate", 40), ("voiced", 3), ("unvoiced", 9)]
    pitches, mcs = synthesis_inputs(61, parts, order)
    clean, st = run_synthesis(gpu, pitches, mcs, LP16, HP16, alpha, pd, P)
    assert (st == 0).all()
    bad_p = [p.copy() for p in pitches]
    bad_m = [m.copy() for m in mcs]
    bad_m[1][4, 7] = np.nan                                  # a NaN coefficient
    bad_p[3][1] = -20.0                                      # a negative pitch
    bad_m[4][:, 0] = 800.0                                   # exp(b0) overflows
    got, st = run_synthesis(gpu, bad_p, bad_m, LP16, HP16, alpha, pd, P)
    assert list(st) == [0, 1, 0, 1, 2]
    assert (got[1] == 0).all() and (got[3] == 0).all()
    assert not np.isfinite(got[4]).all()
    assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2]), "a neighbour of a flagged utterance changed"
    # the two-call form: the filter flags the coefficient, the excitation of a bad pitch is zeros
    es = run_excitation(gpu, bad_p, LP16, HP16, P)
    assert (es[3] == 0).all()
    y2, st2 = run_filter(gpu, es, bad_m, alpha, pd, P)
    assert list(st2) == [0, 1, 0, 0, 2] and (y2[1] == 0).all() and (y2[3] == 0).all()
    assert np.array_equal(y2[0], clean[0]) and np.array_equal(y2[2], clean[2])


def test_argument_limits(gpu):
    torch, W, ctx = gpu
    P = 5
    Ts = [3, 9]
    rng = np.random.default_rng(71)
    pitch = dev(torch, np.concatenate([pitch_of("voiced", T, rng) for T in Ts]), np.float32)

    def mc_of(order, total=sum(Ts)):
        return dev(torch, np.zeros((total, order + 1)), np.float32)

    def refused(call, *a, **k):
        with pytest.raises(RuntimeError, match="bad argument"):
            call(*a, **k)

    b = make_batch(gpu, Ts, P)
    try:
        e = torch.zeros(b.total_out, dtype=torch.float64, device="cuda")
        y, st = b.mlsa_synthesis(pitch, mc_of(62), LP16, HP16, alpha=0.99, pade_order=7, frame_shift=P)   # the limits themselves
        assert (st.cpu().numpy() == 0).all()
        b.mlsa_synthesis(pitch, mc_of(1), np.ones(256), np.ones(1), pade_order=1, frame_shift=P)
        for order in (0, 63):
            refused(b.mlsa_synthesis, pitch, mc_of(order), LP16, HP16, frame_shift=P)
            refused(b.mlsa_filter, e, mc_of(order), frame_shift=P)
        for pd in (0, 8):
            refused(b.mlsa_synthesis, pitch, mc_of(12), LP16, HP16, pade_order=pd, frame_shift=P)
            refused(b.mlsa_filter, e, mc_of(12), pade_order=pd, frame_shift=P)
        for alpha in (1.0, -1.0, 1.5, float("nan")):
            refused(b.mlsa_synthesis, pitch, mc_of(12), LP16, HP16, alpha=alpha, frame_shift=P)
            refused(b.mlsa_filter, e, mc_of(12), alpha=alpha, frame_shift=P)
        for shift in (0, -1, P + 1):                         # the last: y_lengths that are not MlsaSamples of f0_lengths
            refused(b.mlsa_synthesis, pitch, mc_of(12), LP16, HP16, frame_shift=shift)
            refused(b.mlsa_excitation, pitch, LP16, HP16, frame_shift=shift)
            refused(b.mlsa_filter, e, mc_of(12), frame_shift=shift)
        for taps in (np.zeros(0), np.ones(257), np.array([np.inf])):
            refused(b.mlsa_synthesis, pitch, mc_of(12), taps, HP16, frame_shift=P)
            refused(b.mlsa_synthesis, pitch, mc_of(12), LP16, taps, frame_shift=P)
            refused(b.mlsa_excitation, pitch, taps, HP16, frame_shift=P)
            refused(b.mlsa_excitation, pitch, LP16, taps, frame_shift=P)
        refused(b.mlsa_filter, e, mc_of(12), pade_order=4, frame_shift=P, pade=(1.0, 0.5, float("nan"), 0.1, 0.0))
    finally:
        b.close()
    b = W.WorldBatch(ctx, W.default_params(16000, 5.0), f0_lengths=[3, 1], y_lengths=[2 * P, 0])   # T < 2
    try:
        refused(b.mlsa_synthesis, dev(torch, np.zeros(4), np.float32), mc_of(12, 4), LP16, HP16, frame_shift=P)
    finally:
        b.close()

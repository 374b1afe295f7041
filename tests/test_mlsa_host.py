"""The host-only helpers of the MLSA calls (WorldMi355MlsaSamples / MlsaPade / MlsaNoise) against tests/mlsa_reference.py,
and the conditions on the reference itself: SPTK is not in the reference tree, so what pins the reference's structure and
its two recalled Pade tables is the anchor -- at constant coefficients the impulse response of the filter must reproduce
the mel-log spectrum of the coefficients in closed form."""
from fractions import Fraction

import numpy as np
import pytest

import mlsa_reference as R


@pytest.fixture(scope="module")
def W(pkg):
    pkg.world.load_library()
    return pkg.world


def test_samples(W):
    for T, P in ((2, 1), (2, 80), (7, 10), (1000, 240)):
        assert W.mlsa_samples(T, P) == R.samples(T, P) == (T - 1) * P
    for T, P in ((1, 80), (0, 80), (-3, 80), (2, 0), (9, -1), (2 ** 20, 2 ** 12)):
        with pytest.raises(RuntimeError, match="bad argument"):
            W.mlsa_samples(T, P)


def test_noise_bit_for_bit(W):
    g = R.noise(4096)
    assert np.array_equal(W.mlsa_noise(4096), g)
    assert np.array_equal(W.mlsa_noise(4095), g[:4095])       # an odd count ends inside a pair
    assert W.mlsa_noise(0).shape == (0,)
    assert abs(g.mean()) < 0.05 and abs(g.std() - 1.0) < 0.05
    with pytest.raises(RuntimeError, match="bad argument"):
        W.mlsa_noise(-1)


def test_pade_rows(W):
    for order in range(1, 8):
        row = W.mlsa_pade(order)
        assert row.shape == (order + 1,) and row[0] == 1.0
        assert np.array_equal(row, np.array(R.pade(order)))
    assert tuple(W.mlsa_pade(4)) == R.PADE4 and tuple(W.mlsa_pade(5)) == R.PADE5
    # the plain rows are the double nearest to the exact rational
    assert R.pade_exact(1) == [1, Fraction(1, 2)]
    assert R.pade_exact(2) == [1, Fraction(1, 2), Fraction(1, 12)]
    assert R.pade_exact(3) == [1, Fraction(1, 2), Fraction(1, 10), Fraction(1, 120)]
    assert R.pade_exact(6)[6] == Fraction(1, 665280) and R.pade_exact(7)[7] == Fraction(1, 17297280)
    for order in (1, 2, 3, 6, 7):
        assert [float(q) for q in R.pade_exact(order)] == list(W.mlsa_pade(order))
    for order in (0, 8, -1):
        with pytest.raises(RuntimeError, match="bad argument"):
            W.mlsa_pade(order)


def test_default_option(W):
    import ctypes as C
    o = W.MlsaOption()
    W.load_library().WorldMi355DefaultMlsaOption(C.byref(o))
    assert (o.alpha, o.order, o.pade_order, o.pipe_float32, o.use_pade) == (0.35, 25, 4, 0, 0) and o.frame_shift >= 1


@pytest.mark.parametrize("pd", sorted(R.ANCHOR_BOUNDS))
def test_reference_anchor(pd):
    """Measured where the reference was written: 1.96e-4, 1.59e-4, 1.9e-10 and 7.3e-13 at orders 4, 5, 6 and 7."""
    P = 64
    mc, e = R.anchor_frames(P)
    y = R.mlsa_filter(e, mc, R.ANCHOR_ALPHA, P, R.pade(pd))
    want = sum(mc[0, k] * np.cos(k * np.linspace(0, np.pi, 5)) for k in range(R.ANCHOR_ORDER + 1))
    assert want.min() > -1.5 and want.max() < 1.6              # ln |H| spans about -1.27 .. 1.45
    err = R.anchor_error(y)
    print("anchor, Pade order %d: %.3e" % (pd, err))
    assert err <= R.ANCHOR_BOUNDS[pd]


def test_interpolation_ends_on_the_next_frame():
    """After P samples b is b_next exactly: with two constant halves the tail of the response is the second filter's."""
    rng = np.random.default_rng(3)
    a, z = rng.normal(size=5) * 0.2, rng.normal(size=5) * 0.2
    mc = np.array([a, z, z, z])
    e = np.zeros(30)
    e[10] = 1.0                                                # an impulse as frame 1 begins: the filter is z's by then
    y = R.mlsa_filter(e, mc, 0.3, 10, R.pade(5))
    ref = R.mlsa_filter(e, np.array([z, z, z, z]), 0.3, 10, R.pade(5))
    assert np.array_equal(y, ref)


def test_excitation_walk_of_the_definition():
    x, pos, amp, used = R.excite([20, 20, 25, 0, 0, 30, 30], 10)
    assert len(x) == 60 and pos == [0, 50] and used == 30
    assert amp == [np.sqrt(20.0), np.sqrt(30.0)]
    assert np.array_equal(x[20:50], R.noise(30))


def test_excitation_of_an_unvoiced_pitch_is_the_noise():
    x, pos, amp, used = R.excite(np.zeros(9), 5)
    assert pos == [] and used == 40 and np.array_equal(x, R.noise(40))


def test_pulse_amplitude_is_the_root_of_the_period():
    pitch = [12.0, 14.0, 17.0, 21.0, 21.0, 16.0]
    P = 25
    x, pos, amp, used = R.excite(pitch, P)
    assert used == 0 and len(pos) >= 5
    p1 = []                                                    # the interpolated period at every sample
    for f in range(1, len(pitch)):
        p, inc = pitch[f - 1], (pitch[f] - pitch[f - 1]) / P
        for _ in range(P):
            p1.append(p)
            p += inc
    for n, a in zip(pos, amp):
        assert a == np.sqrt(p1[n]) == x[n]
    assert np.count_nonzero(x) == len(pos)


def test_fir_and_float32_pipes():
    rng = np.random.default_rng(5)
    taps, x = rng.normal(size=7), rng.normal(size=40)
    assert np.allclose(R.fir(taps, x), np.convolve(taps, x)[:40], rtol=0, atol=1e-14)
    pitch = [20.0, 22.0, 0.0, 0.0, 25.0]
    e = R.excitation(pitch, taps, taps[::-1], 8, True)
    assert np.array_equal(e, e.astype(np.float32).astype(np.float64))
    assert np.abs(e - R.excitation(pitch, taps, taps[::-1], 8, False)).max() < 1e-5

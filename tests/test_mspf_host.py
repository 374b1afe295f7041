"""The modulation-spectrum postfilter (scripts/Training.pl:2950-3038 postfiltering_mspf, :3133-3221 make_mspf): what can
be checked without a GPU.  The definition in tests/mspf_reference.py reproduces the fixture tests/golden/sptk_mspf.npz
(written by tools/gen_golden_mspf.py from that definition in long double), returns its input with equal tables and
rests on a window that sums to one at the hop; the ABI is declared, exported, has its defaults and refuses every bad
argument set without a device; mspf_finalize and the label arithmetic of the recipe agree with numpy."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_mspf as gen  # noqa: E402
import mspf_reference as R  # noqa: E402

PATH = os.path.join(GOLDEN, "sptk_mspf.npz")
SETTINGS = [(25, 64), (3, 16), (15, 16), (31, 32)]


@pytest.fixture(scope="module")
def fx():
    return np.load(PATH)


def test_fixture_is_complete_and_was_admitted(fx):
    assert os.path.getsize(PATH) < 1 << 20
    assert sorted(fx["keys"]) == sorted(gen.OPTIONS)
    seen = set()
    for key, (Lw, N, dim, e) in gen.OPTIONS.items():
        K = N // 2 + 1
        assert list(fx[key + "/opt"]) == [Lw, N, dim, e]
        assert list(fx[key + "/lengths"]) == gen.lengths(Lw)
        total = sum(gen.lengths(Lw))
        assert fx[key + "/x"].shape == (total, dim) and fx[key + "/x"].dtype == np.float32
        assert fx[key + "/out"].shape == (total, dim) and fx[key + "/sens"].shape == (dim,)
        for name in ("mean_gen", "std_gen", "mean_nat", "std_nat"):
            assert fx[key + "/" + name].shape == (dim, K) and np.isfinite(fx[key + "/" + name]).all()
        assert (fx[key + "/std_gen"] > 0).all() and (fx[key + "/std_nat"] > 0).all()
        assert np.isfinite(fx[key + "/out"]).all()
        x = fx[key + "/x"].astype(np.float64)
        assert (x == np.concatenate(gen.inputs(key))).all()
        # the admission rule of the generator; no column is constant
        assert (10.0 * fx[key + "/sens"] <= 1e-9 * np.abs(x).max(axis=0)).all(), key
        longest = x[-gen.lengths(Lw)[-1]:]
        assert (longest.std(axis=0) > 0.1).all()
        seen |= {("set", Lw, N), ("dim", dim), ("e", e)}
    assert {("set", a, b) for a, b in SETTINGS} | {("dim", d) for d in (1, 50, 64, 65)} | {("e", 1.0), ("e", 0.5)} <= seen


@pytest.mark.parametrize("key", sorted(gen.OPTIONS))
def test_reference_reproduces_the_golden_file(fx, key):
    """The double chain against the stored long-double result, inside the tolerance of the GPU test."""
    Lw, N, dim, e = gen.OPTIONS[key]
    x = fx[key + "/x"].astype(np.float64)
    tabs = [fx[key + "/" + n] for n in ("mean_gen", "std_gen", "mean_nat", "std_nat")]
    off = np.concatenate([[0], np.cumsum(fx[key + "/lengths"])])
    got = gen.run([x[off[i]:off[i + 1]] for i in range(len(off) - 1)], tabs, Lw, N, e, np.float64)
    err = np.abs(got - fx[key + "/out"]).max(axis=0)
    tol = np.maximum(10.0 * fx[key + "/sens"], 64.0 * np.spacing(np.abs(x).max(axis=0)))
    assert (err <= tol).all() and (err <= fx[key + "/sens"]).all(), (key, (err / tol).max())
    assert np.abs(got - x).max() > 0.1                                            # the tables differ: the values move


@pytest.mark.parametrize("Lw,N", SETTINGS)
def test_identity_with_equal_tables(Lw, N):
    """64 ulp of max|x| plus 1e-15 K: the 1e-30 under the logarithm of step 4 puts up to 1e-15 on an amplitude."""
    S, K = R.hops(Lw), N // 2 + 1
    rng = np.random.default_rng(Lw * N)
    mg, sg = rng.standard_normal(K) - 2.0, 0.5 + rng.random(K)
    for T in (1, 2, S - 1, S, S + 1, 2 * S, 2 * S + 1, 5 * S + 7, 300):
        if T < 1:
            continue
        x = gen.smooth(gen.ar1(rng, T + 4, 1))[:, 0]
        out = R.postfilter_column(x, mg, sg, mg, sg, Lw, N, 1.0)
        assert np.abs(out - x).max() <= 64.0 * np.spacing(np.abs(x).max()) + 1e-15 * K, (Lw, N, T)


@pytest.mark.parametrize("Lw", [3, 15, 25, 31])
def test_bartlett_window_sums_to_one_at_the_hop(Lw):
    S = R.hops(Lw)
    w = R.bartlett(Lw)
    assert w[0] == 0 and w[S] == 1 and w[-1] == 0 and np.abs(w - w[::-1]).max() <= np.finfo(float).eps
    assert w[1] == 2.0 / (Lw - 1)                                                 # a triangle, not a raised cosine
    tot = np.zeros(6 * S + Lw)
    for j in range(7):
        tot[j * S:j * S + Lw] += w
    assert np.abs(tot[S:6 * S] - 1.0).max() <= 4 * np.finfo(float).eps


def test_frame_count_and_padding():
    for Lw in (3, 15, 25):
        S = R.hops(Lw)
        for T in (1, 2, S, S + 1, 2 * S, 5 * S + 7):
            J = R.n_frames(T, Lw)
            assert J == -(-(T + S) // S) and (J - 1) * S >= T                     # the last frame is centred past the end
            f = R.frames(np.ones(T), Lw)
            assert f.shape == (J, Lw) and f[0, :S].sum() == 0                     # frame 0 is centred on sample 0
    assert R.n_frames(0, 25) == 0


def test_abi_declared_exported_with_defaults(pkg):
    text = open(os.path.join(ROOT, "include", "world_mi355.h")).read()
    for name in ("WorldMi355ModulationSpectrumPostfilter", "WorldMi355ModulationSpectrumStats", "WorldMi355ColumnMeans",
                 "WorldMi355MspfSegmentFrames"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert re.search(r"\bvoid\s+WorldMi355DefaultMspfOption\s*\(", text)
    assert "Training.pl:2950-3000" in text and '"mspf_kernel"' in text and "(:2950) are not offered" not in text
    assert "WorldMi355*" in open(os.path.join(ROOT, "hts-train-world_amd", "csrc", "exports.map")).read()
    lib = pkg.load_library()
    for name in ("WorldMi355ModulationSpectrumPostfilter", "WorldMi355ModulationSpectrumStats", "WorldMi355ColumnMeans",
                 "WorldMi355DefaultMspfOption", "WorldMi355MspfSegmentFrames"):
        assert hasattr(lib, name), name
    o = pkg.world.MspfOption()
    lib.WorldMi355DefaultMspfOption(ctypes.byref(o))
    assert (o.frame_length, o.fft_length, o.emphasis) == (25, 64, 1.0)
    assert ctypes.sizeof(pkg.world.MspfOption) == 16 and pkg.world.MspfOption.emphasis.offset == 8
    lib.WorldMi355DefaultMspfOption(None)                                         # a null option struct is left alone
    assert pkg.world.mspf_segment_frames() >= 64


def test_every_refusal_without_a_device(pkg):
    """No context, no batch, no device memory: the answer is WM_ERR_BAD_ARG (2) from the host checks alone.  The
    pointers that stand for device memory are never followed."""
    lib = pkg.load_library()
    M = pkg.world.MspfOption
    dim, N = 2, 16
    K = N // 2 + 1
    fake = ctypes.c_void_p(4096)                                                  # stands for a device address
    other = ctypes.c_void_p(8192)
    good = [np.zeros((dim, K)), np.ones((dim, K)), np.zeros((dim, K)), np.ones((dim, K))]
    n = ctypes.c_int64(-1)

    def h(a):
        return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def post(x=fake, d=dim, opt=(7, N, 1.0), t=good, out=other):
        o = None if opt is None else ctypes.byref(M(*opt))
        return lib.WorldMi355ModulationSpectrumPostfilter(None, x, d, o, h(t[0]), h(t[1]), h(t[2]), h(t[3]), out, None)

    def stats(x=fake, d=dim, opt=(7, N, 1.0), s1=other, s2=other, cnt=n):
        o = None if opt is None else ctypes.byref(M(*opt))
        return lib.WorldMi355ModulationSpectrumStats(None, x, d, o, None, s1, s2,
                                                     None if cnt is None else ctypes.byref(cnt))

    def poisoned(i, v):
        t = [a.copy() for a in good]
        t[i][1, 3] = v
        return t

    for opt in (None, (7, 8, 1.0), (7, 128, 1.0), (7, 48, 1.0), (7, 0, 1.0), (8, N, 1.0), (1, N, 1.0), (N + 1, N, 1.0),
                (-3, N, 1.0), (7, N, float("nan")), (7, N, float("inf")), (7, N, float("-inf"))):
        assert post(opt=opt) == 2 and stats(opt=opt) == 2, opt
    assert post(x=None) == 2 and post(out=None) == 2 and post(d=0) == 2 and post(d=-1) == 2 and post(out=fake) == 2
    for i in range(4):
        assert post(t=[a if k != i else None for k, a in enumerate(good)]) == 2, i
        for v in (float("nan"), float("inf"), float("-inf")):
            assert post(t=poisoned(i, v)) == 2, (i, v)
    assert post(t=poisoned(1, 0.0)) == 2 and post(t=poisoned(1, -0.5)) == 2
    assert stats(x=None) == 2 and stats(s1=None) == 2 and stats(s2=None) == 2 and stats(cnt=None) == 2 and stats(d=0) == 2
    assert lib.WorldMi355ColumnMeans(None, None, dim, other) == 2
    assert lib.WorldMi355ColumnMeans(None, fake, dim, None) == 2
    assert lib.WorldMi355ColumnMeans(None, fake, 0, other) == 2
    # sound arguments get as far as the missing batch
    assert post() == 2 and stats() == 2 and lib.WorldMi355ColumnMeans(None, fake, dim, other) == 2
    assert n.value == -1


def test_finalize_against_numpy(pkg):
    rng = np.random.default_rng(1)
    m = rng.standard_normal((37, 3, 9)) * 2.0 - 5.0                               # [frame][dim][K]
    mean, std = pkg.world.mspf_finalize(m.sum(axis=0), (m * m).sum(axis=0), len(m))
    assert np.abs(mean - m.mean(axis=0)).max() < 1e-13 and np.abs(std - m.std(axis=0)).max() < 1e-12
    rmean, rstd = R.finalize(m.sum(axis=0), (m * m).sum(axis=0), len(m))
    assert (mean == rmean).all() and (std == rstd).all()
    # a constant bin: rounding may take the variance below zero, the deviation is 0 and not NaN
    c = np.full((5, 1, 2), 0.1)
    _, std = pkg.world.mspf_finalize(c.sum(axis=0), (c * c).sum(axis=0), 5)
    assert np.isfinite(std).all() and (std < 1e-8).all()
    import torch
    tm, ts = pkg.world.mspf_finalize(torch.from_numpy(m.sum(axis=0)), torch.from_numpy((m * m).sum(axis=0)), len(m))
    assert np.abs(tm.numpy() - mean).max() < 1e-15 and np.abs(ts.numpy() - rstd).max() < 1e-12


def test_label_segments_have_inclusive_ends(pkg):
    rows = pkg.recipe.mspf_label_rows
    lab = ["0 500001 sil", "500001 1500001 a", "1500001 2000001 b", "2000001 9000000 sil"]
    # 5 ms frames: 50 ms is frame 10, 150 ms frame 30, 200 ms frame 40 (a hair past each: 500000 * 1e-7 / 0.005 is
    # 9.999999999999998 in double, frame 9 in the script's arithmetic as well)
    assert list(rows(["500000 500000 x"], 0.005, 100)) == [9]
    keep = rows(lab, 0.005, 100, silences=("sil",))
    assert list(keep) == list(range(10, 31)) + list(range(30, 41))                # frame 30 twice: both ends inclusive
    assert list(rows(lab, 0.005, 100)) == (list(range(0, 11)) + list(range(10, 31)) + list(range(30, 41))
                                           + list(range(40, 100)))                # clipped to the file
    assert list(rows(lab, 0.005, 35, silences=("sil", "a"))) == list(range(30, 35))
    assert len(rows(["0 100 sil"], 0.005, 10, silences=("sil",))) == 0
    assert (rows(lab, 0.005, 100, ("sil",)) == R.label_segments(lab, 0.005, 100, ("sil",))).all()
    # the script's integer arithmetic, int(t * 1e-7 / shift): 14.99990 ms is frame 2, 25.0001 ms frame 5
    assert list(rows(["149999 250001 x"], 0.005, 100)) == [2, 3, 4, 5]

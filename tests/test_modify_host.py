"""Voice modification without a device: tests/modify_reference.py -- the yardstick of the GPU tests -- held to the golden
file and to the compiled reference's interp1; the factor refusals of modify.modify_features on a batch made by hand whose
device is the CPU; the `modify` and `generate` command lines with the drivers replaced; the header and the export."""
import os
import re

import numpy as np
import pytest

import generate_setup as G
import modify_reference as mr
from conftest import GOLDEN, ROOT

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "modify_handmade.npz"))


def agree(mine, theirs, what):
    """Every non-finite value and every zero at the same place, the rest within 2 ulp; returns the worst distance."""
    assert mine.shape == theirs.shape, what
    assert mr.same_class(mine, theirs).all(), what
    ok = np.isfinite(theirs) & (theirs != 0)
    worst = int(mr.ulps(mine[ok], theirs[ok]).max()) if ok.any() else 0
    assert worst <= 2, (what, worst)
    return worst


def test_reference_against_the_golden_file(golden):
    """The interpolation step of the file ran in the compiled reference.  Equal bits are what is seen (worst distance 0):
    both sides round the same expressions in the same order."""
    assert os.path.getsize(os.path.join(GOLDEN, "modify_handmade.npz")) <= os.path.getsize(
        os.path.join(GOLDEN, "codec_handmade.npz"))
    worst = 0
    for fs, F in mr.GOLDEN_SHAPES:
        for family, ratio in mr.GOLDEN_CASES:
            rows = golden["in_%s_%d" % (family, F)]
            assert rows.shape == (mr.ROWS, F // 2 + 1)
            assert rows.tobytes() == mr.rows(family, F).tobytes(), "the generator moved away from the stored inputs"
            theirs = golden[mr.golden_key(family, ratio, F)]
            worst = max(worst, agree(mr.modify_sp(rows, ratio, fs, F), theirs, (family, ratio, F)))
    print("worst distance to the golden file: %d ulp" % worst)
    assert worst == 0


def test_the_tie_patterns_of_the_golden_file(golden):
    """Where the reference puts NaN for zero bins at 7 and 10: at ratio 0.5 bins 3 and 5 and nowhere else before the fill
    (which starts at F/4 and repeats the finite bin before it), at ratio 1.0 a zero at bin i gives NaN at i - 1 and i."""
    for fs, F in mr.GOLDEN_SHAPES:
        half = golden[mr.golden_key("zeros", 0.5, F)][0]
        assert np.flatnonzero(np.isnan(half)).tolist() == [3, 5]
        assert (half[F // 4:] == half[F // 4 - 1]).all()
        one = golden[mr.golden_key("zeros", 1.0, F)][0]
        assert np.flatnonzero(np.isnan(one)).tolist() == [6, 7, 9, 10]
        ends = golden[mr.golden_key("zeros", 1.0, F)][1]
        # the last bin is no tie: its count is clamped to n - 1, s is 1, and finite + 1 * (-inf) is -inf, a zero
        assert np.flatnonzero(np.isnan(ends)).tolist() == [0, F // 2 - 1] and ends[F // 2] == 0.0


@pytest.mark.parametrize("fs, F", mr.SHAPES)
def test_reference_against_the_compiled_interp1(reference, fs, F):
    """Every family at every ratio of the test list, the interpolation step in matlabfunctions.cpp's interp1."""
    worst = 0
    for family in mr.FAMILIES:
        rows = mr.rows(family, F)
        for ratio in mr.ratios(F):
            theirs = mr.modify_sp(rows, ratio, fs, F, interp=reference.interp1)
            worst = max(worst, agree(mr.modify_sp(rows, ratio, fs, F), theirs, (family, ratio, F)))
    assert worst == 0


@pytest.mark.parametrize("fs, F", mr.SHAPES)
def test_axes_and_the_count(fs, F):
    """What the kernel relies on: the knots increase strictly for every ratio of the list, and floor(i / ratio) + 1
    (capped at the number of knots) is the count of knots <= the query."""
    i = np.arange(F // 2 + 1, dtype=np.float64)
    for ratio in mr.ratios(F):
        x1, x2 = mr.axes(ratio, fs, F)
        assert (np.diff(x1) > 0).all()
        count = np.searchsorted(x1, x2, side="right")
        assert (np.minimum(np.floor(i / ratio) + 1, F // 2 + 1) == count).all(), ratio
        assert 1 <= mr.fill_start(ratio, F) <= F // 2 + 1


def test_bound_is_the_derived_one():
    row = np.exp(np.linspace(-20.0, 3.0, 257))
    assert mr.bound(row) == 8.0 * 21.0 * 2.0 ** -52
    row[[3, 9]] = 0.0, np.inf
    assert mr.bound(row) == 8.0 * 21.0 * 2.0 ** -52


# ---- modify_features ahead of the library ----------------------------------------------------------------------------
NU, TS, TF, TO, FFT, BINS = 2, 2000, 27, 2000, 1024, 513


@pytest.fixture(scope="module")
def batch(pkg):
    W = pkg.world
    W.load_library()
    b = W.WorldBatch.__new__(W.WorldBatch)
    b.handle, b.ctx, b.params = None, None, W.default_params(16000, 5.0)
    b.n_utt, b.total_samples, b.total_frames, b.total_out, b.fft_size, b.bins = NU, TS, TF, TO, FFT, BINS
    b.sample_offsets, b.frame_offsets = np.array([0, 800, TS]), np.array([0, 11, TF])
    b.out_offsets = np.array([0, 800, TO])
    b.device = torch.device("cpu")
    return b


@pytest.fixture()
def library_not_reached(pkg, monkeypatch):
    def reached():
        raise AssertionError("the library was called for a refused argument")
    monkeypatch.setattr(pkg.world, "load_library", reached)


def test_factor_refusals(pkg, batch, library_not_reached):
    mod = pkg.modify.modify_features
    f0, sp = torch.zeros(TF, dtype=torch.float64), torch.ones(TF, BINS, dtype=torch.float64)
    with pytest.raises(ValueError, match="give f0_scale, formant_ratio or both"):
        mod(batch, f0, sp)
    for bad in mr.refused_ratios(FFT) + [float("inf"), [1.0, 0.0], [1.0, 2.0, 3.0], [[1.0, 1.0]]]:
        with pytest.raises(ValueError, match="formant_ratio"):
            mod(batch, f0, sp, formant_ratio=bad)
    for bad in (0.0, -2.0, float("inf"), float("nan"), [1.0, float("inf")], [1.0]):
        with pytest.raises(ValueError, match="f0_scale"):
            mod(batch, f0, sp, f0_scale=bad)
    with pytest.raises(ValueError, match="f0_scale"):                                  # the good ratio does not hide it
        mod(batch, f0, sp, f0_scale=0.0, formant_ratio=1.2)
    with pytest.raises(ValueError, match=r"modify_features: f0 must be"):              # a part that is asked for
        mod(batch, None, sp, f0_scale=1.2)
    with pytest.raises(ValueError, match=r"modify_features: sp must be"):
        mod(batch, f0, None, formant_ratio=1.2)
    with pytest.raises(ValueError, match=r"modify_features: sp must be"):
        mod(batch, f0, sp.float(), formant_ratio=1.2)
    with pytest.raises(ValueError, match=r"modify_features: sp must be"):
        mod(batch, f0, sp[:, :-1], formant_ratio=1.2)
    with pytest.raises(ValueError, match=r"modify_features: out\[1\] must be"):
        mod(batch, f0, sp, formant_ratio=1.2, out=(None, sp.t()))
    with pytest.raises(ValueError, match=r"out must be \(f0_out, sp_out\)"):
        mod(batch, f0, sp, formant_ratio=1.2, out=sp)


def test_accepted_factors_reach_the_library(pkg, batch):
    """The smallest and largest legal ratios and a factor per utterance get as far as the library, which refuses the
    NULL batch (RuntimeError); the part that is not asked for is not looked at."""
    mod = pkg.modify.modify_features
    f0, sp = torch.zeros(TF, dtype=torch.float64), torch.ones(TF, BINS, dtype=torch.float64)
    for kw in (dict(formant_ratio=2.0 / FFT), dict(formant_ratio=float(FFT)), dict(formant_ratio=[0.5, 2.0]),
               dict(f0_scale=[0.5, 2.0]), dict(f0_scale=1.0, formant_ratio=1.0)):
        with pytest.raises(RuntimeError):
            mod(batch, f0, sp, **kw)
    with pytest.raises(RuntimeError):
        mod(batch, f0, "not looked at", f0_scale=2.0)
    with pytest.raises(RuntimeError):
        mod(batch, None, sp, formant_ratio=2.0, out=(None, sp))
    a = pkg.modify.factor_array("w", "n", 1.5, 3)
    assert a.dtype == np.float64 and a.tolist() == [1.5, 1.5, 1.5] and pkg.modify.factor_array("w", "n", None, 3) is None


def test_uses_no_assert_and_forwards_to_the_batch_method(pkg):
    text = open(os.path.join(ROOT, "hts-train-world_amd", "modify.py")).read()
    assert not re.search(r"^\s*assert\b", text, re.M)
    assert "modify_features" in vars(pkg.world.WorldBatch) and not hasattr(pkg.world.WorldBatch, "convert")
    assert pkg.modify.factor_array is pkg.world.factor_array
    assert not re.search(r"\._(f64|out)\b", text)                      # the batch's private checks stay in world.py


def test_header_and_export(pkg):
    text = open(os.path.join(ROOT, "include", "world_mi355.h")).read()
    assert re.search(r"\bint\s+WorldMi355ModifyFeatures\s*\(", text)
    assert "test/test.cpp:201-238" in text and '"modify_kernel"' in text
    lib = pkg.load_library()
    assert hasattr(lib, "WorldMi355ModifyFeatures")
    one = (np.ones(1) * 1.2).ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_double))
    assert lib.WorldMi355ModifyFeatures(None, one, one, None, None, None, None) == 2      # WM_ERR_BAD_ARG: a NULL batch


# ---- the command lines -------------------------------------------------------------------------------------------------
@pytest.fixture()
def no_context(pkg, monkeypatch):
    def opened(*a, **k):
        raise AssertionError("a context was opened ahead of the argument checks")
    monkeypatch.setattr(pkg.recipe, "_own_context", opened)
    monkeypatch.setattr(pkg.world, "Context", opened)
    monkeypatch.setattr(pkg.world, "WorldBatch", opened)
    monkeypatch.setattr(pkg.world, "LabelFeatureSet", opened)


def test_modify_command_line(pkg, tmp_path, no_context, capsys, monkeypatch):
    rec = pkg.recipe
    scp = tmp_path / "jobs.scp"
    scp.write_text("a.wav oa.wav\n# a comment\nb.wav ob.wav 1.5\n\nc.wav oc.wav 0.8 1.25\n")
    calls = []
    monkeypatch.setattr(rec, "modify_files", lambda jobs, *a, **kw: calls.append((jobs, a, kw)) or 11)
    assert rec.main(["modify", "--scp", str(scp)]) == 0
    assert "complete. 11 frames" in capsys.readouterr().out
    jobs, a, kw = calls.pop()
    assert jobs == [("a.wav", "oa.wav", None, None), ("b.wav", "ob.wav", 1.5, None), ("c.wav", "oc.wav", 0.8, 1.25)]
    assert a == (5.0, "dio", 71.0, 800.0, 0.85) and kw == dict(max_batch_frames=rec.MAX_BATCH_FRAMES, resume=False)
    assert rec.main(["modify", "--scp", str(scp), "--f0-scale", "2", "--formant-ratio", "0.9", "--frame-period", "2.5",
                     "--f0", "harvest", "--f0-floor", "60", "--f0-ceil", "500", "--d4c-threshold", "0.5", "--resume",
                     "--max-batch-frames", "5000"]) == 0
    jobs, a, kw = calls.pop()
    assert jobs == [("a.wav", "oa.wav", 2.0, 0.9), ("b.wav", "ob.wav", 1.5, 0.9), ("c.wav", "oc.wav", 0.8, 1.25)]
    assert a == (2.5, "harvest", 60.0, 500.0, 0.5) and kw == dict(max_batch_frames=5000, resume=True)
    for text in ("a.wav\n", "a.wav b.wav 1 2 3\n", "a.wav b.wav x\n"):
        scp.write_text(text)
        with pytest.raises(SystemExit):
            rec.main(["modify", "--scp", str(scp)])
    with pytest.raises(SystemExit):
        rec.main(["modify"])
    with pytest.raises(SystemExit):
        rec.main(["modify", "--scp", str(scp), "--f0", "swipe"])
    assert not calls


def test_modify_files_checks_factors_ahead_of_a_context(pkg, tmp_path, no_context):
    rec = pkg.recipe
    wav = str(tmp_path / "a.wav")
    rec.write_wav(wav, np.zeros(1600), 16000)
    out = str(tmp_path / "o.wav")
    with pytest.raises(ValueError, match="f0_scale"):
        rec.modify_files([(wav, out, 0.0, None)])
    with pytest.raises(ValueError, match="formant_ratio"):
        rec.modify_files([(wav, out, 1.0, 1025.0)])                                    # 16 kHz: fft_size 1024
    with pytest.raises(ValueError, match="formant_ratio"):
        rec.modify_files([(wav, out, None, float("nan"))])
    with pytest.raises(ValueError, match="a job is"):
        rec.modify_files([(wav, out)])
    with pytest.raises(ValueError, match="f0_estimator"):
        rec.modify_files([(wav, out, 1.0, 1.0)], f0_estimator="swipe")
    assert rec.modify_files([]) == 0
    n = rec.modify_samples(1600, 16000, 5.0)
    assert n == int((int(1000.0 * 1600 / 16000 / 5.0) + 1 - 1) * 5.0 / 1000.0 * 16000) + 1 == 1601
    rec.write_wav(out, np.zeros(n), 16000)
    assert rec.modify_files([(wav, out, 1.2, 0.9)], resume=True) == 0                  # complete: nothing to do
    p = rec.modify_params(16000)
    assert p.d4c_threshold == 0.85 and p.f0_floor == 71.0 and p.frame_period == 5.0


def generate_argv(world, scp, wins, extra=()):
    w = lambda n: ",".join(str(wins / ("%s.win%d" % (n, k))) for k in (1, 2, 3))
    return ["generate", "--scp", str(scp), "--config", world.config, "--frame-shift", "50000", "--model",
            world.models["sd"][0], "--stream", "mgc:50:0:" + w("mgc"), "--stream", "lf0:1:1:" + w("lf0"), "--stream",
            "bap:25:0:" + w("bap"), "--fs", "48000", "--fft-size", "2048", "--alpha", "0.55"] + list(extra)


def test_generate_command_line_and_checks(pkg, tmp_path_factory, tmp_path, no_context, monkeypatch):
    world = G.World(pkg, tmp_path_factory.mktemp("modify_generate_host"))
    rec = pkg.recipe
    wins = tmp_path / "win"
    wins.mkdir()
    for n in ("mgc", "lf0", "bap"):
        for k, w in enumerate(G.WINDOWS, 1):
            (wins / ("%s.win%d" % (n, k))).write_text("%d %s\n" % (len(w), " ".join(repr(v) for v in w)))
    jobs = [(p, str(tmp_path / (os.path.basename(p)[:-4] + ".wav"))) for p in world.labels]
    scp = tmp_path / "jobs.scp"
    scp.write_text("".join("%s %s\n" % j for j in jobs))
    calls = []
    with monkeypatch.context() as m:
        m.setattr(pkg.generate, "generate_files", lambda jobs, **kw: calls.append(kw) or (7, []))
        assert rec.main(generate_argv(world, scp, wins)) == 0
        kw = calls.pop()
        assert kw["f0_scale"] is None and kw["formant_ratio"] is None                   # the default: not done
        assert rec.main(generate_argv(world, scp, wins, ["--f0-scale", "1.2", "--formant-ratio", "1.1"])) == 0
        kw = calls.pop()
        assert (kw["f0_scale"], kw["formant_ratio"]) == (1.2, 1.1)
        assert rec.main(generate_argv(world, scp, wins, ["--formant-ratio", "0.9"])) == 0
        kw = calls.pop()
        assert (kw["f0_scale"], kw["formant_ratio"]) == (None, 0.9)
    gen = pkg.generate.generate_files                                                   # the real one: checks first
    args = world.arguments()
    for bad in (dict(f0_scale=0.0), dict(f0_scale=float("inf")), dict(f0_scale=[1.0, 2.0])):
        with pytest.raises(ValueError, match="f0_scale"):
            gen(jobs, **dict(args, **bad))
    F = args["fft_size"]
    for r in mr.refused_ratios(F):
        with pytest.raises(ValueError, match="formant_ratio"):
            gen(jobs, **dict(args, formant_ratio=r))
    s = pkg.generate._Setup(**dict({k: v for k, v in args.items() if k not in ("keep_dir", "max_batch_frames", "resume",
                                                                                "io_threads", "ctx")},
                                   f0_scale=2, formant_ratio=2.0 / F))
    assert (s.f0_scale, s.formant_ratio) == (2.0, 2.0 / F)

"""generate.Generator / generate_files against the five staged drivers they compose, byte for byte, on the small world
of tests/generate_setup.py (16 kHz, fft 512, four streams, utterances of 1, 33, 97 and 161 frames).

The staged run of every (postfilter, model) pair is made once and shared; in it no stage flags an utterance (asserted on
what the drivers print), the lf0 files hold voiced and unvoiced frames, and two utterances are unvoiced whole."""
import contextlib
import io
import os

import numpy as np
import pytest

import generate_setup as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(pkg, tmp_path_factory):
    return G.World(pkg, tmp_path_factory.mktemp("generate"))


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def staged(gpu, pkg, world, tmp_path_factory):
    """staged(which, kind) -> {(utterance, extension): the bytes of the staged run's file}, `wav` among the extensions."""
    done = {}

    def run(which="mcp", kind="sd"):
        if (which, kind) not in done:
            err = io.StringIO()
            with contextlib.redirect_stderr(err):
                base = world.staged(pkg.recipe, tmp_path_factory.mktemp("staged_%s_%s" % (which, kind)), which, kind, ctx=gpu[2])
            assert "warning: " not in err.getvalue(), err.getvalue()                   # no stage flagged an utterance
            files = {(k, ext): read(b + "." + ext) for k, b in enumerate(base) for ext in G.World.extensions(which) + ["wav"]}
            lf0 = [np.frombuffer(files[k, "lf0"], dtype=np.float32) for k in range(len(base))]
            voiced = [v > -1.0e9 for v in lf0]
            assert [int(v.sum()) for v in voiced][:2] == [0, 0] and all(0 < v.sum() < len(v) for v in voiced[2:])
            for v, m in zip(lf0, voiced):
                assert (v[~m] == np.float32(-1.0e10)).all() and (v[m] > np.log(80.0)).all() and (v[m] < np.log(400.0)).all()
            for k, T in enumerate(G.LENGTHS):
                assert len(files[k, "wav"]) == 44 + 2 * (int((T - 1) * G.FRAME_PERIOD / 1000.0 * G.FS) + 1)
                assert len(files[k, "ffo"]) == 4 * G.WIDTH * T and len(files[k, "var"]) == 4 * G.WIDTH
            assert any(np.frombuffer(files[k, "wav"][44:], dtype="<i2").any() for k in range(len(base)))
            done[which, kind] = files
        return done[which, kind]
    return run


def jobs_of(world, out_dir, labels=None):
    os.makedirs(str(out_dir), exist_ok=True)
    return [(p, os.path.join(str(out_dir), os.path.basename(p)[:-4] + ".wav")) for p in (labels or world.labels)]


@pytest.mark.parametrize("kind", ["sd", "sat"])
@pytest.mark.parametrize("which", G.POSTFILTERS)
def test_chain_equals_staged_byte_for_byte(gpu, pkg, world, staged, tmp_path, which, kind):
    want = staged(which, kind)
    jobs, keep = jobs_of(world, tmp_path / "wav"), tmp_path / "keep"
    n, flagged = pkg.generate.generate_files(jobs, **world.arguments(which, kind), ctx=gpu[2], keep_dir=str(keep))
    assert n == sum(G.LENGTHS) and flagged == []
    exts = G.World.extensions(which)
    assert sorted(os.listdir(str(keep))) == sorted("a%d.%s" % (k, e) for k in range(len(jobs)) for e in exts)
    for k, (_, wav) in enumerate(jobs):
        for ext in exts:
            assert read(str(keep / ("a%d.%s" % (k, ext)))) == want[k, ext], (k, ext)
        assert read(wav) == want[k, "wav"], k
    if which != "none":                                                                # the postfilter did something
        assert any(want[k, "p_mgc"] != want[k, "mgc"] for k in range(len(jobs)))
    # resume: nothing left to do; one wav cut short: that one alone, the same bytes again
    assert pkg.generate.generate_files(jobs, **world.arguments(which, kind), ctx=gpu[2], resume=True) == (0, [])
    os.truncate(jobs[2][1], 100)
    assert pkg.generate.generate_files(jobs, **world.arguments(which, kind), ctx=gpu[2], resume=True) == (G.LENGTHS[2], [])
    assert read(jobs[2][1]) == want[2, "wav"]


def test_independence_of_batch_composition(gpu, pkg, world, staged, tmp_path, monkeypatch):
    """One batch of four against [161], [97, 33], [1]: the same wavs, and the staged run's."""
    want = staged()
    calls = []
    real = pkg.generate.Generator.__call__
    monkeypatch.setattr(pkg.generate.Generator, "__call__",
                        lambda self, labels, *a, **k: calls.append(len(labels)) or real(self, labels, *a, **k))
    one, three = jobs_of(world, tmp_path / "one"), jobs_of(world, tmp_path / "three")
    assert pkg.generate.generate_files(one, **world.arguments(), ctx=gpu[2]) == (sum(G.LENGTHS), [])
    assert calls == [4]
    assert pkg.generate.generate_files(three, **world.arguments(), ctx=gpu[2], max_batch_frames=130) == (sum(G.LENGTHS), [])
    assert calls == [4, 1, 2, 1]
    for k in range(len(one)):
        assert read(one[k][1]) == read(three[k][1]) == want[k, "wav"], k


def labels_of(pkg, paths):
    return [pkg.recipe.read_label(p, G.FRAME_SHIFT) for p in paths]


def check_clean(out, want, torch):
    """A Generated of the four clean utterances against the staged files."""
    assert out.flagged == {} and (out.status >> 4 == 0).all()
    assert out.y.is_cuda and out.y.dtype == torch.float64 and out.pcm.dtype == torch.int16
    for k in range(len(G.LENGTHS)):
        assert out.samples(k).cpu().numpy().astype("<i2").tobytes() == want[k, "wav"][44:], k
        assert out.waveform(k).shape == out.samples(k).shape
        for name, t in list(out.streams.items()) + [("p_mgc", out.p_mgc), ("ffi", out.ffi), ("ffo", out.ffo)]:
            assert t.is_cuda and t.dtype == torch.float32
            assert out.rows(t, k).contiguous().cpu().numpy().tobytes() == want[k, name], (k, name)


def test_generator_in_memory(gpu, pkg, world, staged, tmp_path, monkeypatch):
    torch, W, ctx = gpu
    want = staged()
    empty = tmp_path / "empty"
    empty.mkdir()
    monkeypatch.chdir(empty)
    monkeypatch.setenv("TMPDIR", str(empty))
    labels = labels_of(pkg, world.labels)
    with pkg.generate.Generator(ctx=ctx, **world.arguments()) as gen:
        assert gen.var_row.is_cuda and gen.var_row.dtype == torch.float32
        assert gen.var_row.cpu().numpy().tobytes() == want[0, "var"]
        for _ in range(2):
            check_clean(gen(labels), want, torch)
        # another order, another batch: the same utterances
        out = gen(labels[::-1][:3])
        for k, u in enumerate((3, 2, 1)):
            assert out.samples(k).cpu().numpy().astype("<i2").tobytes() == want[u, "wav"][44:]
    assert os.listdir(str(empty)) == []
    ctx.synchronize()                                                                  # the caller's context lives on


def test_a_flagged_utterance_is_contained(gpu, pkg, world, staged, tmp_path, capsys):
    """Flagged by the forward pass: the utterance with a `zz`, whose output column 0 overflows float32, between two
    clean ones.  Flagged by MLPG: a variance of 0 in the bap stream's columns (the input of test_gpu_mlpg.py's
    test_status_and_untouched_neighbours), which flags every utterance.  Then the clean list again, on the same Generator."""
    torch, W, ctx = gpu
    want = staged()
    mixed = [world.labels[2], world.flagged_label, world.labels[0]]
    with pkg.generate.Generator(ctx=ctx, **world.arguments()) as gen:
        out = gen(labels_of(pkg, mixed), mixed)
        assert list(out.flagged) == [1] and out.flagged[1][0] == "forward" and out.flagged[1][1] != 0
        assert (out.status[[0, 2]] >> 4 == 0).all()
        assert "z0.lab: flagged by forward" in capsys.readouterr().err
        for k, u in ((0, 2), (2, 0)):                                                  # its neighbours are the staged run's
            assert out.samples(k).cpu().numpy().astype("<i2").tobytes() == want[u, "wav"][44:]
            assert out.rows(out.ffo, k).contiguous().cpu().numpy().tobytes() == want[u, "ffo"]
        assert not out.rows(out.ffo, 1).any()                                          # "its rows are zeros"
        (_, c0, n) = gen.setup.layout[2]
        kept = gen.var_row[c0:c0 + n].clone()
        gen.var_row[c0:c0 + n] = 0.0
        out = gen(labels_of(pkg, world.labels))
        assert out.flagged == {k: ("mlpg", 1) for k in range(len(G.LENGTHS))}
        assert capsys.readouterr().err.count("flagged by mlpg (status 1), no waveform") == len(G.LENGTHS)
        assert not out.streams["bap"].any()                                            # "the flagged columns are zeros"
        gen.var_row[c0:c0 + n] = kept
        check_clean(gen(labels_of(pkg, world.labels)), want, torch)
    # the driver: no wav for the flagged one, the return value names it, nothing raises
    jobs = jobs_of(world, tmp_path / "wav", mixed)
    n, flagged = pkg.generate.generate_files(jobs, **world.arguments(), ctx=ctx, keep_dir=str(tmp_path / "keep"))
    assert n == G.LENGTHS[2] + 40 + G.LENGTHS[0]
    assert len(flagged) == 1 and flagged[0][:2] == (world.flagged_label, "forward")
    assert "z0.lab: flagged by forward" in capsys.readouterr().err
    assert sorted(os.listdir(str(tmp_path / "wav"))) == ["a0.wav", "a2.wav"]
    assert read(jobs[0][1]) == want[2, "wav"] and read(jobs[2][1]) == want[0, "wav"]
    assert os.path.getsize(str(tmp_path / "keep" / "z0.ffo")) == 4 * G.WIDTH * 40       # what the stages left of it is kept


def test_chain_on_the_callers_stream(gpu, pkg, world, staged):
    """The chain on a context bound to the caller's non-blocking stream U, made as tests/test_gpu_caller_stream.py makes
    its calls: a warm-up on stale inputs (the model with other output biases and variances: a legitimate, different
    voice), U synchronised, then on U a delay of about 50 ms, the copy of the fresh parameters over the stale ones, and
    the call at once.  Work on stream 0, or on a side stream not forked from U, reads the stale parameters; work not
    joined back into U leaves the warm-up's result.  Either way the staged run's bytes, made on stream 0, are missed."""
    import test_gpu_caller_stream as CS
    torch, W, ctx0 = gpu
    want = staged()
    labels = labels_of(pkg, world.labels)
    env = CS.Env(torch, W, ctx0)
    try:
        with torch.cuda.stream(env.U):
            with pkg.generate.Generator(ctx=env.ctx, **world.arguments()) as gen:
                held = [gen.model.output.si_biases, gen.model.variance.variances]
                fresh = [p.detach().clone() for p in held]
                with torch.no_grad():
                    held[0] += 0.25
                    held[1] *= 1.5
                warm = gen(labels)
                assert warm.flagged == {}
                stale = [warm.samples(k).cpu().numpy().astype("<i2").tobytes() for k in range(len(labels))]
                env.U.synchronize()
                done = env.delay()
                with torch.no_grad():
                    for p, f in zip(held, fresh):
                        p.copy_(f)
                out = gen(labels)
                print("the delay was %s when the chain returned (synthesize and label_features wait for the stream)"
                      % ("still running" if not done.query() else "over"))
                check_clean(out, want, torch)
                assert any(s != want[k, "wav"][44:] for k, s in enumerate(stale))      # the stale voice is another one
            env.U.synchronize()
    finally:
        with torch.cuda.stream(env.U):
            env.ctx.close()
        torch.cuda.synchronize()

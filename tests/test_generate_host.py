"""generate.py without a device: every argument check of generate_files ahead of a context, the `generate` command
line, the resume predicate, the y-length formula against synth_files, and the status word."""
import os

import numpy as np
import pytest

import generate_setup as G
import synth_features as SF


@pytest.fixture(scope="module")
def world(pkg, tmp_path_factory):
    return G.World(pkg, tmp_path_factory.mktemp("generate_host"))


@pytest.fixture()
def no_context(pkg, monkeypatch):
    """A context that is opened fails the test: the checks come first."""
    def opened(*a, **k):
        raise AssertionError("a context was opened ahead of the argument checks")
    monkeypatch.setattr(pkg.recipe, "_own_context", opened)
    monkeypatch.setattr(pkg.world, "Context", opened)
    monkeypatch.setattr(pkg.world, "WorldBatch", opened)
    monkeypatch.setattr(pkg.world, "LabelFeatureSet", opened)


def jobs_of(world, tmp_path):
    return [(p, str(tmp_path / (os.path.basename(p)[:-4] + ".wav"))) for p in world.labels]


def streams_with(**changed):
    """G.STREAMS with some streams replaced ((name, dim, windows, msd)), dropped (None) or added."""
    out = [changed.pop(s[0], s) for s in G.STREAMS]
    return [s for s in out if s is not None] + list(changed.values())


def test_model_against_config_and_streams(pkg, world, tmp_path, no_context):
    gen = pkg.generate.generate_files
    args = world.arguments()
    short = tmp_path / "short.conf"
    short.write_text("\n".join(G.config_text().split("\n")[:-2]) + "\n")              # one feature fewer
    with pytest.raises(ValueError, match=r"takes 9 inputs.* yields 8 features"):
        gen(jobs_of(world, tmp_path), **dict(args, config=str(short)))
    with pytest.raises(ValueError, match=r"takes 9 inputs.* yields 8 features"):      # a parsed config as well
        gen(jobs_of(world, tmp_path), **dict(args, config=pkg.recipe.read_question_config(str(short))))
    with pytest.raises(ValueError, match=r"has 34 outputs.* has 37"):
        gen(jobs_of(world, tmp_path), **dict(args, streams=streams_with(vib=("vib", 3, G.WINDOWS, False))))
    with pytest.raises(ValueError, match=r"has 34 outputs.* has 35"):
        gen(jobs_of(world, tmp_path), **dict(args, streams=streams_with(vib=("vib", 2, G.WINDOWS, True))))
    with pytest.raises(ValueError, match=r"speaker 1: the model has 1"):
        gen(jobs_of(world, tmp_path), **dict(args, spkr=1))
    with pytest.raises(ValueError, match=r"speaker 3: the model has 3"):
        gen(jobs_of(world, tmp_path), **dict(world.arguments(kind="sat"), spkr=3))


def test_synthesis_streams(pkg, world, tmp_path, no_context):
    gen = pkg.generate.generate_files
    args = world.arguments()
    for name in ("mgc", "lf0", "bap"):
        with pytest.raises(ValueError, match=r"stream %s is given 0 times, synthesis needs it 1 time" % name):
            gen(jobs_of(world, tmp_path), **dict(args, streams=streams_with(**{name: None})))
        twice = G.STREAMS[[s[0] for s in G.STREAMS].index(name)]
        with pytest.raises(ValueError, match=r"stream %s is given 2 times, synthesis needs it 1 time" % name):
            gen(jobs_of(world, tmp_path), **dict(args, streams=streams_with(again=twice)))
    with pytest.raises(ValueError, match=r"5 streams carry 4 names"):
        gen(jobs_of(world, tmp_path), **dict(args, streams=streams_with(again=("vib", 2, G.WINDOWS, False))))
    with pytest.raises(ValueError, match=r"lf0 has dimension 2 and msd 1: synthesis needs 1 and 1"):
        gen(jobs_of(world, tmp_path), **dict(args, streams=streams_with(lf0=("lf0", 2, G.WINDOWS, True))))
    with pytest.raises(ValueError, match=r"lf0 has dimension 1 and msd 0: synthesis needs 1 and 1"):
        gen(jobs_of(world, tmp_path), **dict(args, streams=streams_with(lf0=("lf0", 1, G.WINDOWS, False))))
    with pytest.raises(ValueError, match=r"bap has dimension 1, its coding order 0 is outside 1 \.\. 63"):
        gen(jobs_of(world, tmp_path), **dict(args, streams=streams_with(bap=("bap", 1, G.WINDOWS, False))))
    with pytest.raises(ValueError, match=r"\(name, dim, windows, msd\)"):
        gen(jobs_of(world, tmp_path), **dict(args, streams=[s[1:] for s in G.STREAMS]))


@pytest.mark.parametrize("fft_size", [0, 256, 1000, 8192])
def test_fft_size_outside_the_supported_range(pkg, world, tmp_path, no_context, fft_size):
    with pytest.raises(ValueError, match=r"fft_size %d is not one of the supported 512 \.\.\. 4096" % fft_size):
        pkg.generate.generate_files(jobs_of(world, tmp_path), **dict(world.arguments(), fft_size=fft_size))


def test_mspf_tables_and_postfilter_choice(pkg, world, tmp_path, no_context):
    gen = pkg.generate.generate_files
    args = world.arguments("mspf")
    post = list(args["postfilter"])
    post[5] = 32                                                                     # the tables hold 64 / 2 + 1 bins
    with pytest.raises(ValueError, match=r"mgc_dim0\.mean holds 33 bins, fft_length 32 needs 17"):
        gen(jobs_of(world, tmp_path), **dict(args, postfilter=tuple(post)))
    nat = G.write_mspf_tables(tmp_path / "nat", 0.1)
    np.zeros(5, dtype=np.float32).tofile(os.path.join(nat, "mgc_dim4.stdd"))
    post = list(args["postfilter"])
    post[2] = nat
    with pytest.raises(ValueError, match=r"mgc_dim4\.stdd holds 5 bins, fft_length 64 needs 33"):
        gen(jobs_of(world, tmp_path), **dict(args, postfilter=tuple(post)))
    for bad in (("mcp", 1.4), ("mspf", "a", "b"), ("other", 1, 2)):
        with pytest.raises(ValueError, match="postfilter is None"):
            gen(jobs_of(world, tmp_path), **dict(args, postfilter=bad))


def test_a_label_without_frames(pkg, world, tmp_path, no_context, monkeypatch):
    gen = pkg.generate
    assert gen.label_frames([([(0, 3, "a", 0), (3, 7, "b", 0)], False), ([(2, 3, "a", 0)], False)]) == [7, 1]
    with pytest.raises(ValueError, match=r"label 1 holds 0 frames, an utterance needs at least 1"):
        gen.label_frames([([(0, 3, "a", 0)], False), ([], False)])
    real = pkg.recipe.read_label
    monkeypatch.setattr(pkg.recipe, "read_label", lambda p, fs: ([], False) if p == world.labels[2] else real(p, fs))
    with pytest.raises(ValueError, match=r"a2\.lab holds 0 frames, an utterance needs at least 1"):
        gen.generate_files(jobs_of(world, tmp_path), **world.arguments())
    with pytest.raises(ValueError, match=r"a job is \(label_file, wav_out\)"):
        gen.generate_files([(world.labels[0],)], **world.arguments())


def test_nothing_to_do_opens_no_context(pkg, world, tmp_path, no_context):
    """An empty list, and a list whose wavs are complete under resume, return ahead of the device as well."""
    gen = pkg.generate
    assert gen.generate_files([], **world.arguments()) == (0, [])
    jobs = jobs_of(world, tmp_path)
    for (_, wav), T in zip(jobs, G.LENGTHS):
        pkg.recipe.write_wav(wav, np.zeros(gen.y_length(T, G.FRAME_PERIOD, G.FS)), G.FS)
    assert gen.generate_files(jobs, **world.arguments(), resume=True) == (0, [])


def test_resume_predicate(pkg, tmp_path):
    gen = pkg.generate
    path = str(tmp_path / "a.wav")
    assert not gen.wav_complete(path, 97, 5.0, 16000)                                  # no file
    n = gen.y_length(97, 5.0, 16000)
    assert n == 96 * 80 + 1
    pkg.recipe.write_wav(path, np.linspace(-1.0, 1.0, n), 16000)
    assert os.path.getsize(path) == gen.wav_size(n) == 44 + 2 * n
    assert gen.wav_complete(path, 97, 5.0, 16000)
    assert not gen.wav_complete(path, 96, 5.0, 16000) and not gen.wav_complete(path, 98, 5.0, 16000)
    assert not gen.wav_complete(path, 97, 5.0, 48000) and not gen.wav_complete(path, 97, 2.5, 16000)
    os.truncate(path, 44 + 2 * n - 2)                                                  # a write that was cut short
    assert not gen.wav_complete(path, 97, 5.0, 16000)
    with open(path, "ab") as f:
        f.write(b"\0" * 4)                                                             # too long
    assert not gen.wav_complete(path, 97, 5.0, 16000)


class _Captured(Exception):
    pass


@pytest.mark.parametrize("fs, frame_period", [(16000, 5.0), (48000, 5.0), (22050, 2.5), (44100, 5.0), (8000, 10.0)])
def test_y_length_is_synth_files_own(pkg, tmp_path, monkeypatch, fs, frame_period):
    """The lengths synth_files hands its batch for files of these frame counts, read off the batch it makes."""
    rec, gen = pkg.recipe, pkg.generate
    frames = [1, 2, 3, 33, 97, 160, 161, 400, 1599, 1600]
    seen = {}

    def batch(ctx, params, f0_lengths=None, y_lengths=None):
        seen["f0"], seen["y"] = list(f0_lengths), list(y_lengths)
        raise _Captured()
    monkeypatch.setattr(rec.W, "WorldBatch", batch)
    monkeypatch.setattr(rec, "_own_context", lambda: type("Ctx", (), {"close": lambda self: None})())
    jobs = []
    for k, T in enumerate(frames):
        np.zeros(T, dtype=np.float32).tofile(str(tmp_path / ("u%d.lf0" % k)))
        jobs.append((str(tmp_path / ("u%d.lf0" % k)), "mgc", "bap", "wav"))
    with pytest.raises(_Captured):
        rec.synth_files(jobs, frame_period, 1024, fs, 6, 2, max_batch_frames=10 ** 9)
    assert sorted(seen["f0"]) == sorted(frames)
    assert seen["y"] == [gen.y_length(T, frame_period, fs) for T in seen["f0"]]
    assert seen["y"] == [SF.recipe_length(T, fs, frame_period) for T in seen["f0"]]


def test_stream_option_with_a_name(pkg):
    rec = pkg.recipe
    assert rec.parse_named_stream("lf0:1:1:lf0.win1,lf0.win2,lf0.win3") == ("lf0", 1, ["lf0.win1", "lf0.win2", "lf0.win3"], True)
    assert rec.parse_named_stream("mgc:50:0:w/mgc.win1") == ("mgc", 50, ["w/mgc.win1"], False)
    assert rec.parse_named_stream("vib:2::a,b") == ("vib", 2, ["a", "b"], False)
    assert rec.parse_named_stream("bap:25:0:a,b")[1:] == rec.parse_stream("25:0:a,b")
    for bad in (":1:1:a", "lf0", "lf0:1", "lf0:x:1:a"):
        with pytest.raises(ValueError):
            rec.parse_named_stream(bad)


def recipe_default_argv(world, scp, wins, extra=()):
    """The recipe's own setting (48 kHz, 5 ms, fft 2048, mgc 50 / lf0 / bap 25, three windows each, alpha 0.55)."""
    w = lambda n: ",".join(str(wins / ("%s.win%d" % (n, k))) for k in (1, 2, 3))
    return ["generate", "--scp", str(scp), "--config", world.config, "--frame-shift", "50000", "--model",
            world.models["sd"][0], "--stream", "mgc:50:0:" + w("mgc"), "--stream", "lf0:1:1:" + w("lf0"), "--stream",
            "bap:25:0:" + w("bap"), "--fs", "48000", "--frame-period", "5", "--fft-size", "2048", "--alpha", "0.55",
            "--postfilter", "mcp", "--beta", "1.4", "--length", "4096"] + list(extra)


def test_command_line(pkg, world, tmp_path, no_context, capsys, monkeypatch):
    rec = pkg.recipe
    wins = tmp_path / "win"
    wins.mkdir()
    for n in ("mgc", "lf0", "bap"):
        for k, w in enumerate(G.WINDOWS, 1):
            (wins / ("%s.win%d" % (n, k))).write_text("%d %s\n" % (len(w), " ".join(repr(v) for v in w)))
    scp = tmp_path / "jobs.scp"
    scp.write_text("".join("%s %s\n" % j for j in jobs_of(world, tmp_path)))
    calls = []
    monkeypatch.setattr(pkg.generate, "generate_files", lambda jobs, **kw: calls.append((jobs, kw)) or (7, []))
    assert rec.main(recipe_default_argv(world, scp, wins)) == 0
    assert "complete. 7 frames, 0 utterances flagged" in capsys.readouterr().out
    jobs, kw = calls.pop()
    assert jobs == jobs_of(world, tmp_path)
    assert kw["streams"] == [(n, d, [str(wins / ("%s.win%d" % (n, k))) for k in (1, 2, 3)], m)
                             for n, d, m in (("mgc", 50, False), ("lf0", 1, True), ("bap", 25, False))]
    assert (kw["fs"], kw["frame_period"], kw["fft_size"], kw["alpha"], kw["frame_shift"]) == (48000, 5.0, 2048, 0.55, 50000)
    assert kw["postfilter"] == ("mcp", 1.4, 4096) and kw["spkr"] is None and kw["keep_dir"] is None and not kw["resume"]
    assert kw["max_batch_frames"] == rec.MAX_BATCH_FRAMES and kw["edge"] == 0 and kw["unvoiced_value"] == -1.0e10
    extra = ["--postfilter", "mspf", "--gen-stats", "g", "--nat-stats", "n", "--emphasis", "0.5", "--keep-dir", "k",
             "--resume", "--max-batch-frames", "4000", "--spkr", "2"]
    assert rec.main(recipe_default_argv(world, scp, wins, extra)) == 0
    _, kw = calls.pop()
    assert kw["postfilter"] == ("mspf", "g", "n", 0.5, 25, 64)
    assert (kw["keep_dir"], kw["resume"], kw["max_batch_frames"], kw["spkr"]) == ("k", True, 4000, 2)
    assert rec.main(recipe_default_argv(world, scp, wins, ["--postfilter", "none"])) == 0
    assert calls.pop()[1]["postfilter"] is None
    for bad in (["--postfilter", "mspf"], ["--postfilter", "mspf", "--gen-stats", "g"], ["--frame-shift", "0"],
                ["--postfilter", "other"], ["--stream", "lf0:1"]):
        with pytest.raises(SystemExit):
            rec.main(recipe_default_argv(world, scp, wins, bad))
    argv = recipe_default_argv(world, scp, wins)
    for k in range(0, len(argv) - 1, 2):                                               # every required option
        if argv[1 + k] in ("--scp", "--config", "--frame-shift", "--model", "--fs", "--fft-size", "--alpha"):
            with pytest.raises(SystemExit):
                rec.main(argv[:1 + k] + argv[3 + k:])
    assert not calls


def test_command_reaches_the_checks_with_the_window_files(pkg, world, tmp_path, no_context):
    """The real generate_files behind the command: the window files are read, the 34-column model does not fit the
    recipe's 229-column row, and the check says so ahead of any context."""
    wins = tmp_path / "win"
    wins.mkdir()
    for n in ("mgc", "lf0", "bap"):
        for k, w in enumerate(G.WINDOWS, 1):
            (wins / ("%s.win%d" % (n, k))).write_text("%d %s\n" % (len(w), " ".join(repr(v) for v in w)))
    scp = tmp_path / "jobs.scp"
    scp.write_text("".join("%s %s\n" % j for j in jobs_of(world, tmp_path)))
    with pytest.raises(ValueError, match=r"has 34 outputs.* has 229"):
        pkg.recipe.main(recipe_default_argv(world, scp, wins))
    assert pkg.recipe.Generator is pkg.generate.Generator and pkg.recipe.generate_files is pkg.generate.generate_files


def test_status_word_and_the_stage_it_names(pkg):
    gen = pkg.generate
    word = gen.status_word([0, 3, 1, 0, 2], [0, 0, 2, 0, 0], [0, 0, 1, 2, 0], [0, 0, 0, 3, 1])
    assert word.dtype == np.int32 and word.tolist() == [0, 3, 1 | 2 << 4 | 1 << 8, 2 << 8 | 3 << 12, 2 | 1 << 12]
    assert [gen.flagged_stage(w) for w in word] == [None, None, ("forward", 2), ("mlpg", 2), ("postfilter", 1)]

"""The two drivers of voice modification on the device: `recipe.py modify` against modify.convert called directly, and
`generate --f0-scale --formant-ratio` against the kept features passed through modify_features and synthesize -- and,
without the two options, against the staged drivers' bytes with no modify kernel launched."""
import contextlib
import importlib
import io
import os

import numpy as np
import pytest

import generate_setup as G

pytestmark = pytest.mark.gpu
sd = importlib.import_module("hts-train-world_amd.synth_data")

FS = 16000


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def wavs(pkg, tmp_path_factory):
    """Three short utterances as 16-bit wavs, and the factors of their lines (None: the line leaves it out)."""
    root = tmp_path_factory.mktemp("modify_wavs")
    items = []
    for k, (dur, shift, ratio) in enumerate([(0.2, 1.2, 0.9), (0.3, 0.8, None), (0.25, None, None)]):
        path = str(root / ("u%d.wav" % k))
        pkg.recipe.write_wav(path, sd.make_utterance(210 + k, FS, duration=dur), FS)
        items.append((path, shift, ratio))
    return items


def direct(gpu, pkg, path, shift, ratio):
    """The int16 samples of convert + samples_to_pcm16 on the utterance alone, with the driver's parameters."""
    torch, W, ctx = gpu
    rec = pkg.recipe
    pcm = rec._read_pcm16(path)
    b = W.WorldBatch(ctx, rec.modify_params(FS), x_lengths=[len(pcm)])
    try:
        x = b.samples_from_pcm16(torch.from_numpy(pcm.astype(np.int16)).cuda())
        y = pkg.modify.convert(b, x, shift, ratio)
        out = b.samples_to_pcm16(y).cpu().numpy()
        assert len(out) == rec.modify_samples(len(pcm), FS, 5.0)
        return out.astype("<i2").tobytes()
    finally:
        b.close()


def test_modify_command_equals_convert(gpu, pkg, wavs, tmp_path, capsys):
    rec = pkg.recipe
    outs = [str(tmp_path / ("o%d.wav" % k)) for k in range(len(wavs))]
    scp = tmp_path / "jobs.txt"
    scp.write_text("".join("%s %s%s%s\n" % (p, o, "" if s is None else " %r" % s, "" if r is None else " %r" % r)
                           for (p, s, r), o in zip(wavs, outs)))
    argv = ["modify", "--scp", str(scp), "--formant-ratio", "1.1"]       # for the lines that give no ratio
    assert rec.main(argv) == 0
    frames = [pkg.sharding.frame_count((len(read(p)) - 44) // 2, FS, 5.0) for p, _, _ in wavs]
    assert "complete. %d frames" % sum(frames) in capsys.readouterr().out
    want = [direct(gpu, pkg, p, s, 1.1 if r is None else r) for p, s, r in wavs]
    for k, o in enumerate(outs):
        data = read(o)
        assert data[:4] == b"RIFF" and len(data) == 44 + len(want[k])
        assert data[44:] == want[k], k
        assert np.frombuffer(want[k], dtype="<i2").any()
    plain = direct(gpu, pkg, wavs[2][0], None, None)
    assert plain != want[2] and want[0] != direct(gpu, pkg, wavs[0][0], None, 0.9)       # each factor does something
    # --resume: nothing left to do; one output cut short: that one alone, the same bytes again
    assert rec.main(argv + ["--resume"]) == 0
    assert "complete. 0 frames" in capsys.readouterr().out
    stamps = [os.stat(o).st_mtime_ns for o in outs]
    os.truncate(outs[1], 100)
    assert rec.main(argv + ["--resume"]) == 0
    assert "complete. %d frames" % frames[1] in capsys.readouterr().out
    assert read(outs[1])[44:] == want[1]
    assert [os.stat(o).st_mtime_ns for o in outs][::2] == stamps[::2]


@pytest.fixture(scope="module")
def world(pkg, tmp_path_factory):
    return G.World(pkg, tmp_path_factory.mktemp("modify_generate"))


def jobs_of(world, out_dir):
    os.makedirs(str(out_dir), exist_ok=True)
    return [(p, os.path.join(str(out_dir), os.path.basename(p)[:-4] + ".wav")) for p in world.labels]


def test_generate_with_the_two_options(gpu, pkg, world, tmp_path):
    """`generate --f0-scale 1.2 --formant-ratio 1.1`: the wav of the kept lf0, p_mgc and bap decoded, modified and
    synthesized one utterance at a time."""
    torch, W, ctx = gpu
    rec = pkg.recipe
    wins = tmp_path / "win"
    wins.mkdir()
    for k, w in enumerate(G.WINDOWS, 1):
        (wins / ("win%d" % k)).write_text("%d %s\n" % (len(w), " ".join(repr(v) for v in w)))
    w3 = ",".join(str(wins / ("win%d" % k)) for k in (1, 2, 3))
    jobs, keep = jobs_of(world, tmp_path / "wav"), tmp_path / "keep"
    scp = tmp_path / "jobs.scp"
    scp.write_text("".join("%s %s\n" % j for j in jobs))
    argv = ["generate", "--scp", str(scp), "--config", world.config, "--frame-shift", str(G.FRAME_SHIFT), "--model",
            world.models["sd"][0], "--fs", str(G.FS), "--frame-period", str(G.FRAME_PERIOD), "--fft-size", str(G.FFT_SIZE),
            "--alpha", str(G.ALPHA), "--postfilter", "mcp", "--beta", str(G.MCP[1]), "--length", str(G.MCP[2]),
            "--keep-dir", str(keep), "--f0-scale", "1.2", "--formant-ratio", "1.1"]
    for name, dim, _, msd in G.STREAMS:
        argv += ["--stream", "%s:%d:%d:%s" % (name, dim, int(msd), w3)]
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        assert rec.main(argv) == 0
    assert "warning: " not in err.getvalue(), err.getvalue()
    dims = {s[0]: s[1] for s in G.STREAMS}
    differs = 0
    for k, (T, (_, wav)) in enumerate(zip(G.LENGTHS, jobs)):
        base = str(keep / ("a%d" % k))
        lf0 = np.fromfile(base + ".lf0", dtype=np.float32)
        mgc = np.fromfile(base + ".p_mgc", dtype=np.float32).reshape(T, dims["mgc"])
        bap = np.fromfile(base + ".bap", dtype=np.float32).reshape(T, dims["bap"])
        b = W.WorldBatch(ctx, W.default_params(G.FS, G.FRAME_PERIOD, fft_size=G.FFT_SIZE), f0_lengths=[T],
                         y_lengths=[pkg.generate.y_length(T, G.FRAME_PERIOD, G.FS)])
        f0, sp, ap = b.recipe_decode(*(torch.from_numpy(a).cuda() for a in (lf0, mgc, bap)))
        plain = b.synthesize(f0, sp, ap).cpu().numpy()
        f0m, spm = pkg.modify.modify_features(b, f0, sp, 1.2, 1.1)
        y = b.synthesize(f0m, spm, ap).cpu().numpy()
        b.close()
        mine = str(tmp_path / ("want%d.wav" % k))
        rec.write_wav(mine, y, G.FS)
        assert read(wav) == read(mine), k
        differs += int(not np.array_equal(y, plain))
    assert differs >= 2                                                # the two factors made other waveforms


def test_generate_without_them_is_todays(gpu, pkg, world, tmp_path):
    """No option: the staged drivers' bytes, as before, and not one modify kernel."""
    torch, W, ctx = gpu
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        base = world.staged(pkg.recipe, tmp_path / "staged", ctx=ctx)
    jobs = jobs_of(world, tmp_path / "wav")
    ctx.timing_enable(True)
    try:
        n, flagged = pkg.generate.generate_files(jobs, **world.arguments(), ctx=ctx)
        assert n == sum(G.LENGTHS) and flagged == []
        assert ctx.timing_query("modify_kernel")[1] == 0
        n, flagged = pkg.generate.generate_files(jobs_of(world, tmp_path / "mod"), **world.arguments(), ctx=ctx,
                                                 formant_ratio=1.1)
        assert ctx.timing_query("modify_kernel")[1] == 1                # the probe sees the kernel when it runs
    finally:
        ctx.timing_enable(False)
    for b, (_, wav) in zip(base, jobs):
        assert read(wav) == read(b + ".wav"), wav

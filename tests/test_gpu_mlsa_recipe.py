"""recipe.mlsa_synth_files / `recipe.py mlsa-synth` (scripts/Training.pl:2873-2899) on three small file sets: the `.raw`
and `.wav` files hold the batch call's samples byte for byte, whatever the batching; resume skips what is complete; two
shards together write what one writes; a flagged utterance is reported and leaves no file."""
import importlib
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN

import test_gpu_mlsa as T

pytestmark = pytest.mark.gpu

FS, P, ORDER, ALPHA, PD = 16000, 80, 12, 0.42, 5
SHAPE = dict(fs=FS, frame_shift=P, order=ORDER, alpha=ALPHA, pade_order=PD)
TAPS = np.load(os.path.join(GOLDEN, "makefilter.npz"))


@pytest.fixture(scope="module")
def recipe():
    return importlib.import_module("hts-train-world_amd.recipe")


def file_sets(tmp_path, tag="u"):
    """Three utterances of 9, 5 and 2 frames: lf0 with unvoiced runs, mel-cepstra scaled to 16-bit amplitudes."""
    rng = np.random.default_rng(91)
    sets = []
    for k, T_ in enumerate((9, 5, 2)):
        lf0 = np.log(100.0 + 80.0 * rng.random(T_)).astype(np.float32)
        if T_ > 4:
            lf0[2:4] = -1.0e10
        mc = T.mel_cepstra(T_, ORDER, rng)
        mc[:, 0] += 7.0                                      # e^6.5: pulses of a few thousand
        base = str(tmp_path / ("%s%d" % (tag, k)))
        lf0.tofile(base + ".lf0")
        mc.tofile(base + ".mgc")
        sets.append((lf0, mc, base))
    return sets


def jobs_of(sets, suffix=""):
    return [(base + ".lf0", base + ".mgc", base + suffix + ".raw", base + suffix + ".wav") for _, _, base in sets]


def in_memory(gpu, recipe, lf0, mc, pipe_float32=True):
    torch = gpu[0]
    b = T.make_batch(gpu, [len(lf0)], P)
    try:
        y, st = b.mlsa_synthesis(T.dev(torch, recipe.mlsa_pitch(lf0, FS), np.float32), T.dev(torch, mc, np.float32),
                                 TAPS["taps_16000_0"], TAPS["taps_16000_1"], alpha=ALPHA, pade_order=PD, frame_shift=P,
                                 pipe_float32=pipe_float32)
        assert st.cpu().numpy()[0] == 0
        return recipe.pcm16_of_pipe(y.cpu().numpy()).tobytes()
    finally:
        b.close()


def wav_of(pcm_bytes):
    n = len(pcm_bytes)
    return (b"RIFF" + struct.pack("<I", 36 + n) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, FS, FS * 2, 2, 16)
            + b"data" + struct.pack("<I", n) + pcm_bytes)


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_pitch_and_pcm_of_the_shell_line(recipe):
    lf0 = np.array([np.log(200.0), -1.0e10, np.log(125.0)], dtype=np.float32)
    pitch = recipe.mlsa_pitch(lf0, 16000)
    assert pitch.dtype == np.float32 and pitch[1] == 0.0
    assert pitch[0] == np.float32(16000.0 * (1.0 / np.exp(np.float64(lf0[0])))) and abs(pitch[2] - 128.0) < 1e-3
    pcm = recipe.pcm16_of_pipe([0.9, -0.9, 1.5, -1.5, 40000.0, -40000.0, 32767.9])
    assert list(pcm) == [0, 0, 1, -1, 32767, -32768, 32767]
    assert list(recipe.read_taps(str(TAPS["text_16000_0"]))) == list(TAPS["taps_16000_0"])


def test_files_are_the_batch_calls_samples(gpu, recipe, tmp_path, capsys):
    ctx = gpu[2]
    sets = file_sets(tmp_path)
    lp, hp = recipe.read_taps(str(TAPS["text_16000_0"])), recipe.read_taps(str(TAPS["text_16000_1"]))
    total = sum(len(lf0) for lf0, _, _ in sets)
    assert recipe.mlsa_synth_files(jobs_of(sets), lp, hp, ctx=ctx, **SHAPE) == (total, [])
    assert recipe.mlsa_synth_files(jobs_of(sets, "_one"), lp, hp, ctx=ctx, max_batch_frames=9, **SHAPE) == (total, [])
    want = [in_memory(gpu, recipe, lf0, mc) for lf0, mc, _ in sets]
    for k, (lf0, _, _) in enumerate(sets):
        assert len(want[k]) == 2 * (len(lf0) - 1) * P
        assert np.abs(np.frombuffer(want[k], dtype="<i2")).max() > 100, "the samples are no 16-bit amplitudes"
        for suffix in ("", "_one"):
            _, _, raw, wav = jobs_of(sets, suffix)[k]
            assert read(raw) == want[k], (suffix, k)
            assert read(wav) == wav_of(want[k]), (suffix, k)
    # resume: what is complete stays, what is missing or short is made
    jobs = jobs_of(sets)
    os.remove(jobs[1][2])
    with open(jobs[2][3], "ab") as f:
        f.write(b"\0\0")
    before = os.stat(jobs[0][2]).st_mtime_ns
    n, flagged = recipe.mlsa_synth_files(jobs, lp, hp, ctx=ctx, resume=True, **SHAPE)
    assert n == len(sets[1][0]) + len(sets[2][0]) and flagged == []
    assert os.stat(jobs[0][2]).st_mtime_ns == before
    for k in (1, 2):
        assert read(jobs[k][2]) == want[k] and read(jobs[k][3]) == wav_of(want[k])
    assert recipe.mlsa_synth_files(jobs, lp, hp, ctx=ctx, resume=True, **SHAPE) == (0, [])
    # the pipes' roundings are part of the bytes
    double = [(jobs[0][0], jobs[0][1], str(tmp_path / "double.raw"), str(tmp_path / "double.wav"))]
    recipe.mlsa_synth_files(double, lp, hp, ctx=ctx, pipe_float32=False, **SHAPE)
    assert read(double[0][2]) == in_memory(gpu, recipe, sets[0][0], sets[0][1], False)


def test_two_shards_write_what_one_writes(gpu, recipe, tmp_path, monkeypatch):
    ctx = gpu[2]
    sets = file_sets(tmp_path)
    lp, hp = TAPS["taps_16000_0"], TAPS["taps_16000_1"]
    recipe.mlsa_synth_files(jobs_of(sets), lp, hp, ctx=ctx, **SHAPE)
    monkeypatch.setenv("WORLD_SIZE", "2")
    done = []
    for rank in (0, 1):
        monkeypatch.setenv("RANK", str(rank))
        n, flagged = recipe.mlsa_synth_files(jobs_of(sets, "_shard"), lp, hp, ctx=ctx, **SHAPE)
        assert flagged == [] and 0 < n < sum(len(lf0) for lf0, _, _ in sets)
        done.append(n)
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert sum(done) == sum(len(lf0) for lf0, _, _ in sets)
    for one, two in zip(jobs_of(sets), jobs_of(sets, "_shard")):
        assert read(one[2]) == read(two[2]) and read(one[3]) == read(two[3])


def test_flagged_utterance_is_reported_and_not_written(gpu, recipe, tmp_path, capsys):
    ctx = gpu[2]
    sets = file_sets(tmp_path)
    bad = sets[1][1].copy()
    bad[2, 3] = np.nan
    bad.tofile(sets[1][2] + ".mgc")
    jobs = jobs_of(sets)
    capsys.readouterr()
    n, flagged = recipe.mlsa_synth_files(jobs, TAPS["taps_16000_0"], TAPS["taps_16000_1"], ctx=ctx, **SHAPE)
    err = capsys.readouterr().err
    assert flagged == [jobs[1][0]] and jobs[1][0] in err and "status 1" in err and jobs[0][0] not in err
    assert not os.path.exists(jobs[1][2]) and not os.path.exists(jobs[1][3])
    assert os.path.getsize(jobs[0][2]) == 2 * 8 * P and os.path.getsize(jobs[2][3]) == 44 + 2 * P


def test_command(gpu, recipe, tmp_path, capsys):
    """`recipe.py mlsa-synth` on a job list, on a context of its own, the taps as makefilter.pl prints them and from a
    file: the bytes of the in-memory call."""
    sets = file_sets(tmp_path)
    scp = tmp_path / "jobs.scp"
    scp.write_text("".join("%s %s %s %s\n" % j for j in jobs_of(sets)))
    (tmp_path / "hfil").write_text(str(TAPS["text_16000_1"]))
    assert recipe.main(["mlsa-synth", "--scp", str(scp), "--lowpass", str(TAPS["text_16000_0"]), "--highpass",
                        str(tmp_path / "hfil"), "--fs", str(FS), "--frame-shift", str(P), "--alpha", str(ALPHA), "--order",
                        str(ORDER), "--pade-order", str(PD)]) == 0
    assert "complete. 16 frames, 0 utterances flagged" in capsys.readouterr().out
    for (lf0, mc, _), job in zip(sets, jobs_of(sets)):
        want = in_memory(gpu, recipe, lf0, mc)
        assert read(job[2]) == want and read(job[3]) == wav_of(want)

"""recipe.mgcep_files / `recipe.py mgcep` (data/Makefile.in:134-137 at gamma 0) on the fixture's integer waveforms: the
files are the in-memory call's rows rounded to float32, whatever the container of the samples and the batching; resume
skips what is complete; an utterance with a flagged frame is reported and leaves no file."""
import importlib
import os
import wave

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SHAPE = dict(frame_length=400, frame_shift=80, fft_length=512, window=1, normalize=1, alpha=0.42, order=12, eps=1e-8)


@pytest.fixture(scope="module")
def recipe():
    return importlib.import_module("hts-train-world_amd.recipe")


@pytest.fixture(scope="module")
def waves():
    fx = np.load(os.path.join(GOLDEN, "sptk_mgcep.npz"))
    x, at = fx["x_wave"], np.concatenate([[0], np.cumsum(fx["T_wave"])])
    return [x[at[k]:at[k + 1]] for k in (1, 4, 5, 6)]                  # 37, 201, 1000 and 1203 samples, int16


def write_wav16(path, pcm, fs=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(fs)
        w.writeframes(pcm.astype("<i2").tobytes())


def in_memory(gpu, pcm, pipe_float32=True):
    torch, W, ctx = gpu
    L, P, F = SHAPE["frame_length"], SHAPE["frame_shift"], SHAPE["fft_length"]
    b = W.WorldBatch(ctx, W.default_params(48000, 5.0, fft_size=F), x_lengths=[len(pcm)],
                     f0_lengths=[W.sptk_frames(len(pcm), L, P)])
    try:
        mc, st = b.mel_cepstrum_of_waveform(torch.from_numpy(pcm.astype(np.float64)).cuda(),
                                            W.sptk_window(SHAPE["window"], SHAPE["normalize"], L), L, P, SHAPE["order"],
                                            SHAPE["alpha"], pipe_float32, etype=1, e=SHAPE["eps"])
        assert (st.cpu().numpy() <= 0).all()
        return mc.float().cpu().numpy().tobytes()
    finally:
        b.close()


def test_files_are_the_in_memory_rows_whatever_container_and_batching(gpu, recipe, waves, tmp_path, capsys):
    ctx = gpu[2]
    jobs = {"raw": [], "wav": [], "three": []}
    for k, pcm in enumerate(waves):
        pcm.astype("<i2").tofile(tmp_path / ("u%d.raw" % k))
        write_wav16(tmp_path / ("u%d.wav" % k), pcm)
        jobs["raw"].append((str(tmp_path / ("u%d.raw" % k)), str(tmp_path / ("raw%d.mgc" % k))))
        jobs["wav"].append((str(tmp_path / ("u%d.wav" % k)), str(tmp_path / ("wav%d.mgc" % k))))
        jobs["three"].append((str(tmp_path / ("u%d.raw" % k)), str(tmp_path / ("three%d.mgc" % k))))
    total = sum(gpu[1].sptk_frames(len(p), 400, 80) for p in waves)
    assert recipe.mgcep_files(jobs["raw"], ctx=ctx, **SHAPE) == (total, [])
    assert recipe.mgcep_files(jobs["wav"], ctx=ctx, **SHAPE) == (total, [])
    assert recipe.mgcep_files(jobs["three"], ctx=ctx, max_batch_frames=20, **SHAPE) == (total, [])   # 18 | 15 | 6, 3 frames
    for k, pcm in enumerate(waves):
        want = in_memory(gpu, pcm)
        assert len(want) == 4 * 13 * gpu[1].sptk_frames(len(pcm), 400, 80)
        for name in ("raw", "wav", "three"):
            assert open(jobs[name][k][1], "rb").read() == want, (name, k)
    # resume: what is complete stays, what is missing or short is made
    os.remove(jobs["raw"][1][1])
    with open(jobs["raw"][2][1], "ab") as f:
        f.write(b"\0\0\0\0")
    before = os.stat(jobs["raw"][0][1]).st_mtime_ns
    n, flagged = recipe.mgcep_files(jobs["raw"], ctx=ctx, resume=True, **SHAPE)
    assert n == sum(gpu[1].sptk_frames(len(waves[k]), 400, 80) for k in (1, 2)) and flagged == []
    assert os.stat(jobs["raw"][0][1]).st_mtime_ns == before
    for k in (1, 2):
        assert open(jobs["raw"][k][1], "rb").read() == in_memory(gpu, waves[k])
    assert recipe.mgcep_files(jobs["raw"], ctx=ctx, resume=True, **SHAPE) == (0, [])
    # the pipe's rounding is part of the bytes
    n, _ = recipe.mgcep_files([(jobs["raw"][3][0], str(tmp_path / "double.mgc"))], ctx=ctx, pipe_float32=False, **SHAPE)
    assert open(tmp_path / "double.mgc", "rb").read() == in_memory(gpu, waves[3], False) != in_memory(gpu, waves[3])


def test_flagged_utterance_is_reported_and_not_written(gpu, recipe, waves, tmp_path, capsys):
    ctx = gpu[2]
    silent = waves[2].copy()
    silent[100:700] = 0                                                # longer than a frame: frames of digital zero
    silent.astype("<i2").tofile(tmp_path / "silent.raw")
    waves[0].astype("<i2").tofile(tmp_path / "fine.raw")
    jobs = [(str(tmp_path / "silent.raw"), str(tmp_path / "silent.mgc")), (str(tmp_path / "fine.raw"), str(tmp_path / "fine.mgc"))]
    shape = dict(SHAPE, eps=0.0)
    capsys.readouterr()
    n, flagged = recipe.mgcep_files(jobs, ctx=ctx, **shape)
    err = capsys.readouterr().err
    assert flagged == [jobs[0][0]] and jobs[0][0] in err and "status 2" in err and jobs[1][0] not in err
    assert not os.path.exists(jobs[0][1]) and os.path.getsize(jobs[1][1]) == 4 * 13 * gpu[1].sptk_frames(len(waves[0]), 400, 80)
    # with the command's eps the same samples are analysed
    assert recipe.mgcep_files(jobs[:1], ctx=ctx, **SHAPE)[1] == [] and os.path.exists(jobs[0][1])


def test_command(gpu, recipe, waves, tmp_path, capsys):
    """`recipe.py mgcep` on a job list, on a context of its own: the bytes of the in-memory call."""
    waves[1].astype("<i2").tofile(tmp_path / "a.raw")
    scp = tmp_path / "jobs.scp"
    scp.write_text("%s %s\n" % (tmp_path / "a.raw", tmp_path / "a.mgc"))
    assert recipe.main(["mgcep", "--scp", str(scp), "--frame-length", "400", "--frame-shift", "80", "--fft-length", "512",
                        "--alpha", "0.42", "--order", "12"]) == 0
    assert "complete. 6 frames, 0 utterances flagged" in capsys.readouterr().out
    assert open(tmp_path / "a.mgc", "rb").read() == in_memory(gpu, waves[1])

"""recipe.mspf_stats_files and recipe.mspf_files: `make_mspf` and `postfiltering_mspf` (scripts/Training.pl:3133-3221,
:2950-3038) for file lists -- float32 rows in, the script's statistics files and float32 `.p_mgc` out -- against
tests/mspf_reference.py to float32 rounding, with and without silence removal, with --resume and through the CLI."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_mspf as gen  # noqa: E402
import mspf_reference as R  # noqa: E402

DIM, LW, N, SHIFT = 5, 15, 16, 0.005
K = N // 2 + 1


def _scp(tmp_path, name, jobs):
    path = tmp_path / name
    path.write_text("".join("%s %s\n" % (a, b if b else "-") for a, b in jobs))
    return str(path)


def _stats_files(directory, name="mgc"):
    mean = np.stack([np.fromfile(os.path.join(str(directory), "%s_dim%d.mean" % (name, d)), np.float32) for d in range(DIM)])
    std = np.stack([np.fromfile(os.path.join(str(directory), "%s_dim%d.stdd" % (name, d)), np.float32) for d in range(DIM)])
    return mean, std


def _close_f32(got, want):
    """float32 files of double results: one rounding, so within one float32 spacing of the reference's value."""
    want = np.asarray(want, np.float64)
    return got.shape == want.shape and (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()


@pytest.mark.gpu
def test_stats_and_postfilter_files(gpu, pkg, tmp_path):
    torch, W, ctx = gpu
    rng = np.random.default_rng(4)
    nat, genr, nat_jobs, gen_jobs, labels = [], [], [], [], []
    for k, T in enumerate((60, 45, 30)):
        full = gen.ar1(rng, T + 4, DIM)
        a, g = full[2:-2].astype(np.float32), gen.smooth(full).astype(np.float32)
        a.tofile(tmp_path / ("n%d.mgc" % k))
        g.tofile(tmp_path / ("g%d.mgc" % k))
        end = int(T * SHIFT * 1e7)
        lab = ["0 500001 sil", "500001 %d a" % (end // 2 + 1), "%d %d b" % (end // 2 + 1, end - 500000 + 1),
               "%d %d sil" % (end - 500000 + 1, end)]
        (tmp_path / ("u%d.lab" % k)).write_text("\n".join(lab) + "\n")
        nat.append(a.astype(np.float64))
        genr.append(g.astype(np.float64))
        labels.append(lab)
        nat_jobs.append((str(tmp_path / ("n%d.mgc" % k)), str(tmp_path / ("u%d.lab" % k))))
        gen_jobs.append((str(tmp_path / ("g%d.mgc" % k)), None))
    frames = sum(R.n_frames(len(a), LW) for a in nat)
    # without silence removal: the whole files, each with its own mean
    assert pkg.recipe.mspf_stats_files(gen_jobs, DIM, tmp_path / "gen", frame_length=LW, fft_length=N, ctx=ctx) == frames
    assert pkg.recipe.mspf_stats_files([(f, None) for f, _ in nat_jobs], DIM, tmp_path / "nat", frame_length=LW,
                                       fft_length=N, ctx=ctx) == frames
    for directory, seqs in ((tmp_path / "gen", genr), (tmp_path / "nat", nat)):
        mean, std = _stats_files(directory)
        rmean, rstd = R.finalize(*R.stats(seqs, LW, N))
        assert mean.shape == (DIM, K) and _close_f32(mean, rmean) and _close_f32(std, rstd)
    # with it: the file's mean, the kept segments butted together (both ends inclusive), through the CLI
    kept = [a[R.label_segments(lab, SHIFT, len(a), ("sil",))] for a, lab in zip(nat, labels)]
    assert all(0 < len(k_) < len(a) for k_, a in zip(kept, nat))
    assert pkg.recipe.main(["mspf-stats", "--scp", _scp(tmp_path, "nat.scp", nat_jobs), "--dim", str(DIM), "--out-dir",
                            str(tmp_path / "nat_sil"), "--silence", "sil", "--frame-length", str(LW), "--fft-length",
                            str(N)]) == 0
    mean, std = _stats_files(tmp_path / "nat_sil")
    rmean, rstd = R.finalize(*R.stats(kept, LW, N, means=[a.mean(axis=0) for a in nat]))
    assert _close_f32(mean, rmean) and _close_f32(std, rstd)
    assert not _close_f32(mean, R.finalize(*R.stats(nat, LW, N))[0])               # the silences were in the way

    # the postfilter on the generated files, from the statistics files as they were written
    jobs = [(f, str(tmp_path / ("g%d.p_mgc" % k))) for k, (f, _) in enumerate(gen_jobs)]
    total = sum(len(g) for g in genr)
    assert pkg.recipe.mspf_files(jobs, DIM, tmp_path / "gen", tmp_path / "nat", frame_length=LW, fft_length=N,
                                 ctx=ctx) == total
    tabs = _stats_files(tmp_path / "gen") + _stats_files(tmp_path / "nat")
    tabs = [t.astype(np.float64) for t in tabs]
    want = []
    for (src, dst), g in zip(jobs, genr):
        got = np.fromfile(dst, dtype=np.float32).reshape(g.shape)
        ref = R.postfilter(g, *tabs, LW, N, 1.0)
        assert _close_f32(got, ref) and np.abs(got - g).max() > 0.05
        want.append(got)
    # resume: nothing is written when every output is complete, a missing file brings its utterance back
    stamp = [os.stat(dst).st_mtime_ns for _, dst in jobs]
    assert pkg.recipe.mspf_files(jobs, DIM, tmp_path / "gen", tmp_path / "nat", frame_length=LW, fft_length=N, ctx=ctx,
                                 resume=True) == 0
    cli = ["mspf", "--scp", _scp(tmp_path, "jobs.scp", jobs), "--dim", str(DIM), "--gen-stats", str(tmp_path / "gen"),
           "--nat-stats", str(tmp_path / "nat"), "--frame-length", str(LW), "--fft-length", str(N), "--resume"]
    assert pkg.recipe.main(cli) == 0
    assert [os.stat(dst).st_mtime_ns for _, dst in jobs] == stamp
    os.remove(jobs[1][1])
    assert pkg.recipe.main(cli) == 0
    assert (np.fromfile(jobs[1][1], dtype=np.float32).reshape(want[1].shape) == want[1]).all()
    assert [os.stat(jobs[k][1]).st_mtime_ns for k in (0, 2)] == [stamp[0], stamp[2]]

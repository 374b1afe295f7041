"""recipe.ffo_files, stats_files and gv_data_files (data/Makefile.in:325-459, scripts/Training.pl:1402-1491) on three
short utterances written as stream files, against tests/ffo_reference.py, and the round trip through gen_param_files
that closes the chain."""
import os
import struct

import numpy as np
import pytest

import ffo_reference as R
import mlpg_reference as M

pytestmark = pytest.mark.gpu
MAGIC = np.float32(-1.0e10)
NAMES = ("mgc", "lf0", "bap")
DIMS = (5, 1, 3)
MSD = (False, True, False)
LENGTHS = (40, 9, 23)
STREAMS = [(d, R.RECIPE, m) for d, m in zip(DIMS, MSD)]
FS, SHIFT = 48000, 240


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """(directory, window files, features [utterance][stream], helper's ffo rows per utterance)."""
    tmp = tmp_path_factory.mktemp("ffo")
    wins = []
    for k, w in enumerate(R.RECIPE):                                  # data/win/NAME.winK: the size, then the taps
        path = tmp / ("x.win%d" % (k + 1))
        path.write_text("%d %s\n" % (len(w), " ".join(repr(v) for v in w)))
        wins.append(str(path))
    rng = np.random.default_rng(17)
    feats = []
    for u, T in enumerate(LENGTHS):
        fs = [M.random_walk(rng, T, d) for d in DIMS]
        fs[1] = (fs[1] * np.float32(0.1) + np.float32(5.0)).astype(np.float32)
        fs[1][rng.random((T, 1)) < 0.4] = MAGIC
        fs[1][:2] = MAGIC                                             # a leading and a trailing gap in every utterance
        fs[1][T - 1] = MAGIC
        fs[1][3] = np.float32(5.25)
        for name, a in zip(NAMES, fs):
            a.tofile(tmp / ("u%d.%s" % (u, name)))
        feats.append(fs)
    rows = [R.ffo_rows(fs, STREAMS)[0] for fs in feats]
    return tmp, wins, feats, rows


def ffo_jobs(tmp, tag="ffo"):
    return [tuple(str(tmp / ("u%d.%s" % (u, e))) for e in NAMES + (tag,)) for u in range(len(LENGTHS))]


def same_bits(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


def within_one_spacing(got, ref):
    """float32 `got` against long-double `ref`: at most one float32 spacing of the reference apart."""
    ref32 = ref.astype(np.float32)
    return (np.abs(got.astype(R.LD) - ref) <= np.spacing(np.abs(ref32)).astype(R.LD)).all()


def test_ffo_files_against_helper(gpu, pkg, corpus):
    torch, W, ctx = gpu
    tmp, wins, feats, rows = corpus
    streams = [(d, wins, m) for d, m in zip(DIMS, MSD)]
    jobs = ffo_jobs(tmp)
    width = pkg.recipe.ffo_layout(STREAMS)[1]
    assert pkg.recipe.ffo_files(jobs, streams, ctx=ctx) == sum(LENGTHS)
    for job, want in zip(jobs, rows):
        assert same_bits(np.fromfile(job[-1], dtype=np.float32).reshape(-1, width), want), job[-1]
    # resume: complete files are skipped, a short one brings its utterance back
    assert pkg.recipe.ffo_files(jobs, streams, ctx=ctx, resume=True) == 0
    rows[1][:4].tofile(jobs[1][-1])
    assert pkg.recipe.ffo_files(jobs, streams, ctx=ctx, resume=True) == LENGTHS[1]
    assert same_bits(np.fromfile(jobs[1][-1], dtype=np.float32).reshape(-1, width), rows[1])
    # coefficient lists in the place of window files; two batches
    again = ffo_jobs(tmp, "ffo2")
    assert pkg.recipe.ffo_files(again, STREAMS, ctx=ctx, max_batch_frames=45) == sum(LENGTHS)
    for job, want in zip(again, rows):
        assert same_bits(np.fromfile(job[-1], dtype=np.float32).reshape(-1, width), want)


def test_ffo_cli_and_an_utterance_without_a_voiced_frame(gpu, pkg, corpus, tmp_path, capsys):
    tmp, wins, feats, rows = corpus
    width = pkg.recipe.ffo_layout(STREAMS)[1]
    jobs = [j[:-1] + (str(tmp_path / os.path.basename(j[-1])),) for j in ffo_jobs(tmp)]
    dead = tuple(str(tmp_path / ("dead.%s" % e)) for e in NAMES + ("ffo",))
    for path, d in zip(dead, DIMS):
        np.full((6, d), MAGIC if d == 1 else 1.0, dtype=np.float32).tofile(path)
    scp = tmp_path / "ffo.scp"
    scp.write_text("".join(" ".join(j) + "\n" for j in jobs + [dead]))
    argv = ["ffo", "--scp", str(scp)]
    for d, m in zip(DIMS, MSD):
        argv += ["--stream", "%d:%d:%s" % (d, m, ",".join(wins))]
    assert pkg.recipe.main(argv) == 0
    io = capsys.readouterr()
    assert "complete. %d frames" % (sum(LENGTHS) + 6) in io.out
    assert "dead.mgc" in io.err and "no valid value" in io.err and not os.path.exists(dead[-1])
    for job, want in zip(jobs, rows):
        assert same_bits(np.fromfile(job[-1], dtype=np.float32).reshape(-1, width), want)
    assert pkg.recipe.main(argv + ["--resume"]) == 0
    assert "complete. 6 frames" in capsys.readouterr().out           # only the one that is never written comes back


def test_stats_files_against_helper(gpu, pkg, corpus, tmp_path):
    torch, W, ctx = gpu
    tmp, wins, feats, rows = corpus
    layout, width = pkg.recipe.ffo_layout(STREAMS)
    paths = []
    for u, r in enumerate(rows):
        paths.append(str(tmp_path / ("u%d.ffo" % u)))
        r.tofile(paths[-1])
    out = tmp_path / "stats"
    assert pkg.recipe.stats_files(paths, STREAMS, str(out), names=NAMES, ctx=ctx) == sum(LENGTHS)
    var = np.fromfile(out / "ffo.var", dtype=np.float32)
    assert var.shape == (width,) and within_one_spacing(var, R.corpus_variance(rows))
    for name, (_, c0, n) in zip(NAMES, layout):
        assert same_bits(np.fromfile(out / (name + ".var"), dtype=np.float32), var[c0:c0 + n]), name
    gv = R.gv(rows)
    want = np.concatenate([gv[c0:c0 + d] for (_, c0, _), d in zip(layout, DIMS)])
    got = np.fromfile(out / "gv.var", dtype=np.float32)
    assert got.shape == (sum(DIMS),) and within_one_spacing(got, want)
    # the same files whatever the batches, and through the command line
    out2 = tmp_path / "stats2"
    assert pkg.recipe.stats_files(paths[::-1], STREAMS, str(out2), names=NAMES, ctx=ctx, max_batch_frames=45) == sum(LENGTHS)
    assert within_one_spacing(np.fromfile(out2 / "ffo.var", dtype=np.float32), R.corpus_variance(rows))
    scp = tmp_path / "stats.scp"
    scp.write_text("".join(p + "\n" for p in paths))
    argv = ["stats", "--scp", str(scp), "--out-dir", str(tmp_path / "stats3")]
    for d, m, n in zip(DIMS, MSD, NAMES):
        argv += ["--stream", "%d:%d:%s" % (d, m, ",".join(wins)), "--name", n]
    assert pkg.recipe.main(argv) == 0
    for f in ("ffo.var", "mgc.var", "lf0.var", "bap.var", "gv.var"):
        assert (tmp_path / "stats3" / f).read_bytes() == (out / f).read_bytes(), f


def gv_row(feats_u, keep):
    out = []
    for x, msd in zip(feats_u, MSD):
        cnt, _, m2 = R.moments(x[keep], -1e10 if msd else None)
        assert (cnt > 0).all()
        out.append(m2 / cnt.astype(R.LD))
    return np.concatenate(out)


def test_gv_data_files_against_helper(gpu, pkg, corpus, tmp_path, capsys):
    torch, W, ctx = gpu
    tmp, wins, feats, rows = corpus
    labels, jobs = [], []
    for u, T in enumerate(LENGTHS):
        end = T * 50000                                               # 5 ms frames in 100 ns units
        a, b = (end // 4 // 50000) * 50000, (3 * end // 4 // 50000) * 50000
        lab = tmp_path / ("u%d.lab" % u)
        lab.write_text("0 %d pau\n%d %d a\n%d %d sil\n" % (a, a, b, b, end))
        labels.append(str(lab))
        jobs.append(tuple(str(tmp / ("u%d.%s" % (u, e))) for e in NAMES) + (str(lab), str(tmp_path / ("u%d.cmp" % u))))
    head = struct.pack("<iihh", 1, 50000, 4 * sum(DIMS), 9)
    assert head == W.htk_header(1, FS, SHIFT, 4 * sum(DIMS), 9)

    def check(silences):
        for u, job in enumerate(jobs):
            raw = open(job[-1], "rb").read()
            assert raw[:12] == head and len(raw) == 12 + 4 * sum(DIMS)
            keep = np.arange(LENGTHS[u])
            if silences:
                with open(labels[u]) as f:
                    keep = pkg.recipe.mspf_label_rows(f.readlines(), SHIFT / FS, LENGTHS[u], silences)
                assert 0 < len(keep) < LENGTHS[u]
            assert within_one_spacing(np.frombuffer(raw[12:], dtype=np.float32), gv_row(feats[u], keep)), (u, silences)

    assert pkg.recipe.gv_data_files(jobs, STREAMS, FS, SHIFT, ctx=ctx) == [j[-1] for j in jobs]
    check(())
    assert pkg.recipe.gv_data_files(jobs, STREAMS, FS, SHIFT, silences=("pau", "sil"), ctx=ctx,
                                    max_batch_frames=45) == [j[-1] for j in jobs]
    check(("pau", "sil"))
    # an utterance whose msd stream keeps no value is reported and left out of the list; so is one that is all silence
    dead = tuple(str(tmp_path / ("dead.%s" % e)) for e in NAMES)
    for path, d in zip(dead, DIMS):
        np.full((6, d), MAGIC if d == 1 else 1.0, dtype=np.float32).tofile(path)
    mute = tmp_path / "mute.lab"
    mute.write_text("0 %d pau\n" % (LENGTHS[0] * 50000))
    extra = [dead + (None, str(tmp_path / "dead.cmp")), jobs[0][:3] + (str(mute), str(tmp_path / "mute.cmp"))]
    capsys.readouterr()
    done = pkg.recipe.gv_data_files(jobs[:1] + extra, STREAMS, FS, SHIFT, silences=("pau", "sil"), ctx=ctx)
    err = capsys.readouterr().err
    assert done == [jobs[0][-1]] and "dead.mgc" in err and "a column without values" in err and "silences" in err
    assert not os.path.exists(extra[0][-1]) and not os.path.exists(extra[1][-1])
    # the command line prints the list
    scp = tmp_path / "gv.scp"
    scp.write_text("".join(" ".join(j) + "\n" for j in jobs))
    argv = ["gv-data", "--scp", str(scp), "--sampling-rate", str(FS), "--frame-shift", str(SHIFT), "--silence", "pau",
            "--silence", "sil"]
    for d, m in zip(DIMS, MSD):
        argv += ["--stream", "%d:%d:" % (d, m)]
    assert pkg.recipe.main(argv) == 0
    assert capsys.readouterr().out.split() == [j[-1] for j in jobs]
    check(("pau", "sil"))


def test_round_trip_through_gen_param(gpu, pkg, corpus, tmp_path):
    """ffo_files -> stats_files -> gen_param_files(var_path=ffo.var, edge=1) returns the features: every static stream
    within the helper's own round-trip error on the same rows plus one float32 spacing (the bound of
    tests/test_gpu_mlpg.py's round trip), lf0 exactly unvoiced_value at the unvoiced frames and the original within
    the same bound at the voiced ones."""
    torch, W, ctx = gpu
    tmp, wins, feats, rows = corpus
    layout, width = pkg.recipe.ffo_layout(STREAMS)
    streams = [(d, wins, m) for d, m in zip(DIMS, MSD)]
    jobs = [j[:-1] + (str(tmp_path / os.path.basename(j[-1])),) for j in ffo_jobs(tmp)]
    assert pkg.recipe.ffo_files(jobs, streams, ctx=ctx) == sum(LENGTHS)
    ffos = [j[-1] for j in jobs]
    assert pkg.recipe.stats_files(ffos, streams, str(tmp_path / "stats"), names=NAMES, ctx=ctx) == sum(LENGTHS)
    var_path = str(tmp_path / "stats" / "ffo.var")
    var = np.fromfile(var_path, dtype=np.float32)
    back = [(f,) + tuple(str(tmp_path / ("u%d.gen.%s" % (u, e))) for e in NAMES) for u, f in enumerate(ffos)]
    assert pkg.recipe.gen_param_files(back, streams, var_path, edge=1, ctx=ctx) == sum(LENGTHS)
    worst = 0.0
    for u, job in enumerate(back):
        r = np.fromfile(job[0], dtype=np.float32).reshape(-1, width)
        for path, (mcol, c0, n), d, x in zip(job[1:], layout, DIMS, feats[u]):
            got = np.fromfile(path, dtype=np.float32).reshape(-1, d)
            voiced = np.ones(len(x), bool) if mcol is None else x[:, 0] != MAGIC
            assert (got[~voiced] == MAGIC).all() and (~voiced).sum() == (0 if mcol is None else (x[:, 0] == MAGIC).sum())
            helper, _ = M.mlpg(r[:, c0:c0 + n], var[c0:c0 + n], R.RECIPE, edge=1, want_cond=False)
            target = x if mcol is None else R.interpolate(x)[0]
            xs = target.astype(np.float64)
            tol = np.abs(helper - xs).max(axis=0) + np.spacing(np.abs(target).max(axis=0)).astype(np.float64)
            err = np.abs(got.astype(np.float64) - x.astype(np.float64))[voiced].max(axis=0)
            worst = max(worst, float((err / tol).max()))
            assert (err <= tol).all(), (path, float((err / tol).max()))
    print("round trip: worst err / (helper's error + one spacing) %.3f" % worst)

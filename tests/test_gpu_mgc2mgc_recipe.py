"""recipe.mgc2mgc_files / `recipe mgc2mgc`, SPTK's mgc2mgc for a file list: float32 [T][m1+1] in, float32 [T][m2+1] out,
equal to the library's float64 result on the widened rows, rounded once; resumable; split between ranks."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORDER, ALPHA, C, OUT_ORDER, OUT_ALPHA, OUT_GAMMA = 24, 0.55, 3, 30, 0.42, -0.5
LENGTHS = (5, 40, 1)


def corpus(tmp_path):
    rng = np.random.default_rng(11)
    jobs, rows = [], []
    for k, T in enumerate(LENGTHS):
        r = (rng.standard_normal((T, ORDER + 1)) / (1.0 + np.arange(ORDER + 1))).astype(np.float32)
        r[:, 0] = rng.uniform(-1.0, 1.0, T).astype(np.float32)          # 1 - c0 / 3 > 0
        r.tofile(tmp_path / ("u%d.mgc" % k))
        rows.append(r)
        jobs.append((str(tmp_path / ("u%d.mgc" % k)), str(tmp_path / ("u%d.out" % k))))
    return jobs, rows


def scp(tmp_path, jobs):
    path = tmp_path / "jobs.scp"
    path.write_text("".join("%s %s\n" % j for j in jobs))
    return str(path)


def stamps(jobs):
    return [os.stat(dst).st_mtime_ns if os.path.exists(dst) else None for _, dst in jobs]


def test_mgc2mgc_files_resume_and_ranks(gpu, pkg, tmp_path, monkeypatch):
    torch, W, ctx = gpu
    rec = pkg.recipe
    jobs, rows = corpus(tmp_path)
    gamma = rec.sptk_gamma(c=C)
    assert gamma == -1.0 / 3.0 and rec.sptk_gamma(g=0.25) == 0.25 and rec.sptk_gamma() == 0.0
    args = (ORDER, ALPHA, gamma, OUT_ORDER, OUT_ALPHA, OUT_GAMMA)
    assert rec.mgc2mgc_files(jobs, *args, ctx=ctx) == sum(LENGTHS)
    b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=list(LENGTHS))
    try:
        out, st = b.convert_mel_generalized_cepstrum(torch.from_numpy(np.concatenate(rows).astype(np.float64)).cuda(),
                                                     ALPHA, gamma, OUT_ORDER, OUT_ALPHA, OUT_GAMMA)
        want = b.split_frames(out.cpu().numpy().astype(np.float32))
        assert (st.cpu().numpy() == 0).all()
    finally:
        b.close()
    for (src, dst), r, w in zip(jobs, rows, want):
        assert os.path.getsize(dst) == 4 * len(r) * (OUT_ORDER + 1)
        with open(dst, "rb") as f:
            assert f.read() == np.ascontiguousarray(w).tobytes() and np.abs(w).max() > 0
    # resume: nothing is written when every output is complete, a missing file brings its utterance back
    stamp = stamps(jobs)
    assert rec.mgc2mgc_files(jobs, *args, ctx=ctx, resume=True) == 0
    assert stamps(jobs) == stamp
    cli = ["mgc2mgc", "--scp", scp(tmp_path, jobs), "-m", str(ORDER), "-a", str(ALPHA), "-c", str(C), "-M", str(OUT_ORDER),
           "-A", str(OUT_ALPHA), "-G", str(OUT_GAMMA)]
    assert rec.main(cli + ["--resume"]) == 0
    assert stamps(jobs) == stamp
    os.remove(jobs[1][1])
    assert rec.mgc2mgc_files(jobs, *args, ctx=ctx, resume=True) == LENGTHS[1]
    with open(jobs[1][1], "rb") as f:
        assert f.read() == np.ascontiguousarray(want[1]).tobytes()
    # the command line without --resume writes every file again, the same bytes
    for _, dst in jobs:
        os.remove(dst)
    assert rec.main(cli) == 0
    for (_, dst), w in zip(jobs, want):
        with open(dst, "rb") as f:
            assert f.read() == np.ascontiguousarray(w).tobytes()
    # two ranks split the list: each writes its share, together every file, the same bytes
    for _, dst in jobs:
        os.remove(dst)
    monkeypatch.setenv("WORLD_SIZE", "2")
    done = []
    for rank in (0, 1):
        monkeypatch.setenv("RANK", str(rank))
        n = rec.mgc2mgc_files(jobs, *args, ctx=ctx)
        mine = [i for i, s in enumerate(stamps(jobs)) if s is not None and i not in [j for d in done for j in d]]
        assert n == sum(LENGTHS[i] for i in mine) and mine
        done.append(mine)
    assert sorted(done[0] + done[1]) == [0, 1, 2]
    for (_, dst), w in zip(jobs, want):
        with open(dst, "rb") as f:
            assert f.read() == np.ascontiguousarray(w).tobytes()


def test_flags_and_refusals_of_the_command_line(gpu, pkg, tmp_path):
    torch, W, ctx = gpu
    rec = pkg.recipe
    jobs, rows = corpus(tmp_path)
    gamma = -1.0 / C
    # -N -U out, fed back with -n -u: the rows return (float32 files: to float32's precision)
    mid = [(src, str(tmp_path / ("u%d.norm" % k))) for k, (src, _) in enumerate(jobs)]
    back = [(m[1], j[1]) for m, j in zip(mid, jobs)]
    assert rec.main(["mgc2mgc", "--scp", scp(tmp_path, mid), "-m", str(ORDER), "-a", str(ALPHA), "-c", str(C), "-M", str(ORDER),
                     "-A", str(ALPHA), "-C", str(C), "-N", "-U"]) == 0
    assert rec.main(["mgc2mgc", "--scp", scp(tmp_path, back), "-m", str(ORDER), "-a", str(ALPHA), "-c", str(C), "-n", "-u",
                     "-M", str(ORDER), "-A", str(ALPHA), "-C", str(C)]) == 0
    for (_, dst), r in zip(back, rows):
        got = np.fromfile(dst, dtype=np.float32).reshape(r.shape)
        assert np.abs(got - r).max() < 1e-5
    for bad in (dict(order=64, out_order=64), dict(alpha=1.0), dict(out_gamma=1.5), dict(gamma=0.0, multiplied=True),
                dict(out_gamma=0.0, out_multiplied=True)):
        kw = dict(order=ORDER, alpha=ALPHA, gamma=gamma, out_order=ORDER, out_alpha=ALPHA, out_gamma=gamma)
        kw.update(bad)
        with pytest.raises(ValueError):
            rec.mgc2mgc_files(jobs, ctx=ctx, **kw)
    with pytest.raises(ValueError):
        rec.sptk_gamma(g=-0.5, c=2)

"""recipe.postfilter_files, `postfiltering_mcp` (scripts/Training.pl:2642-2687) for a file list: float32 `.mgc` in,
float32 `.p_mgc` out, equal to the library's float64 result on the widened rows, rounded once."""
import os

import numpy as np
import pytest


@pytest.mark.gpu
def test_postfilter_files_and_resume(gpu, pkg, tmp_path):
    torch, W, ctx = gpu
    order, alpha, beta, length = 24, 0.42, 1.4, 512
    rng = np.random.default_rng(3)
    jobs, rows = [], []
    for k, T in enumerate((5, 40, 1)):
        r = (rng.standard_normal((T, order + 1)) / (1.0 + np.arange(order + 1))).astype(np.float32)
        r.tofile(tmp_path / ("u%d.mgc" % k))
        rows.append(r)
        jobs.append((str(tmp_path / ("u%d.mgc" % k)), str(tmp_path / ("u%d.p_mgc" % k))))
    assert pkg.recipe.postfilter_files(jobs, order, alpha, beta, length, ctx=ctx) == 46
    b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=[len(r) for r in rows])
    try:
        out, st = b.postfilter_mel_cepstrum(torch.from_numpy(np.concatenate(rows).astype(np.float64)).cuda(), alpha,
                                            beta, length)
        want = b.split_frames(out.cpu().numpy().astype(np.float32))
        assert (st.cpu().numpy() == 0).all()
    finally:
        b.close()
    for (src, dst), r, w in zip(jobs, rows, want):
        assert os.path.getsize(dst) == os.path.getsize(src)
        got = np.fromfile(dst, dtype=np.float32).reshape(r.shape)
        assert (got == w).all() and (got[:, 1] == r[:, 1]).all() and (got[:, 0] != r[:, 0]).all()
    # resume: nothing is written when every output is complete, a missing file brings its utterance back
    stamp = [os.stat(dst).st_mtime_ns for _, dst in jobs]
    assert pkg.recipe.postfilter_files(jobs, order, alpha, beta, length, ctx=ctx, resume=True) == 0
    assert [os.stat(dst).st_mtime_ns for _, dst in jobs] == stamp
    assert pkg.recipe.main(["postfilter", "--scp", _scp(tmp_path, jobs), "--order", str(order), "--alpha", str(alpha),
                            "--length", str(length), "--resume"]) == 0
    assert [os.stat(dst).st_mtime_ns for _, dst in jobs] == stamp
    os.remove(jobs[1][1])
    assert pkg.recipe.postfilter_files(jobs, order, alpha, beta, length, ctx=ctx, resume=True) == 40
    assert (np.fromfile(jobs[1][1], dtype=np.float32).reshape(rows[1].shape) == want[1]).all()


def _scp(tmp_path, jobs):
    path = tmp_path / "jobs.scp"
    path.write_text("".join("%s %s\n" % j for j in jobs))
    return str(path)

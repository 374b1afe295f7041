"""recipe.lsp2mgc_files / `recipe lsp2mgc` and recipe.postfilter_lsp_files / `recipe postfilter-lsp` on three short files
of MGC-LSP rows: float32 in, float32 out, equal to the float32 rounding of lsp.py's calls on the widened rows; a resumed
run rewrites nothing."""
import importlib
import os

import numpy as np
import pytest

import lsp_reference as L

pytestmark = pytest.mark.gpu

ORDER, ALPHA, GAMMA = 34, 0.55, -1.0 / 3.0
LENGTHS = (5, 40, 1)


def corpus(tmp_path, ext):
    jobs, rows = [], []
    for k, T in enumerate(LENGTHS):
        r, _ = L.rows(ORDER, T, 50 + k, log_gain=True)
        r = r.astype(np.float32)
        r.tofile(tmp_path / ("u%d.mgc" % k))
        rows.append(r)
        jobs.append((str(tmp_path / ("u%d.mgc" % k)), str(tmp_path / ("u%d.%s" % (k, ext)))))
    return jobs, rows


def scp(tmp_path, jobs):
    path = tmp_path / "jobs.scp"
    path.write_text("".join("%s %s\n" % j for j in jobs))
    return str(path)


def stamps(jobs):
    return [os.stat(dst).st_mtime_ns if os.path.exists(dst) else None for _, dst in jobs]


def written(jobs, want):
    for (_, dst), w in zip(jobs, want):
        with open(dst, "rb") as f:
            if f.read() != np.ascontiguousarray(w).tobytes():
                return False
    return True


def run_stage(gpu, pkg, tmp_path, ext, files, cli, call, width):
    torch, W, ctx = gpu
    rec = pkg.recipe
    lsp = importlib.import_module(pkg.__name__ + ".lsp")
    jobs, rows = corpus(tmp_path, ext)
    assert files(rec, jobs, ctx=ctx) == sum(LENGTHS)
    b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=list(LENGTHS))
    try:
        out, st = call(lsp, b, torch.from_numpy(np.concatenate(rows).astype(np.float64)).cuda())
        want = b.split_frames(out.cpu().numpy().astype(np.float32))
        st = st.cpu().numpy()
    finally:
        b.close()
    assert ((st & 12) != 0).sum() == 1                                     # the 40-row file's NaN row
    assert all(w.shape == (T, width) for w, T in zip(want, LENGTHS)) and written(jobs, want)
    assert np.abs(want[0]).max() > 0
    # resume: nothing is written when every output is complete; a missing file brings its utterance back
    stamp = stamps(jobs)
    assert files(rec, jobs, ctx=ctx, resume=True) == 0 and stamps(jobs) == stamp
    argv = cli(scp(tmp_path, jobs))
    assert rec.main(argv + ["--resume"]) == 0 and stamps(jobs) == stamp
    os.remove(jobs[1][1])
    assert files(rec, jobs, ctx=ctx, resume=True) == LENGTHS[1] and written(jobs, want)
    # the command line without --resume writes every file again, the same bytes
    for _, dst in jobs:
        os.remove(dst)
    assert rec.main(argv) == 0 and written(jobs, want)


def test_lsp2mgc_files(gpu, pkg, tmp_path):
    run_stage(gpu, pkg, tmp_path, "c_mgc",
              lambda rec, jobs, **kw: rec.lsp2mgc_files(jobs, ORDER, ALPHA, GAMMA, log_gain=True, **kw),
              lambda path: ["lsp2mgc", "--scp", path, "--order", str(ORDER), "--alpha", str(ALPHA), "--gamma", repr(GAMMA),
                            "--log-gain"],
              lambda lsp, b, rows: lsp.lsp_to_mel_generalized_cepstrum(b, rows, ALPHA, GAMMA, log_gain=True), ORDER + 1)


def test_lsp2mgc_files_towards_another_set(gpu, pkg, tmp_path):
    run_stage(gpu, pkg, tmp_path, "c_mgc",
              lambda rec, jobs, **kw: rec.lsp2mgc_files(jobs, ORDER, ALPHA, GAMMA, True, 40, 0.42, 0.0, **kw),
              lambda path: ["lsp2mgc", "--scp", path, "--order", str(ORDER), "--alpha", str(ALPHA), "--gamma", repr(GAMMA),
                            "--log-gain", "--out-order", "40", "--out-alpha", "0.42", "--out-gamma", "0"],
              lambda lsp, b, rows: lsp.lsp_to_mel_generalized_cepstrum(b, rows, ALPHA, GAMMA, 40, 0.42, 0.0, True), 41)


@pytest.mark.parametrize("compensate", [False, True])
def test_postfilter_lsp_files(gpu, pkg, tmp_path, compensate):
    run_stage(gpu, pkg, tmp_path, "p_mgc",
              lambda rec, jobs, **kw: rec.postfilter_lsp_files(jobs, ORDER, ALPHA, GAMMA, 0.7, 256, True, compensate, **kw),
              lambda path: ["postfilter-lsp", "--scp", path, "--order", str(ORDER), "--alpha", str(ALPHA), "--gamma",
                            repr(GAMMA), "--log-gain", "--beta", "0.7", "--length", "256"] + (["--compensate"] if compensate else []),
              lambda lsp, b, rows: lsp.postfilter_lsp(b, rows, ALPHA, GAMMA, 0.7, 256, compensate, True), ORDER + 1)

"""recipe.gen_param_files, `gen_param` (scripts/Training.pl:2755-2810) for a file list: the row layout and the size
check on the CPU, the files it writes against tests/mlpg_reference.py on the GPU."""
import os

import numpy as np
import pytest

import mlpg_reference as ref

# the recipe's streams in an ffo row: mgc, lf0 behind its voicing column, bap (small dims: the layout is the point)
STREAMS = [(4, ref.RECIPE, False), (1, ref.RECIPE, True), (3, ref.RECIPE, False)]


def test_ffo_layout(pkg):
    layout, width = pkg.recipe.ffo_layout(STREAMS)
    assert layout == [(None, 0, 12), (12, 13, 3), (None, 16, 9)] and width == 25
    assert pkg.recipe.ffo_layout([(1, ref.STATIC, True)]) == ([(0, 1, 1)], 2)
    assert pkg.recipe.parse_stream("1:1:a.win1,a.win2") == (1, ["a.win1", "a.win2"], True)
    assert pkg.recipe.parse_stream("50:0:m.win1") == (50, ["m.win1"], False)


def test_size_check_behind_resume(pkg, tmp_path):
    job = [str(tmp_path / n) for n in ("a.ffo", "a.mgc", "a.lf0", "a.bap")]
    done = lambda: pkg.recipe.gen_param_complete(job, 7, STREAMS)
    assert not done()                                             # nothing written yet
    for p, (dim, _, _) in zip(job[1:], STREAMS):
        np.zeros((7, dim), dtype=np.float32).tofile(p)
    assert done()
    np.zeros((6, 3), dtype=np.float32).tofile(job[3])             # a file cut short
    assert not done()
    os.remove(job[2])
    assert not done()


def test_window_file_drops_its_leading_size(pkg, tmp_path):
    p = tmp_path / "lf0.win2"
    p.write_text("3 -0.5 0.0 0.5\n")
    assert pkg.recipe.read_window(p) == [-0.5, 0.0, 0.5]


@pytest.mark.gpu
def test_gen_param_files_against_helper(gpu, pkg, tmp_path):
    torch, W, ctx = gpu
    layout, width = pkg.recipe.ffo_layout(STREAMS)
    wins = []
    for k, w in enumerate(ref.RECIPE):                            # data/win/NAME.winK: the size, then the taps
        path = tmp_path / ("x.win%d" % (k + 1))
        path.write_text("%d %s\n" % (len(w), " ".join(repr(v) for v in w)))
        wins.append(str(path))
    streams = [(d, wins, m) for d, _, m in STREAMS]
    rng = np.random.default_rng(5)
    var = (10.0 ** rng.uniform(-3, 3, width)).astype(np.float32)
    var.tofile(tmp_path / "global.var")
    jobs, rows = [], []
    for k, T in enumerate((5, 40, 1)):
        r = np.zeros((T, width), dtype=np.float32)
        for s, ((mcol, c0, n), (dim, w, _)) in enumerate(zip(layout, STREAMS)):
            r[:, c0:c0 + n] = ref.make_stream(100 * k + s, [T], dim, w)[0]
            if mcol is not None:
                r[:, mcol] = rng.uniform(0, 1, T).astype(np.float32)
        r.tofile(tmp_path / ("u%d.ffo" % k))
        rows.append(r)
        jobs.append(tuple(str(tmp_path / ("u%d.%s" % (k, e))) for e in ("ffo", "mgc", "lf0", "bap")))
    assert pkg.recipe.gen_param_files(jobs, streams, str(tmp_path / "global.var"), ctx=ctx) == 46
    for job, r in zip(jobs, rows):
        assert pkg.recipe.gen_param_complete(job, len(r), STREAMS)
        for path, (mcol, c0, n), (dim, w, _) in zip(job[1:], layout, STREAMS):
            got = np.fromfile(path, dtype=np.float32).reshape(len(r), dim)
            c, cond = ref.mlpg(r[:, c0:c0 + n], var[c0:c0 + n], w)
            voiced = np.ones(len(r), bool) if mcol is None else r[:, mcol] >= np.float32(0.5)
            assert (got[~voiced] == np.float32(-1e10)).all()
            err = np.abs(got.astype(np.float64) - c)[voiced]
            assert (err <= ref.bound(c, cond)[None]).all(), (path, float(err.max()))
    # resume: complete utterances are skipped, a missing file brings its utterance back
    os.remove(jobs[1][2])
    assert pkg.recipe.gen_param_files(jobs, streams, str(tmp_path / "global.var"), ctx=ctx, resume=True) == 40
    assert pkg.recipe.gen_param_complete(jobs[1], 40, STREAMS)

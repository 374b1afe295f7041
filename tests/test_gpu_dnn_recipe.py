"""recipe.forward_files (the `dnn-forward` verb: DNNSynthesis.py frame by frame) on five utterances of 1 - 40 frames in a
temp dir: the files equal acoustic_model_forward's rows bit for bit, `.var` is the speaker's variance row, the printed
cost is the batch call's, and the outputs feed gen_param_files unchanged."""
import os
import re

import numpy as np
import pytest

import dnn_reference as R
import mlpg_reference as M

pytestmark = pytest.mark.gpu

LENGTHS = (1, 7, 40, 33, 16)
STREAMS = ((50, False), (1, True), (25, False))        # the recipe's ffo row: 229 columns


def test_forward_files(gpu, pkg, tmp_path, capsys):
    torch, W, ctx = gpu
    params, x, _, ref, _ = R.cached_case(0, "sat", "sigmoid", "linear", LENGTHS)
    m = pkg.training.AcousticModel(37, [48, 130], 229, R.N_SPKRS, "sigmoid", "linear")
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
    model_path = str(tmp_path / "model.npz")
    m.save(model_path)
    rng = np.random.default_rng(3)
    obs = (ref + rng.standard_normal(ref.shape)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    jobs = []
    for u in range(len(LENGTHS)):
        ffi, ffo = str(tmp_path / ("utt%d.ffi" % u)), str(tmp_path / ("utt%d.ffo" % u))
        x[off[u]:off[u + 1]].tofile(ffi)
        obs[off[u]:off[u + 1]].tofile(ffo)
        jobs.append((ffi, ffo if u % 2 == 0 else None))                  # utterances 1 and 3 have no targets
    out_dir = str(tmp_path / "gen")
    spkr = 1
    costs = pkg.recipe.forward_files(jobs, model_path, out_dir, spkr=spkr, ctx=ctx)
    printed = capsys.readouterr().out

    b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=list(LENGTHS))
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    want, want_cost, status = m.cuda().infer(b, dev(x), [spkr] * len(LENGTHS), dev(obs))
    want, want_cost = want.cpu().numpy(), want_cost.cpu().numpy()
    assert int(status.abs().sum()) == 0
    b.close()
    for u in range(len(LENGTHS)):
        rows = np.fromfile(os.path.join(out_dir, "utt%d.ffo" % u), dtype=np.float32)
        assert rows.tobytes() == want[off[u]:off[u + 1]].tobytes(), u
        var = np.fromfile(os.path.join(out_dir, "utt%d.var" % u), dtype=np.float32)
        assert var.tobytes() == params["variance.variances"][spkr].tobytes()
        if u % 2 == 0:
            assert costs[u] == want_cost[u]
            line = [ln for ln in printed.splitlines() if "utt%d.ffi" % u in ln]
            assert len(line) == 1 and re.match(r"\s+Evaluation: cost = (\S+) \(", line[0]).group(1) == "%e" % want_cost[u]
        else:
            assert costs[u] is None and "utt%d.ffi" % u not in printed

    # the way on: gen_param_files reads the written means and the written variance row as they are
    streams = [(dim, M.RECIPE, msd) for dim, msd in STREAMS]
    gen = [(os.path.join(out_dir, "utt%d.ffo" % u),) + tuple(str(tmp_path / ("utt%d.%s" % (u, n))) for n in ("mgc", "lf0", "bap"))
           for u in range(len(LENGTHS))]
    n = pkg.recipe.gen_param_files(gen, streams, os.path.join(out_dir, "utt0.var"), ctx=ctx)
    assert n == sum(LENGTHS)
    for u, T in enumerate(LENGTHS):
        for name, dim in (("mgc", 50), ("lf0", 1), ("bap", 25)):
            got = np.fromfile(str(tmp_path / ("utt%d.%s" % (u, name))), dtype=np.float32)
            assert got.size == T * dim
    mgc = np.fromfile(str(tmp_path / "utt2.mgc"), dtype=np.float32).reshape(40, 50).astype(np.float64)
    c, cond = M.mlpg(want[off[2]:off[3], :150], params["variance.variances"][spkr][:150], M.RECIPE, 0)
    assert (np.abs(mgc - c) <= M.bound(c, cond)[None, :]).all()

"""recipe.gen_param_gv_files / `gen-param-gv` against WorldBatch.parameter_generation_gv in memory (which
tests/test_gpu_mlpg_gv.py holds to the numpy reference), its resume rule, and generate's ("gv", ...) choice against the
staged gen-param-gv + synth pair, byte for byte, on the small world of tests/generate_setup.py."""
import os

import numpy as np
import pytest

import generate_setup as GS
import mlpg_reference as M

pytestmark = pytest.mark.gpu

STREAMS = [(4, M.RECIPE, False), (1, M.RECIPE, True), (3, M.RECIPE, False)]
LENGTHS = (5, 40, 1)
OPTIONS = dict(max_iter=7, epsilon=0.0, step_init=0.8)


def read(path):
    with open(path, "rb") as f:
        return f.read()


def write_case(pkg, root):
    """ffo files, the variance row, gv.mean / gv.var and labels with a silence at each end.  Returns (jobs, rows, var,
    gv_mean, gv_var, label lines per utterance)."""
    layout, width = pkg.recipe.ffo_layout(STREAMS)
    rng = np.random.default_rng(12)
    var = (10.0 ** rng.uniform(-2, 2, width)).astype(np.float32)
    var.tofile(root / "global.var")
    gm = rng.uniform(0.5, 3.0, 8).astype(np.float32)
    gm.tofile(root / "gv.mean")
    gvar = ((0.2 * gm) ** 2).astype(np.float32)
    gvar.tofile(root / "gv.var")
    os.makedirs(str(root / "lab"), exist_ok=True)
    jobs, rows, labels = [], [], []
    for k, T in enumerate(LENGTHS):
        r = np.zeros((T, width), dtype=np.float32)
        for s, ((mcol, c0, n), (dim, w, _)) in enumerate(zip(layout, STREAMS)):
            r[:, c0:c0 + n] = M.make_stream(300 * k + s, [T], dim, w)[0]
            if mcol is not None:
                r[:, mcol] = rng.uniform(0.3, 1, T).astype(np.float32)
        r.tofile(root / ("u%d.ffo" % k))
        rows.append(r)
        cut = max(T // 4, 0)
        lines = ["%d %d x-sil+a\n" % (0, cut * 50000 + 25000), "%d %d sil-a+b\n" % (cut * 50000 + 25000, (T - cut) * 50000 - 25000),
                 "%d %d b-sil+x\n" % ((T - cut) * 50000 - 25000, T * 50000)] if T > 1 else ["0 50000 x-sil+a\n"]
        with open(str(root / "lab" / ("u%d.lab" % k)), "w") as f:
            f.writelines(lines)
        labels.append(lines)
        jobs.append(tuple(str(root / ("u%d.%s" % (k, e))) for e in ("ffo", "mgc", "lf0", "bap")))
    return jobs, rows, var, gm, gvar, labels


@pytest.mark.parametrize("silences", [(), ("x-sil+a", "b-sil+x")], ids=["whole", "nosilgv"])
def test_files_equal_the_call_in_memory_and_resume(gpu, pkg, tmp_path, silences, capsys):
    torch, W, ctx = gpu
    R = pkg.recipe
    jobs, rows, var, gm, gvar, labels = write_case(pkg, tmp_path)
    layout, width = R.ffo_layout(STREAMS)
    n = R.gen_param_gv_files(jobs, STREAMS, str(tmp_path / "global.var"), str(tmp_path / "gv.mean"), str(tmp_path / "gv.var"),
                             label_dir=str(tmp_path / "lab"), silences=silences, ctx=ctx, **OPTIONS)
    assert n == sum(LENGTHS)
    assert "u2.ffo: status 4" in capsys.readouterr().err                          # one frame: mlpg's, and said so
    order = sorted(range(len(jobs)), key=lambda i: -LENGTHS[i])                   # the driver's plan
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=[LENGTHS[i] for i in order])
    mat, dvar = dev(np.concatenate([rows[i] for i in order])), dev(var)
    args = [(mat[:, c0:c0 + k], dvar[c0:c0 + k], w, None if mcol is None else mat[:, mcol])
            for (mcol, c0, k), (_, w, _) in zip(layout, STREAMS)]
    mask = None
    if silences:
        mask = dev(np.concatenate([R.gv_label_mask(labels[i], 0.005, LENGTHS[i], silences) for i in order]))
        assert 0 < int(mask.sum()) < sum(LENGTHS)
    at = np.concatenate([[0], np.cumsum([d for d, _, _ in STREAMS])])
    outs, status = b.parameter_generation_gv(args, [dev(gm[at[s]:at[s + 1]]) for s in range(3)],
                                             [dev(gvar[at[s]:at[s + 1]]) for s in range(3)], gv_mask=mask, **OPTIONS)
    plain, _ = b.parameter_generation(args)
    off = np.concatenate([[0], np.cumsum([LENGTHS[i] for i in order])])
    for k, i in enumerate(order):
        for s, o in enumerate(outs):
            assert read(jobs[i][1 + s]) == o[off[k]:off[k + 1]].cpu().numpy().tobytes(), (i, s)
    assert not torch.equal(outs[0], plain[0])                                     # and it is not gen-param's
    b.close()
    # resume: complete utterances are skipped, a missing file brings its utterance back with the same bytes
    want = read(jobs[1][2])
    os.remove(jobs[1][2])
    again = R.gen_param_gv_files(jobs, STREAMS, str(tmp_path / "global.var"), str(tmp_path / "gv.mean"), str(tmp_path / "gv.var"),
                                 label_dir=str(tmp_path / "lab"), silences=silences, ctx=ctx, resume=True, **OPTIONS)
    assert again == LENGTHS[1] and read(jobs[1][2]) == want


def test_command_line(gpu, pkg, tmp_path):
    """`gv-pdf` and `gen-param-gv` through recipe.main, on the process's current device."""
    R = pkg.recipe
    jobs, rows, var, gm, gvar, labels = write_case(pkg, tmp_path)
    cmps = []
    for k in range(4):
        cmps.append(str(tmp_path / ("g%d.cmp" % k)))
        with open(cmps[-1], "wb") as f:
            f.write(pkg.world.htk_header(1, 48000, 240, 32, 9) + (gm * (1.0 + 0.1 * k)).astype(np.float32).tobytes())
    (tmp_path / "gv.scp").write_text("\n".join(cmps) + "\n")
    assert R.main(["gv-pdf", "--scp", str(tmp_path / "gv.scp"), "--out-dir", str(tmp_path / "pdf")]) == 0
    assert os.path.getsize(str(tmp_path / "pdf" / "gv.mean")) == 32 == os.path.getsize(str(tmp_path / "pdf" / "gv.var"))
    wins = []
    for k, w in enumerate(M.RECIPE):
        (tmp_path / ("x.win%d" % (k + 1))).write_text("%d %s\n" % (len(w), " ".join(repr(v) for v in w)))
        wins.append(str(tmp_path / ("x.win%d" % (k + 1))))
    (tmp_path / "jobs.scp").write_text("".join(" ".join(j) + "\n" for j in jobs))
    argv = ["gen-param-gv", "--scp", str(tmp_path / "jobs.scp"), "--var", str(tmp_path / "global.var"),
            "--gv-mean", str(tmp_path / "pdf" / "gv.mean"), "--gv-var", str(tmp_path / "pdf" / "gv.var"), "--max-iter", "3"]
    for d, _, m in STREAMS:
        argv += ["--stream", "%d:%d:%s" % (d, int(m), ",".join(wins))]
    assert R.main(argv) == 0
    assert all(R.gen_param_complete(j, T, STREAMS) for j, T in zip(jobs, LENGTHS))


def test_generate_with_gv_equals_the_staged_pair(gpu, pkg, tmp_path):
    torch, W, ctx = gpu
    R = pkg.recipe
    os.makedirs(str(tmp_path / "world"))
    world = GS.World(pkg, tmp_path / "world")
    dims = [s[1] for s in GS.STREAMS]
    gm = np.concatenate([np.full(d, 0.01 if name == "lf0" else 0.05) for (name, d, _, _) in GS.STREAMS]).astype(np.float32)
    gvar = ((0.2 * gm) ** 2).astype(np.float32)
    gm.tofile(tmp_path / "gv.mean")
    gvar.tofile(tmp_path / "gv.var")
    options = {"max_iter": 10}
    out = tmp_path / "staged"
    os.makedirs(str(out))
    model, spkr = world.models["sd"]
    base = [os.path.join(str(out), os.path.splitext(os.path.basename(p))[0]) for p in world.labels]
    names = [s[0] for s in GS.STREAMS]
    R.ffi_files([(p, b + ".ffi") for p, b in zip(world.labels, base)], world.config, GS.FRAME_SHIFT, ctx=ctx)
    R.forward_files([(b + ".ffi", None) for b in base], model, str(out), spkr=spkr, ctx=ctx)
    R.gen_param_gv_files([(b + ".ffo",) + tuple(b + "." + n for n in names) for b in base], [s[1:] for s in GS.STREAMS],
                         base[0] + ".var", str(tmp_path / "gv.mean"), str(tmp_path / "gv.var"), ctx=ctx, **options)
    R.synth_files([(b + ".lf0", b + ".mgc", b + ".bap", b + ".wav") for b in base], GS.FRAME_PERIOD, GS.FFT_SIZE, GS.FS,
                  dims[0], dims[2], ctx=ctx)
    plain = tmp_path / "plain"
    os.makedirs(str(plain))
    R.gen_param_files([(b + ".ffo",) + tuple(os.path.join(str(plain), os.path.basename(b)) + "." + n for n in names) for b in base],
                      [s[1:] for s in GS.STREAMS], base[0] + ".var", ctx=ctx)
    assert any(read(b + ".mgc") != read(os.path.join(str(plain), os.path.basename(b)) + ".mgc") for b in base)
    jobs = [(p, str(tmp_path / (os.path.basename(p)[:-4] + ".wav"))) for p in world.labels]
    args = world.arguments("none")
    args["postfilter"] = ("gv", str(tmp_path / "gv.mean"), str(tmp_path / "gv.var"), options)
    n, flagged = pkg.generate.generate_files(jobs, **args, ctx=ctx, keep_dir=str(tmp_path / "keep"))
    assert n == sum(GS.LENGTHS) and flagged == []                                 # status 4 (one frame; unvoiced whole) is no flag
    for k, (b, (_, wav)) in enumerate(zip(base, jobs)):
        for ext in names:
            assert read(str(tmp_path / "keep" / ("a%d.%s" % (k, ext)))) == read(b + "." + ext), (k, ext)
        assert read(wav) == read(b + ".wav"), k
    assert not os.path.exists(str(tmp_path / "keep" / "a0.p_mgc"))                # no postfilter after GV generation
    with pkg.generate.Generator(ctx=ctx, **args) as gen:
        res = gen([R.read_label(p, GS.FRAME_SHIFT) for p in world.labels], report=False)
    field = (res.status >> pkg.generate.MLPG_SHIFT) & 0xF
    assert field.tolist() == [4, 4, 0, 0] and res.flagged == {} and res.p_mgc is None

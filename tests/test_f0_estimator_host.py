"""The f0 estimator of the one-call analysis, as far as it goes without a device: the three entry points are declared and
exported, the setter and getter refuse a null batch, Harvest's workspace is sized on the host, the batch plan respects
both caps, and the command line takes the new options."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("WorldMi355BatchSetF0Estimator", "WorldMi355BatchGetF0Estimator", "WorldMi355HarvestWorkspaceBytes")
BAD_ARG = 2


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.world.load_library()


def test_the_entry_points_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "world_mi355.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert hasattr(lib, name), name
    assert re.search(r"^#define WM_F0_DIO 0$", header, re.M) and re.search(r"^#define WM_F0_HARVEST 1$", header, re.M)


def test_setter_and_getter_refuse_a_null_batch(lib):
    est, ref = C.c_int(-7), C.c_int(-7)
    for estimator in (0, 1):
        assert lib.WorldMi355BatchSetF0Estimator(None, estimator, 1) == BAD_ARG
    assert lib.WorldMi355BatchGetF0Estimator(None, C.byref(est), C.byref(ref)) == BAD_ARG
    assert (est.value, ref.value) == (-7, -7)


@pytest.mark.parametrize("fs", [16000, 48000])
def test_harvest_workspace_bytes_on_the_host(pkg, lib, fs):
    W = pkg.world
    p = W.default_params(fs, 5.0)
    sizes = [W.harvest_workspace_bytes(p, [n]) for n in (1, 17, fs // 100, fs // 3, fs, 3 * fs + 1, 30 * fs, 600 * fs)]
    assert sizes[0] > 0
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes                    # non-decreasing in n
    for n in (17, fs, 3 * fs + 1):
        assert W.harvest_workspace_bytes(p, [n, n]) >= W.harvest_workspace_bytes(p, [n])
    # the frame period is not read: Harvest analyses at 1 ms whatever the caller's hop
    assert W.harvest_workspace_bytes(W.default_params(fs, 1.0), [fs]) == W.harvest_workspace_bytes(p, [fs])
    # the figure the header and DESIGN.md state: about 33 KB per 1 ms frame at the default range, for long utterances
    per_frame = (W.harvest_workspace_bytes(p, [100 * fs]) - W.harvest_workspace_bytes(p, [10 * fs])) / 90000.0
    assert 30e3 < per_frame < 36e3, per_frame
    # a wider range has more channels and more candidates a frame
    assert W.harvest_workspace_bytes(W.default_params(fs, 5.0, f0_floor=40.0, f0_ceil=1100.0), [fs]) > sizes[4]
    # refused: null arguments, no utterance, an empty utterance
    out, one = C.c_int64(-1), (C.c_int * 1)(fs)
    f = lib.WorldMi355HarvestWorkspaceBytes
    assert f(None, 1, one, C.byref(out)) == BAD_ARG
    assert f(C.byref(p), 1, None, C.byref(out)) == BAD_ARG
    assert f(C.byref(p), 1, one, None) == BAD_ARG
    assert f(C.byref(p), 0, one, C.byref(out)) == BAD_ARG
    assert f(C.byref(p), 1, (C.c_int * 1)(0), C.byref(out)) == BAD_ARG
    assert out.value == -1
    assert f(C.byref(p), 1, one, C.byref(out)) == 0 and out.value == sizes[4]
    with pytest.raises(RuntimeError):
        W.harvest_workspace_bytes(p, [])


def test_a_bad_estimator_name_is_a_value_error(pkg):
    W = pkg.world
    assert W.F0_ESTIMATORS == ("dio", "harvest") and W.f0_estimator_code("harvest") == 1
    with pytest.raises(ValueError, match="yin"):
        W.f0_estimator_code("yin")
    with pytest.raises(ValueError, match="yin"):                     # ahead of the context: no device is needed to be told
        W.WorldBatch(None, W.default_params(16000, 5.0), x_lengths=[1600], f0_estimator="yin")
    with pytest.raises(ValueError, match="yin"):
        pkg.sweep.ShardedSweep(None, 16000, 5.0, [1600, 3200], f0_estimator="yin")
    with pytest.raises(ValueError, match="yin"):
        pkg.recipe.analysis_files([], f0_estimator="yin")


FS = 16000


def corpus(n=60, seed=3):
    rng = np.random.default_rng(seed)
    samples = [int(v) for v in rng.integers(FS // 10, 9 * FS, n)]
    samples[7] = 40 * FS                                             # one utterance over the byte cap used below
    frames = [int(1000.0 * s / FS / 5.0) + 1 for s in samples]
    return samples, frames


def test_the_plan_respects_both_caps(pkg):
    rec, W = pkg.recipe, pkg.world
    samples, frames = corpus()
    order = list(range(len(samples)))
    p = W.default_params(FS, 5.0)
    cap = W.harvest_workspace_bytes(p, [20 * FS])                    # about 20 s of audio per batch
    assert W.harvest_workspace_bytes(p, [samples[7]]) > cap
    for limit in (1_500_000, 3000):                                  # the byte cap closes first, then the frame cap
        plan = rec.analysis_plan(order, frames, samples, limit, p, "harvest", cap)
        assert sorted(i for g in plan for i in g) == order           # every utterance exactly once
        assert [7] in plan                                           # over the cap: a batch of its own
        closed_by = set()
        for g, nxt in zip(plan, plan[1:] + [None]):
            if len(g) > 1:
                assert sum(frames[i] for i in g) <= limit
                assert W.harvest_workspace_bytes(p, [samples[i] for i in g]) <= cap
            if nxt is not None and len(g) >= 1 and g != [7]:          # and it was closed for a reason: the next one did not fit
                over_f = sum(frames[i] for i in g) + frames[nxt[0]] > limit
                over_b = W.harvest_workspace_bytes(p, [samples[i] for i in g + [nxt[0]]]) > cap
                assert over_f or over_b
                closed_by.add("frames" if over_f else "bytes")
        assert ("bytes" if limit == 1_500_000 else "frames") in closed_by
    # Dio: today's plan, whatever the byte cap says
    today = list(rec._batches(sorted(order, key=lambda i: -frames[i]), frames, 3000))
    assert rec.analysis_plan(order, frames, samples, 3000, p, "dio", 1) == today
    assert rec.analysis_plan(order, frames, samples, 3000) == today
    # the default cap is the 32 GiB setting
    assert pkg.sweep.HARVEST_BATCH_BYTES == 32 << 30


def test_the_sweep_plans_alike_on_every_rank_and_sums_its_resident_workspaces(pkg):
    sweep, W = pkg.sweep, pkg.world
    samples, frames = corpus()
    p = W.default_params(FS, 5.0)
    cap = W.harvest_workspace_bytes(p, [20 * FS])
    make = lambda rank, **kw: sweep.ShardedSweep(None, FS, 5.0, samples, rank=rank, world=2, backend="gloo", **kw)
    dio = [make(r) for r in (0, 1)]
    old = [list(sweep.batches(sorted(s, key=lambda i: (-frames[i], i)), frames, sweep.MAX_BATCH_FRAMES)) for s in dio[0].shards]
    assert dio[0].plan == dio[1].plan == old and dio[0].harvest_resident_bytes() == 0
    for rounds in (1, 3):
        hv = [make(r, f0_estimator="harvest", refine=False, f0_floor=60.0, f0_ceil=600.0, harvest_batch_bytes=cap,
                   rounds=rounds) for r in (0, 1)]
        assert hv[0].plan == hv[1].plan and hv[0].shards == dio[0].shards
        assert sorted(i for shard in hv[0].plan for g in shard for i in g) == list(range(len(samples)))
        assert (hv[0].params.f0_floor, hv[0].params.f0_ceil, hv[0].params.fft_size) == (60.0, 600.0, 1024)
        for r in (0, 1):
            sizes = [W.harvest_workspace_bytes(hv[r].params, [samples[i] for i in g]) for g in hv[r].plan[r]]
            assert all(s <= cap for s, g in zip(sizes, hv[r].plan[r]) if len(g) > 1)
            need = hv[r].harvest_resident_bytes()
            assert need == sum(sizes) > 0
            hv[r].check_resident(2 * need)                            # exactly half: allowed
            with pytest.raises(ValueError) as e:
                hv[r].check_resident(2 * need - 1)
            assert str(need) in str(e.value) and str(2 * need - 1) in str(e.value)   # both figures are named


def test_the_command_line_takes_the_estimator(pkg, tmp_path, capsys):
    rec = pkg.recipe
    scp = tmp_path / "none.scp"
    scp.write_text("")
    with pytest.raises(SystemExit) as e:
        rec.main(["analysis", "--scp", str(scp), "--f0", "yin"])
    assert e.value.code == 2 and "yin" in capsys.readouterr().err
    seen = {}

    def fake(jobs, *args, **kw):
        seen.update(kw, args=args)
        return 0
    real, rec.analysis_files = rec.analysis_files, fake
    try:
        assert rec.main(["analysis", "--scp", str(scp), "--f0", "harvest", "--no-refine", "--f0-floor", "60",
                         "--f0-ceil", "600", "--spec-dim", "50", "--ap-dim", "25"]) == 0
        assert (seen["f0_estimator"], seen["refine"], seen["f0_floor"], seen["f0_ceil"]) == ("harvest", False, 60.0, 600.0)
        assert seen["args"] == (5.0, 0, 50, 25)
        assert rec.main(["analysis", "--scp", str(scp)]) == 0
        assert (seen["f0_estimator"], seen["refine"], seen["f0_floor"], seen["f0_ceil"]) == ("dio", True, 71.0, 800.0)
    finally:
        rec.analysis_files = real

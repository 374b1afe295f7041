"""The skeleton that recipe.py's file-list drivers share -- plan, sharding, resume, who closes what, and what is left
behind when something fails -- without a device: world.WorldBatch is a stand-in whose every stage is rows x 2 on the
host, recipe._own_context hands out counted stand-ins and recipe._upload is torch.from_numpy.

The corpus is four utterances of 3, 5, 8 and 13 frames of 4 float32 with max_batch_frames = 13: three batches in
descending frame order, [13], [8, 5] and [3]."""
import os
import types

import numpy as np
import pytest
import torch

FRAMES = (3, 5, 8, 13)
WIDTH = 4
LIMIT = 13
PLAN = [[13], [8, 5], [3]]
DRIVERS = ("postfilter", "mspf", "gen_param", "ffo", "cmp", "ffi")
RESUMING = tuple(d for d in DRIVERS if d != "cmp")                 # cmp_files has no resume
READING = tuple(d for d in DRIVERS if d != "ffi")                  # ffi_files reads its labels before the first batch


class Ctx:
    def __init__(self):
        self.closed = 0

    def close(self):
        self.closed += 1


def stand_ins(state):
    """(WorldBatch, LabelFeatureSet) that count in `state`; the stage call number state.fail_at raises."""

    class Set:
        def __init__(self, ctx, features):
            self.n_features = len(features)
            state.sets_opened += 1

        def close(self):
            state.sets_closed += 1

    class Batch:
        def __init__(self, ctx, params, f0_lengths=None):
            state.opened += 1
            state.plan.append([int(n) for n in f0_lengths])
            self.frame_offsets = np.concatenate([[0], np.cumsum(f0_lengths)]).astype(np.int64)
            self.total_frames, self.n_utt = int(self.frame_offsets[-1]), len(f0_lengths)

        def close(self):
            state.closed += 1

        def _stage(self, rows):
            state.calls += 1
            if state.calls == state.fail_at:
                raise RuntimeError("the stand-in stage fails")
            return (rows * 2).contiguous()

        def _clean(self, n):
            return torch.zeros(n, dtype=torch.int32)

        def postfilter_mel_cepstrum(self, rows, alpha, beta, length):
            return self._stage(rows), self._clean(self.total_frames)

        def postfilter_modulation_spectrum(self, rows, *tables_and_settings):
            return self._stage(rows), self._clean(self.n_utt)

        def parameter_generation(self, args, edge=0, unvoiced_value=-1.0e10):
            (rows, var, wins, voicing), = args
            return [self._stage(rows[:, :rows.shape[1] // len(wins)])], self._clean(self.n_utt)

        def compose_ffo(self, streams):
            (rows, wins, voiced), = streams
            return self._stage(rows)

        def compose_cmp(self, streams):
            (rows, wins), = streams
            return self._stage(rows)

        def label_features(self, fset, labels):
            assert [sum(e - s for s, e, _, _ in lines) for lines, _ in labels] == list(np.diff(self.frame_offsets))
            rows = [torch.from_numpy(label_rows(e - s)) for lines, _ in labels for s, e, _, _ in lines]
            return self._stage(torch.cat(rows)), self._clean(self.n_utt)

    return Batch, Set


def label_rows(n):
    return np.arange(n * WIDTH, dtype=np.float32).reshape(n, WIDTH)


def rows_of(i):
    return np.arange(FRAMES[i] * WIDTH, dtype=np.float32).reshape(FRAMES[i], WIDTH) + 100.0 * (i + 1)


class Corpus:
    """The four jobs of one driver under `d`: job[0] is the input a batch reads, job[-1] the output; want[i] the
    output's bytes (the stand-in's rows x 2, rounded to float32 as the driver rounds); run(jobs, **more) the call."""

    def __init__(self, name, rec, d):
        self.name = name
        ins = [str(d / ("u%d.in" % i)) for i in range(4)]
        outs = [str(d / ("u%d.out" % i)) for i in range(4)]
        self.jobs = list(zip(ins, outs))
        for i, path in enumerate(ins):
            rows_of(i).tofile(path)
        self.want = [(rows_of(i) * 2).tobytes() for i in range(4)]
        more = dict(max_batch_frames=LIMIT, io_threads=2)
        if name == "postfilter":
            self.run = lambda jobs, **kw: rec.postfilter_files(jobs, WIDTH - 1, 0.5, **more, **kw)
        elif name == "mspf":
            for side in ("gen", "nat"):
                os.makedirs(str(d / side))
                for k in range(WIDTH):
                    for ext in ("mean", "stdd"):
                        np.ones(33, dtype=np.float32).tofile(str(d / side / ("mgc_dim%d.%s" % (k, ext))))
            self.run = lambda jobs, **kw: rec.mspf_files(jobs, WIDTH, str(d / "gen"), str(d / "nat"), **more, **kw)
        elif name == "gen_param":
            np.ones(WIDTH, dtype=np.float32).tofile(str(d / "ffo.var"))
            streams = [(2, [[1.0], [-0.5, 0.0, 0.5]], False)]
            self.want = [(rows_of(i)[:, :2] * 2).tobytes() for i in range(4)]
            self.run = lambda jobs, **kw: rec.gen_param_files(jobs, streams, str(d / "ffo.var"), **more, **kw)
        elif name == "ffo":
            self.run = lambda jobs, **kw: rec.ffo_files(jobs, [(WIDTH, [[1.0]], False)], **more, **kw)
        elif name == "cmp":
            self.want = [rec.W.htk_header(FRAMES[i], 48000, 240, 4 * WIDTH, 9) + self.want[i] for i in range(4)]
            self.run = lambda jobs, **kw: rec.cmp_files(jobs, [(WIDTH, [[1.0]])], 48000, 240, **more, **kw)
        else:
            for i, path in enumerate(ins):
                with open(path, "w") as f:
                    f.write("0 %d a\n" % (50000 * FRAMES[i]))
            self.want = [(label_rows(n) * 2).tobytes() for n in FRAMES]
            config = (["q%d" % k for k in range(WIDTH)], [(0, "*a*", 0, 0)] * WIDTH)
            self.run = lambda jobs, **kw: rec.ffi_files(jobs, config, 50000, **more, **kw)

    def written(self, i):
        with open(self.jobs[i][1], "rb") as f:
            return f.read()


@pytest.fixture
def state(pkg, monkeypatch):
    rec = pkg.recipe
    st = types.SimpleNamespace(opened=0, closed=0, plan=[], calls=0, fail_at=None, sets_opened=0, sets_closed=0, made=[])
    batch, fset = stand_ins(st)
    monkeypatch.setattr(rec.W, "WorldBatch", batch)
    monkeypatch.setattr(rec.W, "LabelFeatureSet", fset)
    monkeypatch.setattr(rec, "_own_context", lambda: st.made.append(Ctx()) or st.made[-1])
    monkeypatch.setattr(rec, "_upload", torch.from_numpy)
    monkeypatch.setenv("WORLD_SIZE", "1")
    return st


def context(own):
    """(the ctx argument, its check after the call): a driver-made context is closed once, a caller's never."""
    given = None if own else Ctx()

    def check(state):
        assert state.opened == state.closed and state.sets_opened == state.sets_closed
        if own:
            assert [c.closed for c in state.made] == [1]
        else:
            assert state.made == [] and given.closed == 0
    return given, check


@pytest.mark.parametrize("own", [True, False], ids=["own-ctx", "callers-ctx"])
@pytest.mark.parametrize("name", DRIVERS)
def test_plan_bytes_and_ownership(pkg, state, tmp_path, name, own):
    c = Corpus(name, pkg.recipe, tmp_path)
    ctx, check = context(own)
    assert c.run(c.jobs, ctx=ctx) == sum(FRAMES)
    assert state.plan == PLAN and all(sum(g) <= LIMIT for g in state.plan)
    for i in range(4):
        assert c.written(i) == c.want[i], c.jobs[i][1]
    check(state)


@pytest.mark.parametrize("name", DRIVERS)
def test_two_ranks_write_every_job_once(pkg, state, tmp_path, monkeypatch, name):
    c = Corpus(name, pkg.recipe, tmp_path)
    monkeypatch.setenv("WORLD_SIZE", "2")
    shares = []
    for rank in (0, 1):
        monkeypatch.setenv("RANK", str(rank))
        before = {j[1] for j in c.jobs if os.path.exists(j[1])}
        done = c.run(c.jobs)
        shares.append([i for i, j in enumerate(c.jobs) if os.path.exists(j[1]) and j[1] not in before])
        assert done == sum(FRAMES[i] for i in shares[-1]) and shares[-1]
    assert sorted(shares[0] + shares[1]) == [0, 1, 2, 3]
    assert all(c.written(i) == c.want[i] for i in range(4))
    assert all(sum(g) <= LIMIT for g in state.plan) and sorted(n for g in state.plan for n in g) == sorted(FRAMES)
    assert state.opened == state.closed and [x.closed for x in state.made] == [1, 1]


@pytest.mark.parametrize("name", RESUMING)
def test_resume_redoes_a_truncated_and_a_deleted_output_only(pkg, state, tmp_path, name):
    c = Corpus(name, pkg.recipe, tmp_path)
    assert c.run(c.jobs) == sum(FRAMES)
    assert c.run(c.jobs, resume=True) == 0
    os.truncate(c.jobs[1][1], 8)
    os.remove(c.jobs[2][1])
    kept = {i: os.stat(c.jobs[i][1]).st_mtime_ns for i in (0, 3)}
    state.plan.clear()
    assert c.run(c.jobs, resume=True) == FRAMES[1] + FRAMES[2]
    assert state.plan == [[FRAMES[2], FRAMES[1]]]
    assert all(c.written(i) == c.want[i] for i in range(4))
    assert all(os.stat(c.jobs[i][1]).st_mtime_ns == t for i, t in kept.items())
    assert state.opened == state.closed


@pytest.mark.parametrize("own", [True, False], ids=["own-ctx", "callers-ctx"])
@pytest.mark.parametrize("name", DRIVERS)
def test_a_stage_that_raises_in_the_second_batch(pkg, state, tmp_path, name, own):
    c = Corpus(name, pkg.recipe, tmp_path)
    ctx, check = context(own)
    state.fail_at = 2
    with pytest.raises(RuntimeError, match="stand-in stage fails"):
        c.run(c.jobs, ctx=ctx)
    assert state.plan == PLAN[:2]
    assert c.written(3) == c.want[3]                               # the first batch's output is whole already
    assert not any(os.path.exists(c.jobs[i][1]) for i in (0, 1, 2))
    check(state)


@pytest.mark.parametrize("own", [True, False], ids=["own-ctx", "callers-ctx"])
@pytest.mark.parametrize("name", DRIVERS)
def test_an_output_directory_that_does_not_exist(pkg, state, tmp_path, name, own):
    """The write's own error reaches the caller: numpy's and open()'s OSError, and from ffi_files the RuntimeError in
    which world.write_files reports the native writer's failure (tests/test_host_logic.py holds it to that)."""
    c = Corpus(name, pkg.recipe, tmp_path)
    ctx, check = context(own)
    jobs = list(c.jobs)
    jobs[2] = (jobs[2][0], str(tmp_path / "no_such_dir" / "u2.out"))
    with pytest.raises(RuntimeError if name == "ffi" else OSError, match="no_such_dir"):
        c.run(jobs, ctx=ctx)
    check(state)


@pytest.mark.parametrize("own", [True, False], ids=["own-ctx", "callers-ctx"])
@pytest.mark.parametrize("name", READING)
def test_an_input_cut_short_after_the_size_scan(pkg, state, tmp_path, monkeypatch, name, own):
    c = Corpus(name, pkg.recipe, tmp_path)
    ctx, check = context(own)
    share = pkg.recipe._my_share

    def cut_then_share(costs):                                     # the drivers have taken the sizes by now
        os.truncate(c.jobs[2][0], 4 * WIDTH * FRAMES[2] - 2)
        return share(costs)
    monkeypatch.setattr(pkg.recipe, "_my_share", cut_then_share)
    with pytest.raises(ValueError, match="reshape"):
        c.run(c.jobs, ctx=ctx)
    assert state.plan == PLAN[:2]
    assert c.written(3) == c.want[3]
    check(state)

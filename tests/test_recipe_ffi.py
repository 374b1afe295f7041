"""recipe.ffi_files / `recipe.py ffi`.  CPU part: the command line, the sharding of the job list over ranks and resume
by file size, with the device stage replaced by a stand-in that writes zeros.  GPU part: the fixture's label files
(tests/golden/label_features.npz, written by the reference's makefeature.pl) through the command, file for file."""
import os

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "label_features.npz"))


def corpus(fx, tmp_path, block="recipe"):
    config = tmp_path / "q.conf"
    config.write_text(str(fx[block + "/config"]))
    jobs, outs = [], []
    for i in range(int(fx[block + "/n_labels"])):
        lab = tmp_path / ("a%d.lab" % i)
        lab.write_text(str(fx["%s/label%d" % (block, i)]))
        jobs.append((str(lab), str(tmp_path / ("a%d.ffi" % i))))
        outs.append(fx["%s/out%d" % (block, i)])
    return str(config), jobs, outs


def test_cli_arguments(pkg, tmp_path, capsys):
    main = pkg.recipe.main
    scp, conf = tmp_path / "empty.scp", tmp_path / "q.conf"
    scp.write_text("")
    conf.write_text("a {*a*}\n")
    assert main(["ffi", "--scp", str(scp), "--config", str(conf), "--frame-shift", "50000", "--resume"]) == 0
    assert "complete. 0 frames" in capsys.readouterr().out
    for argv in (["ffi", "--scp", str(scp), "--config", str(conf)], ["ffi", "--scp", str(scp), "--frame-shift", "50000"],
                 ["ffi", "--config", str(conf), "--frame-shift", "50000"],
                 ["ffi", "--scp", str(scp), "--config", str(conf), "--frame-shift", "0"]):
        with pytest.raises(SystemExit):
            main(argv)
    scp.write_text("only-one-path\n")
    with pytest.raises(SystemExit):
        main(["ffi", "--scp", str(scp), "--config", str(conf), "--frame-shift", "50000"])
    conf.write_text("a\n")
    scp.write_text("")
    with pytest.raises(ValueError, match="Cannot specify feature type"):
        main(["ffi", "--scp", str(scp), "--config", str(conf), "--frame-shift", "50000"])
    conf.write_text("# nothing\n")
    with pytest.raises(ValueError, match="no feature"):
        pkg.recipe.ffi_files([], str(conf), 50000)
    with pytest.raises(ValueError):
        pkg.recipe.ffi_files([("a.lab",)], (["a"], [(0, "a", 0, 0)]), 50000)


class StandIn:
    """What ffi_files asks of world.py, without a device: rows of zeros."""
    groups = []

    class Set:
        def __init__(self, ctx, features):
            self.n_features = len(features)

        def close(self):
            pass

    class Batch:
        def __init__(self, ctx, params, f0_lengths=None):
            self.frame_offsets = np.concatenate([[0], np.cumsum(f0_lengths)])
            self.total_frames = int(self.frame_offsets[-1])

        def label_features(self, fset, labels):
            import torch
            assert [sum(e - s for s, e, _, _ in lines) for lines, _ in labels] == list(np.diff(self.frame_offsets))
            StandIn.groups.append(list(np.diff(self.frame_offsets)))
            return torch.zeros(self.total_frames, fset.n_features), torch.zeros(len(labels), dtype=torch.int32)

        def close(self):
            pass


def test_sharding_and_resume_by_file_size(pkg, fx, tmp_path, monkeypatch):
    config, jobs, outs = corpus(fx, tmp_path)
    frames = [o.shape[0] for o in outs]
    nf = outs[0].shape[1]
    rec = pkg.recipe
    monkeypatch.setattr(rec.W, "LabelFeatureSet", StandIn.Set)
    monkeypatch.setattr(rec.W, "WorldBatch", StandIn.Batch)
    monkeypatch.setattr(rec, "_own_context", lambda: type("Ctx", (), {"close": lambda self: None})())
    monkeypatch.setenv("WORLD_SIZE", "2")
    written = []
    for rank in (0, 1):
        monkeypatch.setenv("RANK", str(rank))
        before = {j[1] for j in jobs if os.path.exists(j[1])}
        done = rec.ffi_files(jobs, config, 50000, max_batch_frames=300)
        mine = [i for i, j in enumerate(jobs) if os.path.exists(j[1]) and j[1] not in before]
        assert done == sum(frames[i] for i in mine) and mine
        written.append(mine)
    assert sorted(written[0] + written[1]) == list(range(len(jobs)))       # every job once
    assert abs(sum(frames[i] for i in written[0]) - sum(frames[i] for i in written[1])) <= max(frames)
    assert all(os.path.getsize(j[1]) == 4 * nf * f for j, f in zip(jobs, frames))
    assert all(sum(g) <= 300 or len(g) == 1 for g in StandIn.groups) and any(len(g) > 1 for g in StandIn.groups)
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert rec.ffi_files(jobs, config, 50000, resume=True) == 0            # complete: nothing to do
    os.truncate(jobs[2][1], 8)
    os.remove(jobs[4][1])
    StandIn.groups.clear()
    assert rec.ffi_files(jobs, config, 50000, resume=True) == frames[2] + frames[4]
    assert sorted(StandIn.groups[0]) == sorted([frames[2], frames[4]])
    assert rec.ffi_files(jobs, config, 50000) == sum(frames)               # without resume: all of them again


@pytest.mark.gpu
def test_ffi_command_file_for_file_with_the_fixture(gpu, pkg, fx, tmp_path, capsys):
    config, jobs, outs = corpus(fx, tmp_path)
    scp = tmp_path / "jobs.scp"
    scp.write_text("".join("%s %s\n" % j for j in jobs))
    assert pkg.recipe.main(["ffi", "--scp", str(scp), "--config", config, "--frame-shift", "50000"]) == 0
    cap = capsys.readouterr()
    assert "complete. %d frames" % sum(o.shape[0] for o in outs) in cap.out
    assert "Out of range in 6 utterances, no state-level information in 3" in cap.err
    for (_, path), want in zip(jobs, outs):
        got = np.fromfile(path, dtype=np.float32).reshape(want.shape)
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), path
    assert pkg.recipe.main(["ffi", "--scp", str(scp), "--config", config, "--frame-shift", "50000", "--resume"]) == 0
    assert "complete. 0 frames" in capsys.readouterr().out
    # the random block through ffi_files on the caller's context; its one file is a batch of its own whatever the limit
    config, jobs, outs = corpus(fx, tmp_path, "random")
    assert pkg.recipe.ffi_files(jobs, config, 50000, ctx=gpu[2], max_batch_frames=64) == 200
    got = np.fromfile(jobs[0][1], dtype=np.float32).reshape(outs[0].shape)
    assert (got.view(np.uint32) == outs[0].view(np.uint32)).all()

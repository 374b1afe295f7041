"""`recipe.py evaluate` on small float32 files: three utterances with mgc:6, lf0:1 and bap:3, a label file with a silence
segment; --align dtw and truncate, --with-c0 and --silence, the JSON object and the per-utterance lines against
tests/dtw_reference.py within the bounds of tests/test_gpu_dtw.py."""
import importlib
import json
import math

import numpy as np
import pytest

import dtw_reference as R

pytestmark = pytest.mark.gpu

PAIRS = ((70, 90), (33, 21), (12, 12))
STREAMS = (("mgc", 6), ("lf0", 1), ("bap", 3))
SHIFT = 0.005


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("evaluate")
    rng = np.random.default_rng(11)
    jobs, data = [], []
    for u, (ta, tb) in enumerate(PAIRS):
        mgc = R.inputs(ta, tb, 6)
        bap = R.inputs(ta, tb, 3, seed=500 + u)
        lf0 = []
        for t in (ta, tb):
            x = (5.0 + 0.2 * rng.standard_normal((t, 1))).astype(np.float32)
            x[t // 3:t // 3 + 4] = -1.0e10
            lf0.append(x)
        lf0[1][:2] = -1.0e10
        row, feats = [], {}
        for name, (g, n) in zip(("mgc", "lf0", "bap"), (mgc, lf0, bap)):
            for side, x in (("gen", g), ("nat", n)):
                p = d / ("u%d_%s.%s" % (u, side, name))
                x.tofile(p)
                row.append(str(p))
            feats[name] = (g, n)
        lab = d / ("u%d.lab" % u)
        cut = int(0.3 * tb) * 50000 + 25000                               # label times in 100 ns, 5 ms frames
        lab.write_text("0 %d sil\n%d %d a\n" % (cut, cut, tb * 50000))
        jobs.append(row + [str(lab)])
        data.append(feats)
    scp = d / "jobs.scp"
    scp.write_text("".join(" ".join(j) + "\n" for j in jobs))
    return d, scp, jobs, data


def reference_rows(recipe, data, jobs, align, with_c0, silences):
    groups = recipe.evaluate_groups(STREAMS, with_c0)
    rows, rows_ld, lens = [], [], []
    for u, (ta, tb) in enumerate(PAIRS):
        if align == "dtw":
            f, c, _ = groups[0]
            pairs = R.dtw(data[u]["mgc"][0][:, f:f + c], data[u]["mgc"][1][:, f:f + c])[0]
        else:
            pairs = R.truncation(ta, tb)
        mask = None
        if silences:
            with open(jobs[u][-1]) as fh:
                mask = recipe.gv_label_mask(fh.readlines(), SHIFT, tb, silences)
        per = [[R.distortion(data[u][name][0][:, f:f + c], data[u][name][1][:, f:f + c], pairs, k, mask, dtype=dt)
                for (name, _), (f, c, k) in zip(STREAMS, groups)] for dt in (np.float64, np.longdouble)]
        rows.append(per[0])
        rows_ld.append(per[1])
        lens.append(len(pairs))
    return np.array(rows, dtype=np.float64), np.array(rows_ld, dtype=np.longdouble), lens, groups


def close(got, want, want_ld, terms):
    return abs(got - want) <= max(10.0 * abs(float(want_ld) - want), 2.0 * terms * 2.0 ** -53 * abs(want))


@pytest.mark.parametrize("align", ["dtw", "truncate"])
@pytest.mark.parametrize("with_c0,silence", [(False, False), (True, False), (False, True)], ids=["plain", "c0", "silence"])
def test_evaluate(gpu, corpus, align, with_c0, silence):
    recipe = importlib.import_module("hts-train-world_amd").recipe
    d, scp, jobs, data = corpus
    out, per = d / ("out_%s_%d_%d.json" % (align, with_c0, silence)), d / ("per_%s_%d_%d.tsv" % (align, with_c0, silence))
    argv = ["evaluate", "--scp", str(scp), "--align", align, "--out", str(out), "--per-utterance", str(per),
            "--frame-shift-s", str(SHIFT)]
    for name, dim in STREAMS:
        argv += ["--stream", "%s:%d" % (name, dim)]
    argv += ["--with-c0"] if with_c0 else []
    argv += ["--silence", "sil"] if silence else []
    assert recipe.main(argv) == 0
    rows, rows_ld, lens, groups = reference_rows(recipe, data, jobs, align, with_c0, ("sil",) if silence else ())
    want = R.pooled(rows, [k for _, _, k in groups])
    obj = json.loads(out.read_text())
    assert obj["align"] == align and obj["utterances"] == 3 and obj["flagged"] == 0
    terms = max(lens) + 6 + 4
    for s, (name, _) in enumerate(STREAMS):
        got = obj["streams"][name]
        assert got["pairs"] == want[s]["pairs"], (name, got, want[s])
        if groups[s][2] == 0:
            assert math.isclose(got["mean_db"], want[s]["mean_db"], rel_tol=4.0 * terms * 2.0 ** -53), (name, got, want[s])
        else:
            assert got["voiced_pairs"] == want[s]["voiced_pairs"]
            assert got["vuv_error_percent"] == want[s]["vuv_error_percent"]
            assert math.isclose(got["rmse_cents"], want[s]["rmse_cents"], rel_tol=4.0 * terms * 2.0 ** -53)
    lines = per.read_text().splitlines()
    assert len(lines) == 3
    for u, line in enumerate(lines):
        col = line.split("\t")
        assert col[0] == jobs[u][0] and [int(c) for c in col[1:5]] == [PAIRS[u][0], PAIRS[u][1], lens[u], 0]
        mgc_mean, mgc_n = float(col[5]), int(col[6])
        assert mgc_n == rows[u, 0, 2]
        assert close(mgc_mean * mgc_n, rows[u, 0, 0], rows_ld[u, 0, 0], lens[u] + groups[0][1] + 4 + 2)
        assert int(col[9]) == rows[u, 1, 1] and int(col[10]) == rows[u, 1, 3]
        assert int(col[12]) == rows[u, 2, 2]
    # what the options change, as the reference says
    plain, _, _, g0 = reference_rows(recipe, data, jobs, align, False, ())
    if with_c0:
        assert want[0]["mean_db"] > R.pooled(plain, [0, 1, 0])[0]["mean_db"]        # one more squared column per pair
    if silence:
        assert want[0]["pairs"] < R.pooled(plain, [0, 1, 0])[0]["pairs"]

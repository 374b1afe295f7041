"""WorldBatch.label_features (label_match_kernel / ffi_rows_kernel, csrc/ffi.hip) against the rows the reference's own
makefeature.pl wrote (tests/golden/label_features.npz, tools/gen_golden_ffi.py), bit for bit, and on hand-made labels
against tests/label_features_reference.py, which tests/test_label_features_host.py pins to that fixture.

Shapes: the fixture's two blocks (42 features x 655 frames in six utterances; 360 features x 200 one-frame lines); feature
counts 1, 63, 64, 65 and 129 as slices of the random block (alternative totals that are no multiple of 64, features
whose alternatives lie across a 64-lane group); a one-frame utterance beside one of 300 frames in 150 lines (more lines
than the 64 probes of one search round); padded and unaligned outputs (the 16-byte and the 4-byte store paths)."""
import os

import numpy as np
import pytest

import label_features_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "label_features.npz"))


def block(fx, pkg, name):
    n = int(fx[name + "/n_labels"])
    shift = int(fx[name + "/frame_shift"])
    config = str(fx[name + "/config"])
    labels = [pkg.recipe.parse_label(str(fx["%s/label%d" % (name, i)]), shift) for i in range(n)]
    outs = [fx["%s/out%d" % (name, i)] for i in range(n)]
    bits = [(1 if fx["%s/warn%d" % (name, i)][0] else 0) | (2 if fx["%s/warn%d" % (name, i)][1] else 0) for i in range(n)]
    return config, pkg.recipe.parse_question_config(config)[1], labels, outs, bits


def frames_of(label):
    return sum(e - s for s, e, _, _ in label[0])


def batch_of(W, ctx, labels):
    return W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=[frames_of(l) for l in labels])


def same_bits(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


def run(gpu, features, labels, out=None):
    torch, W, ctx = gpu
    fset = W.LabelFeatureSet(ctx, features)
    b = batch_of(W, ctx, labels)
    try:
        rows, status = b.label_features(fset, labels, out=out)
        return rows.cpu().numpy(), status.cpu().numpy(), b.frame_offsets
    finally:
        b.close()
        fset.close()


@pytest.mark.parametrize("name", ["recipe", "random"])
def test_fixture_as_one_batch_and_utterance_by_utterance(gpu, fx, pkg, name):
    config, features, labels, outs, bits = block(fx, pkg, name)
    rows, status, fo = run(gpu, features, labels)
    assert rows.shape == (sum(o.shape[0] for o in outs), len(features))
    for u, want in enumerate(outs):
        assert same_bits(rows[fo[u]:fo[u + 1]], want), u
    assert list(status) == bits
    for u in range(len(labels) - 1, -1, -1):                              # ... alone, in another order
        alone, st, _ = run(gpu, features, [labels[u]])
        assert same_bits(alone, outs[u]) and list(st) == [bits[u]], u


def alternatives(features):
    return [len(p.split(",")) if k == 0 else 0 for k, p, _, _ in features]


@pytest.mark.parametrize("first,count", [(0, 1), (3, 63), (0, 64), (40, 65), (231, 129), (191, 129)])
def test_feature_counts_as_slices_of_the_random_block(gpu, fx, pkg, first, count):
    config, features, labels, outs, bits = block(fx, pkg, "random")
    part = features[first:first + count]
    rows, status, _ = run(gpu, part, labels)
    assert same_bits(rows, outs[0][:, first:first + count])
    clamped = np.asarray(R.rows("\n".join(config.split("\n")[first:first + count]), str(fx["random/label0"]), 50000)[1][0] > 0)
    assert list(status) == [int(clamped)]


def test_the_slices_hold_the_layouts_the_match_kernel_can_get_wrong(fx, pkg):
    """Of the slices above: alternative totals below 64, above it and no multiple of 64; a feature whose alternatives
    straddle a multiple of 64; a slice that ends in float features (the float table and the answers side by side)."""
    features = block(fx, pkg, "random")[1]
    totals, straddles = [], 0
    for first, count in ((0, 1), (3, 63), (0, 64), (40, 65), (231, 129), (191, 129)):
        n = alternatives(features[first:first + count])
        totals.append(sum(n))
        at = 0
        for k in n:
            straddles += 1 if k > 1 and at // 64 != (at + k - 1) // 64 else 0
            at += k
    print("alternatives per slice", totals, "features across a group boundary", straddles)
    assert min(totals) < 64 and max(totals) > 128 and all(t % 64 for t in totals) and straddles >= 3
    assert sum(1 for k, _, _, _ in features[231:360] if k == 1) == 40 and sum(1 for k, _, _, _ in features[191:320] if k == 1) == 0


def test_padded_and_unaligned_outputs(gpu, fx, pkg):
    torch, W, ctx = gpu
    config, features, labels, outs, bits = block(fx, pkg, "recipe")
    want = np.concatenate(outs)
    T, nf = want.shape
    assert nf % 4 == 2
    for ld, shift in ((48, 0), (48, 1), (45, 0), (43, 3), (nf, 0), (nf, 2)):   # 16-byte rows; off by a float; odd strides; tight
        buf = torch.full((T * ld + 8,), 7.5, dtype=torch.float32, device="cuda")
        view = buf[shift:shift + T * ld].view(T, ld)
        assert (view.data_ptr() % 16 == 0) == (shift == 0)
        rows, status, _ = run(gpu, features, labels, out=view)
        assert same_bits(rows, want), (ld, shift)
        host = buf.cpu().numpy()
        body = host[shift:shift + T * ld].reshape(T, ld)
        assert (body[:, nf:] == 7.5).all() and (host[:shift] == 7.5).all() and (host[shift + T * ld:] == 7.5).all(), (ld, shift)
        assert list(status) == bits


def test_one_frame_beside_three_hundred(gpu, fx, pkg):
    config = str(fx["recipe/config"])
    features = pkg.recipe.parse_question_config(config)[1]
    short = "0 50000 x^sil-k+o=N/A:1+2_03/B:1@1/C:ab/D:+1|x$f/E:_1_22_333[2]\n"
    long_, t = "", 0
    for i in range(150):                                                   # 30 phonemes of five states, two frames each
        long_ += "%d %d x^a-o+i=x/A:-6+%d_%02d/B:1@1/C:a.b/D:%+d|y$f/E:_1_22_3[%d]\n" % (
            t * 50000, (t + 2) * 50000, i % 7, i % 25, i - 70, 2 + i % 5)
        t += 2
    texts = [short, long_, short]
    labels = [pkg.recipe.parse_label(s, 50000) for s in texts]
    assert [frames_of(l) for l in labels] == [1, 300, 1]
    rows, status, fo = run(gpu, features, labels)
    for u, text in enumerate(texts):
        want, warn = R.rows(config, text, 50000)
        assert same_bits(rows[fo[u]:fo[u + 1]], want), u
        assert status[u] == (1 if warn[0] else 0) | (2 if warn[1] else 0)
    assert status[1] & 1 and not status[1] & 2


def test_refusals_that_need_a_batch(gpu, fx, pkg):
    torch, W, ctx = gpu
    features = [(0, "*a*", 0, 0), (1, "*_%d", 0, 9), (4, None, 1, 5)]
    fset = W.LabelFeatureSet(ctx, features)
    assert fset.n_features == 3
    good = ([(0, 2, "ab_3", 2), (2, 5, "b", 3)], True)
    b = batch_of(W, ctx, [good])
    rows, status = b.label_features(fset, [good])
    assert rows.shape == (5, 3) and list(rows[:, 0].cpu().numpy()) == [1, 1, 0, 0, 0]
    bad = lambda: pytest.raises(RuntimeError, match="bad argument")
    for lines in ([(0, 2, "a", 2), (2, 4, "b", 3)],                        # four frames in a batch of five
                  [(0, 2, "a", 2), (2, 6, "b", 3)],
                  [(0, 5, "a", 2), (7, 7, "b", 3)],                        # end <= start
                  [(3, 2, "a", 2), (0, 6, "b", 3)],
                  [(-1, 2, "a", 2), (2, 4, "b", 3)],                       # start < 0
                  [(0, 5, "", 2)]):
        with bad():
            b.label_features(fset, [(lines, True)])
    for name in ("a" * 1024, "a b", "a\x7f", "\xe9"):
        with pytest.raises(RuntimeError, match="unsupported"):
            b.label_features(fset, [([(0, 5, name, 2)], True)])
    assert b.label_features(fset, [([(0, 5, "a" * 1023, 0)], False)])[0].shape == (5, 3)
    with bad():                                                            # ld_out < n_features
        b.label_features(fset, [good], out=torch.zeros(5, 2, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        b.label_features(fset, [good, good])
    with pytest.raises(ValueError):
        b.label_features(fset, [good], out=torch.zeros(4, 3, dtype=torch.float32, device="cuda"))
    other = W.Context()
    try:
        theirs = W.LabelFeatureSet(other, features)
        with bad():                                                        # a set of another context
            b.label_features(theirs, [good])
        theirs.close()
    finally:
        other.close()
    b.close()
    fset.close()
    for feats, kind in (([(1, "*_%d", 3, 3)], "bad argument"), ([(4, None, 5, 1)], "bad argument"),
                        ([(1, "*_%d", 0, 2 ** 20 + 1)], "bad argument"), ([(1, "*", 0, 1)], "bad argument"),
                        ([(8, "a", 0, 1)], "bad argument"), ([], "bad argument"), ([(0, "a(b", 0, 0)], "unsupported"),
                        ([(0, "a" * 64, 0, 0)], "unsupported"), ([(0, "a\xe9", 0, 0)], "unsupported")):
        with pytest.raises(RuntimeError, match=kind):
            W.LabelFeatureSet(ctx, feats)
    ok = W.LabelFeatureSet(ctx, [(1, "*_%d", 0, 2 ** 20), (0, "", 0, 0)])
    assert ok.n_features == 2
    ok.close()


def test_a_batch_of_zero_frames_cannot_be_made(gpu):
    """The stage returns WM_OK for a batch of zero frames, as the other stages do, but CreateBatch refuses an utterance
    without frames: no such batch reaches it from here."""
    torch, W, ctx = gpu
    with pytest.raises(RuntimeError, match="bad argument"):
        W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=[0])


def test_rows_go_straight_into_the_acoustic_model(gpu, fx, pkg):
    torch, W, ctx = gpu
    config, features, labels, outs, bits = block(fx, pkg, "recipe")
    nf = len(features)
    rng = np.random.default_rng(9)
    dev = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).cuda()
    model = {"weights": [dev(rng.standard_normal((nf, 24)) * 0.3), dev(rng.standard_normal((24, 7)) * 0.3)],
             "biases": [dev(rng.standard_normal(24)), dev(rng.standard_normal(7))], "spkr_weights": None, "variances": None,
             "n_spkrs": 1, "hidden_activation": "sigmoid", "output_activation": "linear"}
    fset = W.LabelFeatureSet(ctx, features)
    b = batch_of(W, ctx, labels)
    padded = torch.zeros(b.total_frames, 48, dtype=torch.float32, device="cuda")
    rows, _ = b.label_features(fset, labels, out=padded)
    assert rows.data_ptr() == padded.data_ptr() and rows.stride(0) == 48
    got, _, status = b.acoustic_model_forward(model, rows)
    want, _, _ = b.acoustic_model_forward(model, torch.from_numpy(np.concatenate(outs)).cuda())
    assert int(status.abs().sum()) == 0 and torch.equal(got, want) and float(want.abs().max()) > 0.1
    b.close()
    fset.close()

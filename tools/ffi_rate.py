"""Rate of the label-features stage (WorldMi355LabelFeatures: label_match_kernel, ffi_rows_kernel) at a corpus-like shape;
never bench.py's `value`.

  --utts utterances (128) of 40 - 80 phonemes, five states each, 1 - 20 frames per state; full-context-like names of
  about 110 bytes; a question config of 1000 binary features (1 - 6 alternatives of the `*-x+*` kind, about 3000 in
  all), 30 float features and the six reserved ones: what make_train_data_dnn pipes through makefeature.pl per file.

Prints, from one process after warm-up calls: the median times of the two kernels (WorldMi355TimingQuery) over --calls
calls, distinct names x alternatives per second of label_match_kernel, frames/s of ffi_rows_kernel and its share of the
HBM peak on its write traffic of 4 x n_features bytes per frame, and the whole call's wall time (host work included:
distinct names, float features, uploads).  With --script PATH (the reference's data/scripts/makefeature.pl, where it
exists) the script is timed on one core on --perl-utts of the same files and the same config, for comparison.

Run on the GPU box: python tools/ffi_rate.py [--utts 128] [--calls 7]; where there is no GPU only the script is timed."""
import argparse
import importlib
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap_ = argparse.ArgumentParser()
ap_.add_argument("--utts", type=int, default=128)
ap_.add_argument("--calls", type=int, default=7)
ap_.add_argument("--warmup", type=int, default=2)
ap_.add_argument("--script", default=None, help="makefeature.pl, to time it on one core")
ap_.add_argument("--perl-utts", type=int, default=2)
args = ap_.parse_args()
pkg = importlib.import_module("hts-train-world_amd")
W, recipe = pkg.world, pkg.recipe

HBM_PEAK = 8.0e12                                        # bytes/s of the data sheet
SHIFT = 50000
PHONES = ["sil", "pau"] + [c + v for c in ("", "k", "s", "t", "n", "h", "m", "y", "r", "w", "g", "z", "d", "b", "p", "ch", "sh", "ts")
                           for v in "aiueo"] + ["N", "cl"]
rng = np.random.default_rng(0)


def question_config():
    text = ""
    for k in range(1000):
        pos = ("*^%s-*", "*-%s+*", "*+%s=*", "%s^*", "*=%s/A:*")[k % 5]
        alts = [pos % PHONES[int(i)] for i in rng.integers(0, len(PHONES), int(rng.integers(1, 7)))]
        text += "Q%d {%s}\n" % (k, ",".join(alts))
    for k, (field, hi) in enumerate([("A:%d+", 10), ("+%d_", 10), ("_%d/B:", 30), ("/B:%d-", 20), ("-%d@", 20), ("@%d/C:", 20)] * 5):
        text += "F%d {*%s*} MIN=%d MAX=%d\n" % (k, field, -(k % 3), hi + k)
    for name, lo, hi in zip(W.RESERVED_LABEL_FEATURES, (2, 2, 1, 1, 1, 1), (6, 6, 20, 20, 100, 100)):
        text += "%s MIN=%d MAX=%d\n" % (name, lo, hi)
    return text


def label_file(n_phones):
    ph = ["sil"] + [PHONES[int(i)] for i in rng.integers(2, len(PHONES), n_phones - 2)] + ["sil"]
    ctx = ["xx", "xx"] + ph + ["xx", "xx"]
    text, t = "", 0
    for i in range(n_phones):
        name = "%s^%s-%s+%s=%s/A:%d+%d_%d/B:%d-%d@%d/C:%02d_%02d+%02d/D:%d_%d/E:%d_%d!%d_xx-%d/F:%d_%d#%d_xx@%d_%d|%d_%d" % (
            ctx[i], ctx[i + 1], ph[i], ctx[i + 3], ctx[i + 4], *[int(v) for v in rng.integers(-9, 30, 22)])
        for s in range(2, 7):
            d = int(rng.integers(1, 21))
            text += "%d %d %s[%d]\n" % (t * SHIFT, (t + d) * SHIFT, name, s)
            t += d
    return text


config = question_config()
names, features = recipe.parse_question_config(config)
texts = [label_file(int(rng.integers(40, 81))) for _ in range(args.utts)]
labels = [recipe.parse_label(s, SHIFT) for s in texts]
frames = [sum(e - s for s, e, _, _ in lines) for lines, _ in labels]
tf, nf = int(sum(frames)), len(features)
n_alt = sum(len(p.split(",")) for k, p, _, _ in features if k == 0)
distinct = len({n for lines, _ in labels for _, _, n, _ in lines})
mean_len = float(np.mean([len(n) for lines, _ in labels for _, _, n, _ in lines]))
print("shape: %d utterances, %d lines, %d frames, %d features (%d alternatives), %d distinct names of %.0f bytes" % (
    args.utts, sum(len(l) for l, _ in labels), tf, nf, n_alt, distinct, mean_len))

if args.script:
    with tempfile.TemporaryDirectory() as tmp:
        cpath = os.path.join(tmp, "q.conf")
        with open(cpath, "w") as f:
            f.write(config)
        t0, done = time.perf_counter(), 0
        for u in range(min(args.perl_utts, args.utts)):
            lpath = os.path.join(tmp, "a.lab")
            with open(lpath, "w") as f:
                f.write(texts[u])
            out = subprocess.run(["perl", args.script, cpath, str(SHIFT), lpath], capture_output=True, check=True).stdout
            assert out.count(b"\n") == frames[u] * nf
            done += frames[u]
        dt = time.perf_counter() - t0
    print("perl makefeature.pl, one core: %d frames in %.2f s, %.3e frames/s (its text output, without x2x)" % (done, dt, done / dt))

if not torch.cuda.is_available():
    print("no GPU here: the kernels are not timed")
    sys.exit(0)

ctx = W.Context(stream_ptr=torch.cuda.current_stream().cuda_stream)
fset = W.LabelFeatureSet(ctx, features)
b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=frames)
out = torch.empty(tf, nf, dtype=torch.float32, device="cuda")
for _ in range(args.warmup):
    b.label_features(fset, labels, out=out)
    torch.cuda.synchronize()
match_ms, rows_ms, wall = [], [], []
for _ in range(args.calls):
    ctx.timing_enable(True)
    t0 = time.perf_counter()
    b.label_features(fset, labels, out=out)
    torch.cuda.synchronize()
    wall.append((time.perf_counter() - t0) * 1e3)
    m, n1 = ctx.timing_query("label_match_kernel")
    r, n2 = ctx.timing_query("ffi_rows_kernel")
    assert n1 == 1 and n2 == 1
    match_ms.append(m)
    rows_ms.append(r)
ctx.timing_enable(False)
m, r, w = float(np.median(match_ms)), float(np.median(rows_ms)), float(np.median(wall))
print("label_match_kernel (TimingQuery, median of %d calls: %s): %.3f ms, %.3e names x alternatives/s" % (
    args.calls, " ".join("%.3f" % t for t in match_ms), m, distinct * n_alt / (m * 1e-3)))
print("ffi_rows_kernel (median of %s): %.3f ms, %.3e frames/s, %.2f TB/s written = %.1f %% of the %.1f TB/s HBM peak" % (
    " ".join("%.3f" % t for t in rows_ms), r, tf / (r * 1e-3), 4.0 * nf * tf / (r * 1e-3) / 1e12,
    100.0 * 4.0 * nf * tf / (r * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12))
print("the whole call, host work included (median wall time): %.1f ms, %.3e frames/s" % (w, tf / (w * 1e-3)))
b.close()
fset.close()
ctx.close()

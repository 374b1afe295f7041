"""Rate of the modulation-spectrum postfilter and of its statistics (WorldMi355ModulationSpectrumPostfilter /
...Stats; mspf_kernel<64>, mspf_stats_kernel<64>) at the recipe's shape; never bench.py's `value`.

  1024 utterances of 400 - 1600 frames (about 1.04 M frames), 50 columns (order 49), frame_length 25, fft_length 64,
  emphasis 1.0: what gen_wave runs on every generated .mgc with USEMSPF (scripts/Training.pl:2950-3038), and what
  make_mspf (:3133-3221) runs over a training set of that size.

Prints, from one process after warm-up calls and as medians over --calls calls: each call's time between two events
on the context's stream (all of its kernels, the tables' upload included) and the time of its main kernel from
WorldMi355TimingQuery; values/s; the compulsory traffic (16 B per value: one read, one write) against the HBM peak and
the counted work (330 flop per value: per frame and column two 32-point complex transforms with their splits, 33
logarithms, exponentials, square roots and divisions, over a hop of 12 frames) against the FP64 vector peak.  Beside
it, on the same rows: mcpf_kernel (the postfilter this one replaces) and tests/mspf_reference.py in numpy on one core
(on --ref-frames frames of one utterance, scaled).

Run on the GPU box: python tools/mspf_rate.py [--utts 1024] [--calls 7]"""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import mspf_reference as R

ap_ = argparse.ArgumentParser()
ap_.add_argument("--utts", type=int, default=1024)
ap_.add_argument("--calls", type=int, default=7)
ap_.add_argument("--warmup", type=int, default=2)
ap_.add_argument("--ref-frames", type=int, default=400)
args = ap_.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
W = importlib.import_module("hts-train-world_amd").world

DIM, LW, N, E = 50, 25, 64, 1.0
FP64_PEAK, HBM_PEAK = 78.6e12, 8.0e12                   # the data sheet's vector FLOP/s and bytes/s
FLOP_PER_VALUE, BYTES_PER_VALUE = 330.0, 16.0
rng = np.random.default_rng(0)
lengths = rng.integers(400, 1601, args.utts).tolist()
tf = int(sum(lengths))
gen = torch.Generator(device="cuda").manual_seed(0)
x = torch.randn(tf, DIM, dtype=torch.float64, device="cuda", generator=gen)
x = torch.cumsum(x, 0) * 0.05                           # slow trajectories, as generated parameters are
x = (x - x.mean(0)) / (1.0 + torch.arange(DIM, dtype=torch.float64, device="cuda"))

ctx = W.Context(stream_ptr=torch.cuda.current_stream().cuda_stream)
b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=lengths)


def timed(name, fn):
    """(median ms between events around the call, median ms of the named kernel scope, all call times)."""
    whole, scope = [], []
    for _ in range(args.calls):
        ctx.timing_enable(True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms, launches = ctx.timing_query(name)
        assert launches == 1, (name, launches)
        whole.append(e0.elapsed_time(e1))
        scope.append(ms)
    ctx.timing_enable(False)
    return float(np.median(whole)), float(np.median(scope)), whole


def stats_call():
    return b.modulation_spectrum_stats(x, LW, N)


for _ in range(args.warmup):
    s1, s2, n = stats_call()
    torch.cuda.synchronize()
mean_gen, std_gen = W.mspf_finalize(s1.cpu().numpy(), s2.cpu().numpy(), n)
tabs = (mean_gen, std_gen, mean_gen + 0.1, std_gen * 1.2)


def post_call():
    return b.postfilter_modulation_spectrum(x, *tabs, emphasis=E, frame_length=LW, fft_length=N)


for _ in range(args.warmup):
    out, status = post_call()
    torch.cuda.synchronize()
assert int(status.abs().sum()) == 0 and bool(torch.isfinite(out).all())
values = tf * DIM
print("shape: %d utterances, %d frames, %d columns (%d values), frame_length %d, fft_length %d" % (
    args.utts, tf, DIM, values, LW, N))
for label, name, fn in (("postfilter", "mspf_kernel", post_call), ("statistics", "mspf_stats_kernel", stats_call)):
    whole, scope, times = timed(name, fn)
    print("%s: %.3f ms per call (events, median of %d: %s), %s scope %.3f ms; %.3e values/s; %.1f %% of the HBM peak on "
          "%.0f B per value, %.1f %% of the FP64 vector peak on %.0f flop per value" % (
              label, whole, args.calls, " ".join("%.3f" % t for t in times), name, scope, values / (whole * 1e-3),
              100.0 * BYTES_PER_VALUE * values / (whole * 1e-3) / HBM_PEAK, BYTES_PER_VALUE,
              100.0 * FLOP_PER_VALUE * values / (whole * 1e-3) / FP64_PEAK, FLOP_PER_VALUE))
    if label == "postfilter":
        post_ms = whole

for _ in range(args.warmup):
    b.postfilter_mel_cepstrum(x, 0.55, 1.4, 4096)
    torch.cuda.synchronize()
whole, scope, _ = timed("mcpf_kernel", lambda: b.postfilter_mel_cepstrum(x, 0.55, 1.4, 4096))
print("mcpf_kernel on the same rows (order 49, alpha 0.55, beta 1.4, length 4096): %.3f ms per call, %.2f x the "
      "modulation-spectrum postfilter's" % (whole, whole / post_ms))

T = min(args.ref_frames, lengths[0])
piece = x[:T].cpu().numpy()
t0 = time.perf_counter()
R.postfilter(piece, *tabs, LW, N, E)
dt = time.perf_counter() - t0
print("numpy reference on one core: %.3f s for %d frames x %d columns, %.3e values/s; the whole shape at that rate "
      "%.0f s, %.0f x the device call" % (dt, T, DIM, T * DIM / dt, values / (T * DIM / dt),
                                          values / (T * DIM / dt) / (post_ms * 1e-3)))
b.close()
ctx.close()

"""Rate of the mel-cepstral postfilter (WorldMi355MelCepstrumPostfilter, mcpf_kernel) at the recipe's shape; never
bench.py's `value`.

  1024 utterances of 400 - 1600 frames (about 1.04 M frames), order 49, alpha 0.55, beta 1.4, length 4096: what
  gen_wave runs on every generated .mgc (scripts/Training.pl:2642-2687, IMPLEN 4096).

Prints, from one process after warm-up calls: the median mcpf_kernel time of WorldMi355TimingQuery over --calls
calls (one launch each), frames/s, and the share of the FP64 vector peak on the count (L/2 + 1) (m - 1) fused
multiply-adds plus two exponentials per bin (an exponential counted as its 16 multiply-add class instructions); the
recurrence as written also spends one addition per multiply-add, which the count leaves out.  Beside it, on the same
box and frame count, mgc2sp_kernel<4096> (spectrum_from_mel_cepstrum, |H|^2 out; --mgc2sp-frames N runs fewer and scales).
The compiled reference chain's one-core rate is printed by tools/gen_golden_postfilter.py.

Run on the GPU box: python tools/postfilter_rate.py [--utts 1024] [--calls 7]"""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap_ = argparse.ArgumentParser()
ap_.add_argument("--utts", type=int, default=1024)
ap_.add_argument("--calls", type=int, default=7)
ap_.add_argument("--warmup", type=int, default=2)
ap_.add_argument("--mgc2sp-frames", type=int, default=0, help="0: the same frame count (17 GB of spectra)")
args = ap_.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
W = importlib.import_module("hts-train-world_amd").world

M, ALPHA, BETA, L = 49, 0.55, 1.4, 4096
FP64_PEAK = 78.6e12                                     # vector FLOP/s of the data sheet: 2 per fused multiply-add
rng = np.random.default_rng(0)
lengths = rng.integers(400, 1601, args.utts).tolist()
tf = int(sum(lengths))
gen = torch.Generator(device="cuda").manual_seed(0)
mc = torch.randn(tf, M + 1, dtype=torch.float64, device="cuda", generator=gen) / (
    1.0 + torch.arange(M + 1, dtype=torch.float64, device="cuda"))

ctx = W.Context(stream_ptr=torch.cuda.current_stream().cuda_stream)
b = W.WorldBatch(ctx, W.default_params(48000, 5.0, fft_size=L), f0_lengths=lengths)


def median_ms(name, fn, calls):
    times = []
    for _ in range(calls):
        ctx.timing_enable(True)
        fn()
        torch.cuda.synchronize()
        ms, launches = ctx.timing_query(name)
        assert launches == 1, (name, launches)
        times.append(ms)
    ctx.timing_enable(False)
    return float(np.median(times)), times


for _ in range(args.warmup):
    out, status = b.postfilter_mel_cepstrum(mc, ALPHA, BETA, L)
    torch.cuda.synchronize()
assert int(status.abs().sum()) == 0
ms, times = median_ms("mcpf_kernel", lambda: b.postfilter_mel_cepstrum(mc, ALPHA, BETA, L), args.calls)
fma = (L // 2 + 1) * ((M - 1) + 2 * 16)
print("shape: %d utterances, %d frames, order %d, alpha %.2f, beta %.1f, length %d" % (args.utts, tf, M, ALPHA, BETA, L))
print("mcpf_kernel (TimingQuery, median of %d calls: %s): %.3f ms per call, %.3e frames/s" % (
    args.calls, " ".join("%.3f" % t for t in times), ms, tf / (ms * 1e-3)))
print("counted work: %d multiply-adds per frame -> %.2f TFLOP/s, %.1f %% of the %.1f TFLOP/s FP64 vector peak" % (
    fma, 2.0 * fma * tf / (ms * 1e-3) / 1e12, 100.0 * 2.0 * fma * tf / (ms * 1e-3) / FP64_PEAK, FP64_PEAK / 1e12))
b.close()

n2 = min(args.mgc2sp_frames, tf) if args.mgc2sp_frames > 0 else tf
b2 = W.WorldBatch(ctx, W.default_params(48000, 5.0, fft_size=L), f0_lengths=lengths if n2 == tf else [n2])
part = mc[:n2].contiguous()
for _ in range(args.warmup):
    b2.spectrum_from_mel_cepstrum(part, ALPHA, 0.0, 4)
    torch.cuda.synchronize()
ms2, times2 = median_ms("mgc2sp_kernel", lambda: b2.spectrum_from_mel_cepstrum(part, ALPHA, 0.0, 4), args.calls)
rate2 = n2 / (ms2 * 1e-3)
print("mgc2sp_kernel<4096> beside it: %.3f ms for %d frames, %.3e frames/s; %d frames at that rate %.1f ms, %.1f x "
      "the postfilter's time" % (ms2, n2, rate2, tf, tf / rate2 * 1e3, tf / rate2 * 1e3 / ms))
b2.close()
ctx.close()

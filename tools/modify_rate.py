"""Rate of the formant shift (WorldMi355ModifyFeatures, modify_kernel = modify_sp_kernel) at two shapes; never bench.py's
`value`.

  16 kHz / fft 1024 and 48 kHz / fft 2048, --frames rows each in utterances of 400 - 1600 frames with a ratio per
  utterance drawn from [0.8, 1.25]; speech-like rows (ln sp ~ N(-10, 4)).  The rows are more than the 256 MiB Infinity
  Cache holds by default (input and output are separate blocks), so the figure is an HBM figure.

Prints, per shape, from one process after warm-up calls: the median modify_kernel time of WorldMi355TimingQuery (HIP
events around the launch) over --calls calls, frames/s, GB/s on the bytes the kernel has to move -- one read and one write
of every row, 2 x 8 x (F/2 + 1) bytes per frame; the factor table and the frame -> utterance map are left out -- and that
rate's share of the 6.29 TB/s a float4 copy reaches on this chip (8.0 TB/s on the data sheet).  In place (sp_out == sp)
is measured beside it.

Run on the GPU box: python tools/modify_rate.py [--frames 400000] [--calls 9]"""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap_ = argparse.ArgumentParser()
ap_.add_argument("--frames", type=int, default=400000)
ap_.add_argument("--calls", type=int, default=9)
ap_.add_argument("--warmup", type=int, default=3)
args = ap_.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
pkg = importlib.import_module("hts-train-world_amd")
W, M = pkg.world, pkg.modify

COPY_RATE, SPEC_RATE = 6.29e12, 8.0e12                  # bytes/s: measured float4 copy, data sheet
ctx = W.Context(stream_ptr=torch.cuda.current_stream().cuda_stream)


def median_ms(fn, calls):
    times = []
    for _ in range(calls):
        ctx.timing_enable(True)
        fn()
        torch.cuda.synchronize()
        ms, launches = ctx.timing_query("modify_kernel")
        assert launches == 1, launches
        times.append(ms)
    ctx.timing_enable(False)
    return float(np.median(times)), times


for fs, F in ((16000, 1024), (48000, 2048)):
    rng = np.random.default_rng(F)
    lengths = []
    while sum(lengths) < args.frames:
        lengths.append(int(rng.integers(400, 1601)))
    tf, bins = int(sum(lengths)), F // 2 + 1
    ratios = rng.uniform(0.8, 1.25, len(lengths))
    gen = torch.Generator(device="cuda").manual_seed(F)
    sp = torch.exp(torch.randn(tf, bins, dtype=torch.float64, device="cuda", generator=gen) * 2.0 - 10.0)
    out = torch.empty_like(sp)
    b = W.WorldBatch(ctx, W.default_params(fs, 5.0, fft_size=F), f0_lengths=lengths)
    for _ in range(args.warmup):
        M.modify_features(b, sp=sp, formant_ratio=ratios, out=(None, out))
        torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    ms, times = median_ms(lambda: M.modify_features(b, sp=sp, formant_ratio=ratios, out=(None, out)), args.calls)
    moved = 2.0 * 8.0 * bins * tf
    rate = moved / (ms * 1e-3)
    print("shape: %d Hz, fft %d, %d utterances, %d frames, %.0f MB in + %.0f MB out" % (
        fs, F, len(lengths), tf, moved / 2e6, moved / 2e6))
    print("  modify_kernel (TimingQuery, median of %d calls: %s): %.3f ms per call, %.3e frames/s" % (
        args.calls, " ".join("%.3f" % t for t in times), ms, tf / (ms * 1e-3)))
    print("  %.0f GB/s of rows read and written: %.1f %% of the %.2f TB/s copy rate, %.1f %% of the %.1f TB/s data sheet rate" % (
        rate / 1e9, 100.0 * rate / COPY_RATE, COPY_RATE / 1e12, 100.0 * rate / SPEC_RATE, SPEC_RATE / 1e12))
    keep = sp.clone()
    ms2, _ = median_ms(lambda: (sp.copy_(keep), M.modify_features(b, sp=sp, formant_ratio=ratios, out=(None, sp))), args.calls)
    print("  in place: %.3f ms per call, %.0f GB/s" % (ms2, moved / (ms2 * 1e-3) / 1e9))
    b.close()
    del sp, out, keep
ctx.close()

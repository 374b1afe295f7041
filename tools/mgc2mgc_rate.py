"""Rate of the conversion between mel-generalized cepstra (WorldMi355MelGeneralizedCepstrumConvert, mgc2mgc_kernel) in
rows per second; never bench.py's `value`.  Three shapes:

  gen_wave      (34, .55, -1/3, -n -u -> 34, .55, -1/3, plain), 10^6 rows: scripts/Training.pl:2861-2868
  gamma         (49, .42, -1 -> 49, .42, -1/3), 10^6 rows: a change of gamma at order 49
  lsp_2047      (34, .55, -1/3, -n -u -> 2047, 0, 1), 65 536 rows: postfiltering_lsp's impulse response at fl - 1 = 2047
                (:2702-2705)

Per shape, from one process: --warmup calls, then the mgc2mgc_kernel time of WorldMi355TimingQuery (device events around
the one launch) over --calls calls: median, all values, rows/s, and the counted work of the recurrence in fused
multiply-adds (two per term of gc2gc's sums) against the FP64 vector peak.  The clocks are whatever the machine's
governor gives a busy device: no performance level is set or read.  The compiled reference's one-thread rate for the
same calls is printed by tools/gen_golden_mgc2mgc.py.

Run on the GPU box: python tools/mgc2mgc_rate.py [--calls 7] [--rows 1000000] [--rows-large 65536]"""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap_ = argparse.ArgumentParser()
ap_.add_argument("--calls", type=int, default=7)
ap_.add_argument("--warmup", type=int, default=2)
ap_.add_argument("--rows", type=int, default=1000000)
ap_.add_argument("--rows-large", type=int, default=65536)
args = ap_.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
W = importlib.import_module("hts-train-world_amd").world

FP64_PEAK = 78.6e12                                     # vector FLOP/s of the data sheet: 2 per fused multiply-add
G3 = -1.0 / 3.0
# name, rows, (m1, a1, g1, n, u), (m2, a2, g2)
SHAPES = (("gen_wave", args.rows, (34, .55, G3, True, True), (34, .55, G3)),
          ("gamma", args.rows, (49, .42, -1.0, False, False), (49, .42, G3)),
          ("lsp_2047", args.rows_large, (34, .55, G3, True, True), (2047, 0.0, 1.0)))


def rows_at(n, m, g, normalized, multiplied, seed):
    """Plain rows c[k] = N(0, 1) / (1 + k), c0 uniform in [-1, 0.9] (1 + g c0 > 0 for -1 <= g < 0), in the flagged form."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.randn(n, m + 1, dtype=torch.float64, device="cuda", generator=gen) / (
        1.0 + torch.arange(m + 1, dtype=torch.float64, device="cuda"))
    c[:, 0] = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) * 1.9 - 1.0
    if normalized:
        k = 1.0 + g * c[:, 0]
        c[:, 1:] = c[:, 1:] / k[:, None]
        c[:, 0] = k ** (1.0 / g)
    elif multiplied:
        c[:, 0] = c[:, 0] * g + 1.0
    if multiplied:
        c[:, 1:] = c[:, 1:] * g
    return c


def terms(m1, m2, warp):
    """Terms of gc2gc's sums over the outputs 1 .. m2: j < i with i - j within gc2gc's input order."""
    mg = m2 if warp else m1
    return sum(min(i - 1, mg) for i in range(1, m2 + 1))


ctx = W.Context(stream_ptr=torch.cuda.current_stream().cuda_stream)
for seed, (name, n, (m1, a1, g1, nf, uf), (m2, a2, g2)) in enumerate(SHAPES):
    mc = rows_at(n, m1, g1, nf, uf, seed)
    b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=[n])
    call = lambda: b.convert_mel_generalized_cepstrum(mc, a1, g1, m2, a2, g2, nf, uf)
    for _ in range(args.warmup):
        out, status = call()
        torch.cuda.synchronize()
    flagged = int((status != 0).sum())
    times = []
    for _ in range(args.calls):
        ctx.timing_enable(True)
        call()
        torch.cuda.synchronize()
        ms, launches = ctx.timing_query("mgc2mgc_kernel")
        assert launches == 1, launches
        times.append(ms)
    ctx.timing_enable(False)
    ms = float(np.median(times))
    fma = 2 * terms(m1, m2, a1 != a2)
    print("%-9s (%d, %.2f, %.3f%s -> %d, %.2f, %.3f), %d rows, %d flagged: median of %d calls %.3f ms (%s), %.3e rows/s; "
          "%d multiply-adds per row -> %.2f TFLOP/s, %.1f %% of the FP64 vector peak; bytes in + out %.2f GB -> %.0f GB/s" % (
              name, m1, a1, g1, " -n -u" if nf else "", m2, a2, g2, n, flagged, args.calls, ms,
              " ".join("%.3f" % t for t in times), n / (ms * 1e-3), fma, 2.0 * fma * n / (ms * 1e-3) / 1e12,
              100.0 * 2.0 * fma * n / (ms * 1e-3) / FP64_PEAK, 8e-9 * n * (m1 + m2 + 2), 8e-9 * n * (m1 + m2 + 2) / (ms * 1e-3)),
          flush=True)
    b.close()
    del mc, out, status
ctx.close()

"""Rates of the MGC-LSP route (csrc/lsp.hip, the energy form of mgc2mgc_kernel); never bench.py's `value`.

  lsp_kernel    lsp.lsp_to_lpc at order 34, 10^6 rows: rows/s of the one launch
  energy        mgc2mgc_kernel at (34, .55, -1/3, -n -u -> 2047, 0, 1), 65 536 rows, postfiltering_lsp's conversion at
                fl = 2048: the energy form (one double per row out; two launches per lsp.postfilter_lsp call, the time
                halved) against the storing form on the same LPC rows (WorldBatch.convert_mel_generalized_cepstrum: 16 KB
                per row out), in ALTERNATING calls of one process, so that both see the same clocks.  The storing form is
                the parent commit's kernel: its instantiations are compiled from the same source text.
  postfilter    lsp.postfilter_lsp with compensation at order 34, length 4096, 65 536 frames: frames/s of the whole call
                (two lsp_kernel launches, two conversions of 4095 coefficients, the gain), between two events

Kernel times are WorldMi355TimingQuery's (device events around the launches) after --warmup calls, over --calls calls:
median, least and largest.  The clocks are whatever the machine's governor gives a busy device: no performance level is
set or read.

Run on the GPU box: python tools/lsp_rate.py [--calls 7] [--rows 1000000] [--rows-large 65536]"""
import argparse
import importlib
import math
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
pkg = importlib.import_module("hts-train-world_amd")
W, lsp = pkg.world, importlib.import_module("hts-train-world_amd.lsp")

M, ALPHA, GAMMA = 34, 0.55, -1.0 / 3.0


def rows_at(n, seed):
    """Jittered evenly spaced LSPs behind a log gain in [-3, 2]."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    k = torch.arange(1, M + 1, dtype=torch.float64, device="cuda")
    w = math.pi / (M + 1) * (k + 0.6 * torch.rand(n, M, dtype=torch.float64, device="cuda", generator=gen) - 0.3)
    g = 5.0 * torch.rand(n, 1, dtype=torch.float64, device="cuda", generator=gen) - 3.0
    return torch.cat([g, w], dim=1).contiguous()


def timed(ctx, name, call):
    ctx.timing_enable(True)
    out = call()
    torch.cuda.synchronize()
    ms, launches = ctx.timing_query(name)
    ctx.timing_enable(False)
    return ms, launches, out


def report(what, n, times, unit="rows"):
    ms = float(np.median(times))
    print("%s: %d %s, median of %d calls %.3f ms (least %.3f, largest %.3f: spread %.1f %%) -> %.3e %s/s" % (
        what, n, unit, len(times), ms, min(times), max(times), 100.0 * (max(times) - min(times)) / ms, n / (ms * 1e-3), unit),
        flush=True)
    return ms


ctx = W.Context(stream_ptr=torch.cuda.current_stream().cuda_stream)

# ---- lsp_kernel
n = args.rows
x = rows_at(n, 0)
b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=[n])
call = lambda: lsp.lsp_to_lpc(b, x, ALPHA, GAMMA, True)
for _ in range(args.warmup):
    lpc, status = call()
    torch.cuda.synchronize()
print("lsp_kernel: %d of %d rows flagged or changed" % (int((status != 0).sum()), n))
times = []
for _ in range(args.calls):
    ms, launches, _ = timed(ctx, "lsp_kernel", call)
    assert launches == 1, launches
    times.append(ms)
report("lsp_kernel, order %d" % M, n, times)
b.close()
del x, lpc, status

# ---- the energy form against the storing form, alternating
n = args.rows_large
x = rows_at(n, 1)
b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=[n])
lpc, _ = lsp.lsp_to_lpc(b, x, ALPHA, GAMMA, True)
store = lambda: b.convert_mel_generalized_cepstrum(lpc, ALPHA, GAMMA, 2047, 0.0, 1.0, True, True)
energy = lambda: lsp.postfilter_lsp(b, x, ALPHA, GAMMA, 0.7, 2048, False, True, energies=True)
for _ in range(args.warmup):
    c2, st = store()
    out, e1, e2, st2 = energy()
    torch.cuda.synchronize()
own = 0.5 * torch.log((c2 * c2).sum(dim=1))
print("energy form against the storing form's own sum: max |difference| %.3e over %d rows, %d flagged" % (
    float((own - e1).abs().max()), n, int(((st2 & 12) != 0).sum())))
del c2, st, out, e1, e2, st2, own
t_store, t_energy = [], []
for _ in range(args.calls):
    ms, launches, _ = timed(ctx, "mgc2mgc_kernel", store)
    assert launches == 1, launches
    t_store.append(ms)
    ms, launches, _ = timed(ctx, "mgc2mgc_kernel", energy)
    assert launches == 2, launches
    t_energy.append(ms / 2.0)
a = report("storing form (34, .55, -1/3 -n -u -> 2047, 0, 1)", n, t_store)
e = report("energy form, per launch, the same option set", n, t_energy)
print("energy / storing: %.3f of the time" % (e / a), flush=True)
b.close()

# ---- the postfilter, compensation 1, length 4096
b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=[n])
call = lambda: lsp.postfilter_lsp(b, x, ALPHA, GAMMA, 0.7, 4096, True, True)
for _ in range(args.warmup):
    call()
    torch.cuda.synchronize()
times = []
for _ in range(args.calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    call()
    t1.record()
    torch.cuda.synchronize()
    times.append(t0.elapsed_time(t1))
report("postfilter_lsp, compensation 1, order %d, length 4096" % M, n, times, "frames")
b.close()
ctx.close()

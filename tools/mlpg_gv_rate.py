"""Rate of parameter generation considering global variance (WorldMi355ParameterGenerationGv: mlpg_kernel for the start,
then mlpg_gv_kernel) at the shape of tools/mlpg_rate.py; never bench.py's `value`.

  1024 utterances of 400 - 1600 frames; mgc 50 x 3, lf0 1 x 3 behind its voicing column, bap 25 x 3: one `ffo` matrix
  of 229 columns, one variance row, edge 0.  The GV mean of a column is three times the mean over the utterances of
  the variance that plain parameter generation leaves, its standard deviation a fifth of that: every column has work to
  do.  Options: the recipe's defaults (50 trials at most, epsilon 1e-4), and --max-iter / --epsilon.

Prints, from one process after warm-up calls: frames/s of the call (host clock around calls that end in a synchronise),
the mlpg_kernel and mlpg_gv_kernel times of WorldMi355TimingQuery, the trials and accepted trials per column from `info`,
the kernel's time per trial and column-frame, and the workspace the call holds (B + 2 doubles per frame and column).

Run on the GPU box: python tools/mlpg_gv_rate.py [--utts 1024] [--calls 5]"""
import argparse
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap_ = argparse.ArgumentParser()
ap_.add_argument("--utts", type=int, default=1024)
ap_.add_argument("--calls", type=int, default=5)
ap_.add_argument("--warmup", type=int, default=2)
ap_.add_argument("--max-iter", type=int, default=None)
ap_.add_argument("--epsilon", type=float, default=None)
args = ap_.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
W = importlib.import_module("hts-train-world_amd").world

WINS = [[1.0], [-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]]
DIMS, MSD = (50, 1, 25), (False, True, False)
rng = np.random.default_rng(0)
lengths = rng.integers(400, 1601, args.utts).tolist()
tf = int(sum(lengths))
width = sum(3 * d + m for d, m in zip(DIMS, MSD))
gen = torch.Generator(device="cuda").manual_seed(0)
rows = torch.randn(tf, width, dtype=torch.float32, device="cuda", generator=gen)
var = torch.exp(torch.empty(width, dtype=torch.float32, device="cuda").uniform_(-3.0, 3.0, generator=gen))
streams, at = [], 0
for d, m in zip(DIMS, MSD):
    msd = None
    if m:
        rows[:, at] = torch.rand(tf, device="cuda", generator=gen)
        msd, at = rows[:, at], at + 1
    streams.append((rows[:, at:at + 3 * d], var[at:at + 3 * d], WINS, msd))
    at += 3 * d

ctx = W.Context(stream_ptr=torch.cuda.current_stream().cuda_stream)
b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=lengths)
plain, _ = b.parameter_generation([(m, v, w, None) for m, v, w, _ in streams])
utt = torch.repeat_interleave(torch.arange(args.utts, device="cuda"), torch.tensor(lengths, device="cuda"))
gv_mean, gv_var = [], []
for o in plain:                                            # per-utterance variance of every column, then its mean
    x = o.double()
    n = torch.tensor(lengths, device="cuda", dtype=torch.float64)[:, None]
    s1 = torch.zeros(args.utts, x.shape[1], dtype=torch.float64, device="cuda").index_add_(0, utt, x) / n
    s2 = torch.zeros_like(s1).index_add_(0, utt, (x - s1[utt]) ** 2) / n
    gm = (3.0 * s2.mean(dim=0)).float()
    gv_mean.append(gm)
    gv_var.append((0.2 * gm) ** 2)
del plain
opts = {k: v for k, v in (("max_iter", args.max_iter), ("epsilon", args.epsilon)) if v is not None}


def call():
    out = b.parameter_generation_gv(streams, gv_mean, gv_var, want_info=True, **opts)
    torch.cuda.synchronize()
    return out


for _ in range(args.warmup):
    outs, status, info = call()
print("status bits over the batch: %d" % int(np.bitwise_or.reduce(status.cpu().numpy())))
ctx.timing_enable(True)
t0 = time.perf_counter()
for _ in range(args.calls):
    call()
wall = (time.perf_counter() - t0) / args.calls
ms_gv, n_gv = ctx.timing_query("mlpg_gv_kernel")
ms_ml, n_ml = ctx.timing_query("mlpg_kernel")
ctx.timing_enable(False)
kern, start = ms_gv / n_gv * 1e-3, ms_ml / n_ml * 1e-3
cols = sum(DIMS)
trials, accepts = info[:, :, 2].cpu().numpy(), info[:, :, 3].cpu().numpy()
work = float((trials * np.asarray(lengths)[:, None]).sum())             # trials x frames, over the columns
print("shape: %d utterances, %d frames, %d columns, row stride %d floats" % (args.utts, tf, cols, width))
print("call (binding + both launches + synchronise): %.3f ms, %.3e frames/s" % (wall * 1e3, tf / wall))
print("mlpg_kernel, the start (TimingQuery, mean of %d launches): %.3f ms" % (n_ml, start * 1e3))
print("mlpg_gv_kernel (TimingQuery, mean of %d launches): %.3f ms, %.3e frames/s" % (n_gv, kern * 1e3, tf / kern))
print("trials per column: mean %.1f, largest %d; accepted: mean %.1f" % (trials.mean(), int(trials.max()), accepts.mean()))
print("kernel time per trial and column-frame: %.3f ns (%.3e trial-column-frames)" % (kern / work * 1e9, work))
print("workspace: %d doubles per frame and column, %.3f GB for the batch" % (4 + 2, tf * cols * 6 * 8 / 1e9))
b.close()
ctx.close()

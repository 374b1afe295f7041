"""Rate of the trajectory training criterion (WorldMi355TrajectoryCost, trj_kernel + trj_reduce_kernel) at the recipe's
shape; never bench.py's `value`.

  1024 utterances of 400 - 1600 frames; mgc 50 x 3, lf0 1 x 3 behind its voicing column, bap 25 x 3: model outputs and
  targets as two `ffo` matrices of 229 columns, one variance row, gv.var of 76 (what DNNTraining.py -w win evaluates
  one utterance at a time, data/scripts/DNNDefine.py:240-399).

Prints, from one process after warm-up calls: frames/s of the call with every output (host clock around calls that end
in a synchronise), the "trj_kernel" time of WorldMi355TimingQuery (the column kernels and the reduction as one record),
the same without the gradients' outputs, the compulsory bytes and the workspace bytes the four sweeps move, and the
time of reference (a) of tests/trj_reference.py -- the reference's dense construction in torch float64 with autograd
-- on one host core over the --host-utts SHORTEST utterances, scaled by frames (its cost grows with T^3, so the scaled
figure flatters it), with the largest difference between its costs and the kernel's.

Run on the GPU box: python tools/trj_rate.py [--utts 1024] [--calls 10]"""
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

ap_ = argparse.ArgumentParser()
ap_.add_argument("--utts", type=int, default=1024)
ap_.add_argument("--calls", type=int, default=10)
ap_.add_argument("--warmup", type=int, default=2)
ap_.add_argument("--host-utts", type=int, default=2)
args = ap_.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
pkg = importlib.import_module("hts-train-world_amd")
W, training = pkg.world, pkg.training

WINS = [[1.0], [-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]]
LAYOUT = [(50, WINS, False), (1, WINS, True), (25, WINS, False)]
HBM_PEAK = 8.0e12
rng = np.random.default_rng(0)
lengths = rng.integers(400, 1601, args.utts).tolist()
tf = int(sum(lengths))
cols = sum(d for d, _, _ in LAYOUT)
width = sum(3 * d + m for d, _, m in LAYOUT)
gen = torch.Generator(device="cuda").manual_seed(0)
pred = torch.randn(tf, width, dtype=torch.float32, device="cuda", generator=gen)
obs = pred + 0.3 * torch.randn(tf, width, dtype=torch.float32, device="cuda", generator=gen)
var = torch.exp(torch.empty(width, dtype=torch.float32, device="cuda").uniform_(-3.0, 3.0, generator=gen))
gv_var = torch.exp(torch.empty(cols, dtype=torch.float32, device="cuda").uniform_(-3.0, 0.0, generator=gen))
views = training.stream_views(pred, obs, LAYOUT)

ctx = W.Context(stream_ptr=torch.cuda.current_stream().cuda_stream)
b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=lengths)


def call(**want):
    out = b.trajectory_cost(views, var, gv_var, 1.0, 1.0, **want)
    torch.cuda.synchronize()
    return out


def timed(**want):
    for _ in range(args.warmup):
        out = call(**want)
    assert int(out[4].abs().sum()) == 0
    ctx.timing_enable(True)
    t0 = time.perf_counter()
    for _ in range(args.calls):
        call(**want)
    wall = (time.perf_counter() - t0) / args.calls
    ms, launches = ctx.timing_query("trj_kernel")
    ctx.timing_enable(False)
    return out, wall, ms / launches * 1e-3, launches


out, wall, kern, launches = timed()
_, wall_c, kern_c, _ = timed(want_grad_pred=False, want_grad_var=False)
# float32 in: 3 windows of pred, the static window of obs (read by sweeps 1 and 4), the voicing columns; out: c, grad_pred
compulsory = tf * ((3 * cols + cols + 2) * 4 + (cols + 3 * cols + 1) * 4)
# per frame and column 4 doubles (B = 2): written by sweep 1, read and one rewritten by each of sweeps 2 - 4
workspace = tf * cols * 8 * (4 + (4 + 1) + (4 + 1) + 4)
print("shape: %d utterances, %d frames, %d columns, row stride %d floats" % (args.utts, tf, cols, width))
print("call, every output (binding + launches + synchronise): %.3f ms, %.3e frames/s" % (wall * 1e3, tf / wall))
print("trj_kernel (TimingQuery, mean of %d calls): %.3f ms, %.3e frames/s" % (launches, kern * 1e3, tf / kern))
print("trj_kernel without grad_pred and grad_var: %.3f ms (call %.3f ms)" % (kern_c * 1e3, wall_c * 1e3))
print("compulsory bytes: %d per frame, %.3f GB per call -> %.3f TB/s, %.1f %% of the 8 TB/s HBM peak"
      % (compulsory // tf, compulsory / 1e9, compulsory / kern / 1e12, 100.0 * compulsory / kern / HBM_PEAK))
print("workspace bytes moved: %d per frame, %.3f GB per call; with them %.3f TB/s, %.1f %% of the peak"
      % (workspace // tf, workspace / 1e9, (compulsory + workspace) / kern / 1e12,
         100.0 * (compulsory + workspace) / kern / HBM_PEAK))

# ---- reference (a), the reference's dense construction, on one host core ---------------------------------------------
try:
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
except (AttributeError, OSError):
    pass
torch.set_num_threads(1)
import trj_reference as R

off = np.concatenate([[0], np.cumsum(lengths)])
short = np.argsort(lengths)[:min(args.host_utts, args.utts)]
h_var, h_gv = var.cpu().numpy(), gv_var.cpu().numpy()
cost = out[0].cpu().numpy()
t_host, hf, worst = 0.0, 0, 0.0
for u in short:
    p_, o_ = pred[off[u]:off[u + 1]].cpu().numpy(), obs[off[u]:off[u + 1]].cpu().numpy()
    t0 = time.perf_counter()
    a = R.dense(p_, o_, h_var, h_gv, LAYOUT, 1.0, 1.0, want_cond=False)
    t_host += time.perf_counter() - t0
    hf += lengths[u]
    worst = max(worst, float((np.abs(a["cost"] - cost[u]) / np.maximum(np.abs(a["cost"]), 1e-300)).max()))
print("reference (a), dense float64 + autograd, one host core: %.3f s for %d frames (the %d shortest utterances) = "
      "%.3e frames/s; the whole shape at that rate %.1f s, %.0f x the kernel's time"
      % (t_host, hf, len(short), hf / t_host, tf / (hf / t_host), tf / (hf / t_host) / kern))
print("kernel against (a) on those utterances: worst relative difference of a cost term %.3e" % worst)
b.close()
ctx.close()

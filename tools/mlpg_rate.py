"""Rate of parameter generation (WorldMi355ParameterGeneration, mlpg_kernel) at the recipe's shape; never bench.py's
`value`.

  1024 utterances of 400 - 1600 frames; mgc 50 x 3, lf0 1 x 3 behind its voicing column, bap 25 x 3: one `ffo` matrix
  of 229 columns, one variance row, edge 0 (what gen_param runs, scripts/Training.pl:2755-2810).

Prints, from one process after warm-up calls: frames/s of the call (host clock around calls that end in a synchronise),
the mlpg_kernel time of WorldMi355TimingQuery, the compulsory bytes (228 float32 read and 76 written per frame: 1216 B)
and the workspace bytes the factor moves (written by the forward sweep, read by the backward one), the share of the
8 TB/s HBM peak both ways, and the time of scipy.linalg.solveh_banded over the same columns on one host core (timed
on --host-utts utterances, compared with the kernel's output on them, and scaled by frames).

Run on the GPU box: python tools/mlpg_rate.py [--utts 1024] [--calls 10]"""
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
ap_.add_argument("--calls", type=int, default=10)
ap_.add_argument("--warmup", type=int, default=2)
ap_.add_argument("--host-utts", type=int, default=8)
args = ap_.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
W = importlib.import_module("hts-train-world_amd").world

WINS = [[1.0], [-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]]
DIMS, MSD = (50, 1, 25), (False, True, False)
HBM_PEAK = 8.0e12
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


def call():
    out = b.parameter_generation(streams)
    torch.cuda.synchronize()
    return out


for _ in range(args.warmup):
    outs, status = call()
assert int(status.abs().sum()) == 0
ctx.timing_enable(True)
t0 = time.perf_counter()
for _ in range(args.calls):
    call()
wall = (time.perf_counter() - t0) / args.calls
ms, launches = ctx.timing_query("mlpg_kernel")
ctx.timing_enable(False)
kern = ms / launches * 1e-3
cols = sum(DIMS)
compulsory = tf * (3 * cols + cols) * 4
workspace = tf * cols * 3 * 8 * 2                       # z / d and two multipliers per frame and column, out and back
print("shape: %d utterances, %d frames, %d columns, row stride %d floats" % (args.utts, tf, cols, width))
print("call (binding + launch + synchronise): %.3f ms, %.3e frames/s" % (wall * 1e3, tf / wall))
print("mlpg_kernel (TimingQuery, mean of %d launches): %.3f ms, %.3e frames/s" % (launches, kern * 1e3, tf / kern))
print("compulsory bytes: %d per frame, %.3f GB per call -> %.3f TB/s, %.1f %% of the 8 TB/s HBM peak"
      % (compulsory // tf, compulsory / 1e9, compulsory / kern / 1e12, 100.0 * compulsory / kern / HBM_PEAK))
print("workspace bytes moved: %d per frame, %.3f GB per call; with them %.3f TB/s, %.1f %% of the peak"
      % (workspace // tf, workspace / 1e9, (compulsory + workspace) / kern / 1e12,
         100.0 * (compulsory + workspace) / kern / HBM_PEAK))

# ---- the same columns by scipy's banded Cholesky on one host core ----------------------------------------------------
try:
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
except (AttributeError, OSError):
    pass
torch.set_num_threads(1)
from scipy import sparse
from scipy.linalg import solveh_banded

n_host = min(args.host_utts, args.utts)
off = np.concatenate([[0], np.cumsum(lengths)])
h_rows = rows[:off[n_host]].cpu().numpy().astype(np.float64)
h_prec = 1.0 / var.cpu().numpy().astype(np.float64)
h_out = [o[:off[n_host]].cpu().numpy() for o in outs]
worst, t_host = 0.0, 0.0
for u in range(n_host):
    T = lengths[u]
    t0 = time.perf_counter()
    Wm = [sparse.diags(w, [k - (len(w) - 1) // 2 for k in range(len(w))], shape=(T, T), format="csr") for w in WINS]
    G = [(m.T @ m).todia() for m in Wm]
    band = np.zeros((3, 3, T))                            # window, upper-band row (2 - offset), column
    for i, g in enumerate(G):
        for o_, d_ in zip(g.offsets, g.data):
            if 0 <= o_ <= 2:
                band[i, 2 - o_, :] = d_[:T]
    res, at = [], 0
    for d, m in zip(DIMS, MSD):
        at += 1 if m else 0
        mu = h_rows[off[u]:off[u + 1], at:at + 3 * d]
        p = h_prec[at:at + 3 * d]
        rhs = sum((Wm[i].T @ mu[:, i * d:(i + 1) * d]) * p[None, i * d:(i + 1) * d] for i in range(3))
        c = np.empty((T, d))
        for j in range(d):
            ab = sum(p[i * d + j] * band[i] for i in range(3))
            c[:, j] = solveh_banded(ab, rhs[:, j])
        res.append(c)
        at += 3 * d
    t_host += time.perf_counter() - t0
    for s, c in enumerate(res):
        g_ = h_out[s][off[u]:off[u + 1]].astype(np.float64)
        keep = g_[:, 0] != -1e10 if MSD[s] else np.ones(T, bool)
        worst = max(worst, float((np.abs(g_ - c)[keep] / np.maximum(np.abs(c[keep]), 1.0)).max()))
hf = int(off[n_host])
print("scipy.linalg.solveh_banded, one host core: %.3f s for %d frames (%d utterances) = %.3e frames/s; "
      "the whole shape at that rate %.1f s, %.0f x the kernel's time" % (t_host, hf, n_host, hf / t_host,
                                                                       tf / (hf / t_host), tf / (hf / t_host) / kern))
print("kernel against scipy on those utterances: worst |difference| / max(|c|, 1) = %.3e (float32 output)" % worst)
b.close()
ctx.close()

"""Rate of the DTW alignment (WorldMi355DtwAlign: dtw_kernel, dtw_path_kernel) in cells per second; never bench.py's
`value`.

  batches of 64, 256 and 1024 pairs of 400 - 1600 frames on each side at count 49 (mgc of order 49 without c0), and one
  pair of 1600 x 1600 alone.

One wavefront fills one pair's T_a x T_b cells, so a batch takes as long as its longest pairs while the wavefronts fit the
device at once.  Per shape, from one process after a warm-up call: the median over --calls calls (host clock around a call
that ends in a device synchronise), cells/s, the two kernels' own times (WorldMi355TimingQuery, one call) and the
workspace.  Beside it the numpy statement of the definition (tests/dtw_reference.py, a Python loop over the cells) on one
host core for one pair of --host-frames frames.  Prints one JSON line.  Stops by itself: a shape is not started once
--time-limit seconds have passed, and SIGALRM ends the process shortly after.

Run on the GPU box: python tools/dtw_rate.py [--calls 3] [--pairs 64 256 1024]"""
import argparse
import importlib
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

ap_ = argparse.ArgumentParser()
ap_.add_argument("--pairs", type=int, nargs="+", default=[64, 256, 1024])
ap_.add_argument("--count", type=int, default=49)
ap_.add_argument("--calls", type=int, default=3)
ap_.add_argument("--host-frames", type=int, default=300)
ap_.add_argument("--time-limit", type=float, default=240.0)
args = ap_.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
signal.alarm(int(args.time_limit) + 60)
t_start = time.perf_counter()
W = importlib.import_module("hts-train-world_amd").world
import dtw_reference as R

ctx = W.Context(stream_ptr=torch.cuda.current_stream().cuda_stream)
result = {"tool": "dtw_rate", "count": args.count, "shapes": []}
for n_pairs in [1] + args.pairs:
    if time.perf_counter() - t_start > args.time_limit:
        result["stopped_before_pairs"] = n_pairs
        break
    rng = np.random.default_rng(n_pairs)
    ta = [1600] if n_pairs == 1 else rng.integers(400, 1601, n_pairs).tolist()
    tb = [1600] if n_pairs == 1 else rng.integers(400, 1601, n_pairs).tolist()
    cells = int(sum(x * y for x, y in zip(ta, tb)))
    gen = torch.Generator(device="cuda").manual_seed(n_pairs)
    # random walks: neighbouring frames are close, as cepstra are (timing only; the tests hold the bits)
    a = torch.cumsum(0.1 * torch.randn(sum(ta), args.count, device="cuda", generator=gen), 0).float().contiguous()
    b = torch.cumsum(0.1 * torch.randn(sum(tb), args.count, device="cuda", generator=gen), 0).float().contiguous()
    batch = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=ta)

    def call():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = batch.dtw_align(a, b, tb, 0, args.count)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    _, (path, n, cost, status) = call()
    assert int(status.abs().max()) == 0 and bool(torch.isfinite(cost).all()) and int(n.min()) > 0
    ts = [call()[0] for _ in range(args.calls)]
    ctx.timing_enable(True)
    call()
    fill_ms, l1 = ctx.timing_query("dtw_kernel")
    walk_ms, l2 = ctx.timing_query("dtw_path_kernel")
    ctx.timing_enable(False)
    assert (l1, l2) == (1, 1), (l1, l2)
    med = float(np.median(ts))
    result["shapes"].append({"pairs": n_pairs, "cells": cells, "ms_per_call": 1e3 * med, "cells_per_s": cells / med,
                             "dtw_kernel_ms": fill_ms, "dtw_path_kernel_ms": walk_ms,
                             "path_pairs": int(n.sum()), "workspace_bytes": W.dtw_workspace_bytes(ta, tb)})
    batch.close()
    del a, b, path, n, cost, status
ctx.close()
t = args.host_frames
ha, hb = R.inputs(t, t, args.count, seed=1)
t0 = time.perf_counter()
R.dtw(ha, hb)
host = time.perf_counter() - t0
result["numpy_reference"] = {"frames": [t, t], "seconds": host, "cells_per_s": t * t / host}
signal.alarm(0)
print(json.dumps(result), flush=True)

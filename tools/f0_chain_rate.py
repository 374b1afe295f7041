"""What the f0 estimator of the one-call form costs (WorldMi355BatchSetF0Estimator); never bench.py's `value`.

  BASELINE.json configs[1]'s shape: 256 synthetic utterances of 2 - 8 s at 16 kHz, 5 ms hop, one batch per setting.

Prints, from one process after warm-up passes and with the variants alternated pass by pass (all see the same clocks
and the same cache state), the milliseconds of one analyze_synthesize pass for (dio, refine), (harvest, no refine) and
(harvest, refine), and beside each the sum of the same stages called one by one on the same batch: what the one-call
form's side streams hide.  Also Harvest's workspace for the batch, as WorldMi355HarvestWorkspaceBytes says it on the host
and as the device's free memory shows it.

Run on the GPU box: python tools/f0_chain_rate.py [--utts 256] [--passes 10] [--time-limit 300]"""
import argparse
import importlib
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

ap_ = argparse.ArgumentParser()
ap_.add_argument("--utts", type=int, default=256)
ap_.add_argument("--passes", type=int, default=10)
ap_.add_argument("--warmup", type=int, default=3)
ap_.add_argument("--workers", type=int, default=8, help="processes that make the synthetic utterances")
ap_.add_argument("--time-limit", type=int, default=300, help="seconds after which the run ends itself")
args = ap_.parse_args()
signal.alarm(args.time_limit)
pkg = importlib.import_module("hts-train-world_amd")
W, sd = pkg.world, pkg.synth_data
FS, FP = 16000, 5.0
xs = sd.make_batch(args.utts, FS, (2.0, 8.0), workers=args.workers)          # before the GPU is touched: it forks
assert torch.cuda.is_available(), "this measurement needs the GPU"

VARIANTS = [("dio", True), ("harvest", False), ("harvest", True)]
lens = [len(v) for v in xs]
params = W.default_params(FS, FP)
x = torch.from_numpy(np.concatenate(xs)).cuda()
ctx = W.Context(stream_ptr=torch.cuda.current_stream().cuda_stream)
planned = W.harvest_workspace_bytes(params, lens)
batches, taken = {}, {}
for est, refine in VARIANTS:
    batches[est, refine] = b = W.WorldBatch(ctx, params, x_lengths=lens, f0_estimator=est, refine=refine)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    if est == "harvest":
        b.harvest(x)                                 # the set-up alone: what the workspace takes from the device
        torch.cuda.synchronize()
        taken[est, refine] = free0 - torch.cuda.mem_get_info()[0]
b0 = batches["dio", True]
frames = int(b0.total_frames)
outs = (torch.empty(frames, dtype=torch.float64, device="cuda"), torch.empty(frames, dtype=torch.float64, device="cuda"),
        torch.empty(frames, b0.bins, dtype=torch.float64, device="cuda"),
        torch.empty(frames, b0.bins, dtype=torch.float64, device="cuda"))
y = torch.empty(int(b0.total_out), dtype=torch.float64, device="cuda")


def one_call(b):
    b.analyze_synthesize(x, out=outs, y=y)
    torch.cuda.synchronize()


def staged(b):
    t, f0 = b.harvest(x) if b.f0_estimator == "harvest" else b.dio(x)
    if b.refine:
        f0 = b.stonemask(x, t, f0)
    b.cheaptrick(x, t, f0, out=outs[2])
    b.d4c(x, t, f0, out=outs[3])
    b.synthesize(f0, outs[2], outs[3], out=y)
    torch.cuda.synchronize()


calls = [(v, kind, fn) for v in VARIANTS for kind, fn in (("one call", one_call), ("stage by stage", staged))]
for _ in range(args.warmup):
    for v, kind, fn in calls:
        fn(batches[v])
times = {(v, kind): [] for v, kind, _ in calls}
for _ in range(args.passes):                         # alternating: variant by variant inside every pass
    for v, kind, fn in calls:
        t0 = time.perf_counter()
        fn(batches[v])
        times[v, kind].append(time.perf_counter() - t0)
print("shape: %d utterances, %.0f s of audio at %d Hz, %d frames at %g ms; %d passes after %d warm-up passes, alternated"
      % (args.utts, sum(lens) / FS, FS, frames, FP, args.passes, args.warmup))
for v in VARIANTS:
    a, s = np.array(times[v, "one call"]) * 1e3, np.array(times[v, "stage by stage"]) * 1e3
    print("(%s, refine %d): analyze_synthesize %.2f ms (median; %.2f - %.2f), %.3e frames/s; stages one by one %.2f ms "
          "(%.2f - %.2f)" % (v[0], v[1], np.median(a), a.min(), a.max(), frames / (np.median(a) * 1e-3), np.median(s),
                             s.min(), s.max()))
print("Harvest's workspace for this batch: %.2f GiB planned on the host (%.1f KB per 1 ms frame), %s GiB taken from the "
      "device by the set-up" % (planned / 2.0 ** 30, planned / 1e3 / (1000.0 * sum(lens) / FS),
                                " / ".join("%.2f" % (v / 2.0 ** 30) for v in taken.values())))
for b in batches.values():
    b.close()
ctx.close()

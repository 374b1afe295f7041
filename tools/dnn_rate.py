"""Rate of the acoustic model's forward pass (WorldMi355AcousticModelForward, dnn_layer_kernel) at the recipe's
configured size; never bench.py's `value`.

  1024 utterances of 400 - 1600 frames (the frames of tools/mlpg_rate.py and tools/trj_rate.py) through three hidden
  layers of 2048 sigmoid units to 229 linear outputs (config.status:600-601).  n_inputs = 1024 is a STAND-IN: the real
  width is the number of questions of the question set plus the numeric features, which the recipe's data decide.

Prints, from one process after warm-up calls and with the two alternating call by call: the "dnn_layer_kernel" time of
WorldMi355TimingQuery (the input check and all layers of a call as one record) with frames/s, the achieved TFLOP/s and
its share of the 157.3 TFLOP/s FP32 matrix peak, the workspace bytes moved per frame; beside it the same layers as a
torch float32 addmm + activation chain on the same tensors in the same 65 536-frame chunks (the vendor GEMM); and the
numpy float64 reference (tests/dnn_reference.py) on one host core over --host-frames frames, scaled by frames.

Run on the GPU box: python tools/dnn_rate.py [--utts 1024] [--calls 10] [--time-limit 300]"""
import argparse
import importlib
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
ap_.add_argument("--utts", type=int, default=1024)
ap_.add_argument("--calls", type=int, default=10)
ap_.add_argument("--warmup", type=int, default=2)
ap_.add_argument("--inputs", type=int, default=1024)
ap_.add_argument("--units", type=int, default=2048)
ap_.add_argument("--layers", type=int, default=3)
ap_.add_argument("--outputs", type=int, default=229)
ap_.add_argument("--host-frames", type=int, default=256)
ap_.add_argument("--time-limit", type=int, default=300, help="seconds after which the run ends itself")
args = ap_.parse_args()
signal.alarm(args.time_limit)
assert torch.cuda.is_available(), "this measurement needs the GPU"
pkg = importlib.import_module("hts-train-world_amd")
W, training = pkg.world, pkg.training

PEAK = 157.3e12
CHUNK = 65536
rng = np.random.default_rng(0)
lengths = rng.integers(400, 1601, args.utts).tolist()
tf = int(sum(lengths))
torch.manual_seed(0)
model = training.AcousticModel(args.inputs, [args.units] * args.layers, args.outputs, 1, "sigmoid", "linear").cuda()
with torch.no_grad():
    for name, p in model.named_parameters():
        if name.endswith("si_biases"):
            p.normal_(0.0, 0.1)
gen = torch.Generator(device="cuda").manual_seed(0)
x = torch.randn(tf, args.inputs, dtype=torch.float32, device="cuda", generator=gen)
x[:, :args.inputs // 2] = (x[:, :args.inputs // 2] > 0).to(torch.float32)          # half the columns binary
ka = model.kernel_args()
ka["variances"] = None

ctx = W.Context(stream_ptr=torch.cuda.current_stream().cuda_stream)
b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=lengths)
fan = [args.inputs] + [args.units] * args.layers + [args.outputs]
flop = 2.0 * tf * sum(fan[i] * fan[i + 1] for i in range(len(fan) - 1))
bufs = [torch.empty(CHUNK, args.units, dtype=torch.float32, device="cuda") for _ in range(2)]
t_out = torch.empty(tf, args.outputs, dtype=torch.float32, device="cuda")


def kernel_call():
    out, _, status = b.acoustic_model_forward(ka, x)
    torch.cuda.synchronize()
    return out, status


def torch_call():
    with torch.no_grad():
        for r0 in range(0, tf, CHUNK):
            h = x[r0:r0 + CHUNK]
            for i in range(args.layers):
                dst = bufs[i & 1][:h.shape[0]]
                torch.addmm(ka["biases"][i], h, ka["weights"][i], out=dst)
                h = torch.sigmoid_(dst)
            torch.addmm(ka["biases"][-1], h, ka["weights"][-1], out=t_out[r0:r0 + CHUNK])
    torch.cuda.synchronize()
    return t_out


for _ in range(args.warmup):
    out, status = kernel_call()
    ref = torch_call()
assert int(status.abs().sum()) == 0
diff = float((out - ref).abs().max()) / float(ref.abs().max())
ctx.timing_enable(True)
wall_k = wall_t = 0.0
for _ in range(args.calls):                      # alternating: both see the same clocks and the same cache state
    t0 = time.perf_counter()
    kernel_call()
    t1 = time.perf_counter()
    torch_call()
    wall_k += t1 - t0
    wall_t += time.perf_counter() - t1
ms, launches = ctx.timing_query("dnn_layer_kernel")
ctx.timing_enable(False)
kern, wall_k, wall_t = ms / launches * 1e-3, wall_k / args.calls, wall_t / args.calls
# hidden activations: each written once and read at least once by the next layer; a layer of N columns reads its input
# once per 128-column tile (ceil(N / 128) times, mostly from L2)
hidden_w = 4 * args.units * args.layers
hidden_r = 4 * sum(fan[i] * ((fan[i + 1] + 127) // 128) for i in range(1, len(fan) - 1))
print("shape: %d utterances, %d frames, %s (n_inputs %d is a stand-in), chunks of %d frames"
      % (args.utts, tf, " -> ".join(str(n) for n in fan), args.inputs, CHUNK))
print("dnn_layer_kernel (TimingQuery, mean of %d calls): %.2f ms, %.3e frames/s, %.1f TFLOP/s = %.1f %% of the %.1f "
      "TFLOP/s FP32 matrix peak" % (launches, kern * 1e3, tf / kern, flop / kern / 1e12, 100.0 * flop / kern / PEAK, PEAK / 1e12))
print("call (binding + launches + synchronise): %.2f ms" % (wall_k * 1e3))
print("workspace bytes per frame: %d written, %d read at least (once per layer), %d read by the tiles (once per "
      "128-column tile of the next layer)" % (hidden_w, hidden_w, hidden_r))
print("torch float32 addmm + sigmoid chain, same tensors and chunks, alternating: %.2f ms, %.1f TFLOP/s; the kernel "
      "takes %.2f x its time" % (wall_t * 1e3, flop / wall_t / 1e12, wall_k / wall_t))
print("largest |kernel - torch chain| / max|out|: %.2e" % diff)

# ---- the numpy float64 reference on one host core ------------------------------------------------------------------
try:
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
except (AttributeError, OSError):
    pass
import dnn_reference as R

n = min(args.host_frames, tf)
params = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
hx = x[:n].cpu().numpy()
t0 = time.perf_counter()
want, e = R.forward(params, hx, np.zeros(n, dtype=np.int64), "sigmoid", "linear")
t_host = time.perf_counter() - t0
ratio = float((np.abs(out[:n].cpu().numpy().astype(np.float64) - want) / e).max())
print("numpy float64 reference with its bound, one host core: %.3f s for %d frames = %.3e frames/s; the whole shape at "
      "that rate %.0f s, %.0f x the kernel's time" % (t_host, n, n / t_host, tf / (n / t_host), tf / (n / t_host) / kern))
print("kernel against it on those frames: worst error / bound %.2e" % ratio)
b.close()
ctx.close()

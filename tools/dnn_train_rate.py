"""Rate of the acoustic model's training pass (WorldMi355AcousticModelTrainForward and WorldMi355AcousticModelBackward,
csrc/dnn_train.hip) at the recipe's configured size; never bench.py's `value`.

  --shape a: the recipe's minibatch, 256 rows (one utterance) through 1024 -> 3 x 2048 sigmoid -> 229, keep_prob 0.5
  --shape b: the batch of tools/dnn_rate.py (1024 utterances of 400 - 1600 frames), the same net
n_inputs = 1024 is the same STAND-IN as in tools/dnn_rate.py.

Prints, from one process after warm-up calls and with the two alternating call by call: the training forward
("dnn_layer_kernel" of WorldMi355TimingQuery), the backward pass ("dnn_backward_kernel") and their sum, the achieved
TFLOP/s of each against the 157.3 TFLOP/s FP32 matrix peak (forward 2 T sum fan_in fan_out; backward that again for the
weight gradients plus the data gradients of all layers but the first), the workspace bytes per frame; beside it the same
step as torch autograd over training.AcousticModel's layers with torch.nn.functional.dropout on the same tensors in the
same 65 536-frame chunks (the vendor GEMM; its masks are torch's own).

Run on the GPU box: python tools/dnn_train_rate.py --shape a|b [--calls 10] [--time-limit 500]"""
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
ap_.add_argument("--shape", choices=("a", "b"), default="a")
ap_.add_argument("--utts", type=int, default=1024)
ap_.add_argument("--calls", type=int, default=10)
ap_.add_argument("--warmup", type=int, default=2)
ap_.add_argument("--inputs", type=int, default=1024)
ap_.add_argument("--units", type=int, default=2048)
ap_.add_argument("--layers", type=int, default=3)
ap_.add_argument("--outputs", type=int, default=229)
ap_.add_argument("--keep-prob", type=float, default=0.5)
ap_.add_argument("--time-limit", type=int, default=500, help="seconds after which the run ends itself")
args = ap_.parse_args()
signal.alarm(args.time_limit)
assert torch.cuda.is_available(), "this measurement needs the GPU"
pkg = importlib.import_module("hts-train-world_amd")
W, training = pkg.world, pkg.training

PEAK = 157.3e12
CHUNK = 65536
lengths = [256] if args.shape == "a" else np.random.default_rng(0).integers(400, 1601, args.utts).tolist()
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
G = torch.randn(tf, args.outputs, dtype=torch.float32, device="cuda", generator=gen) / (tf * args.outputs)
ka = model.kernel_args()
ka["variances"] = None
ctx = W.Context(stream_ptr=torch.cuda.current_stream().cuda_stream)
b = W.WorldBatch(ctx, W.default_params(48000, 5.0), f0_lengths=lengths)
fan = [args.inputs] + [args.units] * args.layers + [args.outputs]
prod = [fan[i] * fan[i + 1] for i in range(len(fan) - 1)]
flop_f = 2.0 * tf * sum(prod)
flop_b = 2.0 * tf * (sum(prod) + sum(prod[1:]))
p = args.keep_prob


def kernel_call(step):
    out, _, status = b.acoustic_model_train_forward(ka, x, None, None, p, 1, step)
    grads = b.acoustic_model_backward(ka, x, None, G, p, 1, step)
    torch.cuda.synchronize()
    return out, status, grads


def torch_call():
    for q in model.parameters():
        q.grad = None
    for r0 in range(0, tf, CHUNK):
        h = x[r0:r0 + CHUNK]
        for i in range(args.layers):
            L = model.hidden(i)
            h = torch.nn.functional.dropout(torch.sigmoid(torch.addmm(L.si_biases, h, L.si_weights)), 1.0 - p, True)
        out = torch.addmm(model.output.si_biases, h, model.output.si_weights)
        out.backward(G[r0:r0 + CHUNK])
    torch.cuda.synchronize()


for k in range(args.warmup):
    out, status, grads = kernel_call(k)
    torch_call()
assert int(status.abs().sum()) == 0 and int(grads["status"].abs().sum()) == 0
ctx.timing_enable(True)
wall_k = wall_t = 0.0
for k in range(args.calls):                      # alternating: both see the same clocks and the same cache state
    t0 = time.perf_counter()
    kernel_call(k)
    t1 = time.perf_counter()
    torch_call()
    wall_k += t1 - t0
    wall_t += time.perf_counter() - t1
ms_f, n_f = ctx.timing_query("dnn_layer_kernel")
ms_b, n_b = ctx.timing_query("dnn_backward_kernel")
ctx.timing_enable(False)
t_f, t_b = ms_f / n_f * 1e-3, ms_b / n_b * 1e-3
wall_k, wall_t = wall_k / args.calls, wall_t / args.calls
width = max(args.units, args.outputs)
ws = 4 * width * (2 + args.layers * (2 if p < 1.0 else 1))
print("shape %s: %d utterances, %d frames, %s (n_inputs %d is a stand-in), keep_prob %g, chunks of %d frames"
      % (args.shape, len(lengths), tf, " -> ".join(str(n) for n in fan), args.inputs, p, CHUNK))
print("training forward (dnn_layer_kernel, mean of %d calls): %.3f ms, %.1f TFLOP/s = %.1f %% of the %.1f TFLOP/s FP32 "
      "matrix peak" % (n_f, t_f * 1e3, flop_f / t_f / 1e12, 100.0 * flop_f / t_f / PEAK, PEAK / 1e12))
print("backward (dnn_backward_kernel, mean of %d calls, its own forward pass included in the time, not in the FLOP): "
      "%.3f ms, %.1f TFLOP/s = %.1f %%; per FLOP %.2f x the forward" % (n_b, t_b * 1e3, flop_b / t_b / 1e12,
                                                                      100.0 * flop_b / t_b / PEAK, (t_b / flop_b) / (t_f / flop_f)))
print("sum: %.3f ms, %.1f TFLOP/s; both calls with binding and synchronise: %.3f ms" % ((t_f + t_b) * 1e3,
                                                                                     (flop_f + flop_b) / (t_f + t_b) / 1e12, wall_k * 1e3))
print("workspace bytes per chunk frame: %d (two dz buffers and %d activation buffers of %d floats)"
      % (ws, args.layers * (2 if p < 1.0 else 1), width))
print("torch autograd step (addmm, sigmoid, dropout; vendor GEMM), same tensors and chunks, alternating: %.3f ms; the "
      "library's two calls take %.2f x its time" % (wall_t * 1e3, wall_k / wall_t))
b.close()
ctx.close()

"""Rate of the optimiser step (WorldMi355OptimizerStep, csrc/optim.hip) on the rate table's net in SAT form
(1024 -> 3 x 2048 sigmoid -> 229, two speakers: 12 tensors, 11.0 M parameters); never bench.py's `value`.

Per rule, from one process after warm-up calls and with the two sides alternating call by call: the fused step (one
launch; "optimizer_step_kernel" of WorldMi355TimingQuery, and the call with its binding and a synchronise) beside
torch.optim's step of the same name (make_optimizer: what recipe.train_files runs with updates="torch") on tensors of the
same sizes with the same gradients, between two events on the stream and with a synchronise.  Then the bytes the rule
moves per parameter (p, g and each slot read, p and each slot written), the fraction of 6.3 TB/s that the kernel's time
amounts to, and the step's share of the 2.47 ms forward + backward of the recipe's minibatch.

Run on the GPU box: python tools/optimizer_rate.py [--calls 10] [--time-limit 500]"""
import argparse
import copy
import importlib
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

ap_ = argparse.ArgumentParser()
ap_.add_argument("--calls", type=int, default=10)
ap_.add_argument("--warmup", type=int, default=2)
ap_.add_argument("--inputs", type=int, default=1024)
ap_.add_argument("--units", type=int, default=2048)
ap_.add_argument("--layers", type=int, default=3)
ap_.add_argument("--outputs", type=int, default=229)
ap_.add_argument("--spkrs", type=int, default=2)
ap_.add_argument("--learning-rate", type=float, default=0.001)
ap_.add_argument("--time-limit", type=int, default=500, help="seconds after which the run ends itself")
args = ap_.parse_args()
signal.alarm(args.time_limit)
assert torch.cuda.is_available(), "this measurement needs the GPU"
pkg = importlib.import_module("hts-train-world_amd")
W, training, recipe = pkg.world, pkg.training, pkg.recipe

HBM, STEP_MS = 6.3e12, 2.47
BYTES = {"sgd": 12, "momentum": 20, "adagrad": 20, "adadelta": 28, "adam": 28, "rmsprop": 20}
torch.manual_seed(0)
base = training.AcousticModel(args.inputs, [args.units] * args.layers, args.outputs, args.spkrs, "sigmoid", "linear").cuda()
n_par = sum(p.numel() for p in base.parameters())
gen = torch.Generator(device="cuda").manual_seed(0)
grads = {k: torch.randn(p.shape, dtype=torch.float32, device="cuda", generator=gen) * 1e-3 for k, p in base.named_parameters()}
ctx = W.Context(stream_ptr=torch.cuda.current_stream().cuda_stream)
print("%d tensors, %d parameters (%s, %d speakers); mean of %d calls after %d, the two sides alternating"
      % (len(grads), n_par, " -> ".join(str(n) for n in [args.inputs] + [args.units] * args.layers + [args.outputs]), args.spkrs,
         args.calls, args.warmup))
print("rule      fused kernel  fused call  torch.optim events  torch.optim call  B/param  of 6.3 TB/s  of the 2.47 ms step")
for rule in recipe.OPTIMIZERS:
    ours, theirs = copy.deepcopy(base), copy.deepcopy(base)
    for m in (ours, theirs):
        for k, p in m.named_parameters():
            p.grad = grads[k]
    fused = recipe.Tf1Optimizer(ours, rule, args.learning_rate, ctx)
    eager = recipe.make_optimizer(theirs, rule, args.learning_rate)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    wall_f = wall_t = ms_t = 0.0
    for k in range(args.warmup + args.calls):
        if k == args.warmup:
            ctx.timing_enable(True)
        t0 = time.perf_counter()
        fused.step()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ev[0].record()
        eager.step()
        ev[1].record()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if k >= args.warmup:
            wall_f += t1 - t0
            wall_t += t2 - t1
            ms_t += ev[0].elapsed_time(ev[1])
    ms_f, n_f = ctx.timing_query("optimizer_step_kernel")
    ctx.timing_enable(False)
    assert n_f == args.calls, "one launch per step"
    t_f = ms_f / n_f * 1e-3
    print("%-9s %9.1f us %8.1f us %16.1f us %14.1f us %8d %11.1f %% %18.2f %%"
          % (rule, t_f * 1e6, wall_f / args.calls * 1e6, ms_t / args.calls * 1e3, wall_t / args.calls * 1e6, BYTES[rule],
             100.0 * BYTES[rule] * n_par / t_f / HBM, 100.0 * t_f * 1e3 / STEP_MS))
ctx.close()

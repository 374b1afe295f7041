"""Rate of waveforms from mel-cepstra (WorldMi355MlsaSynthesis, mlsa_filter_kernel): `excite | dfs | mglsadf` of `recipe.py
mlsa-synth`; never bench.py's `value`.

  16 kHz: frame shift 80, order 24, alpha 0.42;  48 kHz: frame shift 240, order 49, alpha 0.55
  Pade orders 5 and 7; batches of 64, 256 and 1024 utterances of 2 - 8 s; makefilter.pl's 31 taps; float32 pipes.

The filter is sequential in time within an utterance and runs one wavefront per utterance, so a batch takes as long as its
longest utterance while the wavefronts fit the device at once.  Printed per shape, from one process after a warm-up call:
the median over --calls calls (host clock around a call that ends in a device synchronise) in ms, samples/s, the filter
kernel's own time (WorldMi355TimingQuery, one call) and what that is per sample of the LONGEST utterance in ns -- the
sequential cost of one sample in one wavefront; times the shader clock it is cycles per sample and wave.

The only CPU statement of this path is tests/mlsa_reference.py, a Python loop: no speed-up is quoted against it.

Run on the GPU box: python tools/mlsa_rate.py [--calls 3] [--utts 64 256 1024]"""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

ap_ = argparse.ArgumentParser()
ap_.add_argument("--utts", type=int, nargs="+", default=[64, 256, 1024])
ap_.add_argument("--pade", type=int, nargs="+", default=[5, 7])
ap_.add_argument("--calls", type=int, default=3)
ap_.add_argument("--clock-ghz", type=float, default=2.4, help="shader clock for the cycles column")
args = ap_.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
W = importlib.import_module("hts-train-world_amd").world
taps = np.load(os.path.join(ROOT, "tests", "golden", "makefilter.npz"))

SHAPES = ((16000, 80, 24, 0.42), (48000, 240, 49, 0.55))
ctx = W.Context(stream_ptr=torch.cuda.current_stream().cuda_stream)
print("%6s %5s %4s %5s | %9s %12s | %10s %12s %8s" % ("fs", "order", "pd", "utts", "ms/batch", "samples/s", "kernel ms",
                                                      "ns/sample", "cycles"))
for fs, P, order, alpha in SHAPES:
    lp, hp = taps["taps_%d_0" % fs], taps["taps_%d_1" % fs]
    for n_utt in args.utts:
        rng = np.random.default_rng(n_utt)
        frames = (rng.integers(2 * fs, 8 * fs + 1, n_utt) // P + 1).tolist()
        samples = [W.mlsa_samples(t, P) for t in frames]
        tf, ty = int(sum(frames)), int(sum(samples))
        gen = torch.Generator(device="cuda").manual_seed(n_utt)
        # voiced and unvoiced runs of about 40 frames; periods of 80 - 300 Hz; small smooth-free cepstra (timing only)
        f0 = 80.0 + 220.0 * torch.rand(tf, device="cuda", generator=gen)
        voiced = (torch.arange(tf, device="cuda") // 40) % 3 != 0
        pitch = torch.where(voiced, fs / f0, torch.zeros_like(f0)).float().contiguous()
        scale = 0.1 / (1.0 + torch.arange(order + 1, device="cuda", dtype=torch.float32))
        mc = (torch.randn(tf, order + 1, device="cuda", generator=gen) * scale).contiguous()
        b = W.WorldBatch(ctx, W.default_params(fs, 5.0), f0_lengths=frames, y_lengths=samples)
        for pd in args.pade:
            def call():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                y, st = b.mlsa_synthesis(pitch, mc, lp, hp, alpha=alpha, pade_order=pd, frame_shift=P, pipe_float32=True)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, y, st
            _, y, st = call()
            assert int(st.abs().max()) == 0 and bool(torch.isfinite(y).all())
            ts = [call()[0] for _ in range(args.calls)]
            del y
            ctx.timing_enable(True)
            call()
            ms, launches = ctx.timing_query("mlsa_kernel")
            ctx.timing_enable(False)
            assert launches == 1, launches
            med = float(np.median(ts))
            ns = 1e6 * ms / max(samples)
            print("%6d %5d %4d %5d | %9.2f %12.3e | %10.2f %12.1f %8.0f" % (fs, order, pd, n_utt, 1e3 * med, ty / med, ms, ns,
                                                                           ns * args.clock_ghz), flush=True)
        b.close()
        del pitch, mc, f0, voiced
ctx.close()

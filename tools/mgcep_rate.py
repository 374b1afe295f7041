"""Rate of mel-cepstra from waveforms (WorldMi355MelCepstrumOfWaveform, mgcep_kernel) at the defaults of `recipe.py mgcep`;
never bench.py's `value`.

  256 utterances of 2 - 8 s at 48 kHz (about 256 000 frames): frame length 1200, shift 240, fft length 2048, Hamming,
  power-normalised, float32 pipe, alpha 0.55, order 49, eps 1e-8, itr1 2, itr2 30, dd 1e-3 (data/Makefile.in:134-137).

Prints, from one process after warm-up calls, the median over --calls ALTERNATING calls (host clock around a call that ends
in a device synchronise) of
  fused    mel_cepstrum_of_waveform on the packed samples;
  staged   torch.fft.rfft of the same windowed frames (made beforehand, not timed), |X|^2, then mel_cepstrum(itype=4) on the
           periodograms with the same eps: what a caller had before the fused call;
the two kernels' own times (WorldMi355TimingQuery) of one call each, and the one-core rate of the compiled reference's
mcep (oracle/_ref/libsptk_ref.so) on --ref-frames of the frames.
Checks that fused and staged agree to 1e-9 on the frames both converge on.

Run on the GPU box: python tools/mgcep_rate.py [--utts 256] [--calls 7]"""
import argparse
import ctypes
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

ap_ = argparse.ArgumentParser()
ap_.add_argument("--utts", type=int, default=256)
ap_.add_argument("--calls", type=int, default=7)
ap_.add_argument("--warmup", type=int, default=2)
ap_.add_argument("--ref-frames", type=int, default=300)
args = ap_.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
W = importlib.import_module("hts-train-world_amd").world

FS, L, P, F, M, ALPHA, EPS = 48000, 1200, 240, 2048, 49, 0.55, 1e-8
rng = np.random.default_rng(0)
lengths = rng.integers(2 * FS, 8 * FS + 1, args.utts).tolist()
counts = [W.sptk_frames(n, L, P) for n in lengths]
tf = int(sum(counts))
gen = torch.Generator(device="cuda").manual_seed(0)
# integer-valued, coloured: white noise through a two-tap smoother, int16 range
x = torch.randn(int(sum(lengths)) + 1, dtype=torch.float64, device="cuda", generator=gen)
x = torch.round(4000.0 * (x[1:] + 0.9 * x[:-1])).clamp_(-32768, 32767).contiguous()
table = W.sptk_window(1, 1, L)

ctx = W.Context(stream_ptr=torch.cuda.current_stream().cuda_stream)
b = W.WorldBatch(ctx, W.default_params(FS, 5.0, fft_size=F), x_lengths=lengths, f0_lengths=counts)

# the staged path's input: the frames of the definition, float32-rounded, zero-padded (not timed)
wd = torch.from_numpy(table).cuda()
frames = torch.zeros(tf, F, dtype=torch.float64, device="cuda")
at_x, at_f = 0, 0
for n, j in zip(lengths, counts):
    pad = torch.zeros(L // 2 + (j - 1) * P + L + n, dtype=torch.float64, device="cuda")
    pad[L // 2:L // 2 + n] = x[at_x:at_x + n]
    frames[at_f:at_f + j, :L] = (pad.unfold(0, L, P)[:j] * wd).float().double()
    at_x, at_f = at_x + n, at_f + j
del pad


def fused():
    return b.mel_cepstrum_of_waveform(x, table, L, P, M, ALPHA, True, etype=1, e=EPS)


def staged():
    s = torch.fft.rfft(frames, dim=1)
    per = s.real * s.real + s.imag * s.imag
    return b.mel_cepstrum(per, M, ALPHA, itype=4, etype=1, e=EPS)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


for _ in range(args.warmup):
    _, (mc_f, st_f) = timed(fused)
    _, (mc_s, st_s) = timed(staged)
both = (st_f == 0) & (st_s == 0)
worst = float((mc_f - mc_s)[both].abs().max())
print("shape: %d utterances, %d samples, %d frames; status fused %s staged %s; max |fused - staged| on %d frames both "
      "converge on: %.2e" % (args.utts, x.numel(), tf, torch.unique(st_f).tolist(), torch.unique(st_s).tolist(),
                             int(both.sum()), worst))
assert worst < 1e-9 and float(both.double().mean()) > 0.9
tfu, tst = [], []
for _ in range(args.calls):
    tfu.append(timed(fused)[0])
    tst.append(timed(staged)[0])
for name, ts in (("fused  mel_cepstrum_of_waveform", tfu), ("staged rfft + mel_cepstrum(itype=4)", tst)):
    med = float(np.median(ts))
    print("%-36s median of %d alternating calls: %.2f ms (%s), %.3e frames/s" % (
        name, args.calls, 1e3 * med, " ".join("%.2f" % (1e3 * t) for t in ts), tf / med))
print("fused / staged time: %.3f" % (np.median(tfu) / np.median(tst)))
for name, fn in (("mgcep_kernel", fused), ("mcep_kernel", staged)):      # the kernels alone, one call each
    ctx.timing_enable(True)
    fn()
    torch.cuda.synchronize()
    ms, launches = ctx.timing_query(name)
    ctx.timing_enable(False)
    assert launches == 1, (name, launches)
    print("%s alone (TimingQuery, one call): %.2f ms" % (name, ms))

# ---- the compiled reference on one core ------------------------------------------------------------------------------
import gen_golden_mcep as base  # noqa: E402
if os.path.exists(base.LIB):
    rows = frames[:args.ref_frames].cpu().numpy()
    lib = ctypes.CDLL(base.LIB)
    fn = getattr(lib, base.mcep_symbol())
    dp = ctypes.POINTER(ctypes.c_double)
    fn.restype = ctypes.c_int
    fn.argtypes = [dp, ctypes.c_int, dp, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                   ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int]
    buf, o = np.zeros(F), np.zeros(M + 1)
    t0 = time.perf_counter()
    for row in rows:
        buf[:] = row
        fn(buf.ctypes.data_as(dp), F, o.ctypes.data_as(dp), M, ALPHA, 2, 30, 1e-3, 1, EPS, 1e-6, 0)
    dt = time.perf_counter() - t0
    print("compiled reference mcep (itype 0), one core, %d frames: %.1f frames/s" % (len(rows), len(rows) / dt))
else:
    print("compiled reference: oracle/_ref/libsptk_ref.so is not built, not measured")
b.close()
ctx.close()

"""Hand-made feature sets for Synthesis: what a caller that did NOT run this library's analysis may hand over.

The recipe calls Synthesis on model-generated lf0 / mgc / bap: arbitrary contours, voicing that flips from frame to
frame, any f0, rough envelopes.  Analysis outputs never look like that (f0 is a smooth contour of 65-330 Hz, voiced
stretches last 0.3 s or more, envelopes are smooth), so the sets here are built by hand, named, and deterministic:
every random number comes from synth_data.uniform, the project's counter-based generator, seeded by the case itself.

    case(name, fs, fft_size, frame_period) -> (f0, sp, ap, y_length)

`name` is "contour[:envelope[:aperiodicity[:length]]]" (defaults smooth, mid, recipe):

contour      alternating  voicing flips on every frame
             singles      single voiced frames between unvoiced ones, the first and the last frame among them
             const41 / const1000 / const03fs   constant 41 Hz, 1000 Hz, 0.3 fs (the sparsest and the densest pulse lists)
             jumps        80 <-> 640 Hz every three frames; ends on a fall, so that the extrapolated knot
                          2 f0[nf-1] - f0[nf-2] of the time base is -480 Hz
             random       log-uniform 45-900 Hz, 30 % of the frames unvoiced
             gate         10 Hz, exactly the gate fs / fft_size + 1 (integer division), the double just below it, 200 Hz
             negative     negative values between voiced frames
             fs16 / fs32 / fs64 / fs128        constant fs / 16 ... fs / 128: the period is a whole number of samples, so
                          every pulse sits on a phase-wrap tie, on or next to every multiple of 128 and 2048 samples
envelope     smooth       decaying over the bins, +-50 % jitter per bin
             rough        every bin log-uniform in 1e-18 ... 1e3
aperiodicity mid          0.05 ... 0.95, rising with the bin
             ap0 / ap1 / apneg   all 0, all 1, all -0.5 (GetSafeAperiodicity clamps to [0.001, 0.999999999999])
             ap0bin       0.9995 in bin 0 only: its square passes the 0.999 above which a voiced pulse has no periodic part
length       recipe       int((nf - 1) frame_period fs / 1000) + 1, what the synth CLI asks for
             len=N        N samples (shorter or longer than the frames cover)
             lenlong      6 frames beyond the last one: the time base extrapolates (f0 < 0 there after a fall)
             lenfar       16 frames beyond: after a fall the accumulated phase itself turns negative
"""
import importlib
import zlib

import numpy as np

sd = importlib.import_module("hts-train-world_amd.synth_data")

CONTOURS = ("alternating", "singles", "const41", "const1000", "const03fs", "jumps", "random", "gate", "negative",
            "fs16", "fs32", "fs64", "fs128")
FRAMES = dict(alternating=61, singles=75, const41=61, const1000=61, const03fs=61, jumps=91, random=121, gate=66,
              negative=64, fs16=61, fs32=61, fs64=61, fs128=61)
# the six instantiations of the pulse kernel: (fs, fft_size, frame_period)
INSTANTIATIONS = ((8000, 512, 5.0), (16000, 1024, 5.0), (16000, 2048, 5.0), (48000, 2048, 5.0), (96000, 4096, 5.0),
                  (22050, 1024, 2.5))
TILE_LENGTHS = (2047, 2048, 2049, 4097, 2 * 2048 * 2 + 1, 2 * 2048 * 3 + 1)


def lowest_f0(fs, fft_size):
    """The gate of synthesis.cpp:359: fs / fft_size + 1.0 with the division done in integers."""
    return fs // fft_size + 1.0


def recipe_length(nf, fs, frame_period):
    return int((nf - 1) * frame_period / 1000.0 * fs) + 1          # synth.cpp:259


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def contour(name, fs, fft_size, seed):
    nf = FRAMES[name]
    i = np.arange(nf)
    if name == "alternating":
        return np.where(i % 2 == 0, 150.0 + i, 0.0)
    if name == "singles":
        f0 = np.zeros(nf)
        f0[[0, 1 + nf // 5, nf // 2, nf // 2 + 2, nf - 1]] = (120.0, 310.0, 95.0, 520.0, 180.0)
        return f0
    if name.startswith("const"):
        return np.full(nf, {"const41": 41.0, "const1000": 1000.0, "const03fs": 0.3 * fs}[name])
    if name == "jumps":
        f0 = np.where((i // 3) % 2 == 0, 80.0, 640.0)
        assert f0[-1] == 80.0 and f0[-2] == 640.0
        return f0
    if name == "random":
        u, v = sd.uniform(seed, 0, nf), sd.uniform(seed, 1, nf)
        return np.where(v < 0.3, 0.0, 45.0 * np.exp(u * np.log(900.0 / 45.0)))
    if name == "gate":
        g = lowest_f0(fs, fft_size)
        return np.array([10.0, g, np.nextafter(g, 0.0), 200.0, g, g, np.nextafter(g, 0.0), 10.0, 200.0, 200.0, g])[i % 11]
    if name == "negative":
        return np.array([120.0, -120.0, -1.0, 240.0, 240.0, -1e9, 0.0, 90.0])[i % 8]
    if name.startswith("fs"):
        return np.full(nf, fs / float(name[2:]))
    raise KeyError(name)


def envelope(name, nf, bins, seed):
    u = sd.uniform(seed, 2, nf * bins).reshape(nf, bins)
    if name == "smooth":
        k = np.arange(bins)
        level = 0.5 + sd.uniform(seed, 3, nf)                           # the frames differ in level too
        return 1e-3 * np.exp(-k / (bins / 5.0))[None, :] * (0.5 + u) * level[:, None]
    if name == "rough":
        return 10.0 ** (-18.0 + 21.0 * u)
    raise KeyError(name)


def aperiodicity(name, nf, bins, seed):
    if name == "mid":
        u = sd.uniform(seed, 4, nf * bins).reshape(nf, bins)
        return 0.05 + 0.9 * u * (np.arange(bins) / (bins - 1.0))[None, :]
    if name == "ap0bin":
        ap = aperiodicity("mid", nf, bins, seed)
        ap[:, 0] = 0.9995
        return ap
    return np.full((nf, bins), {"ap0": 0.0, "ap1": 1.0, "apneg": -0.5}[name])


def case(name, fs, fft_size, frame_period):
    """(f0 [nf], sp [nf][fft_size / 2 + 1], ap [same], y_length) of the named case; see the module's docstring."""
    parts = name.split(":")
    c, e, a, ln = parts + ["smooth", "mid", "recipe"][len(parts) - 1:]
    seed = _seed(c, fs, fft_size, frame_period)
    f0 = contour(c, fs, fft_size, seed)
    nf, bins = len(f0), fft_size // 2 + 1
    sp = envelope(e, nf, bins, seed)
    ap = aperiodicity(a, nf, bins, seed)
    frame = frame_period / 1000.0 * fs
    y_length = {"recipe": recipe_length(nf, fs, frame_period), "lenlong": int((nf + 5) * frame) + 1,
                "lenfar": int((nf + 15) * frame) + 1}.get(ln) or int(ln[len("len="):])
    return (np.ascontiguousarray(f0, dtype=np.float64), np.ascontiguousarray(sp), np.ascontiguousarray(ap), y_length)


def time_base(f0, fs, fft_size, frame_period, y_length):
    """GetTimeBase (synthesis.cpp:223-320) restated in numpy, for the assertions that a case is what its name says:
    returns (pulse sample indices, voicing of each pulse, accumulated phase per sample)."""
    nf, fp = len(f0), frame_period / 1000.0
    cf0 = np.where(f0 < lowest_f0(fs, fft_size), 0.0, f0)
    cf0 = np.append(cf0, cf0[-1] * 2 - cf0[-2])
    cv = (cf0[:nf] != 0.0).astype(np.float64)
    cv = np.append(cv, cv[-1] * 2 - cv[-2])
    ct = np.arange(nf + 1) * fp
    t = np.arange(y_length) / float(fs)
    k = np.clip(np.searchsorted(ct, t, side="right"), 1, nf)            # histc + interp1: the last segment extrapolates
    s = (t - ct[k - 1]) / (ct[k] - ct[k - 1])
    vuv = (cv[k - 1] + s * (cv[k] - cv[k - 1])) > 0.5
    if0 = np.where(vuv, cf0[k - 1] + s * (cf0[k] - cf0[k - 1]), 500.0)
    total = np.cumsum(2.0 * np.pi * if0 / fs)
    wrap = np.fmod(total, 2.0 * np.pi)
    idx = np.nonzero(np.abs(np.diff(wrap)) > np.pi)[0]
    return idx, vuv[idx], total


def checks(a):
    return np.array([a.sum(), (a * a).sum(), np.abs(a).max()])


def input_check(f0, sp, ap, y_length):
    """Ten numbers that pin a case's inputs (a drift of the generator shows here, not as a wrong y)."""
    return np.concatenate([checks(f0), checks(sp), checks(ap), [float(y_length)]])


def grid():
    """Every (name, fs, fft_size, frame_period) that the suite runs: oracle against the compiled reference on the CPU,
    the kernels against the oracle on the GPU, and the golden fixture."""
    g = []
    for inst in INSTANTIATIONS:                                         # every contour at every kernel instantiation
        g += [(c,) + inst for c in CONTOURS]
    for inst in ((16000, 1024, 5.0), (48000, 2048, 5.0)):               # rough envelopes, aperiodicity extremes
        g += [(c + ":rough",) + inst for c in ("random", "jumps", "const1000")]
        g += [(c + ":smooth:" + a,) + inst for c in ("random", "alternating") for a in ("ap0", "ap1", "apneg", "ap0bin")]
        g += [("random:rough:ap0",) + inst, ("random:rough:ap1",) + inst]
    for fp in (1.0, 10.0):                                              # other hops at 16 kHz
        g += [(c, 16000, 1024, fp) for c in ("random", "alternating", "jumps", "gate", "fs32")]
    g += [("singles", 16000, 1024, 10.0)]                               # (at 1 ms a single voiced frame holds no pulse)
    for c in ("random", "jumps"):                                       # output lengths
        g += [("%s:smooth:mid:%s" % (c, ln), 16000, 1024, 5.0)
              for ln in ("len=1", "len=2", "len=100", "len=4097", "lenlong", "lenfar")]
    g += [("jumps:smooth:mid:lenfar", 48000, 2048, 5.0), ("jumps:rough:mid:lenlong", 48000, 2048, 5.0)]
    for c in ("fs16", "fs32", "fs64", "fs128"):                         # ties on the tile edges of the pulse search
        g += [("%s:smooth:mid:len=%d" % (c, n), 16000, 1024, 5.0) for n in TILE_LENGTHS]
    g += [("fs32:smooth:mid:len=%d" % n, 48000, 2048, 5.0) for n in TILE_LENGTHS]
    for fs, F, fp in ((48000, 2048, 1.0), (48000, 2048, 2.5), (48000, 2048, 10.0), (22050, 1024, 1.0),
                      (22050, 1024, 5.0), (22050, 1024, 10.0), (8000, 512, 1.0), (8000, 512, 2.5), (8000, 512, 10.0)):
        g += [("random", fs, F, fp), ("alternating:rough", fs, F, fp)]  # the remaining rates and hops
    assert len(set(g)) == len(g)
    return g


def case_id(c):
    return "%s-%d-%d-%g" % c

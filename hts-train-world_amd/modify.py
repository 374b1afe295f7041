"""Voice modification between analysis and synthesis: F0 scaling and formant shift on the device.

WorldMi355ModifyFeatures (csrc/modify.hip) restates ParameterModification of the reference's own example
(externs/WORLD_v2/test/test.cpp:201-238): f0 times a factor, and the spectral envelope stretched along the frequency
axis by interp1 on its logarithm.  Here are its two callers' forms:

    modify_features(batch, f0, sp, f0_scale, formant_ratio)    the features of a WorldBatch, one factor pair per utterance
    convert(batch, x, f0_scale, formant_ratio)                 analyze -> modify -> synthesize, waveforms to waveforms

A factor of None means "not done": that part's tensor is not read and comes back as it was given.  A ratio of exactly
1.0 is done (exp(log(sp)), as test.cpp does whenever it is given a fourth argument).  The aperiodicity is never touched.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import world as W


def factor_array(where, name, value, n_utt, fft_size=None):
    """`value` -- None, a number, or one number per utterance -- as a float64 array [n_utt] (None stays None), checked as
    the library checks it: finite and > 0, and for the formant ratio (fft_size given) inside [2 / fft_size, fft_size]:
    below it the reference's fill reads the bin before the first, above it nothing is left to stretch.  ValueError."""
    if value is None:
        return None
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(n_utt, float(a))
    if a.shape != (n_utt,):
        raise ValueError(f"{where}: {name} must be a number or one per utterance ({n_utt}), got shape {list(a.shape)}")
    a = np.ascontiguousarray(a)
    for u, v in enumerate(a):
        if not (math.isfinite(v) and v > 0.0):
            raise ValueError(f"{where}: {name}[{u}] = {v!r} must be finite and > 0")
        if fft_size is not None and not 2.0 / fft_size <= v <= fft_size:
            raise ValueError(f"{where}: {name}[{u}] = {v!r} is outside [2 / fft_size, fft_size] = "
                             f"[{2.0 / fft_size!r}, {fft_size}]")
    return a


def modify_features(batch, f0=None, sp=None, f0_scale=None, formant_ratio=None, out=None):
    """f0 [total_frames] times f0_scale and sp [total_frames][bins] stretched by formant_ratio, per utterance of `batch`.

    f0_scale, formant_ratio: None, a number for every utterance, or one number per utterance.  At least one is given; the
    tensor of a part that is given must be given too.  out: None for fresh tensors, or (f0_out, sp_out) with None for a
    part that is to be fresh; an output may be its own input (in place), not a shifted view of it.
    Returns (f0_out, sp_out); a part that is not done is the argument as it came (None included).  Bad factors and bad
    tensors raise ValueError before the library is called.  Asynchronous on the context's stream."""
    where = "modify_features"
    if f0_scale is None and formant_ratio is None:
        raise ValueError(f"{where}: give f0_scale, formant_ratio or both")
    shift = factor_array(where, "f0_scale", f0_scale, batch.n_utt)
    ratio = factor_array(where, "formant_ratio", formant_ratio, batch.n_utt, batch.fft_size)
    if out is None:
        out = (None, None)
    if not isinstance(out, (tuple, list)) or len(out) != 2:
        raise ValueError(f"{where}: out must be (f0_out, sp_out), either of them None")
    f0_out, sp_out = f0, sp
    f0p = spp = f0op = spop = None
    if shift is not None:
        f0p = batch._f64(where, "f0", f0, batch.total_frames)
        f0_out, f0op = batch._out(where, out[0], batch.total_frames, name="out[0]")
    if ratio is not None:
        spp = batch._f64(where, "sp", sp, batch.total_frames, batch.bins)
        sp_out, spop = batch._out(where, out[1], batch.total_frames, batch.bins, name="out[1]")
    dp = C.POINTER(C.c_double)
    W._check(W.load_library().WorldMi355ModifyFeatures(
        batch.handle, None if shift is None else shift.ctypes.data_as(dp),
        None if ratio is None else ratio.ctypes.data_as(dp), f0p, spp, f0op, spop), "ModifyFeatures")
    return f0_out, sp_out


def convert(batch, x, f0_scale=None, formant_ratio=None):
    """analyze -> modify_features (in place) -> synthesize on the device: x [total_samples] to y [total_out], the three
    calls made one after another, bit for bit.  With both factors None the features are synthesized as analysed."""
    _, f0, sp, ap = batch.analyze(x)
    if f0_scale is not None or formant_ratio is not None:
        f0, sp = modify_features(batch, f0, sp, f0_scale, formant_ratio, out=(f0, sp))
    return batch.synthesize(f0, sp, ap)

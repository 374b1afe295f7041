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

from .world import factor_array            # noqa: F401 -- re-exported: generate.py and the recipe take it from here


def modify_features(batch, f0=None, sp=None, f0_scale=None, formant_ratio=None, out=None):
    """WorldBatch.modify_features of `batch`."""
    return batch.modify_features(f0, sp, f0_scale, formant_ratio, out)


def convert(batch, x, f0_scale=None, formant_ratio=None):
    """analyze -> modify_features (in place) -> synthesize on the device: x [total_samples] to y [total_out], the three
    calls made one after another, bit for bit.  With both factors None the features are synthesized as analysed."""
    _, f0, sp, ap = batch.analyze(x)
    if f0_scale is not None or formant_ratio is not None:
        f0, sp = modify_features(batch, f0, sp, f0_scale, formant_ratio, out=(f0, sp))
    return batch.synthesize(f0, sp, ap)

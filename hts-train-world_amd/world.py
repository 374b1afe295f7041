"""ctypes host layer over libworld_mi355.so (the C ABI declared in include/).

Mirrors the reference's per-utterance operator interface
(externs/WORLD_v2/src/world/{dio,stonemask,cheaptrick,d4c,synthesis,harvest}.h)
for numpy callers and adds ``WorldBatch`` for device-resident batches (torch
tensors on ``cuda``).  torch is used only for device memory and streams.
The C ABI takes raw pointers, so every tensor passes ``check_tensor`` first.

The library is mandatory: nothing here computes WORLD on the CPU.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# WORLD_MI355_LIB names another build of the same library (tools/ab_lib.sh: A/B runs that leave the in-tree file alone)
LIB_PATH = os.environ.get("WORLD_MI355_LIB") or os.path.join(HERE, "libworld_mi355.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

ERRORS = {1: "HIP error", 2: "bad argument", 3: "unsupported fft_size", 4: "no HIP device",
          5: "unsupported configuration"}


def _window_tables(window_lists):
    """The windows of the stream/window bundle four calls take, from one list of coefficient lists per stream:
    (n_windows array, window pointer table, size pointer table, what to keep alive until the call returns)."""
    n = len(window_lists)
    nwin = (C.c_int * n)(*[len(wins) for wins in window_lists])
    keep, wptrs, sptrs = [], (C.POINTER(_dp) * n)(), (C.POINTER(C.c_int) * n)()
    for s, wins in enumerate(window_lists):
        arrs = [(C.c_double * len(w))(*w) for w in wins]
        pa = (_dp * len(wins))(*[C.cast(a, _dp) for a in arrs])
        sz = (C.c_int * len(wins))(*[len(w) for w in wins])
        keep += [arrs, pa, sz]
        wptrs[s] = C.cast(pa, C.POINTER(_dp))
        sptrs[s] = C.cast(sz, _ip)
    return nwin, wptrs, sptrs, keep


class _LazyTorch:
    """Stands in for torch until something here first needs it, then makes way for it: importing this module does not
    import torch."""

    def __getattr__(self, name):
        global torch
        import torch
        return getattr(torch, name)


torch = _LazyTorch()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def row_stride(t):
    """The row stride the library is given for a 2-D tensor: the tensor's own, except that a tensor of one row reports
    any stride, so its width."""
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def torch_device(device):
    """The torch device of a context made with `device`: cuda of that index, torch's current device for None; a
    torch.device or its name stays what it is."""
    if device is None:
        device = torch.cuda.current_device()
    return torch.device("cuda", device) if isinstance(device, int) else torch.device(device)


def check_tensor(where, name, t, dtype, shape, device, layout="contiguous", optional=False):
    """The one check of a tensor handed to the library, whose C ABI takes raw pointers and can check nothing itself.
    shape: a tuple with, per dimension, an int for "exactly this" or None for "free, at least 1"; an int alone: that many
    elements in any shape; None: any shape.  layout: "contiguous"; "rows" (2-D, unit column stride, rows that do not
    overlap: passed by its row stride); "any" (the caller makes the copy it needs).  optional: None passes through as
    None, a NULL pointer.
    Returns the c_void_p, then with "rows" the row stride (row_stride), then the free dimensions in order (the element
    count for shape None) -- alone when nothing follows it, else as a tuple.  Anything else -- no tensor, another dtype,
    shape, layout or device -- raises ValueError naming the method, the argument, what was wanted and what was given."""
    if t is None and optional:
        return None
    ok, free = torch.is_tensor(t) and t.dtype == dtype and t.device == device, []
    if ok and isinstance(shape, tuple):
        ok = t.dim() == len(shape) and all(g == w if w is not None else g >= 1 for w, g in zip(shape, t.shape))
        free = [int(g) for w, g in zip(shape, t.shape) if w is None]
    elif ok:
        ok, free = shape is None or t.numel() == shape, [int(t.numel())] if shape is None else []
    if ok and layout == "rows":
        ok = t.dim() == 2 and (t.stride(1) == 1 or t.shape[1] == 1) and (t.shape[0] < 2 or t.stride(0) >= t.shape[1])
        free.insert(0, row_stride(t) if ok else 0)
    elif ok and layout == "contiguous":
        ok = t.is_contiguous()
    if not ok:
        dims = ("" if shape is None else "of %d elements " % shape if isinstance(shape, int)
                else "".join("[%s]" % ("any" if w is None else w) for w in shape) + " ")
        want = {"contiguous": "contiguous ", "rows": "unit-column-stride ", "any": ""}[layout]
        given = (f"{t.dtype} {list(t.shape)} with strides {list(t.stride())} on {t.device}" if torch.is_tensor(t)
                 else type(t).__name__)
        raise ValueError(f"{where}: {name} must be a {want}{dtype} tensor {dims}on {device}, got {given}")
    return (C.c_void_p(t.data_ptr()), *free) if free else C.c_void_p(t.data_ptr())


def _option(where, Struct, default, fields, allowed=None, *args):
    """A Struct as the library's `default` call (with `args` in front of the struct) fills it, then `fields` set: a
    value of None keeps the default, a name outside `allowed` (None: every field of the Struct) raises TypeError."""
    o = Struct()
    getattr(load_library(), default)(*args, C.byref(o))
    names = [f[0] for f in Struct._fields_] if allowed is None else allowed
    for k, v in fields.items():
        if k not in names:
            raise TypeError(f"{where}: unknown option {k!r}")
        if v is not None:
            setattr(o, k, v)
    return o


def _shared_row_stride(rows, cols, total_frames):
    """One row stride for the matrices `rows` and the column vectors `cols` (None entries stay None): as given when
    all share one, else packed side by side.  Returns (row stride, rows, cols, what to keep alive)."""
    ts = list(rows) + [c for c in cols if c is not None]
    ld = {row_stride(t) for t in rows} | {int(c.stride(0)) for c in cols if c is not None}
    if total_frames > 1 and len(ld) == 1 and all(t.stride(1) == 1 for t in rows):
        return ld.pop(), rows, cols, ts
    mat = torch.cat(list(rows) + [c[:, None] for c in cols if c is not None], dim=1)
    at, r2, c2 = 0, [], []
    for t in rows:
        r2.append(mat[:, at:at + t.shape[1]])
        at += int(t.shape[1])
    for c in cols:
        c2.append(None if c is None else mat[:, at])
        at += 0 if c is None else 1
    return int(mat.shape[1]), r2, c2, [mat]


class WorldParams(C.Structure):
    """include/world_mi355.h: WorldMi355Params."""
    _fields_ = [("fs", C.c_int), ("frame_period", C.c_double), ("f0_floor", C.c_double),
                ("f0_ceil", C.c_double), ("channels_in_octave", C.c_double), ("speed", C.c_int),
                ("allowed_range", C.c_double), ("q1", C.c_double), ("fft_size", C.c_int),
                ("d4c_threshold", C.c_double)]


class McepOption(C.Structure):
    """include/world_mi355.h: WorldMi355McepOption (the arguments of SPTK's mcep)."""
    _fields_ = [("alpha", C.c_double), ("order", C.c_int), ("itr1", C.c_int), ("itr2", C.c_int), ("dd", C.c_double),
                ("etype", C.c_int), ("e", C.c_double), ("f", C.c_double), ("itype", C.c_int)]


class Mgc2spOption(C.Structure):
    """include/world_mi355.h: WorldMi355Mgc2spOption (the arguments of SPTK's mgc2sp)."""
    _fields_ = [("alpha", C.c_double), ("gamma", C.c_double), ("order", C.c_int), ("out_format", C.c_int)]


class MgcConvertOption(C.Structure):
    """include/world_mi355.h: WorldMi355MgcConvertOption (the arguments and flags of SPTK's mgc2mgc)."""
    _fields_ = [("in_order", C.c_int), ("in_alpha", C.c_double), ("in_gamma", C.c_double), ("in_normalized", C.c_int),
                ("in_multiplied", C.c_int), ("out_order", C.c_int), ("out_alpha", C.c_double), ("out_gamma", C.c_double),
                ("out_normalized", C.c_int), ("out_multiplied", C.c_int)]


class LspOption(C.Structure):
    """include/world_mi355.h: WorldMi355LspOption (lspcheck | lsp2lpc | mgc2mgc -n -u; the functions are lsp.py's)."""
    _fields_ = [("order", C.c_int), ("alpha", C.c_double), ("gamma", C.c_double), ("log_gain", C.c_int),
                ("min_distance", C.c_double), ("min_gain", C.c_double)]


class LspPostfilterOption(C.Structure):
    """include/world_mi355.h: WorldMi355LspPostfilterOption (the recipe's postfiltering_lsp)."""
    _fields_ = LspOption._fields_ + [("beta", C.c_double), ("length", C.c_int), ("compensation", C.c_int)]


class MlsaOption(C.Structure):
    """include/world_mi355.h: WorldMi355MlsaOption (SPTK's excite | dfs | mglsadf, gen_wave's first branch)."""
    _fields_ = [("alpha", C.c_double), ("order", C.c_int), ("pade_order", C.c_int), ("frame_shift", C.c_int),
                ("pipe_float32", C.c_int), ("use_pade", C.c_int), ("pade", C.c_double * 8)]


class DistortionGroup(C.Structure):
    """include/world_mi355.h: WorldMi355DistortionGroup (one scored column group of WorldMi355FeatureDistortion)."""
    _fields_ = [("a", C.c_void_p), ("ld_a", C.c_int64), ("b", C.c_void_p), ("ld_b", C.c_int64), ("first", C.c_int),
                ("count", C.c_int), ("kind", C.c_int)]


class DistortionOption(C.Structure):
    """include/world_mi355.h: WorldMi355DistortionOption."""
    _fields_ = [("voiced_above", C.c_double)]


DISTORTION_KINDS = ("cepstral", "lf0")                   # kind 0 and 1 of WorldMi355FeatureDistortion


class MlpgOption(C.Structure):
    """include/world_mi355.h: WorldMi355MlpgOption (parameter generation, SPTK's mlpg)."""
    _fields_ = [("edge", C.c_int), ("var_per_frame", C.c_int), ("input_type", C.c_int),
                ("unvoiced_value", C.c_double)]


class GvOption(C.Structure):
    """include/world_mi355.h: WorldMi355GvOption (parameter generation considering global variance)."""
    _fields_ = [("max_iter", C.c_int), ("scale", C.c_int), ("epsilon", C.c_double), ("step_init", C.c_double),
                ("step_inc", C.c_double), ("step_dec", C.c_double), ("hmm_weight", C.c_double), ("gv_weight", C.c_double)]


class TrajectoryOption(C.Structure):
    """include/world_mi355.h: WorldMi355TrajectoryOption (the trajectory training criterion, DNNDefine.trajectory_cost)."""
    _fields_ = [("edge", C.c_int), ("msd_weight", C.c_double), ("gv_weight", C.c_double)]


class AcousticModelDesc(C.Structure):
    """include/world_mi355.h: WorldMi355AcousticModel (the acoustic model's forward pass, DNNDefine.inference)."""
    _fields_ = [("n_layers", C.c_int), ("n_inputs", C.c_int), ("n_outputs", C.c_int), ("n_spkrs", C.c_int),
                ("hidden_activation", C.c_int), ("output_activation", C.c_int), ("units", C.POINTER(C.c_int)),
                ("weights", C.POINTER(C.c_void_p)), ("biases", C.POINTER(C.c_void_p)),
                ("spkr_weights", C.POINTER(C.c_void_p)), ("variances", C.c_void_p), ("max_chunk_frames", C.c_int64)]


class Dropout(C.Structure):
    """include/world_mi355.h: WorldMi355Dropout (the acoustic model's training pass)."""
    _fields_ = [("keep_prob", C.c_float), ("seed", C.c_uint64), ("offset", C.c_uint32)]


ACTIVATIONS = ("linear", "sigmoid", "tanh", "relu")      # Config.pm.in:228: the codes 0 .. 3


class OptimizerOption(C.Structure):
    """include/world_mi355.h: WorldMi355OptimizerOption (the update rules of TF 1.x's tf.train.* optimisers)."""
    _fields_ = [("rule", C.c_int), ("momentum", C.c_float), ("rho", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("epsilon", C.c_float), ("beta1_power", C.c_float), ("beta2_power", C.c_float)]


OPTIMIZER_RULES = ("sgd", "momentum", "adagrad", "adadelta", "adam", "rmsprop")      # the codes 0 .. 5
OPTIMIZER_SLOTS = (0, 1, 1, 2, 2, 1)                     # the slots a rule keeps per parameter
OPTIMIZER_SLOT_INIT = ((), (0.0,), (0.1,), (0.0, 0.0), (0.0, 0.0), (1.0,))      # TF 1.x's initial values


def default_optimizer_option(rule, **over) -> OptimizerOption:
    """TF 1.x's defaults of `rule` (a name or its code); the powers are the betas."""
    return _option("default_optimizer_option", OptimizerOption, "WorldMi355DefaultOptimizerOption", over, None,
                   OPTIMIZER_RULES.index(rule) if isinstance(rule, str) else int(rule))


class McpfOption(C.Structure):
    """include/world_mi355.h: WorldMi355McpfOption (the recipe's mel-cepstral postfilter, postfiltering_mcp)."""
    _fields_ = [("alpha", C.c_double), ("beta", C.c_double), ("order", C.c_int), ("length", C.c_int)]


class MspfOption(C.Structure):
    """include/world_mi355.h: WorldMi355MspfOption (the recipe's modulation-spectrum postfilter, postfiltering_mspf)."""
    _fields_ = [("frame_length", C.c_int), ("fft_length", C.c_int), ("emphasis", C.c_double)]


class LabelFeature(C.Structure):
    """include/world_mi355.h: WorldMi355LabelFeature (one feature of makefeature.pl's question config)."""
    _fields_ = [("kind", C.c_int), ("pattern", C.c_char_p), ("min", C.c_int), ("max", C.c_int)]


# makefeature.pl:55, in the order of the kinds 2 .. 7
RESERVED_LABEL_FEATURES = ("Pos_C-State_in_Phone(Fw)", "Pos_C-State_in_Phone(Bw)", "Pos_C-Frame_in_State(Fw)",
                           "Pos_C-Frame_in_State(Bw)", "Pos_C-Frame_in_Phone(Fw)", "Pos_C-Frame_in_Phone(Bw)")


def build_library() -> None:
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "csrc"), "-j8"])


_lib = None


def load_library():
    """Load libworld_mi355.so; raises if it is missing (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc, gfx950); "
                           "this package has no CPU path")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.WorldMi355LastError.restype = C.c_char_p
    L.WorldMi355DefaultParams.argtypes = [C.c_int, C.c_double, C.POINTER(WorldParams)]
    L.WorldMi355CreateContext.argtypes = [C.c_int, vp, C.POINTER(vp)]
    L.WorldMi355DestroyContext.argtypes = [vp]
    L.WorldMi355SetStream.argtypes = [vp, vp]
    L.WorldMi355Synchronize.argtypes = [vp]
    L.WorldMi355CreateBatch.argtypes = [vp, C.POINTER(WorldParams), C.c_int, _ip, _ip, _ip, C.POINTER(vp)]
    L.WorldMi355DestroyBatch.argtypes = [vp]
    for name in ("TotalSamples", "TotalFrames", "TotalOutputSamples"):
        f = getattr(L, "WorldMi355Batch" + name)
        f.restype = C.c_int64
        f.argtypes = [vp]
    L.WorldMi355BatchFftSize.argtypes = [vp]
    for name in ("SampleOffsets", "FrameOffsets", "OutputOffsets"):
        f = getattr(L, "WorldMi355Batch" + name)
        f.restype = C.POINTER(C.c_int64)
        f.argtypes = [vp]
    L.WorldMi355Dio.argtypes = [vp, vp, vp, vp]
    L.WorldMi355Harvest.argtypes = [vp, vp, vp, vp]
    L.WorldMi355StoneMask.argtypes = [vp, vp, vp, vp, vp]
    L.WorldMi355CheapTrick.argtypes = [vp, vp, vp, vp, vp]
    L.WorldMi355D4C.argtypes = [vp, vp, vp, vp, vp]
    L.WorldMi355Synthesis.argtypes = [vp, vp, vp, vp, vp]
    L.WorldMi355SamplesFromPcm16.argtypes = [vp, vp, vp]
    L.WorldMi355SamplesToPcm16.argtypes = [vp, vp, vp]
    L.WorldMi355Analyze.argtypes = [vp, vp, vp, vp, vp, vp]
    L.WorldMi355AnalyzeSynthesize.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.WorldMi355UtteranceStatus.argtypes = [vp, vp, vp, vp, vp, vp]
    L.WorldMi355BatchSetF0Estimator.argtypes = [vp, C.c_int, C.c_int]
    L.WorldMi355BatchGetF0Estimator.argtypes = [vp, _ip, _ip]
    L.WorldMi355HarvestWorkspaceBytes.argtypes = [C.POINTER(WorldParams), C.c_int, _ip, C.POINTER(C.c_int64)]
    L.WorldMi355Vibrato.argtypes = [vp, vp, _ip, _ip, _ip, _dp, vp, vp, _ip]
    L.WorldMi355GetNumberOfAperiodicities.argtypes = [C.c_int]
    L.WorldMi355CodeSpectralEnvelope.argtypes = [vp, vp, C.c_int, vp]
    L.WorldMi355DecodeSpectralEnvelope.argtypes = [vp, vp, C.c_int, vp]
    L.WorldMi355CodeAperiodicity.argtypes = [vp, vp, vp]
    L.WorldMi355DecodeAperiodicity.argtypes = [vp, vp, vp]
    L.WorldMi355RecipeFeatures.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.WorldMi355RecipeDecode.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.WorldMi355DefaultMcepOption.restype = None
    L.WorldMi355DefaultMcepOption.argtypes = [C.POINTER(McepOption)]
    L.WorldMi355MelCepstrum.argtypes = [vp, vp, C.POINTER(McepOption), vp, vp]
    L.WorldMi355SptkFrames.argtypes = [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    L.WorldMi355SptkWindow.argtypes = [C.c_int, C.c_int, C.c_int, _dp]
    L.WorldMi355MelCepstrumOfFrames.argtypes = [vp, vp, C.POINTER(McepOption), vp, vp]
    L.WorldMi355MelCepstrumOfWaveform.argtypes = [vp, vp, _dp, C.c_int, C.c_int, C.c_int, C.POINTER(McepOption), vp, vp]
    L.WorldMi355DefaultMlsaOption.restype = None
    L.WorldMi355DefaultMlsaOption.argtypes = [C.POINTER(MlsaOption)]
    L.WorldMi355MlsaSamples.argtypes = [C.c_int, C.c_int, _ip]
    L.WorldMi355MlsaPade.argtypes = [C.c_int, _dp]
    L.WorldMi355MlsaNoise.argtypes = [C.c_int64, _dp]
    L.WorldMi355MlsaExcitation.argtypes = [vp, vp, _dp, C.c_int, _dp, C.c_int, C.POINTER(MlsaOption), vp]
    L.WorldMi355MlsaFilter.argtypes = [vp, vp, vp, C.POINTER(MlsaOption), vp, vp]
    L.WorldMi355MlsaSynthesis.argtypes = [vp, vp, vp, _dp, C.c_int, _dp, C.c_int, C.POINTER(MlsaOption), vp, vp]
    L.WorldMi355DtwWorkspaceBytes.argtypes = [C.c_int, _ip, _ip, C.POINTER(C.c_int64)]
    L.WorldMi355DtwAlign.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.POINTER(C.c_int64), C.c_int, C.c_int, vp, vp, vp, vp]
    L.WorldMi355DefaultDistortionOption.restype = None
    L.WorldMi355DefaultDistortionOption.argtypes = [C.POINTER(DistortionOption)]
    L.WorldMi355FeatureDistortion.argtypes = [vp, vp, vp, C.POINTER(C.c_int64), vp, C.c_int, C.POINTER(DistortionGroup),
                                              C.POINTER(DistortionOption), vp]
    L.WorldMi355DefaultMgc2spOption.restype = None
    L.WorldMi355DefaultMgc2spOption.argtypes = [C.POINTER(Mgc2spOption)]
    L.WorldMi355MelCepstrumToSpectrum.argtypes = [vp, vp, C.POINTER(Mgc2spOption), vp, vp, vp]
    L.WorldMi355DefaultMgcConvertOption.restype = None
    L.WorldMi355DefaultMgcConvertOption.argtypes = [C.POINTER(MgcConvertOption)]
    L.WorldMi355MelGeneralizedCepstrumConvert.argtypes = [vp, vp, C.POINTER(MgcConvertOption), vp, vp]
    L.WorldMi355DefaultLspOption.restype = None
    L.WorldMi355DefaultLspOption.argtypes = [C.POINTER(LspOption)]
    L.WorldMi355DefaultLspPostfilterOption.restype = None
    L.WorldMi355DefaultLspPostfilterOption.argtypes = [C.POINTER(LspPostfilterOption)]
    L.WorldMi355LspToLpc.argtypes = [vp, vp, C.POINTER(LspOption), vp, vp, vp]
    L.WorldMi355LspToMelGeneralizedCepstrum.argtypes = [vp, vp, C.POINTER(LspOption), C.c_int, C.c_double, C.c_double, vp,
                                                        vp]
    L.WorldMi355LspPostfilter.argtypes = [vp, vp, C.POINTER(LspPostfilterOption), vp, vp, vp, vp]
    L.WorldMi355DefaultMcpfOption.restype = None
    L.WorldMi355DefaultMcpfOption.argtypes = [C.POINTER(McpfOption)]
    L.WorldMi355MelCepstrumPostfilter.argtypes = [vp, vp, C.POINTER(McpfOption), vp, vp, vp]
    L.WorldMi355ModifyFeatures.argtypes = [vp, _dp, _dp, vp, vp, vp, vp]
    L.WorldMi355DefaultMspfOption.restype = None
    L.WorldMi355DefaultMspfOption.argtypes = [C.POINTER(MspfOption)]
    L.WorldMi355ModulationSpectrumPostfilter.argtypes = [vp, vp, C.c_int, C.POINTER(MspfOption), vp, vp, vp, vp, vp, vp]
    L.WorldMi355ModulationSpectrumStats.argtypes = [vp, vp, C.c_int, C.POINTER(MspfOption), vp, vp, vp,
                                                    C.POINTER(C.c_int64)]
    L.WorldMi355ColumnMeans.argtypes = [vp, vp, C.c_int, vp]
    L.WorldMi355MspfSegmentFrames.argtypes = []
    L.WorldMi355ComposeCmp.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.WorldMi355InterpolateGaps.argtypes = [vp, vp, C.c_int, C.c_double, vp, vp, vp]
    L.WorldMi355ComposeFfo.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.WorldMi355ColumnMoments.argtypes = [vp, vp, C.c_int64, C.c_int, C.POINTER(C.c_double), vp, vp, vp]
    L.WorldMi355DefaultMlpgOption.restype = None
    L.WorldMi355DefaultMlpgOption.argtypes = [C.POINTER(MlpgOption)]
    L.WorldMi355ParameterGeneration.argtypes = [vp, C.c_int, vp, C.c_int64, vp, C.c_int64, vp, vp, vp, vp, vp,
                                                C.POINTER(MlpgOption), vp, vp]
    L.WorldMi355DefaultGvOption.restype = None
    L.WorldMi355DefaultGvOption.argtypes = [C.POINTER(GvOption)]
    L.WorldMi355ParameterGenerationGv.argtypes = [vp, C.c_int, vp, C.c_int64, vp, C.c_int64, vp, vp, vp, vp, vp,
                                                  C.POINTER(MlpgOption), vp, vp, vp, C.POINTER(GvOption), vp, vp, vp]
    L.WorldMi355DefaultTrajectoryOption.restype = None
    L.WorldMi355DefaultTrajectoryOption.argtypes = [C.POINTER(TrajectoryOption)]
    L.WorldMi355TrajectoryCost.argtypes = [vp, C.c_int, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                           C.POINTER(TrajectoryOption), vp, vp, vp, vp, C.c_int64, vp, vp]
    L.WorldMi355AcousticModelForward.argtypes = [vp, C.POINTER(AcousticModelDesc), vp, C.c_int64, vp, vp, C.c_int64, vp,
                                                 C.c_int64, vp, vp]
    L.WorldMi355AcousticModelTrainForward.argtypes = [vp, C.POINTER(AcousticModelDesc), C.POINTER(Dropout), vp, C.c_int64, vp,
                                                      vp, C.c_int64, vp, C.c_int64, vp, vp, C.c_int64, vp, vp]
    L.WorldMi355AcousticModelBackward.argtypes = [vp, C.POINTER(AcousticModelDesc), C.POINTER(Dropout), vp, C.c_int64, vp,
                                                  vp, C.c_int64, vp, vp, vp, vp]
    L.WorldMi355DefaultOptimizerOption.restype = None
    L.WorldMi355DefaultOptimizerOption.argtypes = [C.c_int, C.POINTER(OptimizerOption)]
    L.WorldMi355OptimizerStep.argtypes = [vp, C.POINTER(OptimizerOption), C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.WorldMi355WriteFiles.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(C.c_size_t), C.c_int]
    L.WorldMi355CreateLabelFeatureSet.argtypes = [vp, C.c_int, C.POINTER(LabelFeature), C.POINTER(vp)]
    L.WorldMi355DestroyLabelFeatureSet.restype = None
    L.WorldMi355DestroyLabelFeatureSet.argtypes = [vp]
    L.WorldMi355LabelFeatureCount.argtypes = [vp]
    L.WorldMi355LabelFeatures.argtypes = [vp, vp, _ip, _ip, _ip, _ip, C.POINTER(C.c_char_p), _ip, vp, C.c_int64, vp]
    L.WorldMi355LabelPatternMatch.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, _ip, _ip]
    L.WorldMi355HtkHeader.restype = None
    L.WorldMi355HtkHeader.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.WorldMi355TimingEnable.argtypes = [vp, C.c_int]
    L.WorldMi355TimingQuery.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    _lib = L
    return L


def _check(rc: int, where: str) -> None:
    if rc != 0:
        msg = load_library().WorldMi355LastError()
        raise RuntimeError(f"{where}: {ERRORS.get(rc, rc)} ({msg.decode() if msg else ''})")


def default_params(fs: int, frame_period: float = 5.0, **over) -> WorldParams:
    p = WorldParams()
    load_library().WorldMi355DefaultParams(fs, frame_period, C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


F0_ESTIMATORS = ("dio", "harvest")                       # include/world_mi355.h: WM_F0_DIO, WM_F0_HARVEST


def f0_estimator_code(name) -> int:
    """WM_F0_* of an estimator's name; ValueError for any other."""
    if name not in F0_ESTIMATORS:
        raise ValueError("f0_estimator %r: one of %s" % (name, ", ".join(F0_ESTIMATORS)))
    return F0_ESTIMATORS.index(name)


def harvest_workspace_bytes(params: WorldParams, x_lengths) -> int:
    """Bytes of device memory Harvest's workspace takes for a batch of these sample counts
    (WorldMi355HarvestWorkspaceBytes: the sizes its set-up allocates; about 33 KB per 1 ms frame at the default range,
    whatever the frame period).  Host only: needs no device."""
    arr, ptr = _ints(x_lengths)
    out = C.c_int64(0)
    _check(load_library().WorldMi355HarvestWorkspaceBytes(C.byref(params), len(arr), ptr, C.byref(out)),
           "HarvestWorkspaceBytes")
    return int(out.value)


class Context:
    """One HIP stream + the universal randn table on one device."""

    def __init__(self, device: int | None = None, stream_ptr: int | None = None):
        L = load_library()
        h = C.c_void_p()
        _check(L.WorldMi355CreateContext(-1 if device is None else device,
                                         C.c_void_p(stream_ptr) if stream_ptr else None, C.byref(h)),
               "CreateContext")
        self.handle = h
        self.device = device                                # None: the current device (torch_device resolves it)

    def set_stream(self, stream_ptr: int | None = None):
        """Move the context to another HIP stream (WorldMi355SetStream): waits on the host for everything queued on the
        stream it had, then points every later call of the context and of its batches at `stream_ptr` (None or 0: the
        legacy default stream, as in the constructor).  Work of other streams is not waited for: the caller orders the
        new stream behind whatever produced its inputs."""
        _check(load_library().WorldMi355SetStream(self.handle, C.c_void_p(stream_ptr) if stream_ptr else None),
               "SetStream")

    def synchronize(self):
        _check(load_library().WorldMi355Synchronize(self.handle), "Synchronize")

    def timing_enable(self, on: bool = True):
        """Record HIP events on the context's stream around every kernel launch."""
        _check(load_library().WorldMi355TimingEnable(self.handle, 1 if on else 0), "TimingEnable")

    def timing_query(self, kernel: str):
        """(total milliseconds, launches) of `kernel` since timing_enable(); synchronises."""
        ms, n = C.c_double(0.0), C.c_int(0)
        _check(load_library().WorldMi355TimingQuery(self.handle, kernel.encode(), C.byref(ms), C.byref(n)),
               "TimingQuery")
        return ms.value, n.value

    def optimizer_step(self, option, params, grads, rates, slot0=None, slot1=None, want_status=False):
        """One update of every tensor in ONE launch (csrc/optim.hip), by TF 1.x's rule option.rule (default_optimizer_option;
        for adam the caller advances option.beta1_power and beta2_power after the call).  params, grads, slot0, slot1:
        lists of float32 cuda contiguous tensors, a parameter's gradient and slots of its own number of elements (slot0:
        every rule but sgd; slot1: adadelta and adam); rates: one float per tensor.  params and the slots are updated in
        place.  Returns None, or with want_status an int32 cuda tensor [len(params)]: 1 where a gradient element of that
        tensor is not finite.  Asynchronous on the context's stream."""
        n = len(params)
        need = OPTIMIZER_SLOTS[option.rule] if 0 <= option.rule < len(OPTIMIZER_SLOTS) else 0
        lists = [params, grads] + [slot0, slot1][:need]
        if any(l is None or len(l) != n for l in lists) or len(rates) != n:
            raise ValueError("optimizer_step: %d parameters need as many gradients, rates and (%d) slots each" % (n, need))
        device = torch_device(self.device)
        sizes = [check_tensor("optimizer_step", "params[%d]" % k, p, torch.float32, None, device)[1]
                 for k, p in enumerate(params)]
        ptrs = [(C.c_void_p * n)(*[check_tensor("optimizer_step", "%s[%d]" % (name, k), t, torch.float32, sizes[k], device)
                                   for k, t in enumerate(l)])
                for name, l in zip(("params", "grads", "slot0", "slot1"), lists)] + [None] * (2 - need)
        count = (C.c_int64 * n)(*sizes)
        rate = (C.c_float * n)(*[float(r) for r in rates])
        status = torch.empty(n, dtype=torch.int32, device=device) if want_status and n else None
        _check(load_library().WorldMi355OptimizerStep(self.handle, C.byref(option), n, ptrs[0], ptrs[1], ptrs[2], ptrs[3],
                                                      count, rate, status.data_ptr() if status is not None else None),
               "OptimizerStep")
        return status

    def close(self):
        if self.handle:
            load_library().WorldMi355DestroyContext(self.handle)
            self.handle = None


class LabelFeatureSet:
    """A compiled question config and its device tables (WorldMi355CreateLabelFeatureSet).  features: a list of
    (kind, pattern, min, max) -- kind 0 binary, 1 float, 2 .. 7 the reserved names in RESERVED_LABEL_FEATURES' order;
    pattern the text between the braces (None for a reserved feature) -- as recipe.read_question_config returns it.
    Close it before its context."""

    def __init__(self, ctx: Context, features):
        feats = [(int(k), None if p is None else (p.encode("latin-1") if isinstance(p, str) else bytes(p)), int(lo), int(hi))
                 for k, p, lo, hi in features]
        if any(not -2 ** 31 <= v < 2 ** 31 for _, _, lo, hi in feats for v in (lo, hi)):
            raise ValueError("LabelFeatureSet: min and max must fit an int")
        arr = (LabelFeature * max(1, len(feats)))(*[LabelFeature(k, p, lo, hi) for k, p, lo, hi in feats])
        h = C.c_void_p()
        _check(load_library().WorldMi355CreateLabelFeatureSet(ctx.handle, len(feats), arr, C.byref(h)),
               "CreateLabelFeatureSet")
        self.ctx = ctx
        self.handle = h
        self.n_features = int(load_library().WorldMi355LabelFeatureCount(h))

    def close(self):
        if self.handle:
            load_library().WorldMi355DestroyLabelFeatureSet(self.handle)
            self.handle = None


def label_pattern_match(pattern, name, is_float=False, engine=0):
    """One pattern (the text between the braces) against one label name on the host (WorldMi355LabelPatternMatch):
    engine 0 the backtracking matcher, 1 the kernel's bit-parallel program (binary patterns only).  Returns (matched,
    captured value)."""
    enc = lambda s: s.encode("latin-1") if isinstance(s, str) else bytes(s)
    m, v = C.c_int(0), C.c_int(0)
    _check(load_library().WorldMi355LabelPatternMatch(enc(pattern), 1 if is_float else 0, enc(name), int(engine),
                                                      C.byref(m), C.byref(v)), "LabelPatternMatch")
    return bool(m.value), int(v.value)


def _ints(a):
    if a is None:
        return None, None
    arr = np.ascontiguousarray(a, dtype=np.int32)
    return arr, arr.ctypes.data_as(_ip)


def sptk_frames(n_samples, frame_length, frame_shift):
    """The number of frames SPTK's `frame -l frame_length -p frame_shift` makes of n_samples samples
    (WorldMi355SptkFrames: ceil((T + frame_length // 2) / frame_shift), 0 for T = 0).  Host only."""
    n = C.c_int64(0)
    _check(load_library().WorldMi355SptkFrames(int(n_samples), int(frame_length), int(frame_shift), C.byref(n)),
           "SptkFrames")
    return int(n.value)


def sptk_window(type, normalize, length):
    """The table of SPTK's `window -l length -w type -n normalize` as float64 [length] (WorldMi355SptkWindow): type 0
    Blackman, 1 Hamming, 2 Hanning, 5 rectangular; normalize 0 none, 1 sum w^2 = 1, 2 sum w = 1.  Host only."""
    w = np.zeros(max(int(length), 1), dtype=np.float64)
    _check(load_library().WorldMi355SptkWindow(int(type), int(normalize), int(length), w.ctypes.data_as(_dp)),
           "SptkWindow")
    return w[:int(length)]


def mlsa_samples(n_frames, frame_shift):
    """The samples `excite -p frame_shift | mglsadf -p frame_shift` make of n_frames frames (WorldMi355MlsaSamples:
    (n_frames - 1) * frame_shift; n_frames < 2 or frame_shift < 1 is refused).  Host only."""
    n = C.c_int(0)
    _check(load_library().WorldMi355MlsaSamples(int(n_frames), int(frame_shift), C.byref(n)), "MlsaSamples")
    return int(n.value)


def mlsa_pade(order):
    """The Pade row pp[0 .. order] of the MLSA filter as float64 (WorldMi355MlsaPade): SPTK's modified tables at orders 4
    and 5 as recalled, the plain approximant of exp at 1, 2, 3, 6 and 7.  Host only."""
    row = np.zeros(8, dtype=np.float64)
    _check(load_library().WorldMi355MlsaPade(int(order), row.ctypes.data_as(_dp)), "MlsaPade")
    return row[:int(order) + 1]


def mlsa_noise(n):
    """The first n values of excite's Gaussian sequence g (nrandom at seed 1) as float64 (WorldMi355MlsaNoise).  Host
    only."""
    out = np.zeros(max(int(n), 1), dtype=np.float64)
    _check(load_library().WorldMi355MlsaNoise(int(n), out.ctypes.data_as(_dp)), "MlsaNoise")
    return out[:max(int(n), 0)]


def dtw_workspace_bytes(a_lengths, b_lengths) -> int:
    """Bytes of device memory WorldBatch.dtw_align keeps for pairs of these frame counts (WorldMi355DtwWorkspaceBytes: one
    back-pointer byte per cell in strips of 64 rows, two rows of D per pair, the descriptors).  Host only: needs no
    device.  A length outside 0 .. 32767 is refused."""
    aa, ap = _ints(a_lengths)
    ba, bp = _ints(b_lengths)
    if len(aa) != len(ba):
        raise ValueError("dtw_workspace_bytes: %d lengths of a and %d of b" % (len(aa), len(ba)))
    out = C.c_int64(0)
    _check(load_library().WorldMi355DtwWorkspaceBytes(len(aa), ap, bp, C.byref(out)), "DtwWorkspaceBytes")
    return int(out.value)


def _b_offsets(where, b_lengths, n_utt):
    lens = np.asarray(b_lengths, dtype=np.int64).reshape(-1)
    if len(lens) != n_utt:
        raise ValueError("%s: %d lengths of b for %d utterances" % (where, len(lens), n_utt))
    off = np.zeros(n_utt + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return off


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


def pool_distortion(out, kinds):
    """The corpus figures of WorldBatch.feature_distortion outputs.  out: [n_utt][n_groups][4] (numpy, or anything
    np.asarray takes; the rows of several batches or ranks stacked in any order); kinds: the n_groups kinds, 0 cepstral
    and 1 log f0.  Returns one dict per group: kind 0 {"kind": 0, "mean_db": sum e / n, "std_db": its spread over the
    pairs, "pairs": n}; kind 1 {"kind": 1, "rmse_cents": (1200 / ln 2) sqrt(sum D^2 / n) over the pairs voiced on
    both sides, "voiced_pairs": n, "vuv_error_percent": 100 differing / counted, "vuv_errors", "pairs"}.  A figure
    without pairs is nan.  Sums are math.fsum's, exact, so the result does not depend on how a job list was split."""
    o = np.asarray(out, dtype=np.float64).reshape(-1, len(kinds), 4)
    res = []
    for g, kind in enumerate(kinds):
        col = [math.fsum(o[:, g, k].tolist()) for k in range(4)]
        if int(kind) == 0:
            n = int(round(col[2]))
            mean = col[0] / n if n else float("nan")
            var = max(col[1] / n - mean * mean, 0.0) if n else float("nan")
            res.append({"kind": 0, "mean_db": mean, "std_db": math.sqrt(var) if n else float("nan"), "pairs": n})
        elif int(kind) == 1:
            nv, ne, n = int(round(col[1])), int(round(col[2])), int(round(col[3]))
            res.append({"kind": 1,
                        "rmse_cents": 1200.0 / math.log(2.0) * math.sqrt(col[0] / nv) if nv else float("nan"),
                        "voiced_pairs": nv, "vuv_error_percent": 100.0 * ne / n if n else float("nan"),
                        "vuv_errors": ne, "pairs": n})
        else:
            raise ValueError("pool_distortion: kind %r is neither 0 nor 1" % (kind,))
    return res


MCEP_OPTIONS = ("order", "alpha", "itr1", "itr2", "dd", "etype", "e", "f", "itype")


class WorldBatch:
    """A batch of utterances resident in HBM (torch cuda tensors, float64).

    x is the concatenation of the waveforms (see ``sample_offsets``); t, f0 have
    ``total_frames`` entries, sp/ap ``total_frames x (fft_size/2+1)``.

    Every tensor argument is checked on the host against the dtype, shape, layout and device its method states
    (check_tensor: ValueError); every output is made on ``device``, the context's.
    """

    def __init__(self, ctx: Context, params: WorldParams, x_lengths=None, f0_lengths=None, y_lengths=None,
                 f0_estimator="dio", refine=True):
        """f0_estimator, refine: the f0 front end of analyze() and analyze_synthesize() (set_f0_estimator)."""
        L = load_library()
        code = f0_estimator_code(f0_estimator)
        self.ctx = ctx
        self.params = params
        n = len(x_lengths) if x_lengths is not None else len(f0_lengths)
        xa, xp = _ints(x_lengths)
        fa, fp = _ints(f0_lengths)
        ya, yp = _ints(y_lengths)
        h = C.c_void_p()
        _check(L.WorldMi355CreateBatch(ctx.handle, C.byref(params), n, xp, fp, yp, C.byref(h)), "CreateBatch")
        self.handle = h
        self.n_utt = n
        self.total_samples = L.WorldMi355BatchTotalSamples(h)
        self.total_frames = L.WorldMi355BatchTotalFrames(h)
        self.total_out = L.WorldMi355BatchTotalOutputSamples(h)
        self.fft_size = L.WorldMi355BatchFftSize(h)
        self.bins = self.fft_size // 2 + 1
        self.sample_offsets = np.ctypeslib.as_array(L.WorldMi355BatchSampleOffsets(h), (n + 1,)).copy()
        self.frame_offsets = np.ctypeslib.as_array(L.WorldMi355BatchFrameOffsets(h), (n + 1,)).copy()
        self.out_offsets = np.ctypeslib.as_array(L.WorldMi355BatchOutputOffsets(h), (n + 1,)).copy()
        self.f0_estimator, self.refine = "dio", True
        try:
            self.device = torch_device(getattr(ctx, "device", None))       # where the library runs: outputs, checks
            if (code, bool(refine)) != (0, True):
                self.set_f0_estimator(f0_estimator, refine)
        except Exception:
            self.close()
            raise

    def set_f0_estimator(self, f0_estimator="dio", refine=True):
        """The f0 front end of analyze() and analyze_synthesize() from the next call on: "dio" (a new batch's) or "harvest",
        with StoneMask behind it (refine) or its contour as it is.  The chain gives the bits of the stages called one by
        one.  A name other than the two raises ValueError; a batch without x_lengths is refused."""
        code = f0_estimator_code(f0_estimator)
        _check(load_library().WorldMi355BatchSetF0Estimator(self.handle, code, 1 if refine else 0), "BatchSetF0Estimator")
        self.f0_estimator, self.refine = f0_estimator, bool(refine)

    def _new(self, *shape, dtype=None, zero=False):
        """Every output and status tensor: on the batch's device, float64 unless `dtype` says otherwise."""
        return (torch.zeros if zero else torch.empty)(shape, dtype=dtype or torch.float64, device=self.device)

    def _f64(self, where, name, t, *shape, **mode):
        return check_tensor(where, name, t, torch.float64, shape, self.device, **mode)

    def _f32(self, where, name, t, *shape, **mode):
        return check_tensor(where, name, t, torch.float32, shape, self.device, **mode)

    def _out(self, where, out, *shape, name="out"):
        """A caller's float64 output, checked, or a fresh one: (tensor, pointer)."""
        if out is None:
            out = self._new(*shape)
            return out, _ptr(out)
        return out, self._f64(where, name, out, *shape)

    def _xtf0(self, where, x, t, f0):
        return (self._f64(where, "x", x, self.total_samples), self._f64(where, "t", t, self.total_frames),
                self._f64(where, "f0", f0, self.total_frames))

    def _f0_sp_ap(self, where, f0, sp, ap, optional=False):
        return (self._f64(where, "f0", f0, self.total_frames, optional=optional),
                self._f64(where, "sp", sp, self.total_frames, self.bins, optional=optional),
                self._f64(where, "ap", ap, self.total_frames, self.bins, optional=optional))

    def _f0_front(self, where, call, x):
        xp = self._f64(where, "x", x, self.total_samples)
        t, f0 = self._new(self.total_frames), self._new(self.total_frames)
        _check(getattr(load_library(), "WorldMi355" + call)(self.handle, xp, _ptr(t), _ptr(f0)), call)
        return t, f0

    def dio(self, x):
        return self._f0_front("dio", "Dio", x)

    def harvest(self, x):
        return self._f0_front("harvest", "Harvest", x)

    def stonemask(self, x, t, f0):
        args = self._xtf0("stonemask", x, t, f0)
        out = self._new(self.total_frames)
        _check(load_library().WorldMi355StoneMask(self.handle, *args, _ptr(out)), "StoneMask")
        return out

    def _per_bin(self, where, call, x, t, f0, out):
        args = self._xtf0(where, x, t, f0)
        out, op = self._out(where, out, self.total_frames, self.bins)
        _check(getattr(load_library(), "WorldMi355" + call)(self.handle, *args, op), call)
        return out

    def cheaptrick(self, x, t, f0, out=None):
        return self._per_bin("cheaptrick", "CheapTrick", x, t, f0, out)

    def d4c(self, x, t, f0, out=None):
        return self._per_bin("d4c", "D4C", x, t, f0, out)

    def samples_from_pcm16(self, pcm, out=None):
        """int16 cuda tensor [total_samples] (the wav payload) -> float64 samples s / 32768 (wavread)."""
        pp = check_tensor("samples_from_pcm16", "pcm", pcm, torch.int16, int(self.total_samples), self.device)
        x, xp = self._out("samples_from_pcm16", out, self.total_samples)
        _check(load_library().WorldMi355SamplesFromPcm16(self.handle, pp, xp), "SamplesFromPcm16")
        return x

    def samples_to_pcm16(self, y, out=None):
        """float64 y [total_out] -> int16 as wavwrite stores it: clamp(int(y * 32767)), truncating towards zero."""
        yp = self._f64("samples_to_pcm16", "y", y, self.total_out)
        pcm = out if out is not None else self._new(self.total_out, dtype=torch.int16)
        pp = check_tensor("samples_to_pcm16", "out", pcm, torch.int16, int(self.total_out), self.device)
        _check(load_library().WorldMi355SamplesToPcm16(self.handle, yp, pp), "SamplesToPcm16")
        return pcm

    def _analysis_out(self, where, out):
        """analyze's (t, f0, sp, ap), fresh or the caller's four, checked: (the tensors, their pointers)."""
        shapes = ((self.total_frames,), (self.total_frames,), (self.total_frames, self.bins), (self.total_frames, self.bins))
        if out is None:
            out = tuple(self._new(*s) for s in shapes)
            return out, [_ptr(t) for t in out]
        if not isinstance(out, (tuple, list)) or len(out) != 4:
            raise ValueError(f"{where}: out must be the four tensors (t, f0, sp, ap)")
        return tuple(out), [self._f64(where, "out[%d]" % k, t, *s) for k, (t, s) in enumerate(zip(out, shapes))]

    def analyze(self, x, out=None):
        """Dio -> StoneMask -> CheapTrick -> D4C (test/analysis.cpp:243-390); with set_f0_estimator, Harvest in Dio's place
        and StoneMask or not."""
        xp = self._f64("analyze", "x", x, self.total_samples)
        out, ptrs = self._analysis_out("analyze", out)
        _check(load_library().WorldMi355Analyze(self.handle, xp, *ptrs), "Analyze")
        return out

    def analyze_synthesize(self, x, out=None, y=None):
        """analyze() then synthesize() of its own features as one call: the f0-only part of Synthesis overlaps
        CheapTrick and D4C on a second stream.  Returns (t, f0, sp, ap, y), bit-identical to the two calls."""
        xp = self._f64("analyze_synthesize", "x", x, self.total_samples)
        out, ptrs = self._analysis_out("analyze_synthesize", out)
        y, yp = self._out("analyze_synthesize", y, self.total_out, name="y")
        _check(load_library().WorldMi355AnalyzeSynthesize(self.handle, xp, *ptrs, yp), "AnalyzeSynthesize")
        return out + (y,)

    def synthesize(self, f0, sp, ap, out=None):
        args = self._f0_sp_ap("synthesize", f0, sp, ap)
        y, yp = self._out("synthesize", out, self.total_out)
        _check(load_library().WorldMi355Synthesis(self.handle, *args, yp), "Synthesis")
        return y

    def vibrato(self, lf0, segments):
        """The recipe's vibrato feature (data/scripts/Extract.py).  lf0: float32 cuda [total_frames];
        segments: per utterance a list of (start_frame, end_frame, note_pitch_hz).  Returns (vib, lf0_2col, n_too_long):
        float32 cuda tensors [total_frames][2] after the script's soprLog."""
        lp = self._f32("vibrato", "lf0", lf0, self.total_frames)
        if len(segments) != self.n_utt:
            raise ValueError(f"vibrato: {len(segments)} segment lists for {self.n_utt} utterances")
        off = np.zeros(self.n_utt + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(s) for s in segments])
        flat = [seg for s in segments for seg in s]
        ss = np.ascontiguousarray([int(v[0]) for v in flat], dtype=np.int32)
        se = np.ascontiguousarray([int(v[1]) for v in flat], dtype=np.int32)
        sp_ = np.ascontiguousarray([float(v[2]) for v in flat], dtype=np.float64)
        vib = self._new(self.total_frames, 2, dtype=torch.float32)
        out = self._new(self.total_frames, 2, dtype=torch.float32)
        n = C.c_int(0)
        _check(load_library().WorldMi355Vibrato(self.handle, lp, off.ctypes.data_as(_ip), ss.ctypes.data_as(_ip),
                                                se.ctypes.data_as(_ip), sp_.ctypes.data_as(_dp), _ptr(vib), _ptr(out),
                                                C.byref(n)), "Vibrato")
        return vib, out, n.value

    def utterance_status(self, x=None, f0=None, sp=None, ap=None):
        """int32 cuda tensor [n_utt] of WM_UTT_* flags (1 non-finite input, 2 too short for Dio -- not set when the batch's
        estimator is Harvest --, 4 non-finite output).  x float64 [total_samples], f0, sp, ap as analyze's, each or None."""
        xp = self._f64("utterance_status", "x", x, self.total_samples, optional=True)
        args = self._f0_sp_ap("utterance_status", f0, sp, ap, optional=True)
        st = self._new(self.n_utt, dtype=torch.int32, zero=True)
        _check(load_library().WorldMi355UtteranceStatus(self.handle, xp, *args, _ptr(st)), "UtteranceStatus")
        return st

    # ---- feature codec (world/codec.h) ----
    def _codec(self, where, call, name, t, cols, out_cols, *dims):
        """One codec call: float64 [total_frames][cols] (None: free, passed on) -> float64 [total_frames][out_cols]."""
        res = self._f64(where, name, t, self.total_frames, cols)
        tp, *free = res if cols is None else (res,)
        out = self._new(self.total_frames, out_cols)
        _check(getattr(load_library(), "WorldMi355" + call)(self.handle, tp, *dims, *free, _ptr(out)), call)
        return out

    def _n_aperiodicities(self):
        return load_library().WorldMi355GetNumberOfAperiodicities(int(self.params.fs))

    def code_spectral_envelope(self, sp, number_of_dimensions):
        """sp float64 [total_frames][fft_size/2+1] -> float64 [total_frames][number_of_dimensions] (codec.cpp:268-295)."""
        return self._codec("code_spectral_envelope", "CodeSpectralEnvelope", "sp", sp, self.bins, number_of_dimensions,
                           number_of_dimensions)

    def decode_spectral_envelope(self, coded):
        """coded float64 [total_frames][number of dimensions] -> sp [total_frames][fft_size/2+1] (codec.cpp:297-324)."""
        return self._codec("decode_spectral_envelope", "DecodeSpectralEnvelope", "coded", coded, None, self.bins)

    def code_aperiodicity(self, ap):
        """ap float64 [total_frames][fft_size/2+1] -> float64 [total_frames][bands of fs] (codec.cpp:217-235)."""
        return self._codec("code_aperiodicity", "CodeAperiodicity", "ap", ap, self.bins, self._n_aperiodicities())

    def decode_aperiodicity(self, coded):
        """coded float64 [total_frames][bands of fs] -> ap [total_frames][fft_size/2+1] (codec.cpp:237-266)."""
        return self._codec("decode_aperiodicity", "DecodeAperiodicity", "coded", coded, self._n_aperiodicities(), self.bins)

    def recipe_features(self, f0, sp, ap, spec_dim=50, ap_dim=25):
        """float32 lf0 / mgc / bap as the recipe's `analysis ... 5 2048 50 25` call writes them."""
        args = self._f0_sp_ap("recipe_features", f0, sp, ap)
        lf0 = self._new(self.total_frames, dtype=torch.float32)
        mgc = self._new(self.total_frames, spec_dim, dtype=torch.float32)
        bap = self._new(self.total_frames, ap_dim, dtype=torch.float32)
        _check(load_library().WorldMi355RecipeFeatures(self.handle, *args, spec_dim, ap_dim, _ptr(lf0), _ptr(mgc),
                                                       _ptr(bap)), "RecipeFeatures")
        return lf0, mgc, bap

    def recipe_decode(self, lf0, mgc, bap):
        """f0 / sp / ap from the recipe's float32 lf0 [total_frames] / mgc [total_frames][spec_dim] / bap
        [total_frames][ap_dim], as the synth CLI rebuilds them (test/synth.cpp:151-256); ap bins beyond the coding order
        are 0 (uninitialised in the reference)."""
        lp = self._f32("recipe_decode", "lf0", lf0, self.total_frames)
        mp, spec_dim = self._f32("recipe_decode", "mgc", mgc, self.total_frames, None)
        bp, ap_dim = self._f32("recipe_decode", "bap", bap, self.total_frames, None)
        f0, sp, ap = self._new(self.total_frames), self._new(self.total_frames, self.bins), self._new(self.total_frames, self.bins)
        _check(load_library().WorldMi355RecipeDecode(self.handle, lp, mp, bp, spec_dim, ap_dim, _ptr(f0), _ptr(sp),
                                                     _ptr(ap)), "RecipeDecode")
        return f0, sp, ap

    def _mcep(self, where, call, src, order, alpha, itype, opt, *front):
        """What the three mel-cepstrum calls share behind their checked input `src`: the option, (mc, status), the call
        with `front` between the input and the option."""
        o = _option(where, McepOption, "WorldMi355DefaultMcepOption",
                    dict({"itype": itype}, **opt, order=int(order), alpha=float(alpha)), MCEP_OPTIONS)
        mc = self._new(self.total_frames, max(int(order), 0) + 1)
        status = self._new(self.total_frames, dtype=torch.int32)
        _check(getattr(load_library(), "WorldMi355" + call)(self.handle, src, *front, C.byref(o), _ptr(mc), _ptr(status)),
               call)
        return mc, status

    def mel_cepstrum(self, spectrum, order=25, alpha=0.35, **opt):
        """SPTK's mcep per frame (test/sptkfunctions.cpp:11-184 with flng = fft_size): spectrum is float64 cuda
        [total_frames][fft_size/2+1], amplitudes (itype=3, the default) or periodograms (itype=4).  Further options
        as WorldMi355McepOption's fields: itr1, itr2, dd, etype, e, f.  Returns (mc float64 [total_frames][order+1],
        status int32 [total_frames]: 0 converged, -1 itr2 steps without meeting dd, 1 singular pivot in theq,
        2 a periodogram value <= 0 or non-finite)."""
        src = self._f64("mel_cepstrum", "spectrum", spectrum, self.total_frames, self.bins)
        return self._mcep("mel_cepstrum", "MelCepstrum", src, order, alpha, 3, opt)

    def mel_cepstrum_of_frames(self, frames, order=25, alpha=0.35, **opt):
        """SPTK's mcep with itype 0 per frame (test/sptkfunctions.cpp:11-184 with flng = fft_size): frames is float64 cuda
        [total_frames][fft_size], windowed and zero-padded.  Options as mel_cepstrum's; etype 2 (the floor e < 0 dB below
        the frame's maximum) is taken here.  Returns (mc, status) as mel_cepstrum does."""
        src = self._f64("mel_cepstrum_of_frames", "frames", frames, self.total_frames, self.fft_size)
        return self._mcep("mel_cepstrum_of_frames", "MelCepstrumOfFrames", src, order, alpha, 0, opt)

    def mel_cepstrum_of_waveform(self, x, window, frame_length, frame_shift, order=25, alpha=0.35, pipe_float32=False,
                                 **opt):
        """`frame -l frame_length -p frame_shift | window | mgcep` at gamma 0 from the batch's packed samples: x float64
        cuda [total_samples]; window the host table of frame_length doubles (sptk_window's); the batch's f0_lengths must
        be sptk_frames of its x_lengths.  pipe_float32 rounds every windowed sample to float32 once, as SPTK's pipe does.
        Options as mel_cepstrum_of_frames'.  Returns (mc, status) as mel_cepstrum does."""
        src = self._f64("mel_cepstrum_of_waveform", "x", x, self.total_samples)
        w = np.ascontiguousarray(window, dtype=np.float64)
        if w.shape != (max(int(frame_length), 0),):
            raise ValueError(f"mel_cepstrum_of_waveform: window must hold frame_length = {frame_length} values, "
                             f"got {w.shape}")
        return self._mcep("mel_cepstrum_of_waveform", "MelCepstrumOfWaveform", src, order, alpha, 0, opt,
                          w.ctypes.data_as(_dp), int(frame_length), int(frame_shift), 1 if pipe_float32 else 0)

    @staticmethod
    def _mlsa_option(where, order=25, alpha=0.35, pade_order=4, frame_shift=100, pipe_float32=False, pade=None):
        o = _option(where, MlsaOption, "WorldMi355DefaultMlsaOption",
                    dict(order=int(order), alpha=float(alpha), pade_order=int(pade_order), frame_shift=int(frame_shift),
                         pipe_float32=1 if pipe_float32 else 0))
        if pade is not None:
            row = [float(v) for v in pade]
            if len(row) != int(pade_order) + 1 or len(row) > 8:
                raise ValueError(f"mlsa: pade must hold pade_order + 1 = {int(pade_order) + 1} values, got {len(row)}")
            o.use_pade = 1
            for k, v in enumerate(row):
                o.pade[k] = v
        return o

    @staticmethod
    def _mlsa_taps(where, name, taps):
        t = np.ascontiguousarray(taps, dtype=np.float64)
        if t.ndim != 1:
            raise ValueError(f"{where}: {name} must be a list of taps, got shape {t.shape}")
        return t.ctypes.data_as(_dp), len(t), t

    def mlsa_excitation(self, pitch, lowpass, highpass, frame_shift=100, pipe_float32=False):
        """`excite -n -p frame_shift pit | dfs -b lowpass` plus `excite` of an all-zero pitch `| dfs -b highpass`
        (scripts/Training.pl:2873-2899): pitch float32 cuda [total_frames], the period in samples with 0 for unvoiced;
        lowpass, highpass the caller's taps (1 to 256 each, host).  The batch's y_lengths must be mlsa_samples of its
        f0_lengths.  Returns e float64 [total output samples]; an utterance with a non-finite or negative pitch is zeros."""
        where = "mlsa_excitation"
        o = self._mlsa_option(where, frame_shift=frame_shift, pipe_float32=pipe_float32)
        lp, hp = self._mlsa_taps(where, "lowpass", lowpass), self._mlsa_taps(where, "highpass", highpass)
        pp = self._f32(where, "pitch", pitch, self.total_frames)
        e = self._new(self.total_out)
        _check(load_library().WorldMi355MlsaExcitation(self.handle, pp, *lp[:2], *hp[:2], C.byref(o), _ptr(e)),
               "MlsaExcitation")
        return e

    def mlsa_filter(self, e, mc, alpha=0.35, pade_order=4, frame_shift=100, pipe_float32=False, pade=None):
        """`mglsadf -m order -a alpha -P pade_order -p frame_shift -c 0` at interpolation period 1: e float64 cuda [total
        output samples], mc float32 cuda [total_frames][order+1]; pade a caller's row of pade_order + 1 values in place of
        mlsa_pade's.  Returns (y float64 [total output samples], status int32 [n_utt]: 0 fine, 1 a non-finite coefficient
        -- the utterance is zeros --, 2 a non-finite output sample)."""
        where = "mlsa_filter"
        mp, cols = self._f32(where, "mc", mc, self.total_frames, None)
        ep = self._f64(where, "e", e, self.total_out)
        o = self._mlsa_option(where, cols - 1, alpha, pade_order, frame_shift, pipe_float32, pade)
        y, status = self._new(self.total_out), self._new(self.n_utt, dtype=torch.int32)
        _check(load_library().WorldMi355MlsaFilter(self.handle, ep, mp, C.byref(o), _ptr(y), _ptr(status)), "MlsaFilter")
        return y, status

    def mlsa_synthesis(self, pitch, mc, lowpass, highpass, order=None, alpha=0.35, pade_order=4, frame_shift=100,
                       pipe_float32=False, pade=None):
        """mlsa_excitation and mlsa_filter in one call, bit for bit, without the excitation in device memory beyond the
        block being filtered.  order, if given, must be mc's.  Returns (y, status) as mlsa_filter does; status 1 also for
        a non-finite or negative pitch."""
        where = "mlsa_synthesis"
        mp, cols = self._f32(where, "mc", mc, self.total_frames, None)
        if order is not None and int(order) != cols - 1:
            raise ValueError(f"{where}: mc must be [total_frames][order+1], got {tuple(mc.shape)} at order {order}")
        pp = self._f32(where, "pitch", pitch, self.total_frames)
        o = self._mlsa_option(where, cols - 1, alpha, pade_order, frame_shift, pipe_float32, pade)
        lp, hp = self._mlsa_taps(where, "lowpass", lowpass), self._mlsa_taps(where, "highpass", highpass)
        y, status = self._new(self.total_out), self._new(self.n_utt, dtype=torch.int32)
        _check(load_library().WorldMi355MlsaSynthesis(self.handle, pp, mp, *lp[:2], *hp[:2], C.byref(o), _ptr(y),
                                                      _ptr(status)), "MlsaSynthesis")
        return y, status

    def dtw_align(self, a, b, b_lengths, first=0, count=None):
        """The dynamic-time-warping path between the batch's utterances in `a` and their counterparts in `b`
        (WorldMi355DtwAlign; the definition is in include/world_mi355.h): a float32 cuda [total_frames][ld_a] on the batch's
        frame layout, b float32 cuda [sum(b_lengths)][ld_b], utterance u's b_lengths[u] rows one after another; the
        Euclidean distance over the columns [first, first + count) of both (count None: every column of `a` from `first`
        on; 1 to 64 columns).  Returns (path int32 [sum(T_a + T_b - 1)][2] -- utterance u's pairs (i, j) from index
        frame_offsets[u] + b_offsets[u] - u on, (-1, -1) behind them --, path_len int32 [n_utt], cost float64 [n_utt],
        status int32 [n_utt]: bit 1 a non-finite value in the used columns, bit 2 an empty side; either way path_len 0)."""
        where = "dtw_align"
        off = _b_offsets(where, b_lengths, self.n_utt)
        ap, ld_a = self._f32(where, "a", a, self.total_frames, None)
        bp, ld_b = self._f32(where, "b", b, int(off[-1]), None)
        if count is None:
            count = ld_a - int(first)
        cap = max(int(self.total_frames + off[-1] - self.n_utt), 0)
        path = self._new(cap, 2, dtype=torch.int32)
        path_len, status = self._new(self.n_utt, dtype=torch.int32), self._new(self.n_utt, dtype=torch.int32)
        cost = self._new(self.n_utt)
        _check(load_library().WorldMi355DtwAlign(self.handle, ap, ld_a, bp, ld_b, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 int(first), int(count), _ptr(path), _ptr(path_len), _ptr(cost),
                                                 _ptr(status)), "DtwAlign")
        return path, path_len, cost, status

    def feature_distortion(self, groups, b_lengths, path=None, path_len=None, b_mask=None, voiced_above=-1e9):
        """The distortion measures along a path (WorldMi355FeatureDistortion).  groups: 1 to 8 of (a, b, first, count, kind)
        with a and b as dtw_align takes them and kind 0 (cepstral: e = (10 / ln 10) sqrt(2 sum D^2) in dB per pair) or 1
        (log f0, count 1; a value above voiced_above is voiced).  path, path_len: dtw_align's, or both None: the pairs
        (k, k) for k < min(T_a, T_b).  b_mask: None or uint8 cuda [sum(b_lengths)], 0 where a frame of b is left out.
        Returns float64 cuda [n_utt][n_groups][4]: kind 0 (sum e, sum e^2, counted pairs, 0); kind 1 (sum D^2 over the
        pairs voiced on both sides, those pairs, the pairs whose voicing differs, counted pairs).  pool_distortion makes
        the corpus figures of it."""
        where = "feature_distortion"
        off = _b_offsets(where, b_lengths, self.n_utt)
        groups = list(groups)
        arr = (DistortionGroup * max(1, len(groups)))()
        for g, (a, b, first, count, kind) in enumerate(groups):
            ap, ld_a = self._f32(where, "groups[%d][0]" % g, a, self.total_frames, None)
            bp, ld_b = self._f32(where, "groups[%d][1]" % g, b, int(off[-1]), None)
            arr[g] = DistortionGroup(ap, ld_a, bp, ld_b, int(first), int(count), int(kind))
        if (path is None) != (path_len is None):
            raise ValueError(f"{where}: path and path_len come together")
        cap = max(int(self.total_frames + off[-1] - self.n_utt), 0)
        pp = check_tensor(where, "path", path, torch.int32, (cap, 2), self.device, optional=True)
        lp = check_tensor(where, "path_len", path_len, torch.int32, (self.n_utt,), self.device, optional=True)
        mp = check_tensor(where, "b_mask", b_mask, torch.uint8, (int(off[-1]),), self.device, optional=True)
        o = _option(where, DistortionOption, "WorldMi355DefaultDistortionOption", {"voiced_above": float(voiced_above)})
        out = self._new(self.n_utt, len(groups), 4)
        _check(load_library().WorldMi355FeatureDistortion(self.handle, pp, lp, off.ctypes.data_as(C.POINTER(C.c_int64)), mp,
                                                          len(groups), arr, C.byref(o), _ptr(out)), "FeatureDistortion")
        return out

    def spectrum_from_mel_cepstrum(self, mc, alpha=0.35, gamma=0.0, out_format=0, phase=False):
        """SPTK's mgc2sp per frame (test/sptkfunctions.cpp:186-219 with flng = fft_size): mc is float64 cuda
        [total_frames][order+1], mel-generalized cepstra at (alpha, gamma), -1 <= gamma <= 0.  out_format 0 gives
        ln|H|, 3 |H|, 4 |H|^2 (as mel_cepstrum's itype).  Returns (spectrum float64 [total_frames][fft_size/2+1],
        status int32 [total_frames]: 0 fine, 1 a non-finite coefficient or 1 + gamma c0 <= 0, the row is zeros), with
        phase=True (spectrum, phase, status), phase being the transform's imaginary part."""
        where = "spectrum_from_mel_cepstrum"
        mp, cols = self._f64(where, "mc", mc, self.total_frames, None)
        o = _option(where, Mgc2spOption, "WorldMi355DefaultMgc2spOption",
                    dict(alpha=float(alpha), gamma=float(gamma), order=cols - 1, out_format=int(out_format)))
        sp = self._new(self.total_frames, self.bins)
        ph = self._new(self.total_frames, self.bins) if phase else None
        status = self._new(self.total_frames, dtype=torch.int32)
        _check(load_library().WorldMi355MelCepstrumToSpectrum(self.handle, mp, C.byref(o), _ptr(sp), _ptr(ph),
                                                              _ptr(status)), "MelCepstrumToSpectrum")
        return (sp, ph, status) if phase else (sp, status)

    def convert_mel_generalized_cepstrum(self, mc, alpha, gamma, out_order, out_alpha, out_gamma, normalized=False,
                                         multiplied=False, out_normalized=False, out_multiplied=False):
        """SPTK's mgc2mgc per frame (the core: test/sptkfunctions.cpp:221-254; the flags as include/world_mi355.h
        defines them, flag semantics unpinned against SPTK's command): mc is float64 cuda [total_frames][order+1] at
        (alpha, gamma), the result float64 [total_frames][out_order+1] at (out_alpha, out_gamma).  normalized /
        multiplied are -n / -u of the input, out_normalized / out_multiplied -N / -U of the output.  |alpha| < 1,
        -1 <= gamma <= 1, orders 1 .. 4095 of which one is at most 63.  Returns (out, status int32 [total_frames]:
        0 fine, 1 a non-finite coefficient or a gain that is not positive, 2 a non-finite result; flagged rows are
        zeros)."""
        where = "convert_mel_generalized_cepstrum"
        mp, cols = self._f64(where, "mc", mc, self.total_frames, None)
        o = _option(where, MgcConvertOption, "WorldMi355DefaultMgcConvertOption",
                    dict(in_order=cols - 1, in_alpha=float(alpha), in_gamma=float(gamma), in_normalized=int(bool(normalized)),
                         in_multiplied=int(bool(multiplied)), out_order=int(out_order), out_alpha=float(out_alpha),
                         out_gamma=float(out_gamma), out_normalized=int(bool(out_normalized)),
                         out_multiplied=int(bool(out_multiplied))))
        out = self._new(self.total_frames, max(int(out_order), 0) + 1)
        status = self._new(self.total_frames, dtype=torch.int32)
        _check(load_library().WorldMi355MelGeneralizedCepstrumConvert(self.handle, mp, C.byref(o), _ptr(out),
                                                                      _ptr(status)), "MelGeneralizedCepstrumConvert")
        return out, status

    def modify_features(self, f0=None, sp=None, f0_scale=None, formant_ratio=None, out=None):
        """f0 [total_frames] times f0_scale and sp [total_frames][bins] stretched by formant_ratio, per utterance
        (WorldMi355ModifyFeatures, csrc/modify.hip; modify.py has the chain around it).

        f0_scale, formant_ratio: None, a number for every utterance, or one number per utterance.  At least one is
        given; the tensor of a part that is given must be given too.  out: None for fresh tensors, or (f0_out, sp_out)
        with None for a part that is to be fresh; an output may be its own input (in place), not a shifted view of it.
        Returns (f0_out, sp_out); a part that is not done is the argument as it came (None included).  Bad factors and
        bad tensors raise ValueError before the library is called.  Asynchronous on the context's stream."""
        where = "modify_features"
        if f0_scale is None and formant_ratio is None:
            raise ValueError(f"{where}: give f0_scale, formant_ratio or both")
        shift = factor_array(where, "f0_scale", f0_scale, self.n_utt)
        ratio = factor_array(where, "formant_ratio", formant_ratio, self.n_utt, self.fft_size)
        if out is None:
            out = (None, None)
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise ValueError(f"{where}: out must be (f0_out, sp_out), either of them None")
        f0_out, sp_out = f0, sp
        f0p = spp = f0op = spop = None
        if shift is not None:
            f0p = self._f64(where, "f0", f0, self.total_frames)
            f0_out, f0op = self._out(where, out[0], self.total_frames, name="out[0]")
        if ratio is not None:
            spp = self._f64(where, "sp", sp, self.total_frames, self.bins)
            sp_out, spop = self._out(where, out[1], self.total_frames, self.bins, name="out[1]")
        _check(load_library().WorldMi355ModifyFeatures(
            self.handle, None if shift is None else shift.ctypes.data_as(_dp),
            None if ratio is None else ratio.ctypes.data_as(_dp), f0p, spp, f0op, spop), "ModifyFeatures")
        return f0_out, sp_out

    def postfilter_mel_cepstrum(self, mc, alpha=0.35, beta=1.4, length=4096, gain=False):
        """The recipe's formant emphasis per frame (scripts/Training.pl:2642-2687, postfiltering_mcp): mc is float64
        cuda [total_frames][order+1], mel-cepstra at warp alpha.  out[0] = c[0] + delta, out[k] = w[k] c[k] with
        w = [1, 1, beta, ..., beta] and delta = 1/2 ln(E(c) / E(w c)), E the mean of the power spectrum over `length`
        bins.  Returns (out float64 [total_frames][order+1], status int32 [total_frames]: 0 fine, 1 a non-finite
        coefficient, 2 a sum that is not finite and positive; flagged rows are zeros), with gain=True
        (out, gain float64 [total_frames] = delta, status).  beta == 1 or order == 1 copies the rows."""
        where = "postfilter_mel_cepstrum"
        mp, cols = self._f64(where, "mc", mc, self.total_frames, None)
        o = _option(where, McpfOption, "WorldMi355DefaultMcpfOption",
                    dict(alpha=float(alpha), beta=float(beta), order=cols - 1, length=int(length)))
        out = self._new(self.total_frames, cols)
        g = self._new(self.total_frames) if gain else None
        status = self._new(self.total_frames, dtype=torch.int32)
        _check(load_library().WorldMi355MelCepstrumPostfilter(self.handle, mp, C.byref(o), _ptr(out), _ptr(g),
                                                              _ptr(status)), "MelCepstrumPostfilter")
        return (out, g, status) if gain else (out, status)

    @staticmethod
    def _mspf_option(where, frame_length, fft_length, emphasis=1.0):
        return _option(where, MspfOption, "WorldMi355DefaultMspfOption",
                       dict(frame_length=int(frame_length), fft_length=int(fft_length), emphasis=float(emphasis)))

    def utterance_means(self, x):
        """Column means per utterance of x, float64 cuda [total_frames][dim]: float64 [n_utt][dim], summed in a fixed
        order that depends on the utterance's length alone (a batch holds no utterance without frames)."""
        xp, dim = self._f64("utterance_means", "x", x, self.total_frames, None)
        mean = self._new(self.n_utt, dim)
        _check(load_library().WorldMi355ColumnMeans(self.handle, xp, dim, _ptr(mean)), "ColumnMeans")
        return mean

    def modulation_spectrum_stats(self, x, frame_length=25, fft_length=64, mean=None):
        """The sums behind make_mspf's statistics (scripts/Training.pl:3133-3221) over this batch: x float64 cuda
        [total_frames][dim]; mean None (each utterance's own column means) or float64 cuda [n_utt][dim] (silence
        removal: the whole utterance's).  Returns (sum, sumsq float64 cuda [dim][fft_length/2+1], n_frames int): add
        them across batches and hand them to mspf_finalize."""
        where = "modulation_spectrum_stats"
        xp, dim = self._f64(where, "x", x, self.total_frames, None)
        mp = self._f64(where, "mean", mean, self.n_utt, dim, optional=True)
        o = self._mspf_option(where, frame_length, fft_length)
        K = int(fft_length) // 2 + 1
        s1, s2 = self._new(dim, K), self._new(dim, K)
        n = C.c_int64(0)
        _check(load_library().WorldMi355ModulationSpectrumStats(self.handle, xp, dim, C.byref(o), mp, _ptr(s1), _ptr(s2),
                                                                C.byref(n)), "ModulationSpectrumStats")
        return s1, s2, int(n.value)

    def postfilter_modulation_spectrum(self, x, mean_gen, std_gen, mean_nat, std_nat, emphasis=1.0, frame_length=25,
                                       fft_length=64):
        """The recipe's modulation-spectrum postfilter (scripts/Training.pl:2950-3038, postfiltering_mspf), which
        gen_wave runs instead of postfilter_mel_cepstrum with USEMSPF: x float64 cuda [total_frames][dim]; the four
        tables [dim][fft_length/2+1] (numpy or tensors; they are validated and uploaded by the library).  Returns
        (out float64 [total_frames][dim], status int32 [n_utt]: bit 1 a column with a non-finite input, bit 2 a result
        that is not finite; such a column is zeros in that utterance)."""
        where = "postfilter_modulation_spectrum"
        xp, dim = self._f64(where, "x", x, self.total_frames, None)
        K = int(fft_length) // 2 + 1
        tabs = []
        for name, t in (("mean_gen", mean_gen), ("std_gen", std_gen), ("mean_nat", mean_nat), ("std_nat", std_nat)):
            a = np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float64)
            if a.shape != (dim, K):
                raise ValueError(f"{where}: {name} must be [{dim}][{K}], got {a.shape}")
            tabs.append(a)
        o = self._mspf_option(where, frame_length, fft_length, emphasis)
        out, status = self._new(self.total_frames, dim), self._new(self.n_utt, dtype=torch.int32)
        _check(load_library().WorldMi355ModulationSpectrumPostfilter(
            self.handle, xp, dim, C.byref(o), *[a.ctypes.data_as(C.c_void_p) for a in tabs], _ptr(out), _ptr(status)),
            "ModulationSpectrumPostfilter")
        return out, status

    def _compose_streams(self, where, tensors, window_lists):
        """What compose_cmp and compose_ffo share: the checked float32 [total_frames][dim] tensors as a pointer table and
        their dims, the window tables, the output columns before any msd column: (n, data, dims, windows, columns)."""
        n = len(tensors)
        checked = [self._f32(where, "streams[%d][0]" % s, t, self.total_frames, None) for s, t in enumerate(tensors)]
        data = (C.c_void_p * n)(*[p for p, _ in checked])
        dims = (C.c_int * n)(*[d for _, d in checked])
        return n, data, dims, _window_tables(window_lists), sum(d * len(w) for (_, d), w in zip(checked, window_lists))

    def compose_cmp(self, streams):
        """streams: list of (float32 cuda tensor [total_frames][dim], list of window coefficient lists).
        Returns float32 [total_frames][sum n_windows * dim] (window.pl + merge of the recipe's cmp stage)."""
        n, data, dims, (nwin, wptrs, sptrs, keep), cols = self._compose_streams(
            "compose_cmp", [t for t, _ in streams], [wins for _, wins in streams])
        out = self._new(self.total_frames, cols, dtype=torch.float32)
        _check(load_library().WorldMi355ComposeCmp(self.handle, n, data, dims, nwin, wptrs, sptrs, _ptr(out)), "ComposeCmp")
        return out

    def interpolate_gaps(self, x, ignore_value=-1e10):
        """data/scripts/interpolate.pl per utterance and column: x float32 cuda [total_frames][dim]; a value equal to
        float32(ignore_value) is a gap (-1e10 the scripts', 0 the analysis CLI's unvoiced lf0, 1e-8 Extract.py's).
        Returns (out float32 [total_frames][dim]: gaps between valid frames on the line through them, leading and
        trailing gaps at the nearest valid value, with the script's bits; voiced float32 [total_frames]: 1 where column
        0 is valid, else 0; status int32 [n_utt]: bit 1 a column without a valid value, which is zeros in out)."""
        xp, dim = self._f32("interpolate_gaps", "x", x, self.total_frames, None)
        if not np.isfinite(float(ignore_value)):
            raise ValueError(f"interpolate_gaps: ignore_value must be finite, got {ignore_value}")
        out = self._new(self.total_frames, dim, dtype=torch.float32)
        voiced = self._new(self.total_frames, dtype=torch.float32)
        status = self._new(self.n_utt, dtype=torch.int32, zero=True)
        _check(load_library().WorldMi355InterpolateGaps(self.handle, xp, dim, float(ignore_value), _ptr(out), _ptr(voiced),
                                                        _ptr(status)), "InterpolateGaps")
        return out, voiced, status

    def compose_ffo(self, streams):
        """An `ffo` row (data/Makefile.in:373-408, recipe.ffo_layout): streams is a list of (float32 cuda tensor
        [total_frames][dim], list of window coefficient lists, msd float32 cuda [total_frames] or None).  A stream with
        msd gets that value as one column in front of its windows; the windows are compose_cmp's.  Returns float32
        [total_frames][row width]."""
        if len(streams) < 1:
            raise ValueError("compose_ffo: no streams")
        if any(len(wins) < 1 or any(len(w) < 1 for w in wins) for _, wins, _ in streams):
            raise ValueError("compose_ffo: a stream needs at least one window, a window at least one coefficient")
        n, data, dims, (nwin, wptrs, sptrs, keep), cols = self._compose_streams(
            "compose_ffo", [t for t, _, _ in streams], [wins for _, wins, _ in streams])
        msds = (C.c_void_p * n)(*[self._f32("compose_ffo", "streams[%d][2]" % s, m, self.total_frames, optional=True)
                                  for s, (_, _, m) in enumerate(streams)])
        out = self._new(self.total_frames, cols + sum(m is not None for _, _, m in streams), dtype=torch.float32)
        _check(load_library().WorldMi355ComposeFfo(self.handle, n, data, dims, nwin, wptrs, sptrs, msds, _ptr(out)),
               "ComposeFfo")
        return out

    def label_features(self, feature_set, labels, out=None):
        """data/scripts/makefeature.pl for the batch (a synthesis-style one: f0_lengths are the labels' frame counts):
        the acoustic model's input rows.  labels: per utterance (lines, state_level) as recipe.read_label returns them,
        lines a list of (start, end, name, state_index) in frames with the state suffix cut from the name.  out: None, or
        a float32 cuda tensor [total_frames][>= n_features] with unit column stride (a view of a wider or an unaligned
        buffer works as it is); only its first n_features columns are written.  Returns (out float32 [total_frames]
        [n_features] with the script's bits, status int32 [n_utt]: bit 1 a value was clamped to 0 or 1 -- the script's
        "Out of range" warning --, bit 2 a state-related reserved feature met a phoneme-level file)."""
        if len(labels) != self.n_utt:
            raise ValueError(f"label_features: {len(labels)} label files for {self.n_utt} utterances")
        nf = feature_set.n_features
        line_off = np.zeros(self.n_utt + 1, dtype=np.int32)
        rows, names = [], []
        for u, (lines, _) in enumerate(labels):
            line_off[u + 1] = line_off[u] + len(lines)
            for start, end, name, state_index in lines:
                raw = name.encode("latin-1") if isinstance(name, str) else bytes(name)
                if b"\0" in raw:
                    raise ValueError("label_features: a label name holds a NUL byte")
                rows.append((start, end, state_index))
                names.append(raw)
        n = len(rows)
        cols = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(n, 3).T)
        if n and (np.abs(cols) >= 2 ** 31).any():
            raise ValueError("label_features: a start, end or state index does not fit an int")
        start, end, sidx = (np.ascontiguousarray(c, dtype=np.int32) for c in cols)
        level = np.ascontiguousarray([1 if lv else 0 for _, lv in labels], dtype=np.int32)
        if out is None:
            out = self._new(self.total_frames, nf, dtype=torch.float32)
        op, ld, width = self._f32("label_features", "out", out, self.total_frames, None, layout="rows")
        ld = min(ld, width) if width < nf else ld                    # refused by the library: ld_out < n_features
        status = self._new(self.n_utt, dtype=torch.int32, zero=True)
        name_ptrs = (C.c_char_p * max(1, n))(*names)
        ip = lambda a: a.ctypes.data_as(_ip)
        _check(load_library().WorldMi355LabelFeatures(self.handle, feature_set.handle, ip(line_off), ip(start), ip(end),
                                                      ip(sidx), name_ptrs, ip(level), op, ld, _ptr(status)),
               "LabelFeatures")
        return out[:, :nf], status

    def column_moments(self, x, width=None, ignore_value=None):
        """Per-utterance moments of the first `width` columns (all of them by default) of x, float32 cuda
        [total_frames][...]: a column view of a wider matrix is taken as it is, by its row stride.  With ignore_value, a
        value equal to float32(ignore_value) is left out of its own column.  Returns (count int64, mean float64, m2
        float64), all cuda [n_utt][width]: the kept values, their mean, and the sum of (x - mean)^2 around it in double
        (two passes); a count of 0 gives mean 0 and m2 0.  The bits do not depend on the batch around an utterance."""
        xp, ld, cols = self._f32("column_moments", "x", x, self.total_frames, None, layout="rows")
        width = cols if width is None else int(width)
        if width < 1 or width > cols:
            raise ValueError(f"column_moments: width must be in 1 .. {cols}, got {width}")
        ig = None
        if ignore_value is not None:
            if not np.isfinite(float(ignore_value)):
                raise ValueError(f"column_moments: ignore_value must be finite, got {ignore_value}")
            ig = C.byref(C.c_double(float(ignore_value)))
        count = self._new(self.n_utt, width, dtype=torch.int64)
        mean, m2 = self._new(self.n_utt, width), self._new(self.n_utt, width)
        _check(load_library().WorldMi355ColumnMoments(self.handle, xp, ld, width, ig, _ptr(count), _ptr(mean), _ptr(m2)),
               "ColumnMoments")
        return count, mean, m2

    def parameter_generation(self, streams, var_per_frame=False, edge=0, input_type=0, unvoiced_value=-1e10):
        """SPTK's mlpg per stream, as gen_param runs it (scripts/Training.pl:2755-2810): the static trajectory c that
        solves (W' P W) c = W' P mean.  streams: list of (mean, var, windows, msd_or_None).  mean: float32 cuda
        [total_frames][len(windows) * dim], laid [window 0: dim | window 1: dim | ...] as compose_cmp writes a stream --
        a tensor of its own or a column view of one matrix (a model's output, compose_cmp's result).  var: the same
        layout, [len(windows) * dim] (one row for every frame) or with var_per_frame [total_frames][...]; precisions
        with input_type=1.  windows: the coefficient lists of compose_cmp.  msd: None, or float32 cuda [total_frames]
        (a column view will do): frames with a value below 0.5 receive unvoiced_value after the solve.  edge 0 drops
        taps beyond an utterance's ends (SPTK), 1 clamps them (window.pl: the inverse of compose_cmp).
        Returns ([float32 [total_frames][dim] per stream], status int32 [n_utt]: bit 1 a column with a non-finite or
        non-positive input, bit 2 a column whose matrix is not positive definite; such columns are zeros).
        The C call takes one row stride for all streams: tensors that do not share one are packed side by side first."""
        a = self._mlpg_args("parameter_generation", streams, var_per_frame, edge, input_type, unvoiced_value)
        _check(load_library().WorldMi355ParameterGeneration(
            self.handle, a.n, a.means, a.ld_mean, a.vars, a.ld_var, a.dims, a.nwin, a.wptrs, a.sptrs, a.msds,
            C.byref(a.opt), a.out_ptrs, _ptr(a.status)), "ParameterGeneration")
        return a.outs, a.status

    def _mlpg_args(self, who, streams, var_per_frame, edge, input_type, unvoiced_value):
        """What parameter_generation and parameter_generation_gv hand to their C calls: the checked streams on one row
        stride, the window tables, the option, and fresh outputs and status."""
        import types
        n = len(streams)
        tf = self.total_frames
        for s, (mean, var, wins, msd) in enumerate(streams):
            _, cols = self._f32(who, "streams[%d][0]" % s, mean, tf, None, layout="any")
            if len(wins) < 1 or cols % len(wins) != 0:
                raise ValueError(f"{who}: streams[{s}][0] must be [total_frames][n_windows * dim]")
            self._f32(who, "streams[%d][1]" % s, var, *((tf, cols) if var_per_frame else (cols,)), layout="any")
            self._f32(who, "streams[%d][3]" % s, msd, tf, layout="any", optional=True)

        ld_mean, means, msds, keep_m = _shared_row_stride([t for t, _, _, _ in streams], [m for _, _, _, m in streams], tf)
        if var_per_frame:
            ld_var, vars_, _, keep_v = _shared_row_stride([v for _, v, _, _ in streams], [], tf)
        else:
            ld_var, vars_, keep_v = 0, [v.contiguous() for _, v, _, _ in streams], []
        vpn = C.c_void_p * n
        dims = (C.c_int * n)(*[int(t.shape[1]) // len(w) for t, _, w, _ in streams])
        nwin, wptrs, sptrs, keep = _window_tables([wins for _, _, wins, _ in streams])
        keep += [keep_m, keep_v, vars_]
        outs = [self._new(tf, int(dims[s]), dtype=torch.float32) for s in range(n)]
        status = self._new(self.n_utt, dtype=torch.int32, zero=True)
        o = _option(who, MlpgOption, "WorldMi355DefaultMlpgOption",
                    dict(edge=int(edge), var_per_frame=1 if var_per_frame else 0, input_type=int(input_type),
                         unvoiced_value=float(unvoiced_value)))
        return types.SimpleNamespace(
            n=n, means=vpn(*[_ptr(t) for t in means]), ld_mean=ld_mean, vars=vpn(*[_ptr(t) for t in vars_]), ld_var=ld_var,
            dims=dims, nwin=nwin, wptrs=wptrs, sptrs=sptrs, msds=vpn(*[_ptr(t) for t in msds]), opt=o,
            out_ptrs=vpn(*[_ptr(t) for t in outs]), outs=outs, status=status, keep=keep)

    def parameter_generation_gv(self, streams, gv_mean, gv_var, gv_mask=None, want_info=False, var_per_frame=False,
                                edge=0, input_type=0, unvoiced_value=-1e10, max_iter=None, epsilon=None, step_init=None,
                                step_inc=None, step_dec=None, hmm_weight=None, gv_weight=None, scale=None):
        """Parameter generation considering global variance (HMGenS with USEHMMGV = 1, OPTKIND = NEWTON; include/
        world_mi355.h states the definition): parameter_generation's trajectory, then up to max_iter trials of a
        diagonal Newton step on  hmm_weight w (-1/2 c'Rc + c'r) - 1/2 gv_weight (v - gv_mean)^2 / gv_var  per column, v
        the variance of the column over the utterance's GV frames.  streams, var_per_frame, edge, input_type and
        unvoiced_value as parameter_generation.  gv_mean, gv_var: per stream float32 cuda [dim] (gv.mean and gv.var over
        the stream's statics).  gv_mask: None, or uint8 cuda [total_frames]: 0 takes a frame out of the GV set (silence);
        an unvoiced frame of a stream with msd is never in it.  Options left None keep the recipe's defaults
        (WorldMi355DefaultGvOption: 50 trials, epsilon 1e-4, steps 1 / 1.2 / 0.5, weights 1, scale 1).
        Returns (outs, status) as parameter_generation -- status further 1 for a gv_mean or gv_var that is not positive,
        4 for a column with fewer than two GV frames or no variance, both returned as parameter_generation's -- and with
        want_info (outs, status, info float64 [n_utt][sum of dims][4]: f at the start, f at the end, trials, accepts)."""
        who = "parameter_generation_gv"
        a = self._mlpg_args(who, streams, var_per_frame, edge, input_type, unvoiced_value)
        if len(gv_mean) != a.n or len(gv_var) != a.n:
            raise ValueError(f"{who}: one gv_mean and one gv_var per stream")
        gvs = []
        for name, rows in (("gv_mean", gv_mean), ("gv_var", gv_var)):
            for s, t in enumerate(rows):
                self._f32(who, "%s[%d]" % (name, s), t, int(a.dims[s]), layout="any")
            gvs.append([t.contiguous() for t in rows])
        check_tensor(who, "gv_mask", gv_mask, torch.uint8, (self.total_frames,), self.device, layout="any", optional=True)
        mask = None if gv_mask is None else gv_mask.contiguous()
        num = lambda v, kind: None if v is None else kind(v)
        g = _option(who, GvOption, "WorldMi355DefaultGvOption",
                    dict(max_iter=num(max_iter, int), epsilon=num(epsilon, float), step_init=num(step_init, float),
                         step_inc=num(step_inc, float), step_dec=num(step_dec, float), hmm_weight=num(hmm_weight, float),
                         gv_weight=num(gv_weight, float), scale=num(scale, lambda v: 1 if v else 0)))
        info = self._new(self.n_utt, sum(int(d) for d in a.dims), 4, zero=True) if want_info else None
        vpn = C.c_void_p * a.n
        _check(load_library().WorldMi355ParameterGenerationGv(
            self.handle, a.n, a.means, a.ld_mean, a.vars, a.ld_var, a.dims, a.nwin, a.wptrs, a.sptrs, a.msds,
            C.byref(a.opt), vpn(*[_ptr(t) for t in gvs[0]]), vpn(*[_ptr(t) for t in gvs[1]]), _ptr(mask), C.byref(g),
            a.out_ptrs, _ptr(info), _ptr(a.status)), "ParameterGenerationGv")
        return (a.outs, a.status, info) if want_info else (a.outs, a.status)

    def trajectory_cost(self, streams, var, gv_var, msd_weight=1.0, gv_weight=1.0e-6, want_c=True, want_grad_pred=True,
                        want_grad_var=True):
        """The recipe's trajectory training criterion with its gradients (DNNDefine.trajectory_cost,
        data/scripts/DNNDefine.py:240-399), every utterance of the batch at once.  streams: list of (pred, obs, windows,
        msd): pred and obs float32 cuda [total_frames][len(windows) * dim] laid as parameter_generation's mean -- tensors
        of their own or column views of `ffo`-layout matrices (a model's output, the targets); of obs only the static
        window is read.  msd: None, or (pred, obs) voicing columns, float32 cuda [total_frames].  var: float32 cuda, ONE
        row in the `ffo` layout of these streams (per stream its voicing column's variance, when it has one, then
        len(windows) * dim); gv_var: float32 cuda, one row over the static columns of all streams in order (gv.var).
        Returns (cost float64 [n_utt][3]: trj, msd, gv -- an utterance's cost is trj + msd_weight msd + gv_weight gv;
        c: per stream float32 [total_frames][dim]; grad_pred: float32 [total_frames][width] in the `ffo` layout, the
        gradient of each utterance's cost in its own rows; grad_var: float64 [n_utt][width], per utterance; status int32
        [n_utt]: bit 1 a non-finite pred or obs or a variance that is not positive and finite, bit 2 a matrix that is
        not positive definite -- such an utterance has costs 0 and gradients 0).  An output that is not wanted is
        None and is not computed."""
        who = "trajectory_cost"
        n, tf = len(streams), self.total_frames
        for s, (pred, obs, wins, msd) in enumerate(streams):
            _, cols = self._f32(who, "streams[%d][0]" % s, pred, tf, None, layout="any")
            self._f32(who, "streams[%d][1]" % s, obs, tf, cols, layout="any")
            if len(wins) < 1 or cols % len(wins) != 0:
                raise ValueError(f"{who}: pred and obs must be float32 cuda [total_frames][n_windows * dim]")
            if msd is not None and len(msd) != 2:
                raise ValueError(f"{who}: msd is None or (pred column, obs column)")
            for k, t in enumerate(msd or ()):
                self._f32(who, "streams[%d][3][%d]" % (s, k), t, tf, layout="any")
        dims = [int(p.shape[1]) // len(w) for p, _, w, _ in streams]
        at, layout = 0, []                                             # (voicing column or None, first column, columns)
        for p, _, _, msd in streams:
            layout.append((at if msd is not None else None, at + (msd is not None), int(p.shape[1])))
            at = layout[-1][1] + layout[-1][2]
        width = at
        self._f32(who, "var", var, width, layout="any")
        self._f32(who, "gv_var", gv_var, sum(dims), layout="any")
        var, gv_var = var.contiguous(), gv_var.contiguous()
        # one row stride for pred, obs and the voicing columns: as given when they share one, else packed side by side
        rows = [t for p, o, _, _ in streams for t in (p, o)]
        cols = [t for _, _, _, msd in streams if msd is not None for t in msd]
        ld, rows, cols, keep_rows = _shared_row_stride(rows, cols, tf)
        cols = iter(cols)
        msds = [(next(cols), next(cols)) if msd is not None else None for _, _, _, msd in streams]
        vpn = C.c_void_p * n
        nwin, wptrs, sptrs, keep = _window_tables([wins for _, _, wins, _ in streams])
        keep += [keep_rows, var, gv_var]
        cost = self._new(self.n_utt, 3, zero=True)                     # a batch of zero frames launches nothing
        status = self._new(self.n_utt, dtype=torch.int32, zero=True)
        c = [self._new(tf, d, dtype=torch.float32) for d in dims] if want_c else None
        grad_pred = self._new(tf, width, dtype=torch.float32, zero=True) if want_grad_pred else None
        grad_var = self._new(self.n_utt, width, zero=True) if want_grad_var else None
        o = _option(who, TrajectoryOption, "WorldMi355DefaultTrajectoryOption",
                    dict(msd_weight=float(msd_weight), gv_weight=float(gv_weight)))
        esz, at = 4, 0
        gv_ptrs = []
        for d in dims:
            gv_ptrs.append(C.c_void_p(gv_var.data_ptr() + esz * at))
            at += d
        col = lambda t, k: None if t is None or k is None else C.c_void_p(t.data_ptr() + esz * k)
        _check(load_library().WorldMi355TrajectoryCost(
            self.handle, n, vpn(*[_ptr(t) for t in rows[0::2]]), vpn(*[_ptr(t) for t in rows[1::2]]), ld,
            vpn(*[col(var, c0) for _, c0, _ in layout]), vpn(*gv_ptrs), (C.c_int * n)(*dims),
            nwin, wptrs, sptrs,
            vpn(*[_ptr(m and m[0]) for m in msds]), vpn(*[_ptr(m and m[1]) for m in msds]),
            vpn(*[col(var, mc) for mc, _, _ in layout]), C.byref(o), _ptr(cost),
            None if c is None else vpn(*[_ptr(t) for t in c]),
            None if grad_pred is None else vpn(*[col(grad_pred, c0) for _, c0, _ in layout]),
            None if grad_pred is None else vpn(*[col(grad_pred, mc) for mc, _, _ in layout]), width, _ptr(grad_var),
            _ptr(status)), "TrajectoryCost")
        return cost, c, grad_pred, grad_var, status

    def _model_rows(self, who, name, t, width):
        """float32 [total_frames][width] passed by its row stride, a view whose strides do not fit copied first:
        (the tensor to keep alive, its pointer, its row stride)."""
        self._f32(who, name, t, self.total_frames, width, layout="any")
        if t.stride(1) != 1 or (self.total_frames > 1 and t.stride(0) < width):
            t = t.contiguous()
        return (t,) + self._f32(who, name, t, self.total_frames, width, layout="rows")

    def _model_tensor(self, who, name, t, shape, keep):
        """A parameter of the model, float32 of `shape`: the address of its detached contiguous self, kept in `keep`."""
        self._f32(who, name, t, *shape, layout="any")
        keep.append(t.detach().contiguous())
        return keep[-1].data_ptr()

    def _acoustic_model_args(self, who, model, x, spkr, obs, max_chunk_frames):
        """What the three acoustic-model calls share: (descriptor, what it points to, x's pointer, ld_x, obs' pointer or
        None, ld_obs, spkr pointer or None, (n_in, units, n_out, n_spkrs, sat))."""
        m = model.kernel_args() if hasattr(model, "kernel_args") else model
        code = lambda a: ACTIVATIONS.index(a) if isinstance(a, str) else int(a)
        keep = []
        dev = lambda t, shape, what: self._model_tensor(who, "model." + what, t, shape, keep)
        weights, biases = list(m["weights"]), list(m["biases"])
        n_layers = len(weights) - 1
        if n_layers < 0 or len(biases) != n_layers + 1:
            raise ValueError(f"{who}: weights and biases are n_layers + 1 matrices and vectors")
        for i, w in enumerate(weights):
            self._f32(who, "model.weights[%d]" % i, w, None, None, layout="any")
        n_in, n_out, n_spkrs = int(weights[0].shape[0]), int(weights[-1].shape[1]), int(m.get("n_spkrs", 1))
        units = [int(w.shape[1]) for w in weights[:-1]]
        fan = [n_in] + units
        vpn = C.c_void_p * (n_layers + 1)
        d = AcousticModelDesc()
        d.n_layers, d.n_inputs, d.n_outputs, d.n_spkrs = n_layers, n_in, n_out, n_spkrs
        d.hidden_activation, d.output_activation = code(m["hidden_activation"]), code(m["output_activation"])
        ua = (C.c_int * max(n_layers, 1))(*units)
        wa = vpn(*[dev(w, (fan[i], (units + [n_out])[i]), f"weights[{i}]") for i, w in enumerate(weights)])
        ba = vpn(*[dev(t, ((units + [n_out])[i],), f"biases[{i}]") for i, t in enumerate(biases)])
        keep += [ua, wa, ba]
        d.units, d.weights, d.biases = ua, wa, ba
        sd = m.get("spkr_weights")
        if sd is not None:
            if len(sd) != n_layers:
                raise ValueError(f"{who}: spkr_weights has one matrix per hidden layer")
            sa = (C.c_void_p * max(n_layers, 1))(*[dev(t, (n_spkrs, units[i]), f"spkr_weights[{i}]") for i, t in enumerate(sd)])
            keep.append(sa)
            d.spkr_weights = sa
        var = m.get("variances")
        if var is not None:
            d.variances = dev(var, (n_spkrs, n_out), "variances")
        d.max_chunk_frames = int(max_chunk_frames)
        x, xp, ld_x = self._model_rows(who, "x", x, n_in)
        op, ld_obs = None, 0
        if obs is not None:
            if var is None:
                raise ValueError(f"{who}: a cost needs the model's variances")
            obs, op, ld_obs = self._model_rows(who, "obs", obs, n_out)
        sp = None
        if spkr is not None:
            sp = np.ascontiguousarray(spkr, dtype=np.int32)
            if sp.shape != (self.n_utt,):
                raise ValueError(f"{who}: spkr has one index per utterance ({self.n_utt})")
            keep.append(sp)
            sp = sp.ctypes.data_as(C.c_void_p)
        keep += [x, obs]
        return d, keep, xp, ld_x, op, ld_obs, sp, (n_in, units, n_out, n_spkrs, sd is not None)

    def acoustic_model_forward(self, model, x, spkr=None, obs=None, max_chunk_frames=0):
        """The forward pass of the recipe's acoustic model (DNNDefine.inference as DNNSynthesis.py runs it) and, with
        targets, its frame-level cost (DNNDefine.cost), every utterance of the batch at once.  model: a mapping (or an
        object whose kernel_args() returns one, such as training.AcousticModel) with "weights" (n_layers + 1 float32
        cuda tensors [fan_in][fan_out], the last the output layer's), "biases" ([fan_out] each), "spkr_weights" (None,
        or n_layers tensors [n_spkrs][units]), "variances" (None, or [n_spkrs][n_outputs]), "hidden_activation",
        "output_activation" (a name of ACTIVATIONS or its code) and "n_spkrs".  x: float32 cuda
        [total_frames][n_inputs], obs: None or float32 cuda [total_frames][n_outputs]; either may be a column view of a
        wider matrix (its row stride is passed, nothing is copied).  spkr: None (n_spkrs - 1 for all), or one index per
        utterance.  Returns (out float32 [total_frames][n_outputs], cost float64 [n_utt] or None without obs, status
        int32 [n_utt]: bit 1 a non-finite x or obs, bit 2 a non-finite output or, with a cost, a variance that is not
        positive and finite -- such an utterance has zero rows and cost 0)."""
        return self._model_forward("acoustic_model_forward", model, x, spkr, obs, max_chunk_frames)

    def acoustic_model_train_forward(self, model, x, spkr=None, obs=None, keep_prob=1.0, seed=0, offset=0, want_grads=False,
                                     max_chunk_frames=0):
        """acoustic_model_forward with dropout between the hidden layers (TF 1.x tf.nn.dropout; the mask is Philox4x32-10
        of (seed, offset, layer, batch row, unit), see include/world_mi355.h) and, with want_grads, the gradients of the
        frame-level cost.  Returns (out, cost or None, status), and with want_grads (obs is then required)
        (out, cost, status, grad_out float32 [total_frames][n_outputs], grad_var float64 [n_utt][n_outputs]): the
        gradients of every utterance's own cost.  With keep_prob 1 out equals acoustic_model_forward's bit for bit."""
        drop = Dropout(float(keep_prob), int(seed) & 0xffffffffffffffff, int(offset) & 0xffffffff)
        return self._model_forward("acoustic_model_train_forward", model, x, spkr, obs, max_chunk_frames, drop, want_grads)

    def _model_forward(self, who, model, x, spkr, obs, max_chunk_frames, drop=None, want_grads=False):
        """The two forward passes: the inference call without `drop`, the training call with it."""
        d, keep, xp, ld_x, op, ld_obs, sp, (_, _, n_out, _, _) = self._acoustic_model_args(who, model, x, spkr, obs,
                                                                                          max_chunk_frames)
        if want_grads and obs is None:
            raise ValueError(f"{who}: the cost gradients need obs")
        tf = self.total_frames
        out = self._new(tf, n_out, dtype=torch.float32, zero=True)
        cost = self._new(self.n_utt, zero=True) if obs is not None else None
        status = self._new(self.n_utt, dtype=torch.int32, zero=True)
        if drop is None:
            _check(load_library().WorldMi355AcousticModelForward(self.handle, C.byref(d), xp, ld_x, sp, _ptr(out), n_out, op,
                                                                 ld_obs, _ptr(cost), _ptr(status)), "AcousticModelForward")
            return out, cost, status
        grad_out = self._new(tf, n_out, dtype=torch.float32, zero=True) if want_grads else None
        grad_var = self._new(self.n_utt, n_out, zero=True) if want_grads else None
        _check(load_library().WorldMi355AcousticModelTrainForward(
            self.handle, C.byref(d), C.byref(drop), xp, ld_x, sp, _ptr(out), n_out, op, ld_obs, _ptr(cost), _ptr(grad_out),
            n_out, _ptr(grad_var), _ptr(status)), "AcousticModelTrainForward")
        if want_grads:
            return out, cost, status, grad_out, grad_var
        return out, cost, status

    def acoustic_model_backward(self, model, x, spkr, grad_out, keep_prob=1.0, seed=0, offset=0, max_chunk_frames=0):
        """The backward pass of the training forward with the same (keep_prob, seed, offset): the gradients of
        sum(out * grad_out) with respect to the model's parameters, as a dict keyed by the reference's parameter names
        (hidden{i}.si_weights, hidden{i}.si_biases, hidden{i}.sd_weights in SAT mode, output.si_weights,
        output.si_biases; float32 cuda, shaped as the parameters), and under "status" the int32 [n_utt] mask: bit 1 a
        non-finite x or grad_out, bit 2 a non-finite output -- such an utterance adds exact zeros.  grad_out: float32 cuda
        [total_frames][n_outputs], or a column view."""
        who = "acoustic_model_backward"
        d, keep, xp, ld_x, _, _, sp, (n_in, units, n_out, n_spkrs, sat) = self._acoustic_model_args(
            who, model, x, spkr, None, max_chunk_frames)
        g, gp, ld_g = self._model_rows(who, "grad_out", grad_out, n_out)
        drop = Dropout(float(keep_prob), int(seed) & 0xffffffffffffffff, int(offset) & 0xffffffff)
        n_layers = len(units)
        fan, wid = [n_in] + units, units + [n_out]
        names = ["hidden%d" % i for i in range(n_layers)] + ["output"]
        z = lambda *shape: self._new(*shape, dtype=torch.float32, zero=True)
        gw = [z(fan[i], wid[i]) for i in range(n_layers + 1)]
        gb = [z(wid[i]) for i in range(n_layers + 1)]
        gs = [z(n_spkrs, units[i]) for i in range(n_layers)] if sat else None
        status = self._new(self.n_utt, dtype=torch.int32, zero=True)
        arr = lambda ts: (C.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])
        wa, ba = arr(gw), arr(gb)
        sa = arr(gs) if sat else None
        _check(load_library().WorldMi355AcousticModelBackward(self.handle, C.byref(d), C.byref(drop), xp, ld_x, sp, gp, ld_g,
                                                              wa, ba, sa, _ptr(status)), "AcousticModelBackward")
        res = {"status": status}
        for i, k in enumerate(names):
            res[k + ".si_weights"], res[k + ".si_biases"] = gw[i], gb[i]
            if sat and i < n_layers:
                res[k + ".sd_weights"] = gs[i]
        return res

    def split_frames(self, a):
        return [a[self.frame_offsets[u]:self.frame_offsets[u + 1]] for u in range(self.n_utt)]

    def split_out(self, y):
        return [y[self.out_offsets[u]:self.out_offsets[u + 1]] for u in range(self.n_utt)]

    def close(self):
        if self.handle:
            load_library().WorldMi355DestroyBatch(self.handle)
            self.handle = None


def mspf_finalize(sum, sumsq, n):
    """make_mspf's statistics from the sums of modulation_spectrum_stats (numpy arrays or tensors, added over all
    batches and ranks): (mean, std) with std the population standard deviation sqrt(E[m^2] - E[m]^2)."""
    mean = sum / n
    return mean, (sumsq / n - mean * mean).clip(0) ** 0.5


def pool_moments(count, mean, m2):
    """(n, mean, M2) of the union of parts given by their own: count, mean, m2 are arrays [parts][width] (numpy or
    tensors) -- column_moments' rows, or triples pooled earlier (another rank's), stacked.  Chan's merge in float64 on
    the host, in index order: n = sum n_u, mean = sum n_u m_u / n, M2 = sum M2_u + sum n_u (m_u - mean)^2.  A part with
    count 0 contributes nothing; n = 0 gives mean 0 and M2 0.  The variance of the union is M2 / n."""
    host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    cnt, mu, ss = host(count), np.asarray(host(mean), dtype=np.float64), np.asarray(host(m2), dtype=np.float64)
    if cnt.ndim != 2 or mu.shape != cnt.shape or ss.shape != cnt.shape:
        raise ValueError(f"pool_moments: count, mean and m2 must share one shape [parts][width], got {cnt.shape}, "
                         f"{mu.shape}, {ss.shape}")
    if (cnt < 0).any() or (cnt != np.floor(cnt)).any():
        raise ValueError("pool_moments: counts must be whole numbers >= 0")
    nf = cnt.astype(np.float64)
    width = cnt.shape[1]
    n, s1, tot = np.zeros(width, dtype=np.int64), np.zeros(width), np.zeros(width)
    for u in range(cnt.shape[0]):
        n += cnt[u].astype(np.int64)
        s1 += nf[u] * np.where(nf[u] > 0, mu[u], 0.0)
    pooled = np.where(n > 0, s1 / np.maximum(n, 1), 0.0)
    for u in range(cnt.shape[0]):
        d = np.where(nf[u] > 0, mu[u] - pooled, 0.0)
        tot += np.where(nf[u] > 0, ss[u], 0.0) + nf[u] * (d * d)
    return n, pooled, tot


def mspf_segment_frames() -> int:
    """The output frames one wave of the modulation-spectrum postfilter handles (csrc/mspf.hip)."""
    return int(load_library().WorldMi355MspfSegmentFrames())


def write_files(items, threads=16):
    """items: [(path, numpy array)] -- every array written raw to its path by native threads in ONE library call
    (WorldMi355WriteFiles: the interpreter lock is released for its duration).  The arrays must be C-contiguous
    (ValueError) and stay alive until the call returns (they do: it is synchronous).  Host only."""
    n = len(items)
    if n == 0:
        return
    paths = (C.c_char_p * n)(*[os.fsencode(str(p)) for p, _ in items])
    ptrs = (C.c_void_p * n)()
    sizes = (C.c_size_t * n)()
    for k, (_, a) in enumerate(items):
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError(f"write_files: the array for {items[k][0]} is not C-contiguous")
        ptrs[k] = a.ctypes.data
        sizes[k] = a.nbytes
    _check(load_library().WorldMi355WriteFiles(n, paths, ptrs, sizes, int(threads)), "WriteFiles")


def htk_header(n_frames, sampling_rate, frame_shift_samples, bytes_per_frame, htk_type=9):
    """12-byte HTK header of the recipe's cmp files (addhtkheader.pl:60-75)."""
    buf = (C.c_ubyte * 12)()
    load_library().WorldMi355HtkHeader(int(n_frames), int(sampling_rate), int(frame_shift_samples), int(bytes_per_frame),
                                       int(htk_type), buf)
    return bytes(buf)

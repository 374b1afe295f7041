"""The argument checks of the ctypes host layer, without a device: every public WorldBatch method that takes a tensor, and
Context.optimizer_step, on a batch made by hand whose device is the CPU.  A valid call gets as far as the library, which
refuses the NULL batch (RuntimeError); every bad tensor is refused before it, by check_tensor (ValueError)."""
import ast
import copy
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from caller_stream_table import ASYNC, NO_DEVICE_WORK, SYNCHRONISES

torch = pytest.importorskip("torch")

NU, TS, TF, TO, FFT, BINS = 2, 2000, 27, 2000, 1024, 513
F64, F32, I16, I32, U8 = torch.float64, torch.float32, torch.int16, torch.int32, torch.uint8
OTHER = {F64: F32, F32: F64, I16: I32, I32: I16, U8: torch.int8}
NO_TENSORS = {"set_f0_estimator", "split_frames", "split_out", "close"}
WIN = [[1.0]]


@pytest.fixture(scope="module")
def W(pkg):
    pkg.load_library()
    return pkg.world


@pytest.fixture(scope="module")
def batch(W):
    b = W.WorldBatch.__new__(W.WorldBatch)
    b.handle, b.ctx, b.params = None, None, W.default_params(16000, 5.0)
    b.n_utt, b.total_samples, b.total_frames, b.total_out, b.fft_size, b.bins = NU, TS, TF, TO, FFT, BINS
    b.sample_offsets, b.frame_offsets = np.array([0, 800, TS]), np.array([0, 11, TF])
    b.out_offsets = np.array([0, 800, TO])
    b.device = torch.device("cpu")
    return b


def z(dtype, *shape):
    return torch.zeros(*shape, dtype=dtype)


def model():
    return {"weights": [z(F32, 4, 3), z(F32, 3, 2)], "biases": [z(F32, 3), z(F32, 2)], "spkr_weights": [z(F32, 1, 3)],
            "variances": z(F32, 1, 2), "n_spkrs": 1, "hidden_activation": "sigmoid", "output_activation": "linear"}


def n_bands():
    import importlib
    return importlib.import_module("hts-train-world_amd").load_library().WorldMi355GetNumberOfAperiodicities(16000)


def analysis_out():
    return [z(F64, TF), z(F64, TF), z(F64, TF, BINS), z(F64, TF, BINS)]


def xtf0(**more):
    return dict(x=z(F64, TS), t=z(F64, TF), f0=z(F64, TF), **more)


def f0_sp_ap(**more):
    return dict(f0=z(F64, TF), sp=z(F64, TF, BINS), ap=z(F64, TF, BINS), **more)


def mlpg_streams():
    return [[z(F32, TF, 2), z(F32, 2), WIN, z(F32, TF)]]


# A tensor argument of a row below: its path in the keyword arguments, the dimensions that are free (or tied to another
# argument, so that the refusal would name that one), and the layout the call takes: "contiguous", "rows" or "any".
def arg(*path, free=(), layout="contiguous"):
    return path, free, layout


MODEL_ARGS = [arg("model", "weights", 0, free=(0, 1), layout="any"), arg("model", "weights", 1, free=(0, 1), layout="any"),
              arg("model", "biases", 0, layout="any"), arg("model", "biases", 1, layout="any"),
              arg("model", "spkr_weights", 0, layout="any"), arg("model", "variances", layout="any"),
              arg("x", layout="any")]
MLPG_ARGS = [arg("streams", 0, 0, free=(1,), layout="any"), arg("streams", 0, 1, layout="any"),
             arg("streams", 0, 3, layout="any")]

# method -> (its valid keyword arguments at the sizes above, its tensor arguments)
TABLE = {
    "dio": (lambda: dict(x=z(F64, TS)), [arg("x")]),
    "harvest": (lambda: dict(x=z(F64, TS)), [arg("x")]),
    "stonemask": (xtf0, [arg("x"), arg("t"), arg("f0")]),
    "cheaptrick": (lambda: xtf0(out=z(F64, TF, BINS)), [arg("x"), arg("t"), arg("f0"), arg("out")]),
    "d4c": (lambda: xtf0(out=z(F64, TF, BINS)), [arg("x"), arg("t"), arg("f0"), arg("out")]),
    "samples_from_pcm16": (lambda: dict(pcm=z(I16, TS), out=z(F64, TS)), [arg("pcm"), arg("out")]),
    "samples_to_pcm16": (lambda: dict(y=z(F64, TO), out=z(I16, TO)), [arg("y"), arg("out")]),
    "analyze": (lambda: dict(x=z(F64, TS), out=analysis_out()), [arg("x")] + [arg("out", k) for k in range(4)]),
    "analyze_synthesize": (lambda: dict(x=z(F64, TS), out=analysis_out(), y=z(F64, TO)),
                           [arg("x"), arg("y")] + [arg("out", k) for k in range(4)]),
    "synthesize": (lambda: f0_sp_ap(out=z(F64, TO)), [arg("f0"), arg("sp"), arg("ap"), arg("out")]),
    "vibrato": (lambda: dict(lf0=z(F32, TF), segments=[[(0, 5, 220.0)], []]), [arg("lf0")]),
    "utterance_status": (lambda: f0_sp_ap(x=z(F64, TS)), [arg("x"), arg("f0"), arg("sp"), arg("ap")]),
    "code_spectral_envelope": (lambda: dict(sp=z(F64, TF, BINS), number_of_dimensions=10), [arg("sp")]),
    "decode_spectral_envelope": (lambda: dict(coded=z(F64, TF, 10)), [arg("coded", free=(1,))]),
    "code_aperiodicity": (lambda: dict(ap=z(F64, TF, BINS)), [arg("ap")]),
    "decode_aperiodicity": (lambda: dict(coded=z(F64, TF, n_bands())), [arg("coded")]),
    "recipe_features": (f0_sp_ap, [arg("f0"), arg("sp"), arg("ap")]),
    "recipe_decode": (lambda: dict(lf0=z(F32, TF), mgc=z(F32, TF, 50), bap=z(F32, TF, 25)),
                      [arg("lf0"), arg("mgc", free=(1,)), arg("bap", free=(1,))]),
    "mel_cepstrum": (lambda: dict(spectrum=z(F64, TF, BINS)), [arg("spectrum")]),
    "mel_cepstrum_of_frames": (lambda: dict(frames=z(F64, TF, FFT)), [arg("frames")]),
    "mel_cepstrum_of_waveform": (lambda: dict(x=z(F64, TS), window=np.ones(400), frame_length=400, frame_shift=80),
                                 [arg("x")]),
    "mlsa_excitation": (lambda: dict(pitch=z(F32, TF), lowpass=[1.0], highpass=[1.0]), [arg("pitch")]),
    "mlsa_filter": (lambda: dict(e=z(F64, TO), mc=z(F32, TF, 26)), [arg("e"), arg("mc", free=(1,))]),
    "mlsa_synthesis": (lambda: dict(pitch=z(F32, TF), mc=z(F32, TF, 26), lowpass=[1.0], highpass=[1.0]),
                       [arg("pitch"), arg("mc", free=(1,))]),
    "dtw_align": (lambda: dict(a=z(F32, TF, 5), b=z(F32, 9, 5), b_lengths=[4, 5]),
                  [arg("a", free=(1,)), arg("b", free=(1,))]),
    "feature_distortion": (lambda: dict(groups=[[z(F32, TF, 5), z(F32, 9, 5), 0, 5, 0]], b_lengths=[4, 5],
                                        path=z(I32, TF + 9 - NU, 2), path_len=z(I32, NU), b_mask=z(U8, 9)),
                           [arg("groups", 0, 0, free=(1,)), arg("groups", 0, 1, free=(1,)), arg("path"), arg("path_len"),
                            arg("b_mask")]),
    "spectrum_from_mel_cepstrum": (lambda: dict(mc=z(F64, TF, 26)), [arg("mc", free=(1,))]),
    "convert_mel_generalized_cepstrum": (lambda: dict(mc=z(F64, TF, 26), alpha=0.42, gamma=-0.5, out_order=30,
                                                      out_alpha=0.0, out_gamma=1.0), [arg("mc", free=(1,))]),
    "modify_features": (lambda: dict(f0=z(F64, TF), sp=z(F64, TF, BINS), f0_scale=1.2, formant_ratio=[0.8, 1.25],
                                     out=[z(F64, TF), z(F64, TF, BINS)]),
                        [arg("f0"), arg("sp"), arg("out", 0), arg("out", 1)]),
    "postfilter_mel_cepstrum": (lambda: dict(mc=z(F64, TF, 26)), [arg("mc", free=(1,))]),
    "utterance_means": (lambda: dict(x=z(F64, TF, 4)), [arg("x", free=(1,))]),
    "modulation_spectrum_stats": (lambda: dict(x=z(F64, TF, 4), mean=z(F64, NU, 4)), [arg("x", free=(1,)), arg("mean")]),
    "postfilter_modulation_spectrum": (lambda: dict(x=z(F64, TF, 4), mean_gen=np.zeros((4, 33)), std_gen=np.ones((4, 33)),
                                                    mean_nat=np.zeros((4, 33)), std_nat=z(F64, 4, 33) + 1),
                                       [arg("x", free=(1,))]),
    "compose_cmp": (lambda: dict(streams=[[z(F32, TF, 3), WIN]]), [arg("streams", 0, 0, free=(1,))]),
    "interpolate_gaps": (lambda: dict(x=z(F32, TF, 3)), [arg("x", free=(1,))]),
    "compose_ffo": (lambda: dict(streams=[[z(F32, TF, 3), WIN, z(F32, TF)]]),
                    [arg("streams", 0, 0, free=(1,)), arg("streams", 0, 2)]),
    "label_features": (lambda: dict(feature_set=types.SimpleNamespace(n_features=3, handle=None),
                                    labels=[([(0, 11, "a", 2)], True), ([(0, 16, "b", 2)], True)], out=z(F32, TF, 3)),
                       [arg("out", free=(1,), layout="rows")]),
    "column_moments": (lambda: dict(x=z(F32, TF, 3)), [arg("x", free=(1,), layout="rows")]),
    "parameter_generation": (lambda: dict(streams=mlpg_streams()), MLPG_ARGS),
    "parameter_generation_gv": (lambda: dict(streams=mlpg_streams(), gv_mean=[z(F32, 2)], gv_var=[z(F32, 2)],
                                             gv_mask=z(U8, TF)),
                                MLPG_ARGS + [arg("gv_mean", 0, layout="any"), arg("gv_var", 0, layout="any"),
                                             arg("gv_mask", layout="any")]),
    "trajectory_cost": (lambda: dict(streams=[[z(F32, TF, 2), z(F32, TF, 2), WIN, [z(F32, TF), z(F32, TF)]]],
                                     var=z(F32, 3), gv_var=z(F32, 2)),
                        [arg("streams", 0, 0, free=(1,), layout="any"), arg("streams", 0, 1, layout="any"),
                         arg("streams", 0, 3, 0, layout="any"), arg("streams", 0, 3, 1, layout="any"),
                         arg("var", layout="any"), arg("gv_var", layout="any")]),
    "acoustic_model_forward": (lambda: dict(model=model(), x=z(F32, TF, 4), obs=z(F32, TF, 2)),
                               MODEL_ARGS + [arg("obs", layout="any")]),
    "acoustic_model_train_forward": (lambda: dict(model=model(), x=z(F32, TF, 4), obs=z(F32, TF, 2), want_grads=True),
                                     MODEL_ARGS + [arg("obs", layout="any")]),
    "acoustic_model_backward": (lambda: dict(model=model(), x=z(F32, TF, 4), spkr=[0, 0], grad_out=z(F32, TF, 2)),
                                MODEL_ARGS + [arg("grad_out", layout="any")]),
}
OPTIMIZER = (lambda W: dict(option=W.default_optimizer_option("adam"), params=[z(F32, 3, 2)], grads=[z(F32, 3, 2)],
                            rates=[0.1], slot0=[z(F32, 3, 2)], slot1=[z(F32, 6)], want_status=True),
             [arg("params", 0, free=(0, 1)), arg("grads", 0), arg("slot0", 0), arg("slot1", 0)])


def test_the_table_covers_every_public_method(W):
    public = {n for n in vars(W.WorldBatch) if not n.startswith("_")}
    assert set(TABLE) | NO_TENSORS == public and not set(TABLE) & NO_TENSORS


def test_the_caller_stream_tables_cover_every_public_method(W):
    """tests/test_gpu_caller_stream.py's tables: every public name is asynchronous, waits inside, or queues nothing."""
    a, s, n = set(ASYNC) - {"optimizer_step"}, set(SYNCHRONISES), NO_DEVICE_WORK     # optimizer_step is the context's
    assert not a & s and not a & n and not s & n and len(a) == len(ASYNC) - 1
    assert a | s | n == {name for name in vars(W.WorldBatch) if not name.startswith("_")}


def rendered(path):
    return str(path[0]) + "".join("[%d]" % k if isinstance(k, int) else "." + k for k in path[1:])


def get(kwargs, path):
    for k in path:
        kwargs = kwargs[k]
    return kwargs


def put(kwargs, path, value):
    kwargs = copy.copy(kwargs)                              # the containers on the way are copied, the tensors shared
    at = kwargs
    for k in path[:-1]:
        at[k] = copy.copy(at[k])
        at = at[k]
    at[path[-1]] = value
    return kwargs


def bad_versions(t, free, layout):
    """(what is wrong, the tensor) for every refusal the check owes this argument."""
    yield "the other width", t.to(OTHER[t.dtype])
    for d, what in ((0, "one row too many"), (1, "one column too many")):
        if d < t.dim() and d not in free:
            shape = list(t.shape)
            shape[d] += 1
            yield what, z(t.dtype, *shape)
    if layout == "contiguous":
        yield "a strided view", z(t.dtype, *([2 * t.shape[0]] + list(t.shape[1:])))[::2]
        if t.dim() == 2 and min(t.shape) > 1:
            yield "a transposed view", z(t.dtype, t.shape[1], t.shape[0]).t()
    if layout == "rows" and t.shape[1] > 1:
        yield "a transposed view", z(t.dtype, t.shape[1], t.shape[0]).t()
        yield "rows that overlap", z(t.dtype, t.shape[0] * t.shape[1]).as_strided(tuple(t.shape), (1, 1))
    yield "a list", t.tolist()
    yield "another device", torch.empty(tuple(t.shape), dtype=t.dtype, device="meta")


def refusals(call, method, kwargs, args):
    with pytest.raises(RuntimeError, match="bad argument"):     # valid: through every check, refused by the library
        call(**kwargs)
    n = 0
    for path, free, layout in args:
        t = get(kwargs, path)
        assert torch.is_tensor(t), (method, path)
        for what, bad in bad_versions(t, free, layout):
            with pytest.raises(ValueError) as e:
                call(**put(kwargs, path, bad))
            assert method + ":" in str(e.value) and rendered(path) in str(e.value), (method, path, what, str(e.value))
            n += 1
    return n


@pytest.mark.parametrize("method", sorted(TABLE))
def test_bad_tensors_are_refused_before_the_library(batch, method):
    make, args = TABLE[method]
    assert refusals(getattr(batch, method), method, make(), args) >= 4 * len(args)


def test_optimizer_step_refuses_bad_tensors(W):
    ctx = W.Context.__new__(W.Context)
    ctx.handle, ctx.device = None, "cpu"
    make, args = OPTIMIZER
    assert refusals(ctx.optimizer_step, "optimizer_step", make(W), args) >= 16


def test_optional_tensors_and_fix_ups_still_pass(batch):
    """None where a call takes it, and the layouts a call repairs itself, reach the library like the plain call."""
    cases = [(batch.utterance_status, dict(x=z(F64, TS))), (batch.utterance_status, dict()),
             (batch.analyze, dict(x=z(F64, TS))), (batch.modulation_spectrum_stats, dict(x=z(F64, TF, 4))),
             (batch.modify_features, dict(f0=z(F64, TF), f0_scale=1.2)),
             (batch.modify_features, dict(sp=z(F64, TF, BINS), formant_ratio=0.8)),
             (batch.compose_ffo, dict(streams=[[z(F32, TF, 3), WIN, None]])),
             (batch.label_features, dict(feature_set=types.SimpleNamespace(n_features=3, handle=None),
                                         labels=[([(0, 11, "a", 2)], True), ([(0, 16, "b", 2)], True)],
                                         out=z(F32, TF, 48)[:, 5:9])),
             (batch.column_moments, dict(x=z(F32, TF, 9)[:, 2:5], width=2)),
             (batch.parameter_generation, dict(streams=[[z(F32, TF, 8)[:, 1:3], z(F32, 4)[::2], WIN, z(F32, TF, 8)[:, 0]]])),
             (batch.parameter_generation_gv, dict(streams=mlpg_streams(), gv_mean=[z(F32, 4)[::2]], gv_var=[z(F32, 4)[::2]],
                                                  gv_mask=z(U8, 2 * TF)[::2])),
             (batch.trajectory_cost, dict(streams=[[z(F32, 2, TF).t(), z(F32, TF, 2), WIN, None]], var=z(F32, 4)[::2],
                                          gv_var=z(F32, 2))),
             (batch.acoustic_model_forward, dict(model=model(), x=z(F32, 4, TF).t(), obs=z(F32, TF, 6)[:, 1:3])),
             (batch.acoustic_model_forward, dict(model=dict(model(), weights=[z(F32, 3, 4).t(), z(F32, 3, 2)]),
                                                 x=z(F32, TF, 1).expand(TF, 4)))]
    for call, kwargs in cases:
        with pytest.raises(RuntimeError, match="bad argument"):
            call(**kwargs)


@pytest.mark.parametrize("width", [1, 3])
@pytest.mark.parametrize("n_rows", [1, 2])
def test_row_stride_rule(W, width, n_rows):
    wide = z(F32, n_rows, width + 4)
    cases = [(z(F32, n_rows, width), width), (wide[:, 2:2 + width], width + 4 if n_rows > 1 else width)]
    if n_rows == 1:                                         # one row reports any stride: here one below its width
        cases.append((z(F32, 8).as_strided((1, width), (width - 1, 1)), width))
    for t, want in cases:
        assert W.row_stride(t) == want
        ptr, ld, cols = W.check_tensor("m", "a", t, F32, (n_rows, None), torch.device("cpu"), layout="rows")
        assert (ptr.value, ld, cols) == (t.data_ptr(), want, width)
    if width > 1 and n_rows > 1:                            # a transposed view: no unit column stride
        with pytest.raises(ValueError, match="m: a must be"):
            W.check_tensor("m", "a", z(F32, width, n_rows).t(), F32, (n_rows, None), torch.device("cpu"), layout="rows")
    with pytest.raises(ValueError, match="m: a must be"):
        W.check_tensor("m", "a", None, F32, (1,), torch.device("cpu"))
    assert W.check_tensor("m", "a", None, F32, (1,), torch.device("cpu"), optional=True) is None


STRUCTS = [("McepOption", "WorldMi355DefaultMcepOption", (), dict(order=8, dd=0.5)),
           ("MlsaOption", "WorldMi355DefaultMlsaOption", (), dict(frame_shift=80, alpha=0.5)),
           ("Mgc2spOption", "WorldMi355DefaultMgc2spOption", (), dict(gamma=-0.5)),
           ("McpfOption", "WorldMi355DefaultMcpfOption", (), dict(beta=1.25, length=512)),
           ("MspfOption", "WorldMi355DefaultMspfOption", (), dict(emphasis=0.5)),
           ("MlpgOption", "WorldMi355DefaultMlpgOption", (), dict(edge=1)),
           ("GvOption", "WorldMi355DefaultGvOption", (), dict(max_iter=7, step_dec=0.25)),
           ("TrajectoryOption", "WorldMi355DefaultTrajectoryOption", (), dict(msd_weight=2.0)),
           ("DistortionOption", "WorldMi355DefaultDistortionOption", (), dict(voiced_above=0.5)),
           ("OptimizerOption", "WorldMi355DefaultOptimizerOption", (4,), dict(beta1=0.5))]


def fields(o):
    return {name: (list(getattr(o, name)) if hasattr(getattr(o, name), "__len__") else getattr(o, name))
            for name, _ in o._fields_}


@pytest.mark.parametrize("struct,default,args,over", STRUCTS, ids=[s[0] for s in STRUCTS])
def test_option_builder(W, struct, default, args, over):
    Struct = getattr(W, struct)
    base = Struct()
    getattr(W.load_library(), default)(*args, C.byref(base))
    want = dict(fields(base), **over)
    assert any(fields(base)[k] != v for k, v in over.items())
    assert fields(W._option("m", Struct, default, over, None, *args)) == want
    keep = dict(over, **{name: None for name, _ in Struct._fields_ if name not in over})
    assert fields(W._option("m", Struct, default, keep, None, *args)) == want              # None keeps the default
    with pytest.raises(TypeError, match="m: unknown option 'no_such_field'"):
        W._option("m", Struct, default, dict(over, no_such_field=1), None, *args)
    with pytest.raises(TypeError, match="unknown option"):                                 # a field, but not allowed
        W._option("m", Struct, default, over, (), *args)


def test_options_through_the_methods(W, batch):
    with pytest.raises(TypeError, match="mel_cepstrum: unknown option 'order2'"):
        batch.mel_cepstrum(z(F64, TF, BINS), order2=3)
    with pytest.raises(TypeError, match="mel_cepstrum_of_frames: unknown option"):
        batch.mel_cepstrum_of_frames(z(F64, TF, FFT), gamma=0.0)
    with pytest.raises(TypeError, match="unknown option 'beta3'"):
        W.default_optimizer_option("adam", beta3=0.5)
    adam = W.default_optimizer_option("adam", epsilon=0.5)
    assert adam.rule == 4 and adam.epsilon == 0.5 and adam.beta1_power == adam.beta1 > 0


def test_no_assert_statements(pkg):
    for name in ("world.py", "sharding.py"):
        tree = ast.parse(open(os.path.join(os.path.dirname(pkg.__file__), name)).read())
        assert not [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Assert)], name


def test_sharding_refusals_are_value_errors(pkg):
    with pytest.raises(ValueError, match="lpt_shards"):
        pkg.sharding.lpt_shards([3, 2, 1], 2, handicap=[1.0])
    with pytest.raises(ValueError, match="lpt_shards"):
        pkg.sharding.lpt_shards([3, 2, 1], 2, handicap=[1.0, 0.5])
    assert pkg.sharding.lpt_shards([3, 2, 1], 2, handicap=[1.5, 1.0]) == [[1], [0, 2]]


def test_world_imports_without_torch(pkg):
    root = os.path.dirname(os.path.dirname(os.path.abspath(pkg.__file__)))
    code = ("import importlib, sys; W = importlib.import_module('hts-train-world_amd.world'); "
            "assert 'torch' not in sys.modules; W.load_library(); W.default_params(16000); "
            "assert 'torch' not in sys.modules; W.torch.float64; assert 'torch' in sys.modules")
    subprocess.run([sys.executable, "-c", code], cwd=root, check=True)

"""The argument checks of the host layer on a real device: a tensor of another device, dtype or length is refused on
the host (ValueError), nothing is launched, and the batch works afterwards as before.  The refused tensors are too long,
never too short: not even a missing check could read out of bounds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS, LENGTHS = 16000, [800, 1200]


def waveform():
    n = np.arange(sum(LENGTHS))
    rng = np.random.default_rng(5)
    return 0.4 * np.sin(2 * np.pi * 140.0 * n / FS) + 0.2 * np.sin(2 * np.pi * 280.0 * n / FS) + 0.01 * rng.standard_normal(len(n))


def test_refusals_leave_the_batch_as_it_was(gpu):
    torch, W, ctx = gpu
    b = W.WorldBatch(ctx, W.default_params(FS, 5.0), x_lengths=LENGTHS)
    try:
        assert np.diff(b.frame_offsets).tolist() == [11, 16] and b.fft_size == 1024 and b.device.type == "cuda"
        x = torch.from_numpy(waveform()).cuda()
        first = b.analyze(x)
        t, f0, sp, ap = first
        assert all(v.device == b.device for v in first) and bool(torch.isfinite(sp).all()) and float(sp.max()) > 0
        calls = [("analyze", b.analyze, {"x": x}), ("synthesize", b.synthesize, {"f0": f0, "sp": sp, "ap": ap}),
                 ("recipe_features", b.recipe_features, {"f0": f0, "sp": sp, "ap": ap})]
        for method, call, kwargs in calls:
            call(**kwargs)
            for name, v in kwargs.items():                                  # a CPU tensor in place of each input
                with pytest.raises(ValueError, match="%s: %s must be" % (method, name)):
                    call(**dict(kwargs, **{name: v.cpu()}))
        with pytest.raises(ValueError, match="analyze: x must be"):
            b.analyze(x.float())
        for k in range(4):                                                  # one output a row too long
            out = [torch.empty_like(v) for v in first]
            out[k] = torch.empty((out[k].shape[0] + 1,) + tuple(out[k].shape[1:]), dtype=out[k].dtype, device="cuda")
            with pytest.raises(ValueError, match=r"analyze: out\[%d\] must be" % k):
                b.analyze(x, out=tuple(out))
        with pytest.raises(ValueError, match="analyze: x must be"):
            b.analyze(torch.cat([x, x[:1]]))
        ctx.synchronize()
        again = b.analyze(x, out=tuple(torch.empty_like(v) for v in first))
        ctx.synchronize()
        for v, w in zip(first, again):
            assert torch.equal(v.view(torch.int64), w.view(torch.int64))
    finally:
        b.close()


def test_outputs_and_checks_follow_the_contexts_device(gpu):
    torch, W, _ = gpu
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU: a context on another device than torch's current one cannot be made")
    assert torch.cuda.current_device() == 0
    ctx = W.Context(device=1)
    b = W.WorldBatch(ctx, W.default_params(FS, 5.0), x_lengths=LENGTHS)
    try:
        x = torch.from_numpy(waveform())
        with pytest.raises(ValueError, match="dio: x must be"):
            b.dio(x.to("cuda:0"))
        t, f0 = b.dio(x.to("cuda:1"))
        ctx.synchronize()
        assert t.device == f0.device == torch.device("cuda", 1) == b.device and torch.cuda.current_device() == 0
    finally:
        b.close()
        ctx.close()

"""WorldBatch.convert_mel_generalized_cepstrum on a caller's own non-blocking stream: the parity case
(24, .42, -1/3 -> 65, 0, -1/3) of tests/test_gpu_mgc2mgc.py under the procedure of tests/test_gpu_caller_stream.py (its
Env: a warm-up on stale rows, then a delay of about 50 ms, the copy of the fresh rows and the call at once, the result
read through the caller's stream alone).  The launch is asynchronous: the delay must still be running when the call
returns.  A launch on another stream than the caller's reads the stale rows and misses the reference."""
import numpy as np
import pytest

import test_gpu_caller_stream as S
import test_gpu_mgc2mgc as T

pytestmark = pytest.mark.gpu
NAME = "convert_mel_generalized_cepstrum"


@pytest.fixture(scope="module")
def env(gpu):
    torch, W, ctx0 = gpu
    e = S.Env(torch, W, ctx0)
    yield e
    with torch.cuda.stream(e.U):
        e.ctx.close()
    torch.cuda.synchronize()


def test_parity_on_a_callers_stream(env):
    torch, W = env.torch, env.W
    fx = np.load(T.gen.PATH)
    key = T.gen.PARITY_STREAM
    opt, _ = T.gen.OPTIONS[key]
    m1, a1, g1, n, u, m2, a2, g2, N, U = opt
    assert (m1, m2, a2) == (24, 65, 0.0)
    rows = fx[key + "/in"]
    with torch.cuda.stream(env.U):
        lengths = T.uneven(len(rows))
        b = W.WorldBatch(env.ctx, W.default_params(48000, 5.0), f0_lengths=lengths)
        with torch.cuda.stream(env.default):
            twin = W.WorldBatch(env.ctx0, W.default_params(48000, 5.0), f0_lengths=lengths)
        try:
            mc = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
            args = (mc, a1, g1, m2, a2, g2)
            out, st = env.pending_call(NAME, getattr(b, NAME), getattr(twin, NAME), args, {}, args)
            out, st = out.cpu().numpy(), st.cpu().numpy()
        finally:
            b.close()
            twin.close()
    env.U.synchronize()
    assert env.pending[NAME] == [True], "the call returned after the %.0f ms delay queued ahead of it" % env.delay_ms
    assert (st == 0).all()
    T.check_rows(out, fx[key + "/out"], fx[key + "/sens"], key + " on a caller's stream")
    assert not env.mismatches, "other bits on a caller's stream than on the stream-0 context"

"""WorldBatch.parameter_generation_gv on a caller's own non-blocking stream, made as tests/test_gpu_caller_stream.py
makes its calls (its Env): a warm-up on stale inputs, the stream synchronised, then a delay of about 50 ms, the copy of
the fresh inputs over the stale ones and the call at once.  The call must return while the delay still runs, read the
fresh inputs, and give the bits of the same call on the session's stream-0 context -- which are held to the reference."""
import numpy as np
import pytest

import gv_cases as K
import gv_reference as G
import mlpg_reference as M
import test_gpu_caller_stream as CS
import test_gpu_mlpg_gv as T_GV

pytestmark = pytest.mark.gpu

LENGTHS = (3, 33, 200)


def test_parameter_generation_gv_on_the_callers_stream(gpu):
    torch, W, ctx0 = gpu
    env = CS.Env(torch, W, ctx0)
    try:
        with torch.cuda.stream(env.U):
            data, voiced = K.inputs(LENGTHS, False)
            streams, gm, gv = T_GV.device_streams(torch, data, voiced)
            mask = torch.from_numpy(K.holes(LENGTHS)).cuda()
            b = CS.DelayedBatch(env, env.ctx, W.default_params(48000, 5.0), f0_lengths=list(LENGTHS))
            env.U.synchronize()
            kwargs = dict(gv_mask=mask, want_info=True, unvoiced_value=T_GV.UNVOICED, max_iter=5, epsilon=0.0)
            args = (streams, gm, gv)
            outs, status, info = env.pending_call("parameter_generation_gv", b._b.parameter_generation_gv,
                                                  b._twin.parameter_generation_gv, args, kwargs, args)
            assert env.pending["parameter_generation_gv"] == [True], "the call waited for the stream"
            assert env.mismatches == [], "other bits than on the stream-0 context"
            c0, _ = b._b.parameter_generation([(m, v, w, None) for m, v, w, _ in streams])
            c0s = [o.cpu().numpy() for o in c0]
            outs, status = [o.cpu().numpy() for o in outs], status.cpu().numpy()
            env.U.synchronize()
            b.close()
        opts = dict(max_iter=5, epsilon=0.0)
        r64 = K.reference(LENGTHS, data, voiced, c0s, K.holes(LENGTHS), 0, np.float64, **opts)
        rld = K.reference(LENGTHS, data, voiced, c0s, K.holes(LENGTHS), 0, np.longdouble, **opts)
        T_GV.compare(LENGTHS, voiced, outs, status, c0s, r64, rld, "on the caller's stream")
    finally:
        with torch.cuda.stream(env.U):
            env.ctx.close()
        torch.cuda.synchronize()

"""WorldBatch.dtw_align and feature_distortion on a caller's own non-blocking stream, made as
tests/test_gpu_caller_stream.py makes its calls (its Env): a warm-up on stale inputs, the stream synchronised, then a delay
of about 50 ms, the copy of the fresh inputs over the stale ones and the call at once.  Each call must return while the
delay still runs, read the fresh inputs, and give the bits of the same call on the session's stream-0 context -- which
are held to the reference."""
import numpy as np
import pytest

import dtw_cases as K
import test_gpu_caller_stream as CS

pytestmark = pytest.mark.gpu

PAIRS = ((65, 130), (7, 1), (129, 64))


def test_dtw_align_and_feature_distortion_on_the_callers_stream(gpu):
    torch, W, ctx0 = gpu
    env = CS.Env(torch, W, ctx0)
    try:
        with torch.cuda.stream(env.U):
            a, b = K.batch_rows(PAIRS, **K.RAGGED_SHAPE)
            da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
            b_len = [tb for _, tb in PAIRS]
            batch = CS.DelayedBatch(env, env.ctx, W.default_params(48000, 5.0), f0_lengths=[ta for ta, _ in PAIRS])
            env.U.synchronize()
            args = (da, db, b_len, 1, 5)
            path, n, cost, status = env.pending_call("dtw_align", batch._b.dtw_align, batch._twin.dtw_align, args, {}, args)
            assert env.pending["dtw_align"] == [True], "the call waited for the stream"
            args = ([(da, db, 1, 5, 0)], b_len, path, n)
            out = env.pending_call("feature_distortion", batch._b.feature_distortion, batch._twin.feature_distortion, args,
                                   {}, args, stale=[da.clone(), db.clone(), path.clone(), n.clone()])
            assert env.pending["feature_distortion"] == [True], "the call waited for the stream"
            assert env.mismatches == [], "other bits than on the stream-0 context"
            path, n, cost, status, out = [t.cpu().numpy() for t in (path, n, cost, status, out)]
            env.U.synchronize()
            batch.close()
        at = 0
        for u, (ta, tb) in enumerate(PAIRS):
            ref_path, ref_cost, _ = K.reference(ta, tb, 5)
            assert status[u] == 0 and n[u] == len(ref_path)
            assert np.array_equal(path[at:at + n[u]], ref_path) and (path[at + n[u]:at + ta + tb - 1] == -1).all()
            assert abs(cost[u] - float(ref_cost)) <= K.cost_bound(ta, tb, 5, ref_cost)
            assert out[u, 0, 2] == n[u] and out[u, 0, 0] > 0.0
            at += ta + tb - 1
    finally:
        with torch.cuda.stream(env.U):
            env.ctx.close()
        torch.cuda.synchronize()

"""WorldBatch.mlsa_synthesis on a caller's own non-blocking stream, made as tests/test_gpu_caller_stream.py makes its
calls (its Env): a warm-up on stale inputs, the stream synchronised, then a delay of about 50 ms, the copy of the fresh
inputs over the stale ones and the call at once.  The call must return while the delay still runs, read the fresh inputs,
and give the bits of the same call on the session's stream-0 context -- which are held to the reference.  A second batch
with a longer utterance follows on the same context, so that the noise table grows between the calls."""
import numpy as np
import pytest

import mlsa_reference as R
import test_gpu_caller_stream as CS
import test_gpu_mlsa as T

pytestmark = pytest.mark.gpu

ORDER, ALPHA, PD = 12, 0.42, 4
# (frame shift, [(kind, frames)]): 195 samples at the most, then 5520 -- past the first table's 4096 spare values
ROUNDS = [(5, [("voiced", 9), ("alternate", 40), ("unvoiced", 3)]), (80, [("alternate", 70), ("voiced", 3)])]


def test_mlsa_synthesis_on_the_callers_stream(gpu):
    torch, W, ctx0 = gpu
    env = CS.Env(torch, W, ctx0)
    try:
        for k, (P, parts) in enumerate(ROUNDS):
            pitches, mcs = T.synthesis_inputs(81 + k, parts, ORDER)
            Ts = [len(m) for m in mcs]
            ys = [R.samples(t, P) for t in Ts]
            with torch.cuda.stream(env.U):
                pitch = T.dev(torch, np.concatenate(pitches), np.float32)
                mc = T.dev(torch, np.concatenate(mcs), np.float32)
                b = CS.DelayedBatch(env, env.ctx, W.default_params(16000, 5.0), f0_lengths=Ts, y_lengths=ys)
                env.U.synchronize()
                args = (pitch, mc, T.LP16, T.HP16)
                kwargs = dict(alpha=ALPHA, pade_order=PD, frame_shift=P)
                y, status = env.pending_call("mlsa_synthesis", b._b.mlsa_synthesis, b._twin.mlsa_synthesis, args, kwargs,
                                             args)
                assert env.pending["mlsa_synthesis"] == [True] * (k + 1), "the call waited for the stream"
                assert env.mismatches == [], "other bits than on the stream-0 context"
                y, status = y.cpu().numpy(), status.cpu().numpy()
                env.U.synchronize()
                b.close()
            assert (status == 0).all()
            es = T.run_excitation(gpu, pitches, T.LP16, T.HP16, P)
            for u, p in enumerate(pitches):
                x = R.excite(p, P)[0]
                g = R.noise(len(x))
                want = R.fir(T.LP16, x) + R.fir(T.HP16, g)
                bound = 64.0 * np.spacing(np.abs(T.LP16).sum() * max(np.abs(x).max(), 1e-300)
                                          + np.abs(T.HP16).sum() * np.abs(g).max())
                assert np.abs(es[u] - want).max() <= bound
            T.check_filter("on the caller's stream, round %d" % k, T.split(y, Ts, P), es, mcs, ALPHA, R.pade(PD), P)
    finally:
        with torch.cuda.stream(env.U):
            env.ctx.close()
        torch.cuda.synchronize()

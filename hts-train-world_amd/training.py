"""The recipe's trajectory training criterion for a torch model (scripts/Training.pl:930-940: DNNTraining.py -w win with
DNNDefine.trajectory_cost, data/scripts/DNNDefine.py:240-399), on whole batches of utterances.

    loss = TrajectoryLoss.apply(batch, pred, var, obs, gv_var, layout).mean()

pred is the model's output in the `ffo` layout, var the trained variance row, obs the `ffo` targets and gv_var the
content of gv.var.  The cost and both gradients come from one call of WorldBatch.trajectory_cost (csrc/trj.hip): nothing
here computes them in torch.  The network, its optimiser, checkpoints and the data reader are the caller's."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .recipe import ffo_layout


def stream_views(pred, obs, layout):
    """The (pred, obs, windows, msd) column views WorldBatch.trajectory_cost takes, of two `ffo`-layout matrices.
    layout: [(dim, windows, msd)] as recipe.ffo_layout takes it; obs may be None (views of pred alone: msd is then the
    predicted voicing column or None)."""
    cols, width = ffo_layout(layout)
    for t in (pred, obs):
        if t is not None and (t.dim() != 2 or t.shape[1] != width):
            raise ValueError(f"a row of this layout has {width} columns, got {tuple(t.shape)}")
    out = []
    for (mcol, c0, n), (_, wins, _) in zip(cols, layout):
        if obs is None:
            out.append((pred[:, c0:c0 + n], None, wins, None if mcol is None else pred[:, mcol]))
        else:
            out.append((pred[:, c0:c0 + n], obs[:, c0:c0 + n], wins,
                        None if mcol is None else (pred[:, mcol], obs[:, mcol])))
    return out


def final_outputs(b, pred, c, layout):
    """The rows DNNSynthesis.py writes in trajectory mode (DNNDefine.py:387-397): per stream the predicted voicing
    column, when it has one, then the trajectory c of the stream.  pred: [total_frames][ffo width]; c: per stream
    [total_frames][dim].  Returns float32 [total_frames][sum_s (msd_s + dim_s)]."""
    cols, width = ffo_layout(layout)
    if pred.shape[0] != b.total_frames or pred.shape[1] != width or len(c) != len(layout):
        raise ValueError(f"final_outputs: pred must be [{b.total_frames}][{width}] with one trajectory per stream")
    parts = []
    for (mcol, _, _), (dim, _, _), cs in zip(cols, layout, c):
        if tuple(cs.shape) != (b.total_frames, int(dim)):
            raise ValueError(f"final_outputs: a trajectory must be [{b.total_frames}][{int(dim)}], got {tuple(cs.shape)}")
        if mcol is not None:
            parts.append(pred[:, mcol:mcol + 1])
        parts.append(cs)
    return torch.cat([p.to(torch.float32) for p in parts], dim=1)


class TrajectoryLoss(torch.autograd.Function):
    """Per-utterance cost [n_utt] (float64) = trj + msd_weight msd + gv_weight gv of a WorldBatch `b`.  pred: float32 cuda
    [total_frames][width], var: float32 cuda [width] (either may require grad); obs: float32 cuda
    [total_frames][width]; gv_var: float32 cuda [sum of dims]; layout: [(dim, windows, msd)].  A non-zero status
    raises, unless skip_flagged: a flagged utterance then costs 0 and sends no gradient."""

    @staticmethod
    def forward(ctx, b, pred, var, obs, gv_var, layout, msd_weight=1.0, gv_weight=1.0e-6, skip_flagged=False):
        need_p, need_v = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        cost, _, grad_pred, grad_var, status = b.trajectory_cost(
            stream_views(pred.detach(), obs, layout), var.detach(), gv_var, msd_weight, gv_weight, want_c=False,
            want_grad_pred=need_p, want_grad_var=need_v)
        flagged = torch.nonzero(status).reshape(-1).tolist()
        if flagged and not skip_flagged:
            raise RuntimeError("TrajectoryLoss: utterances %s are flagged (status %s): bit 1 a non-finite input or a "
                               "variance that is not positive, bit 2 a matrix that is not positive definite"
                               % (flagged, [int(status[u]) for u in flagged]))
        ctx.grad_pred, ctx.grad_var = grad_pred, grad_var          # intermediates, not differentiable themselves
        ctx.offsets = torch.as_tensor(b.frame_offsets, device=pred.device)
        return cost[:, 0] + msd_weight * cost[:, 1] + gv_weight * cost[:, 2]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gp = gv = None
        if ctx.grad_pred is not None:
            per_frame = torch.repeat_interleave(g, ctx.offsets[1:] - ctx.offsets[:-1])
            gp = ctx.grad_pred * per_frame[:, None].to(torch.float32)
        if ctx.grad_var is not None:
            gv = (ctx.grad_var * g[:, None]).sum(0).to(torch.float32)
        return None, gp, gv, None, None, None, None, None, None

"""The recipe's trajectory training criterion for a torch model (scripts/Training.pl:930-940: DNNTraining.py -w win with
DNNDefine.trajectory_cost, data/scripts/DNNDefine.py:240-399), on whole batches of utterances.

    loss = TrajectoryLoss.apply(batch, pred, var, obs, gv_var, layout).mean()

pred is the model's output in the `ffo` layout, var the trained variance row, obs the `ffo` targets and gv_var the
content of gv.var.  The cost and both gradients come from one call of WorldBatch.trajectory_cost (csrc/trj.hip): nothing
here computes them in torch.

AcousticModel is the recipe's network itself (DNNDefine.inference, data/scripts/DNNDefine.py:113-191) under the
reference's parameter names: a plain torch forward with autograd, infer() for the forward pass of whole batches on the
library's own kernel (csrc/dnn.hip), train_outputs() for the training pass on the library's kernels (csrc/dnn_train.hip:
the forward pass with TF 1.x dropout, and as its autograd backward the library's backward pass through the network), and
save() / load() of one `.npz` -- the interchange format, since TF checkpoints cannot be read here.

    out = model.train_outputs(batch, x, spkr, keep_prob=0.5, seed=seed, offset=step)
    loss = (FrameLoss.apply(batch, out, model.variance.variances, obs, spkr) * weights).sum()

FrameLoss is DNNDefine.cost per utterance with both gradients from the library; TrajectoryLoss takes the same `out`.
The training loop itself (minibatches, the optimisers' groups, checkpoints) is recipe.train_files."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .recipe import ffo_layout
from .world import ACTIVATIONS


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


def frame_cost(pred, obs, var):
    """DNNDefine.cost (DNNDefine.py:231-237) in torch: 0.5 (ln 2 pi + mean ln var + mean (obs - pred)^2 / var)."""
    import math
    return 0.5 * (math.log(2.0 * math.pi) + torch.log(var).mean() + ((obs - pred) ** 2 / var).mean())


class FrameLoss(torch.autograd.Function):
    """Per-utterance frame-level cost [n_utt] (float64) of a WorldBatch `b` (DNNDefine.cost, DNNDefine.py:231-237).
    pred: float32 cuda [total_frames][D]; variances: float32 cuda [n_spkrs][D] (either may require grad); obs: float32
    cuda [total_frames][D]; spkr: None (the last speaker) or one index per utterance.  The cost and both gradients come
    from one WorldBatch.acoustic_model_train_forward call on a one-layer linear net with the identity as its weights
    (pred 1 + 0 is pred, bit for bit): nothing here computes them in torch.  Weights T_u / sum T on the result give the
    reference's mean over a minibatch.  A non-zero status raises, unless skip_flagged: a flagged utterance then costs 0
    and sends no gradient."""

    @staticmethod
    def forward(ctx, b, pred, variances, obs, spkr=None, skip_flagged=False):
        n_spkrs, D = int(variances.shape[0]), int(variances.shape[1])
        eye = {"weights": [torch.eye(D, dtype=torch.float32, device=pred.device)],
               "biases": [torch.zeros(D, dtype=torch.float32, device=pred.device)], "spkr_weights": None,
               "variances": variances.detach(), "n_spkrs": n_spkrs, "hidden_activation": 0, "output_activation": 0}
        _, cost, status, grad_pred, grad_var = b.acoustic_model_train_forward(eye, pred.detach(), spkr, obs, want_grads=True)
        flagged = torch.nonzero(status).reshape(-1).tolist()
        if flagged and not skip_flagged:
            raise RuntimeError("FrameLoss: utterances %s are flagged (status %s): bit 1 a non-finite input, bit 2 a variance "
                               "that is not positive and finite" % (flagged, [int(status[u]) for u in flagged]))
        ctx.grad_pred, ctx.grad_var = grad_pred, grad_var          # intermediates, not differentiable themselves
        ctx.offsets = torch.as_tensor(b.frame_offsets, device=pred.device)
        ctx.spk = [n_spkrs - 1] * b.n_utt if spkr is None else [int(v) for v in spkr]
        ctx.n_spkrs = n_spkrs
        return cost

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gp = gv = None
        if ctx.needs_input_grad[1]:
            per_frame = torch.repeat_interleave(g, ctx.offsets[1:] - ctx.offsets[:-1])
            gp = ctx.grad_pred * per_frame[:, None].to(torch.float32)
        if ctx.needs_input_grad[2]:
            # a speaker's utterances are added one by one in the batch's order, in double, and rounded once: a scatter
            # with atomic additions would leave the order, and so the bits, to chance
            w = ctx.grad_var * g[:, None]
            gv = torch.zeros(ctx.n_spkrs, w.shape[1], dtype=torch.float64, device=g.device)
            for u, s in enumerate(ctx.spk):
                gv[s] += w[u]
            gv = gv.to(torch.float32)
        return None, gp, gv, None, None, None


class _TrainOutputs(torch.autograd.Function):
    """AcousticModel.train_outputs: forward WorldBatch.acoustic_model_train_forward, backward
    WorldBatch.acoustic_model_backward with the same (keep_prob, seed, offset).  params: the module's parameters in
    AcousticModel.train_parameters' order, so that autograd hands their gradients back."""

    @staticmethod
    def forward(ctx, model, b, x, spkr, keep_prob, seed, offset, max_chunk_frames, *params):
        out, _, status = b.acoustic_model_train_forward(model, x, spkr, None, keep_prob, seed, offset, False, max_chunk_frames)
        flagged = torch.nonzero(status).reshape(-1).tolist()
        if flagged:
            raise RuntimeError("train_outputs: utterances %s are flagged (status %s): bit 1 a non-finite input, bit 2 a "
                               "non-finite output" % (flagged, [int(status[u]) for u in flagged]))
        ctx.call = (model, b, x, spkr, keep_prob, seed, offset, max_chunk_frames)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        model, b, x, spkr, keep_prob, seed, offset, max_chunk_frames = ctx.call
        grads = b.acoustic_model_backward(model, x, spkr, g.contiguous(), keep_prob, seed, offset, max_chunk_frames)
        flagged = torch.nonzero(grads["status"]).reshape(-1).tolist()
        if flagged:
            raise RuntimeError("train_outputs: the backward pass flagged utterances %s: a non-finite gradient" % (flagged,))
        return (None,) * 8 + tuple(grads[name].to(p.dtype) for name, p in model.train_parameters())


def _activate(name, v):
    return {"linear": lambda t: t, "sigmoid": torch.sigmoid, "tanh": torch.tanh, "relu": torch.relu}[name](v)


def _truncated_normal(shape, std):
    # tf.truncated_normal_initializer: values beyond two standard deviations are drawn again
    return torch.nn.init.trunc_normal_(torch.empty(*shape), 0.0, std, -2.0 * std, 2.0 * std)


class _Layer(torch.nn.Module):
    def __init__(self, fan_in, fan_out, n_spkrs, sat):
        super().__init__()
        self.si_weights = torch.nn.Parameter(_truncated_normal((fan_in, fan_out), 1.0 / fan_in ** 0.5))
        self.si_biases = torch.nn.Parameter(torch.zeros(fan_out))
        if sat:
            self.sd_weights = torch.nn.Parameter(_truncated_normal((n_spkrs, fan_out), 1.0 / n_spkrs ** 0.5))


class _Variance(torch.nn.Module):
    def __init__(self, n_spkrs, n_outputs):
        super().__init__()
        self.variances = torch.nn.Parameter(torch.ones(n_spkrs, n_outputs))


class AcousticModel(torch.nn.Module):
    """DNNDefine.inference: n_inputs -> units[0] -> ... -> n_outputs.  Parameters, as the reference names them:
    hidden{i}.si_weights [fan_in][units[i]], hidden{i}.si_biases, hidden{i}.sd_weights [n_spkrs][units[i]] (SAT mode:
    by default when there is more than one speaker), output.si_weights, output.si_biases, variance.variances
    [n_spkrs][n_outputs]; initialised as DNNDefine.py:135-183 does (truncated normal of deviation 1 / sqrt(fan_in), for
    the speaker rows 1 / sqrt(n_spkrs); biases 0; variances 1)."""

    def __init__(self, n_inputs, units, n_outputs, n_spkrs=1, hidden_activation="sigmoid", output_activation="linear",
                 sat=None):
        super().__init__()
        units = [int(n) for n in units]
        if hidden_activation not in ACTIVATIONS or output_activation not in ACTIVATIONS:
            raise ValueError("an activation is one of %s" % (ACTIVATIONS,))
        if n_inputs < 1 or n_outputs < 1 or n_spkrs < 1 or any(n < 1 for n in units) or len(units) > 8:
            raise ValueError("AcousticModel: at most 8 hidden layers; every width and n_spkrs at least 1")
        self.n_inputs, self.units, self.n_outputs, self.n_spkrs = int(n_inputs), units, int(n_outputs), int(n_spkrs)
        self.hidden_activation, self.output_activation = hidden_activation, output_activation
        self.sat = n_spkrs > 1 if sat is None else bool(sat)
        fan = [self.n_inputs] + units
        for i, n in enumerate(units):
            setattr(self, "hidden%d" % i, _Layer(fan[i], n, self.n_spkrs, self.sat))
        self.output = _Layer(fan[-1], self.n_outputs, self.n_spkrs, False)
        self.variance = _Variance(self.n_spkrs, self.n_outputs)

    def hidden(self, i):
        return getattr(self, "hidden%d" % i)

    def forward(self, x, spkr=None):
        """x: [rows][n_inputs]; spkr: None (the last speaker, DNNSynthesis.py:139), one index, or one index per row.
        Returns the outputs [rows][n_outputs]; no dropout (the caller's, between the layers of its training step)."""
        if spkr is None:
            spkr = self.n_spkrs - 1
        h = x
        for i in range(len(self.units)):
            L = self.hidden(i)
            z = h @ L.si_weights + L.si_biases
            if self.sat:
                z = z + L.sd_weights[spkr]
            h = _activate(self.hidden_activation, z)
        return _activate(self.output_activation, h @ self.output.si_weights + self.output.si_biases)

    def kernel_args(self):
        """What WorldBatch.acoustic_model_forward takes: the module's own parameters, float32, not copied when they
        already are."""
        f = lambda t: t.detach().to(torch.float32)
        layers = [self.hidden(i) for i in range(len(self.units))]
        return {"weights": [f(L.si_weights) for L in layers] + [f(self.output.si_weights)],
                "biases": [f(L.si_biases) for L in layers] + [f(self.output.si_biases)],
                "spkr_weights": [f(L.sd_weights) for L in layers] if self.sat else None,
                "variances": f(self.variance.variances), "n_spkrs": self.n_spkrs,
                "hidden_activation": self.hidden_activation, "output_activation": self.output_activation}

    def infer(self, batch, x, spkr=None, obs=None, max_chunk_frames=0):
        """The forward pass of a WorldBatch on the library's kernel: (out, cost or None, status), see
        WorldBatch.acoustic_model_forward.  spkr: None or one index per utterance."""
        return batch.acoustic_model_forward(self, x, spkr, obs, max_chunk_frames)

    def train_parameters(self):
        """[(name, parameter)] of the network (not the variances), the reference's names, in a fixed order."""
        keep = [(k, p) for k, p in self.named_parameters() if not k.startswith("variance.")]
        return keep

    def train_outputs(self, batch, x, spkr=None, keep_prob=1.0, seed=0, offset=0, max_chunk_frames=0):
        """The training forward of a WorldBatch on the library's kernels, differentiable with respect to the module's
        parameters (not to x): out float32 [total_frames][n_outputs].  keep_prob, seed, offset: the dropout of the hidden
        layers, see WorldBatch.acoustic_model_train_forward; offset is the caller's step counter.  The result feeds
        FrameLoss or TrajectoryLoss.  A flagged utterance raises."""
        return _TrainOutputs.apply(self, batch, x, spkr, float(keep_prob), int(seed), int(offset), int(max_chunk_frames),
                                   *[p for _, p in self.train_parameters()])

    def save(self, path, step=None, optimizer_state=None):
        """One `.npz`: float32 arrays under the parameters' names, and the two activation names; with `step`, the number
        of training steps behind the parameters (load() leaves it in the module's `step`, 0 without one); with
        optimizer_state (recipe.Tf1Optimizer.state_arrays: the rule's name, slot0/<parameter name>, slot1/<parameter
        name>, beta1_power, beta2_power), those arrays under optimizer/<key> (load() leaves the dictionary in the module's
        `optimizer_state`, None without one)."""
        import numpy as np
        arrays = {k: v.detach().to(torch.float32).cpu().numpy() for k, v in self.state_dict().items()}
        if step is not None:
            arrays["step"] = np.array(int(step), dtype=np.int64)
        for k, v in (optimizer_state or {}).items():
            arrays["optimizer/" + k] = np.asarray(v)
        arrays["hidden_activation"] = np.array(self.hidden_activation)
        arrays["output_activation"] = np.array(self.output_activation)
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path):
        import numpy as np
        with np.load(path, allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
        step = int(arrays.pop("step", 0))
        state = {k[len("optimizer/"):]: arrays.pop(k) for k in [k for k in arrays if k.startswith("optimizer/")]}
        n = 0
        while "hidden%d.si_weights" % n in arrays:
            n += 1
        for k in ("output.si_weights", "output.si_biases", "variance.variances", "hidden_activation", "output_activation"):
            if k not in arrays:
                raise ValueError("%s: no %s" % (path, k))
        units = [int(arrays["hidden%d.si_weights" % i].shape[1]) for i in range(n)]
        wo, var = arrays["output.si_weights"], arrays["variance.variances"]
        n_in = int(arrays["hidden0.si_weights"].shape[0]) if n else int(wo.shape[0])
        m = cls(n_in, units, int(wo.shape[1]), int(var.shape[0]), str(arrays.pop("hidden_activation")),
                str(arrays.pop("output_activation")), sat="hidden0.sd_weights" in arrays)
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in arrays.items()})
        m.step = step
        m.optimizer_state = state or None
        return m

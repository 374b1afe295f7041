"""TF 1.x's update rules, as published (the training_ops kernels behind tf.train.GradientDescentOptimizer,
MomentumOptimizer, AdagradOptimizer, AdadeltaOptimizer, AdamOptimizer and RMSPropOptimizer at their default
hyper-parameters), restated in numpy.  With g the gradient, p the parameter, r the rate:

  sgd                                        p <- p - r g
  momentum (mu 0.9)             a (0)        a <- a mu + g;  p <- p - a r
  adagrad                       a (0.1)      a <- a + g g;  p <- p - (g r) / sqrt(a)
  adadelta (rho 0.95, eps 1e-8) a, b (0)     a <- a rho + (g g) (1 - rho);  u = (sqrt(b + eps) / sqrt(a + eps)) g;
                                             p <- p - u r;  b <- b rho + (u u) (1 - rho)
  adam (0.9, 0.999, eps 1e-8)   m, v (0)     alpha = r sqrt(1 - pi2) / (1 - pi1);  m <- m + (g - m) (1 - beta1);
                                             v <- v + (g g - v) (1 - beta2);  p <- p - (m alpha) / (sqrt(v) + eps)
  rmsprop (rho 0.9, eps 1e-10)  s (1)        s <- s + (g g - s) (1 - rho);  p <- p - (g r) / sqrt(s + eps)

pi1, pi2 are beta1_power and beta2_power: they start at beta1 and beta2 and are multiplied by them after each step.

step64 evaluates this in float64 with float64 constants.  step32 is the float32 twin: exactly this sequence, one rounded
numpy float32 operation per operation written, the constants float32 and 1 - rho, 1 - beta float32 differences of them --
what the library's kernel must reproduce bit for bit.

The inputs (inputs()): tensors of SIZES elements -- around the float4 width, a wave, a block of 256 and many blocks --
at rates cycling RATES, standard normal parameters and, per step, gradients of magnitude log-uniform in 1e-10 .. 10 with
a random sign and every 97th element exactly 0.  The small magnitudes are what make epsilon's place visible.  Results are
computed once per (rule, dtype), shared and read-only."""
import functools

import numpy as np

RULES = ("sgd", "momentum", "adagrad", "adadelta", "adam", "rmsprop")
SLOT_INIT = {"sgd": (), "momentum": (0.0,), "adagrad": (0.1,), "adadelta": (0.0, 0.0), "adam": (0.0, 0.0), "rmsprop": (1.0,)}
SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 4099, 2 ** 20 + 1)
RATES = (0.5, 0.25, 0.005, 0.0)
STEPS = 5
SEED = 20261019
MU, BETA1, BETA2 = 0.9, 0.9, 0.999
RHO = {"adadelta": 0.95, "rmsprop": 0.9}
EPS = {"adadelta": 1e-8, "adam": 1e-8, "rmsprop": 1e-10}


def rates(n=len(SIZES)):
    return [RATES[k % len(RATES)] for k in range(n)]


def make_gradient(rng, n):
    g = np.exp(rng.uniform(np.log(1e-10), np.log(10.0), n)) * rng.choice([-1.0, 1.0], n)
    g[::97] = 0.0
    return g.astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(sizes=SIZES, steps=STEPS, seed=SEED):
    """(params [tensor], grads [step][tensor]): float32, read-only."""
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    grads = [[make_gradient(rng, n) for n in sizes] for _ in range(steps)]
    for a in params + [g for gs in grads for g in gs]:
        a.setflags(write=False)
    return params, grads


def initial_powers(dtype):
    return dtype(BETA1), dtype(BETA2)


def advance_powers(powers, dtype):
    """What the caller does after each step."""
    return dtype(powers[0] * dtype(BETA1)), dtype(powers[1] * dtype(BETA2))


def initial_slots(rule, like, dtype):
    return [np.full(like.shape, v, dtype=dtype) for v in SLOT_INIT[rule]]


def _step(rule, dtype, p, g, slots, r, powers):
    """One update of one tensor in `dtype`: every line one rounded operation.  Returns (p, slots), new arrays."""
    p, g, r = np.asarray(p, dtype=dtype), np.asarray(g, dtype=dtype), dtype(r)
    slots = [np.asarray(s, dtype=dtype) for s in slots]
    one = dtype(1.0)
    if rule == "sgd":
        d = r * g
        return p - d, []
    if rule == "momentum":
        am = slots[0] * dtype(MU)
        a = am + g
        d = a * r
        return p - d, [a]
    if rule == "adagrad":
        gg = g * g
        a = slots[0] + gg
        gr = g * r
        d = gr / np.sqrt(a)
        return p - d, [a]
    if rule == "adadelta":
        rho, eps = dtype(RHO[rule]), dtype(EPS[rule])
        omr = dtype(one - rho)
        gg = g * g
        ar = slots[0] * rho
        gs = gg * omr
        a = ar + gs
        nb = slots[1] + eps
        na = a + eps
        q = np.sqrt(nb) / np.sqrt(na)
        u = q * g
        d = u * r
        br = slots[1] * rho
        uu = u * u
        us = uu * omr
        return p - d, [a, br + us]
    if rule == "adam":
        b1, b2, eps = dtype(BETA1), dtype(BETA2), dtype(EPS[rule])
        scale = np.sqrt(dtype(one - dtype(powers[1])))
        rs = dtype(r * scale)
        alpha = dtype(rs / dtype(one - dtype(powers[0])))
        gm = g - slots[0]
        dm = gm * dtype(one - b1)
        m = slots[0] + dm
        gg = g * g
        gv = gg - slots[1]
        dv = gv * dtype(one - b2)
        v = slots[1] + dv
        ma = m * alpha
        den = np.sqrt(v) + eps
        d = ma / den
        return p - d, [m, v]
    if rule == "rmsprop":
        rho, eps = dtype(RHO[rule]), dtype(EPS[rule])
        gg = g * g
        gs = gg - slots[0]
        ds = gs * dtype(one - rho)
        s = slots[0] + ds
        gr = g * r
        se = s + eps
        d = gr / np.sqrt(se)
        return p - d, [s]
    raise ValueError(rule)


def step64(rule, p, g, slots, r, powers=None):
    return _step(rule, np.float64, p, g, slots, r, powers if powers is not None else initial_powers(np.float64))


def step32(rule, p, g, slots, r, powers=None):
    out = _step(rule, np.float32, p, g, slots, r, powers if powers is not None else initial_powers(np.float32))
    assert out[0].dtype == np.float32 and all(s.dtype == np.float32 for s in out[1])
    return out


def run_steps(rule, dtype, params, grads, tensor_rates):
    """`len(grads)` steps over all tensors: (params, slots [slot][tensor], powers), the powers advanced after each step."""
    params = [np.asarray(p, dtype=dtype) for p in params]
    slots = [initial_slots(rule, p, dtype) for p in params]
    powers = initial_powers(dtype)
    for gs in grads:
        for k, g in enumerate(gs):
            params[k], slots[k] = _step(rule, dtype, params[k], g, slots[k], tensor_rates[k], powers)
        powers = advance_powers(powers, dtype)
    by_slot = [[slots[k][j] for k in range(len(params))] for j in range(len(SLOT_INIT[rule]))]
    return params, by_slot, powers


@functools.lru_cache(maxsize=None)
def reference(rule, dtype):
    """run_steps on inputs() at rates(): computed once, read-only."""
    params, grads = inputs()
    p, slots, powers = run_steps(rule, dtype, params, grads, rates())
    for a in p + [t for s in slots for t in s]:
        a.setflags(write=False)
    return p, slots, powers

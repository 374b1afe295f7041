"""The acoustic model's forward pass and frame-level cost (data/scripts/DNNDefine.py:113-191 inference, :231-237 cost,
as DNNSynthesis.py:129-229 runs them) restated in numpy float64 -- the yardstick of WorldMi355AcousticModelForward --
with the running error bound of a float32 evaluation next to the values.  No torch here.

Per frame with speaker s:  h_{i+1} = act_h((h_i W_i + b_i) + sd_i[s])  (the speaker row in SAT mode only),
out = act_o(h_L W_o + b_o);  activations 0 linear, 1 sigmoid, 2 tanh, 3 ReLU (Config.pm.in:228).

The bound, u = 2^-24, gamma_n = n u / (1 - n u), e_0 = 0; per layer with fan-in K:
    m = |h| |W| + |b| + |sd|,   e_z = e |W| + gamma_{K+2} (m + e |W|),   e' = L e_z + (eps + u) |v|,
L = 1/4 for sigmoid and 1 otherwise, eps = 8 u for sigmoid and tanh and 0 otherwise: the forward error of a length-K
fma chain and two additions, pushed through the activation's Lipschitz constant, plus the activation's own error and
the rounding of its result.  Nothing in it is measured."""
import functools

import numpy as np

ACTIVATIONS = ("linear", "sigmoid", "tanh", "relu")
U = 2.0 ** -24

# the shapes of the GPU tests: utterance lengths on either side of an MFMA tile (32) and of a block tile (128), so that
# utterance boundaries fall inside tiles; nets (inputs, hidden units, outputs)
LENGTHS = (1, 2, 31, 32, 33, 127, 128, 129, 257)
NETS = ((37, (48, 130), 229), (1, (1,), 1), (3, (), 33), (65, (129,), 31), (700, (), 229))
N_SPKRS = 3
SEED = 20240


def act(name, z):
    if name == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    if name == "tanh":
        return np.tanh(z)
    if name == "relu":
        return np.maximum(z, 0.0)
    assert name == "linear"
    return z


def n_layers(params):
    n = 0
    while "hidden%d.si_weights" % n in params:
        n += 1
    return n


def layers(params):
    """[(W, b, sd or None)] of the hidden layers, then the output layer's, as float64."""
    f = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    out = []
    for i in range(n_layers(params)):
        sd = params.get("hidden%d.sd_weights" % i)
        out.append((f(params["hidden%d.si_weights" % i]), f(params["hidden%d.si_biases" % i]), None if sd is None else f(sd)))
    out.append((f(params["output.si_weights"]), f(params["output.si_biases"]), None))
    return out


def forward(params, x, spkr_rows, hidden, output):
    """x: float32 [rows][n_inputs]; spkr_rows: int [rows], the speaker of every row (read in SAT mode).  Returns
    (out float64 [rows][n_outputs], e float64 the same shape: the bound on a float32 evaluation's error)."""
    h = np.asarray(x, dtype=np.float32).astype(np.float64)
    e = np.zeros_like(h)
    ls = layers(params)
    for i, (W, b, sd) in enumerate(ls):
        name = output if i == len(ls) - 1 else hidden
        K = W.shape[0]
        z = h @ W + b
        m = np.abs(h) @ np.abs(W) + np.abs(b)
        if sd is not None:
            z = z + sd[spkr_rows]
            m = m + np.abs(sd[spkr_rows])
        eW = e @ np.abs(W)
        g = (K + 2) * U / (1.0 - (K + 2) * U)
        ez = eW + g * (m + eW)
        v = act(name, z)
        lip = 0.25 if name == "sigmoid" else 1.0
        eps = 8.0 * U if name in ("sigmoid", "tanh") else 0.0
        h, e = v, lip * ez + (eps + U) * np.abs(v)
    return h, e


def forward_f32(params, x, spkr_rows, hidden, output):
    """The same pass in plain numpy float32 (whatever order its matrix product sums in): what the bound must cover."""
    f = np.float32
    h = np.asarray(x, dtype=f)
    ls = layers(params)
    for i, (W, b, sd) in enumerate(ls):
        name = output if i == len(ls) - 1 else hidden
        z = (h @ W.astype(f)).astype(f) + b.astype(f)
        if sd is not None:
            z = z + sd.astype(f)[spkr_rows]
        assert z.dtype == f
        if name == "sigmoid":
            h = (f(1.0) / (f(1.0) + np.exp(-z))).astype(f)
        elif name == "tanh":
            h = np.tanh(z).astype(f)
        elif name == "relu":
            h = np.maximum(z, f(0.0))
        else:
            h = z
    return h


def cost(out, obs, var):
    """One utterance: (cost, S) -- 0.5 (ln 2 pi + mean_d ln var_d + mean_td (obs - out)^2 / var_d) in float64 from the
    float32 values given, and S, the sum of the magnitudes of the terms added."""
    out, obs, var = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (out, obs, var))
    T, D = out.shape
    ln, q = np.log(var), (obs - out) ** 2 / var[None, :]
    c = 0.5 * (np.log(2.0 * np.pi) + ln.sum() / D + q.sum() / (T * D))
    S = 0.5 * (np.log(2.0 * np.pi) + np.abs(ln).sum() / D + q.sum() / (T * D))
    return c, S


def spkr_rows(lengths, spkr):
    return np.repeat(np.asarray(spkr, dtype=np.int64), lengths)


# ---- deterministic cases ------------------------------------------------------------------------------------------
def _truncated_normal(rng, shape, std):
    a = rng.standard_normal(shape)
    while True:
        bad = np.abs(a) > 2.0
        if not bad.any():
            return (a * std).astype(np.float32)
        a[bad] = rng.standard_normal(int(bad.sum()))


def make_model(seed, n_in, units, n_out, n_spkrs=1, sat=False):
    """float32 parameters under the reference's names: weights as the reference initialises them (truncated normal,
    1 / sqrt(fan_in); the speaker rows 1 / sqrt(n_spkrs)), biases 0.1 normal so that a dropped bias shows, variances
    log-uniform in 0.25 .. 4."""
    rng = np.random.default_rng(seed)
    p, fan = {}, n_in
    for i, n in enumerate(units):
        p["hidden%d.si_weights" % i] = _truncated_normal(rng, (fan, n), 1.0 / np.sqrt(fan))
        p["hidden%d.si_biases" % i] = (0.1 * rng.standard_normal(n)).astype(np.float32)
        if sat:
            p["hidden%d.sd_weights" % i] = _truncated_normal(rng, (n_spkrs, n), 1.0 / np.sqrt(n_spkrs))
        fan = n
    p["output.si_weights"] = _truncated_normal(rng, (fan, n_out), 1.0 / np.sqrt(fan))
    p["output.si_biases"] = (0.1 * rng.standard_normal(n_out)).astype(np.float32)
    p["variance.variances"] = np.exp(rng.uniform(np.log(0.25), np.log(4.0), (n_spkrs, n_out))).astype(np.float32)
    return p


def make_inputs(seed, rows, n_in):
    """float32 [rows][n_in]: half the columns binary (question answers), half standard normal."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, n_in))
    nb = n_in // 2
    x[:, :nb] = rng.integers(0, 2, (rows, nb))
    return x.astype(np.float32)


def utterance_spkrs(n_utt, n_spkrs=N_SPKRS):
    return [(2 * u + 1) % n_spkrs for u in range(n_utt)]


MODES = ("sd", "sat", "sat_default")      # SAT with per-utterance indices, SAT with the NULL default (the last speaker)


@functools.lru_cache(maxsize=None)
def cached_case(net, mode, hidden, output, lengths=LENGTHS):
    """(params, x, spkr per utterance or None, out, e) of one test case, computed once per process and read-only."""
    n_in, units, n_out = NETS[net]
    sat = mode != "sd"
    n_spkrs = N_SPKRS if sat else 1
    params = make_model(SEED + net, n_in, units, n_out, n_spkrs, sat)
    x = make_inputs(SEED + 100 + net, int(sum(lengths)), n_in)
    spkr = utterance_spkrs(len(lengths)) if mode == "sat" else None
    rows = spkr_rows(lengths, spkr if spkr is not None else [n_spkrs - 1] * len(lengths))
    out, e = forward(params, x, rows, hidden, output)
    for a in list(params.values()) + [x, out, e]:
        a.setflags(write=False)
    return params, x, spkr, out, e


def all_cases():
    """Every (net, mode, hidden activation, output activation) of the GPU tests; a net without a hidden layer takes
    one hidden activation only (it has none)."""
    for net, (_, units, _) in enumerate(NETS):
        for mode in MODES:
            for hidden in (ACTIVATIONS if units else ACTIVATIONS[:1]):
                for output in ("linear", "sigmoid"):
                    yield net, mode, hidden, output


def exact_case(net, mode, hidden, lengths=LENGTHS):
    """Small-integer inputs, weights, biases and speaker rows, W[k][n] = ((3 k + 5 n + layer) mod 7) - 3: every partial
    sum of a float32 evaluation is an integer below 2^24 in magnitude (asserted here from sum |a| |b|), so float32 and
    float64 agree exactly and the result does not depend on the order of the sum.  Linear output.  Returns
    (params, x, spkr or None, out float64)."""
    n_in, units, n_out = NETS[net]
    sat = mode != "sd"
    n_spkrs = N_SPKRS if sat else 1
    rng = np.random.default_rng(SEED + 500 + net)
    p, fan = {}, n_in
    for i, n in enumerate(list(units) + [n_out]):
        name = "output" if i == len(units) else "hidden%d" % i
        k, c = np.arange(fan)[:, None], np.arange(n)[None, :]
        p[name + ".si_weights"] = (((3 * k + 5 * c + i) % 7) - 3).astype(np.float32)
        p[name + ".si_biases"] = rng.integers(-4, 5, n).astype(np.float32)
        if sat and i < len(units):
            p[name + ".sd_weights"] = rng.integers(-3, 4, (n_spkrs, n)).astype(np.float32)
        fan = n
    p["variance.variances"] = np.ones((n_spkrs, n_out), dtype=np.float32)
    rows = int(sum(lengths))
    x = rng.integers(-1, 2, (rows, n_in)).astype(np.float32)
    x[np.arange(rows), np.arange(rows) % n_in] = 2.0                     # every row differs from its neighbours
    spkr = utterance_spkrs(len(lengths)) if mode == "sat" else None
    sr = spkr_rows(lengths, spkr if spkr is not None else [n_spkrs - 1] * len(lengths))
    h = x.astype(np.float64)
    ls = layers(p)
    for i, (W, b, sd) in enumerate(ls):
        m = np.abs(h) @ np.abs(W) + np.abs(b) + (0.0 if sd is None else np.abs(sd[sr]))
        assert m.max() < 2.0 ** 24, ("a partial sum may leave the exact integers", net, i, m.max())
        z = h @ W + b + (0.0 if sd is None else sd[sr])
        h = act("linear" if i == len(ls) - 1 else hidden, z)
    return p, x, spkr, h

"""The acoustic model's training pass (DNNTraining.py's step: DNNDefine.inference at keep_prob < 1 with TF 1.x
tf.nn.dropout, DNNDefine.cost, and their gradients) restated in numpy float64 -- the yardstick of
WorldMi355AcousticModelTrainForward / WorldMi355AcousticModelBackward -- with the running error bound of a float32
evaluation next to every value, built as dnn_reference.forward builds its bound.  No torch here.

Mask of hidden layer i, batch row t, unit n:  m = 1 iff float32(w >> 8) * 2^-24 < p, w word n & 3 of Philox4x32-10 at
counter (t, n >> 2, i, offset), key (seed & 0xffffffff, seed >> 32).
Forward:   a_i = act_h((h_{i-1} W_i + b_i) + sd_i[s]),  h_i = m a_i / p  (h_i = a_i at p = 1),  out = act_o(h W_o + b_o).
Backward:  dz_o = G act_o'(out),  dh_{i-1} = dz_i W_i',  da_i = m dh_i / p,  dz_i = da_i act_h'(a_i),
           dW_i = h_{i-1}' dz_i,  db_i = sum_t dz_i,  dsd_i[s] = sum over the rows of speaker s.

The bound, u = 2^-24, gamma_n = n u / (1 - n u); e_X is the bound on the float32 evaluation's error of X:
  dropout     e_h = m (e_a / p + u |a / p|)                                   (one division; nothing at p = 1)
  product     P = A B over a reduction of length K with erroneous operands:
              c = e_A |B| + |A| e_B + e_A e_B,   e_P = c + gamma_{K+2} (|A| |B| + c)
  derivative  d = act'(a) from the float32 a, delta = e_a:
              sigmoid a (1 - a):  e_d = delta + delta^2 + 3 u |d|            (|1 - 2a| <= 1; a subtraction and a product)
              tanh 1 - a^2:       e_d = 2 delta + delta^2 + 3 u (|d| + a^2)  (|2a| <= 2; the rounding of a^2 is absolute)
              ReLU [a > 0]:       e_d = 1 where |a| <= delta (the derivative jumps: |da| in full), else 0;  linear: 0
  dz = g d    e_dz = c + u (|g d| + c),  c = e_g |d| + |g| e_d + e_g e_d     (an elementwise product, one rounding)
  db, dsd     v = sum of dz in double, rounded once:  e = u |v| + sum e_dz + rows 2^-53 sum |dz|.
Nothing in it is measured."""
import numpy as np

import dnn_reference as R

U = R.U
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two ints.  Returns the four output words (uint32 arrays)."""
    c = [np.asarray(v, dtype=np.uint64) & 0xffffffff for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)           # 32 x 32 bits: no overflow of uint64
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & np.uint64(0xffffffff), p1 >> np.uint64(32), p1 & np.uint64(0xffffffff)
        c = [h1 ^ c[1] ^ np.uint64(k0), l1, h0 ^ c[3] ^ np.uint64(k1), l0]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return [v.astype(np.uint32) for v in c]


def mask(seed, offset, layer, rows, units, p):
    """bool [rows][units]: the kept elements of hidden layer `layer`."""
    nb = (units + 3) // 4
    t, b = np.arange(rows, dtype=np.uint64)[:, None], np.arange(nb, dtype=np.uint64)[None, :]
    w = philox4x32_10((t, b, np.uint64(layer), np.uint64(int(offset) & 0xffffffff)),
                      (int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff))
    words = np.stack(w, axis=2).reshape(rows, 4 * nb)[:, :units]
    r = (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return r < np.float32(p)


def masks(seed, offset, rows, units, p):
    return [mask(seed, offset, i, rows, n, p) for i, n in enumerate(units)]


def gamma(n):
    return n * U / (1.0 - n * U)


def deriv(name, a, e_a):
    """(act'(a) from the activation value, the bound on its float32 evaluation given |a32 - a| <= e_a)."""
    if name == "sigmoid":
        d = a * (1.0 - a)
        return d, e_a + e_a ** 2 + 3.0 * U * np.abs(d)
    if name == "tanh":
        d = 1.0 - a * a
        return d, 2.0 * e_a + e_a ** 2 + 3.0 * U * (np.abs(d) + a * a)
    if name == "relu":
        return (a > 0.0).astype(np.float64), (np.abs(a) <= e_a).astype(np.float64)
    assert name == "linear"
    return np.ones_like(a), np.zeros_like(a)


def _times(g, e_g, d, e_d):
    c = e_g * np.abs(d) + np.abs(g) * e_d + e_g * e_d
    return g * d, c + U * (np.abs(g * d) + c)


def _matmul(A, e_A, B, e_B, K):
    c = e_A @ np.abs(B) + np.abs(A) @ e_B + e_A @ e_B
    return A @ B, c + gamma(K + 2) * (np.abs(A) @ np.abs(B) + c)


def train_forward(params, x, spkr_rows, hidden, output, p=1.0, seed=0, offset=0, ms=None):
    """The training forward.  p: keep_prob (taken as float32); ms: the masks to use instead of Philox's (bool
    [rows][units[i]] per hidden layer).  Returns a dict: x, a / e_a and h / e_h per hidden layer, out, e_out, masks, p."""
    p = float(np.float32(p))
    ls = R.layers(params)
    h = np.asarray(x, dtype=np.float32).astype(np.float64)
    e = np.zeros_like(h)
    fw = {"x": h, "a": [], "e_a": [], "h": [], "e_h": [], "masks": [], "p": p}
    for i, (W, b, sd) in enumerate(ls):
        last = i == len(ls) - 1
        name = output if last else hidden
        K = W.shape[0]
        z = h @ W + b
        m = np.abs(h) @ np.abs(W) + np.abs(b)
        if sd is not None:
            z = z + sd[spkr_rows]
            m = m + np.abs(sd[spkr_rows])
        eW = e @ np.abs(W)
        ez = eW + gamma(K + 2) * (m + eW)
        v = R.act(name, z)
        lip = 0.25 if name == "sigmoid" else 1.0
        eps = 8.0 * U if name in ("sigmoid", "tanh") else 0.0
        ev = lip * ez + (eps + U) * np.abs(v)
        if last:
            fw["out"], fw["e_out"] = v, ev
            break
        fw["a"].append(v)
        fw["e_a"].append(ev)
        if p < 1.0:
            mk = ms[i] if ms is not None else mask(seed, offset, i, v.shape[0], v.shape[1], p)
            h = np.where(mk, v / p, 0.0)
            e = np.where(mk, ev / p + U * np.abs(v / p), 0.0)
        else:
            mk = np.ones(v.shape, dtype=bool)
            h, e = v, ev
        fw["masks"].append(mk)
        fw["h"].append(h)
        fw["e_h"].append(e)
    return fw


def names_of(n_layers):
    return ["hidden%d" % i for i in range(n_layers)] + ["output"]


def backward(params, fw, G, spkr_rows, hidden, output, e_G=None):
    """(grads, bounds): dicts keyed by the reference's parameter names, float64, of sum(out * G).  e_G: None -- G is
    the float32 matrix that the float32 evaluation receives too, without error -- or the element-wise bound on the error
    of the G that reaches the float32 evaluation: G is then taken in float64 as it is given (a whole training step,
    tests/train_step_reference.py, where G comes from the forward pass's own outputs)."""
    ls = R.layers(params)
    L = len(ls) - 1
    names = names_of(L)
    p = fw["p"]
    rows = fw["x"].shape[0]
    if e_G is None:
        G = np.asarray(G, dtype=np.float32).astype(np.float64)
        e_G = np.zeros_like(G)
    else:
        G, e_G = np.asarray(G, dtype=np.float64), np.broadcast_to(np.asarray(e_G, dtype=np.float64), np.shape(G))
    d, e_d = deriv(output, fw["out"], fw["e_out"])
    dz, e_dz = _times(G, e_G, d, e_d)
    grads, bounds = {}, {}
    for i in range(L, -1, -1):
        W, _, sd = ls[i]
        hin = fw["x"] if i == 0 else fw["h"][i - 1]
        e_hin = np.zeros_like(hin) if i == 0 else fw["e_h"][i - 1]
        grads[names[i] + ".si_weights"], bounds[names[i] + ".si_weights"] = _matmul(hin.T, e_hin.T, dz, e_dz, rows)
        dbl = rows * 2.0 ** -53 * np.abs(dz).sum(0)
        v = dz.sum(0)
        grads[names[i] + ".si_biases"], bounds[names[i] + ".si_biases"] = v, U * np.abs(v) + e_dz.sum(0) + dbl
        if sd is not None:
            gs, bs = np.zeros_like(sd), np.zeros_like(sd)
            for s in range(sd.shape[0]):
                sel = spkr_rows == s
                gs[s] = dz[sel].sum(0)
                bs[s] = U * np.abs(gs[s]) + e_dz[sel].sum(0) + dbl
            grads[names[i] + ".sd_weights"], bounds[names[i] + ".sd_weights"] = gs, bs
        if i == 0:
            break
        dh, e_dh = _matmul(dz, e_dz, W.T, np.zeros_like(W.T), W.shape[1])
        if p < 1.0:
            mk = fw["masks"][i - 1]
            da = np.where(mk, dh / p, 0.0)
            e_da = np.where(mk, e_dh / p + U * np.abs(dh / p), 0.0)
        else:
            da, e_da = dh, e_dh
        d, e_d = deriv(hidden, fw["a"][i - 1], fw["e_a"][i - 1])
        dz, e_dz = _times(da, e_da, d, e_d)
    return grads, bounds


def products_stay_exact(params, fw, G, hidden, output):
    """The largest sum |a| |b| over every product of the backward pass: below 2^24 on small integers, every partial sum
    of a float32 evaluation is exact."""
    ls = R.layers(params)
    L = len(ls) - 1
    p = fw["p"]
    G = np.asarray(G, dtype=np.float32).astype(np.float64)
    dz = G * deriv(output, fw["out"], 0.0 * fw["out"])[0]
    worst = 0.0
    for i in range(L, -1, -1):
        W = ls[i][0]
        hin = fw["x"] if i == 0 else fw["h"][i - 1]
        worst = max(worst, float((np.abs(hin).T @ np.abs(dz)).max()), float(np.abs(dz).sum(0).max()))
        if i == 0:
            break
        worst = max(worst, float((np.abs(dz) @ np.abs(W).T).max()))
        da = np.where(fw["masks"][i - 1], (dz @ W.T) / p, 0.0)
        dz = da * deriv(hidden, fw["a"][i - 1], 0.0 * da)[0]
    return worst


def _act_f32(name, z):
    f = np.float32
    if name == "sigmoid":
        return (f(1.0) / (f(1.0) + np.exp(-z))).astype(f)
    if name == "tanh":
        return np.tanh(z).astype(f)
    if name == "relu":
        return np.maximum(z, f(0.0))
    return z


def _deriv_f32(name, a):
    f = np.float32
    if name == "sigmoid":
        return a * (f(1.0) - a)
    if name == "tanh":
        return f(1.0) - a * a
    if name == "relu":
        return (a > 0).astype(f)
    return np.ones_like(a)


def backward_f32(params, x, spkr_rows, hidden, output, p, ms, G):
    """Forward and backward in plain numpy float32 (whatever order its products sum in) with the masks given: what the
    bound must cover.  G: the matrix, or a function of the float32 outputs that returns it (a criterion evaluated on
    them).  Returns the gradients, float32, keyed as backward's."""
    f = np.float32
    p = f(p)
    ls = [(W.astype(f), b.astype(f), None if sd is None else sd.astype(f)) for W, b, sd in R.layers(params)]
    L = len(ls) - 1
    names = names_of(L)
    h = np.asarray(x, dtype=f)
    acts, hs = [], [h]
    for i, (W, b, sd) in enumerate(ls):
        z = (h @ W).astype(f) + b
        if sd is not None:
            z = z + sd[spkr_rows]
        a = _act_f32(output if i == L else hidden, z)
        assert a.dtype == f
        if i == L:
            out = a
            break
        acts.append(a)
        h = np.where(ms[i], a / p, f(0.0)).astype(f) if p < 1 else a
        hs.append(h)
    dz = np.asarray(G(out) if callable(G) else G, dtype=f) * _deriv_f32(output, out)
    grads = {}
    for i in range(L, -1, -1):
        W, _, sd = ls[i]
        grads[names[i] + ".si_weights"] = (hs[i].T @ dz).astype(f)
        grads[names[i] + ".si_biases"] = dz.astype(np.float64).sum(0).astype(f)
        if sd is not None:
            grads[names[i] + ".sd_weights"] = np.stack([dz[spkr_rows == s].astype(np.float64).sum(0)
                                                        for s in range(sd.shape[0])]).astype(f)
        if i == 0:
            break
        dh = (dz @ W.T).astype(f)
        da = np.where(ms[i - 1], dh / p, f(0.0)).astype(f) if p < 1 else dh
        dz = da * _deriv_f32(hidden, acts[i - 1])
        assert dz.dtype == f
    return grads


def cost_grads(out, obs, var):
    """One utterance, from the float32 values given: (grad_out float64 [T][D] = (out - obs) / (var T D),
    grad_var float64 [D] = (1 / var - (1 / T) sum_t (obs - out)^2 / var^2) / (2 D), S [D]: the sum of the magnitudes
    of grad_var's terms)."""
    out, obs, var = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (out, obs, var))
    T, D = out.shape
    q = ((obs - out) ** 2).sum(0) / (T * var * var)
    return (out - obs) / (var[None, :] * T * D), (1.0 / var - q) / (2.0 * D), (1.0 / var + q) / (2.0 * D)


def exact_G(rows, D, step=8):
    """G[t][d] = ((3 t + 5 d) mod 3) - 1 where (t + d) mod step = 0, else 0."""
    t, d = np.arange(rows)[:, None], np.arange(D)[None, :]
    return np.where((t + d) % step == 0, ((3 * t + 5 * d) % 3) - 1, 0).astype(np.float32)


def random_G(seed, rows, D):
    return np.random.default_rng(seed).standard_normal((rows, D)).astype(np.float32)


# ---- a small corpus for recipe.train_files ----------------------------------------------------------------------------
CORPUS_NET = (37, (48,), 229)
CORPUS_LENGTHS = (33, 129, 257, 64)
CORPUS_LR, CORPUS_STEPS, CORPUS_BATCH = 2.0, 20, 128      # SGD; the host test confirms that the cost falls at this rate


def write_corpus(directory, n_spkrs=1, lengths=CORPUS_LENGTHS):
    """`.ffi` / `.ffo` files of `lengths` frames: inputs as make_inputs draws them, targets a random net's outputs
    (sigmoid hidden units, linear outputs) plus 0.1 normal noise.  Returns [(ffi, ffo, speaker index)]."""
    import os
    n_in, units, n_out = CORPUS_NET
    teacher = R.make_model(R.SEED + 700, n_in, units, n_out)
    rng = np.random.default_rng(R.SEED + 701)
    jobs = []
    for k, T_ in enumerate(lengths):
        x = R.make_inputs(R.SEED + 710 + k, T_, n_in)
        out, _ = R.forward(teacher, x, np.zeros(T_, dtype=np.int64), "sigmoid", "linear")
        obs = (out + 0.1 * rng.standard_normal(out.shape)).astype(np.float32)
        ffi, ffo = os.path.join(str(directory), "u%d.ffi" % k), os.path.join(str(directory), "u%d.ffo" % k)
        x.tofile(ffi)
        obs.tofile(ffo)
        jobs.append((ffi, ffo, k % n_spkrs))
    return jobs

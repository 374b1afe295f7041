"""The MGC-LSP route (lspcheck | lsp2lpc | mgc2mgc -n -u) and postfiltering_lsp: what can be checked without a GPU.
SPTK's lspcheck and lsp2lpc are not in the reference tree, so the numpy restatement (tests/lsp_reference.py) is pinned by
what it must satisfy: the roots of P and Q, closed forms at orders 1 and 2, the impulse response of K / A(z) through
tests/mgc2mgc_reference.py, and hand-computed rows of the check and the filter.  Then the ABI: structs, defaults, the
refusals made on the host, and the recipe's two commands."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import lsp_reference as L
import mgc2mgc_reference as M

PI = np.pi


def valid_set(m, seed):
    rng = np.random.default_rng(seed)
    return PI / (m + 1) * (np.arange(1, m + 1) + rng.uniform(-0.3, 0.3, m))


@pytest.mark.parametrize("m", [1, 2, 3, 34, 35, 63])
def test_roots_of_p_and_q_sit_at_their_lsps_and_a_is_minimum_phase(m):
    w = valid_set(m, 100 + m)
    P, Q = L.polynomials(w)
    assert len(P) == len(Q) == m + 2
    for poly, own, extra in ((P, w[0::2], [PI] if m % 2 == 0 else []),
                             (Q, w[1::2], [0.0] if m % 2 == 0 else [0.0, PI])):
        roots = np.roots(poly)
        assert np.abs(np.abs(roots) - 1).max() < 1e-6
        ang = np.sort(np.abs(np.angle(roots)))
        want = np.sort(np.concatenate([own, own, extra]))
        assert np.abs(ang - want).max() < 1e-6, m
    a = L.lsp2lpc(w)
    full = 0.5 * (P + Q)
    assert a[0] == 1 and np.abs(a - full[:m + 1]).max() < 1e-12 and abs(full[m + 1]) < 1e-12
    assert np.abs(np.roots(a)).max() < 1


def test_the_order_of_the_factors_keeps_the_partial_products_small():
    """Why lsp2lpc does not take the factors in ascending i: the partial products of roots on one arc grow with the
    order, and P + Q then cancels what float64 holds.  In factor_order() they stay small."""
    for m, lost, kept in ((34, 1e-11, 1e-12), (63, 1e-5, 1e-11)):
        assert sorted(L.factor_order(m)) == list(range(1, m + 1))
        worst_asc = worst = 0.0
        for seed in range(5):
            w = valid_set(m, seed)
            exact = L.lsp2lpc(w, L.LD)
            worst = max(worst, float(np.abs(L.lsp2lpc(w) - exact).max()))
            worst_asc = max(worst_asc, float(np.abs(L.lsp2lpc(w, order=range(1, m + 1)) - exact).max()))
        print("m %d: ascending %.1e, factor_order %.1e" % (m, worst_asc, worst))
        assert worst_asc > lost and worst < kept
    assert L.factor_order(1) == [1] and L.factor_order(2) == [1, 2] and L.factor_order(7) == [1, 2, 5, 6, 3, 4, 7]


def test_closed_forms_at_orders_1_and_2():
    w1 = 0.7
    assert abs(L.lsp2lpc([w1])[1] - (-math.cos(w1))) < 1e-16
    # m = 2: P = f_1 (1 + z^-1), Q = f_2 (1 - z^-1): a_1 = -(cos w_1 + cos w_2), a_2 = 1 - cos w_1 + cos w_2
    w1, w2 = 0.9, 2.1
    a = L.lsp2lpc([w1, w2])
    assert abs(a[1] + (math.cos(w1) + math.cos(w2))) < 1e-15 and abs(a[2] - (1 - math.cos(w1) + math.cos(w2))) < 1e-15


@pytest.mark.parametrize("m", [3, 34])
def test_conversion_towards_gamma_1_is_the_impulse_response_of_k_over_a(m):
    """At alpha 0, gamma -1 step 3 towards (L - 1, 0, 1) gives c2[k] = h[k] of K / A(z) for k >= 1 and c2[0] = K - 1."""
    n = 256
    K = 0.37
    row = np.concatenate([[K], valid_set(m, 7)])
    lpc, checked, st = L.to_lpc(row)
    assert st == 0 and lpc[0] == K and (checked == row).all()
    c2 = L.lpc_to_mgc(lpc, 0.0, -1.0, n - 1, 0.0, 1.0)
    h = np.zeros(n)
    for t in range(n):
        acc = K if t == 0 else 0.0
        for k in range(1, min(t, m) + 1):
            acc -= lpc[k] * h[t - k]
        h[t] = acc
    assert abs(c2[0] - (K - 1)) < 1e-15
    assert np.abs(c2[1:] - h[1:]).max() < 1e-10 * np.abs(h).max()
    # and through the general entry of the restatement, a row at a time
    opt = M.option(m, 0.0, -1.0, n - 1, 0.0, 1.0, n=1, u=1)
    assert (M.convert_rows(lpc[None], opt)[0] == c2).all()
    # the energy is that of the response with its first sample less one
    want = 0.5 * math.log((K - 1) ** 2 + math.fsum(v * v for v in h[1:]))
    assert abs(L.energy(lpc, 0.0, -1.0, n) - want) < 1e-12


def test_check_step_on_hand_computed_rows():
    m, r = 4, 0.1
    d = np.float64(0.1) * np.float64(PI) / np.float64(5)
    assert L.distance(m, r) == d
    spaced = np.array([2.0, 0.5, 1.0, 1.5, 2.0])
    got, K, st = L.check(spaced, r)
    assert st == 0 and K == 2.0 and got.tobytes() == spaced.tobytes()
    # exactly d apart is far enough
    edge = np.array([2.0, 0.5, 0.5 + 2 * d, 1.5, 2.0])
    edge[1] = edge[2] - d
    if edge[2] - edge[1] >= d:
        got, _, st = L.check(edge, r)
        assert st == 0 and got.tobytes() == edge.tobytes()
    # reflected: a negative value and one beyond pi
    big = 2 * PI - 2.0
    got, _, st = L.check([2.0, -0.5, 1.0, 1.5, big], r)
    assert st == 1 and (got == [2.0, 0.5, 1.0, 1.5, 2 * np.float64(PI) - np.float64(big)]).all()
    # swapped
    got, _, st = L.check([2.0, 1.0, 0.5, 1.5, 2.0], r)
    assert st == 1 and (got == spaced).all()
    # too close: the pair is moved apart by half of what is missing, each
    lo, hi = np.float64(0.5), np.float64(0.51)
    s = np.float64(0.5) * (d - (hi - lo))
    got, _, st = L.check([2.0, lo, hi, 1.5, 2.0], r)
    assert st == 1 and (got == [2.0, lo - s, hi + s, 1.5, 2.0]).all() and abs((got[2] - got[1]) - d) < 1e-15
    # a later step sees what an earlier one left: three values close together
    a, b, c = np.float64(0.5), np.float64(0.52), np.float64(0.53)
    s1 = np.float64(0.5) * (d - (b - a))
    b1 = b + s1
    s2 = np.float64(0.5) * (d - (c - b1))
    got, _, st = L.check([2.0, a, b, c, 2.0], r)
    assert st == 1 and (got == [2.0, a - s1, b1 - s2, c + s2, 2.0]).all()
    # the single pass guarantees nothing: a pair near 0 is moved below it
    got, _, st = L.check([2.0, 0.001, 0.002, 1.5, 2.0], r)
    assert st == 1 | 16 and got[1] < 0
    # r = 0 moves nothing, equal values stay equal and are flagged
    got, _, st = L.check([2.0, 0.5, 0.5, 1.5, 2.0], 0.0)
    assert st == 16 and (got == [2.0, 0.5, 0.5, 1.5, 2.0]).all()
    # the gain, in both forms
    got, K, st = L.check([1e-12, 0.5, 1.0, 1.5, 2.0], r, 1e-10, False)
    assert st == 2 and K == 1e-10 and got[0] == 1e-10
    got, K, st = L.check([-30.0, 0.5, 1.0, 1.5, 2.0], r, 1e-10, True)
    assert st == 2 and K == 1e-10 and got[0] == math.log(1e-10)
    got, K, st = L.check([-3.0, 0.5, 1.0, 1.5, 2.0], r, 1e-10, True)
    assert st == 0 and K == np.exp(-3.0) and got[0] == -3.0
    # a non-finite value
    got, K, st = L.check([2.0, 0.5, np.nan, 1.5, 2.0], r)
    assert st == 4 and (got == 0).all()
    lpc, chk, st = L.to_lpc([2.0, 0.5, np.inf, 1.5, 2.0], r)
    assert st == 4 and (lpc == 0).all() and (chk == 0).all()


def test_filter_step():
    x = np.concatenate([[0.8], valid_set(9, 3)])
    assert L.filter_row(x, 1.0)[0] == x[0] and np.abs(L.filter_row(x, 1.0) - x).max() < 1e-15    # beta 1: p[i] = w[i]
    out, e1, e2, st = L.postfilter(x, 0.55, -1 / 3, 1.0, 64, compensation=True)
    assert st == 0 and out.tobytes() == x.tobytes() and e1 == 0 and e2 == 0                      # and the call copies
    p = L.filter_row(x, 0.7)
    assert p[0] == x[0] and p[1] == x[1] and p[9] == x[9] and (p[2:9] != x[2:9]).all()
    i = 4
    d1, d2 = 0.7 * (x[i + 1] - x[i]), 0.7 * (x[i] - x[i - 1])
    assert p[i] == x[i - 1] + d2 + (d2 * d2 * ((x[i + 1] - x[i - 1]) - (d1 + d2))) / ((d2 * d2) + (d1 * d1))
    # the filter moves an LSP towards its nearer neighbour: formants sharpen
    assert ((p[2:9] - x[2:9]) * ((x[3:10] - x[2:9]) - (x[2:9] - x[1:8])) < 0).all()
    # three equal values: Perl would divide by zero, the row keeps the value
    y = x.copy()
    y[4] = y[5] = y[6]
    q = L.filter_row(y, 0.7)
    assert np.isfinite(q).all() and q[5] == y[5]
    # m <= 2 is the identity
    out, _, _, st = L.postfilter([0.8, 1.0, 2.0], 0.55, -1 / 3, 0.7, 64)
    assert st == 0 and (out == [0.8, 1.0, 2.0]).all()
    # compensation 0: the gain's bits; compensation 1: the energy difference, in both gain forms
    plain, _, _, st = L.postfilter(x, 0.55, -1 / 3, 0.7, 64)
    assert st == 0 and plain[0] == x[0] and (plain[1:] == p[1:]).all()
    lin, e1, e2, st = L.postfilter(x, 0.55, -1 / 3, 0.7, 64, compensation=True)
    assert st == 0 and e1 != e2 and lin[0] == x[0] * np.exp(e1 - e2)
    xl = x.copy()
    xl[0] = math.log(x[0])
    log, f1, f2, st = L.postfilter(xl, 0.55, -1 / 3, 0.7, 64, log_gain=True, compensation=True)
    assert st == 0 and log[0] == xl[0] + (f1 - f2) and abs((f1 - f2) - (e1 - e2)) < 1e-12


FIELDS = ("order", "alpha", "gamma", "log_gain", "min_distance", "min_gain")
PF_FIELDS = FIELDS + ("beta", "length", "compensation")


def test_abi_declared_exported_with_defaults_and_layout(pkg):
    text = open(os.path.join(ROOT, "include", "world_mi355.h")).read()
    for name in ("int WorldMi355LspToLpc", "int WorldMi355LspToMelGeneralizedCepstrum", "int WorldMi355LspPostfilter",
                 "void WorldMi355DefaultLspOption", "void WorldMi355DefaultLspPostfilterOption"):
        assert re.search(r"\b%s\s*\(" % name.replace(" ", r"\s+"), text), name
    assert "PARITY WITH SPTK'S COMMANDS IS UNPINNED" in text and "tests/lsp_reference.py" in text and '"lsp_kernel"' in text
    assert "Not offered: LSP in either direction" not in text and "the LSP postfilter (:2690-2752) are not offered" not in text
    from importlib import import_module
    mod = import_module(pkg.__name__ + ".lsp")
    lib = pkg.load_library()
    kinds = {ctypes.c_int: "int", ctypes.c_double: "double"}
    for cname, O, names, default, want in (
            ("WorldMi355LspOption", mod.LspOption, FIELDS, "WorldMi355DefaultLspOption", (25, 0.35, -1.0, 0, 0.1, 1e-10)),
            ("WorldMi355LspPostfilterOption", mod.LspPostfilterOption, PF_FIELDS, "WorldMi355DefaultLspPostfilterOption",
             (25, 0.35, -1.0, 0, 0.1, 1e-10, 0.7, 4096, 0))):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % cname, text).group(1)
        fields = re.findall(r"\b(int|double)\s+(\w+);", body)
        assert tuple(f for _, f in fields) == names
        assert [(n, kinds[t]) for n, t in O._fields_] == [(f, t) for t, f in fields]
        o = O()
        getattr(lib, default)(ctypes.byref(o))
        assert tuple(getattr(o, f) for f in names) == want
        getattr(lib, default)(None)                                   # a null option struct is left alone
    O, P = mod.LspOption, mod.LspPostfilterOption
    assert ctypes.sizeof(O) == 48 and (O.alpha.offset, O.log_gain.offset, O.min_distance.offset, O.min_gain.offset) == (8, 24, 32, 40)
    assert ctypes.sizeof(P) == 64 and (P.beta.offset, P.length.offset, P.compensation.offset) == (48, 56, 60)
    assert O is pkg.world.LspOption and P is pkg.world.LspPostfilterOption
    for f in ("lsp_to_lpc", "lsp_to_mel_generalized_cepstrum", "postfilter_lsp"):
        assert callable(getattr(mod, f)) and f not in vars(pkg.world.WorldBatch)
    assert "lsp.hip" in open(os.path.join(ROOT, "hts-train-world_amd", "csrc", "Makefile")).read()
    import ast
    tree = ast.parse(open(mod.__file__).read())
    assert not [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Assert)]


def test_every_refusal_without_a_device(pkg):
    """No context, no batch, no device memory: WM_ERR_BAD_ARG (2) from the host alone; the pointers are never followed."""
    lib = pkg.load_library()
    O, P = pkg.world.LspOption, pkg.world.LspPostfilterOption
    a, b, c, d, e = (ctypes.c_void_p(k << 20) for k in (1, 2, 3, 4, 5))
    good = dict(order=34, alpha=0.55, gamma=-1 / 3, log_gain=1, min_distance=0.1, min_gain=1e-10)
    pf = dict(good, beta=0.7, length=4096, compensation=1)
    nan, inf = float("nan"), float("inf")
    bad = [dict(order=0), dict(order=64), dict(order=-1), dict(alpha=1.0), dict(alpha=-1.0), dict(alpha=nan),
           dict(gamma=0.0), dict(gamma=-1.01), dict(gamma=0.5), dict(gamma=nan), dict(min_distance=-0.1),
           dict(min_distance=1.1), dict(min_distance=nan), dict(min_gain=0.0), dict(min_gain=-1.0), dict(min_gain=inf),
           dict(min_gain=nan)]
    for over in bad:
        o = O(**dict(good, **over))
        assert lib.WorldMi355LspToLpc(None, a, ctypes.byref(o), b, None, None) == 2, over
        assert lib.WorldMi355LspToMelGeneralizedCepstrum(None, a, ctypes.byref(o), 34, 0.55, -1 / 3, b, c) == 2, over
        p = P(**dict(pf, **over))
        assert lib.WorldMi355LspPostfilter(None, a, ctypes.byref(p), b, None, None, c) == 2, over
    for over in (dict(beta=nan), dict(beta=inf), dict(length=32), dict(length=8192), dict(length=100), dict(length=0)):
        p = P(**dict(pf, **over))
        assert lib.WorldMi355LspPostfilter(None, a, ctypes.byref(p), b, None, None, c) == 2, over
    o, p = O(**good), P(**pf)
    assert lib.WorldMi355LspToLpc(None, None, ctypes.byref(o), b, None, None) == 2
    assert lib.WorldMi355LspToLpc(None, a, None, b, None, None) == 2
    assert lib.WorldMi355LspToLpc(None, a, ctypes.byref(o), None, None, None) == 2
    assert lib.WorldMi355LspToMelGeneralizedCepstrum(None, a, ctypes.byref(o), 34, 0.55, -1 / 3, None, c) == 2
    assert lib.WorldMi355LspToMelGeneralizedCepstrum(None, a, ctypes.byref(o), 34, 0.55, -1 / 3, b, None) == 2
    for m2, a2, g2 in ((0, 0.55, -0.5), (4096, 0.55, -0.5), (34, 1.0, -0.5), (34, 0.55, 1.5)):      # mgc2mgc's own rules
        assert lib.WorldMi355LspToMelGeneralizedCepstrum(None, a, ctypes.byref(o), m2, a2, g2, b, c) == 2
    assert lib.WorldMi355LspPostfilter(None, None, ctypes.byref(p), b, None, None, c) == 2
    assert lib.WorldMi355LspPostfilter(None, a, ctypes.byref(p), None, None, None, c) == 2
    assert lib.WorldMi355LspPostfilter(None, a, ctypes.byref(p), b, None, None, None) == 2
    assert lib.WorldMi355LspPostfilter(None, a, None, b, None, None, c) == 2
    # sound arguments get as far as the missing batch
    assert lib.WorldMi355LspToLpc(None, a, ctypes.byref(o), b, c, d) == 2
    assert lib.WorldMi355LspPostfilter(None, a, ctypes.byref(p), a, d, e, c) == 2


def test_bad_tensors_are_refused_before_the_library(pkg):
    import torch
    import test_world_arguments_host as A
    from importlib import import_module
    mod = import_module(pkg.__name__ + ".lsp")
    W = pkg.world
    pkg.load_library()
    b = W.WorldBatch.__new__(W.WorldBatch)                          # a batch made by hand, as that file makes its own
    b.handle, b.ctx, b.total_frames, b.device = None, None, A.TF, torch.device("cpu")
    for fn, kw in ((mod.lsp_to_lpc, {}), (mod.lsp_to_mel_generalized_cepstrum, dict(alpha=0.55, gamma=-0.5)),
                   (mod.postfilter_lsp, dict(alpha=0.55, gamma=-0.5))):
        kwargs = dict(lsp=A.z(A.F64, A.TF, 35), **kw)
        n = A.refusals(lambda **k: fn(b, **k), fn.__name__, kwargs, [A.arg("lsp", free=(1,))])
        assert n >= 4
    with pytest.raises(ValueError, match="postfilter_lsp: out"):
        mod.postfilter_lsp(b, A.z(A.F64, A.TF, 35), 0.55, -0.5, out=A.z(A.F64, A.TF, 34))


def test_recipe_refusals_come_before_any_file_is_read(pkg, tmp_path):
    rec = pkg.recipe
    jobs = [(str(tmp_path / "missing.mgc"), str(tmp_path / "out.c_mgc"))]
    good = dict(order=34, alpha=0.55, gamma=-1 / 3)
    for bad in (dict(order=0), dict(order=64), dict(alpha=1.0), dict(gamma=0.0), dict(gamma=-1.5), dict(gamma=0.5),
                dict(out_order=0), dict(out_alpha=-1.0), dict(out_gamma=2.0), dict(out_order=4096)):
        with pytest.raises(ValueError):
            rec.lsp2mgc_files(jobs, **dict(good, **bad))
    for bad in (dict(order=64), dict(alpha=-1.0), dict(gamma=0.0), dict(beta=float("nan")), dict(beta=float("inf")),
                dict(length=32), dict(length=8192), dict(length=1000)):
        with pytest.raises(ValueError):
            rec.postfilter_lsp_files(jobs, **dict(good, **bad))
    scp = tmp_path / "jobs.scp"
    scp.write_text("%s %s\n" % jobs[0])
    base = ["--scp", str(scp), "--order", "34", "--alpha", "0.55"]
    for argv in (["lsp2mgc"] + base + ["--gamma", "0"], ["lsp2mgc"] + base + ["--gamma", "-0.5", "--out-gamma", "3"],
                 ["postfilter-lsp"] + base + ["--gamma", "-0.5", "--length", "100"],
                 ["postfilter-lsp"] + base + ["--gamma", "0.25"], ["lsp2mgc"] + base):
        with pytest.raises(SystemExit):
            rec.main(argv)
    assert not os.path.exists(jobs[0][1])

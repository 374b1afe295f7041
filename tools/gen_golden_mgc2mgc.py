#!/usr/bin/env python3
"""Writes tests/golden/sptk_mgc2mgc.npz: mel-generalized cepstra and what the COMPILED reference's mgc2mgc, gnorm and
ignorm (test/sptkfunctions.cpp:221-254, :313-345, built by oracle/Makefile into oracle/_ref/libsptk_ref.so) make of
them, for tests/test_mgc2mgc_host.py and tests/test_gpu_mgc2mgc*.py.

    make -C oracle ref && python tools/gen_golden_mgc2mgc.py

The port keeps static buffers sized at first use, so every option set runs in a child process of its own (this file
with --child).  Only data is stored: options, input rows, the reference's outputs, status.

An option set is WorldMi355MgcConvertOption's fields (tests/mgc2mgc_reference.py: option()).  Its inputs: 12 seeded
rows c[k] = N(0, 1) / (1 + k) with c0 uniform in [-3, 3] at gamma 0 (the two largest sets: the first 2 of them),
brought to (alpha 1, gamma 1) by the reference's own mgc2mgc(row, m1, alpha 1, 0 -> m1, alpha 1, gamma 1), which keeps
1 + gamma 1 c0 > 0 (asserted); for a flagged input, then the compiled gnorm (-n) and plain arithmetic (-u).  No
candidate is left out.  The reference's output: the compiled ignorm and plain arithmetic for -n / -u, the compiled
mgc2mgc, the compiled gnorm and plain arithmetic for -N / -U -- include/world_mi355.h's definition with the compiled
pieces (flag semantics unpinned against SPTK's command).  Every output is finite (asserted).

Per option set (`key`, OPTIONS below):
  <key>/opt     the ten fields as float64
  <key>/in      [rows][m1+1]   the rows given to the conversion
  <key>/out     [rows][m2+1]   the reference's result
  <key>/sens    [rows]         the larger of (a) max |change| of the reference's result when its input is multiplied by
                               1 + 4 * 2^-52 * xi, xi uniform in [-1, 1] (seeded), and (b) max |reference - the same
                               chain in np.longdouble| (tests/mgc2mgc_reference.py): the reference's own rounding error,
                               which is what a reordered gc2gc sum differs by
  <key>/sens_ab [rows][2]      the two figures apart
The status case S: four rows of which row 1 has 1 + gamma 1 c0 < 0 and row 3 a NaN coefficient; S/status is
[0, 1, 0, 1], S/out holds zeros in the flagged rows (what the library writes), the reference's values elsewhere.
Also prints the compiled reference's one-thread rate for the three calls of tools/mgc2mgc_rate.py (a record for
DESIGN.md).
"""
import ctypes
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mgc2mgc_reference as R  # noqa: E402

LIB = os.path.join(ROOT, "oracle", "_ref", "libsptk_ref.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")
PATH = os.path.join(GOLDEN, "sptk_mgc2mgc.npz")
PERTURB_SEED = 20241                                   # as tools/gen_golden_mgc2sp.py
N_ROWS = 12
G3 = -1.0 / 3.0

# key -> (option set, rows)
OPTIONS = {
    "c24_g0_to_g3": (R.option(24, .42, 0, 24, .42, G3), N_ROWS),
    "c24_g3_to_g0": (R.option(24, .42, G3, 24, .42, 0), N_ROWS),
    "c24_g3_to_m63": (R.option(24, .55, G3, 63, .55, G3), N_ROWS),
    "c8_g0_to_g1p": (R.option(8, 0, 0, 8, 0, 1), N_ROWS),
    "c1_g1_to_a30": (R.option(1, 0, -1, 1, .3, 0), N_ROWS),
    "c24_g3_to_an30_g1": (R.option(24, .42, G3, 24, -.3, -1), N_ROWS),
    "c49_g1_to_m63_a55_g3": (R.option(49, .42, -1, 63, .55, G3), N_ROWS),
    "c63_g1_to_g1p": (R.option(63, .55, -1, 63, .55, 1), N_ROWS),
    "c24_g0_to_m64_a0": (R.option(24, .42, 0, 64, 0, 0), N_ROWS),
    "c24_g3_to_m65_a0": (R.option(24, .42, G3, 65, 0, G3), N_ROWS),
    "c24_g3_to_m127_a0_g1p": (R.option(24, .55, G3, 127, 0, 1), N_ROWS),
    "c24_g3_to_m128_a10_g2": (R.option(24, .42, G3, 128, .1, -.5), N_ROWS),
    "c24_g2_to_m200_g4": (R.option(24, 0, -.5, 200, 0, -.25), N_ROWS),
    "c127_g0_to_m24_a42": (R.option(127, 0, 0, 24, .42, 0), N_ROWS),
    "c2047_g0_to_m24_a55_g3": (R.option(2047, 0, 0, 24, .55, G3), N_ROWS),
    "c24_g2_to_m2047_a0_g1p": (R.option(24, .55, -.5, 2047, 0, 1), 2),
    "c34_g3_to_m4095_a0_g1p": (R.option(34, .55, G3, 4095, 0, 1), 2),
    # the flags, on (24, .55, -1/3 -> 24, .55, -1/3)
    "f_nu": (R.option(24, .55, G3, 24, .55, G3, n=1, u=1), N_ROWS),                  # gen_wave's call
    "f_u": (R.option(24, .55, G3, 24, .55, G3, u=1), N_ROWS),
    "f_N": (R.option(24, .55, G3, 24, .55, G3, N=1), N_ROWS),
    "f_NU": (R.option(24, .55, G3, 24, .55, G3, N=1, U=1), N_ROWS),
    "f_U": (R.option(24, .55, G3, 24, .55, G3, U=1), N_ROWS),
    "f_nu_to_m127_a0_g1p": (R.option(24, .55, G3, 127, 0, 1, n=1, u=1), N_ROWS),     # postfiltering_lsp's call
}
GEN_WAVE, PARITY_STREAM = "f_nu", "c24_g3_to_m65_a0"
STATUS_OPT = R.option(24, .42, G3, 24, -.3, 0)      # towards gamma 0: the reference takes the log of a negative gain
STATUS = (0, 1, 0, 1)
# the three calls whose rate tools/mgc2mgc_rate.py measures on the device
RATE_CALLS = (("gen_wave", R.option(34, .55, G3, 34, .55, G3, n=1, u=1)),
              ("gamma_change_m49", R.option(49, .42, -1, 49, .42, G3)),
              ("postfiltering_lsp_2047", R.option(34, .55, G3, 2047, 0, 1, n=1, u=1)))


def seed_of(opt):
    m1, a1, g1 = opt[0], opt[1], opt[2]
    return 300000 + m1 * 131 + int(round((a1 + 1.0) * 100)) + int(round((g1 + 1.0) * 12)) * 7919


def candidates(opt, rows=N_ROWS):
    """The seeded rows at gamma 0 and order m1."""
    m1 = opt[0]
    rs = np.random.RandomState(seed_of(opt))
    c = rs.randn(N_ROWS, m1 + 1) / (1.0 + np.arange(m1 + 1))
    c[:, 0] = rs.uniform(-3.0, 3.0, N_ROWS)
    return c[:rows]


def perturb(c):
    xi = np.random.RandomState(PERTURB_SEED).uniform(-1.0, 1.0, c.shape)
    return c * (1.0 + 4.0 * 2.0 ** -52 * xi)


def symbol(name):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = [ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("_Z%d%sP" % (len(name), name))]
    assert len(names) == 1, (name, names)
    return names[0]


class Compiled:
    """mgc2mgc, gnorm and ignorm of libsptk_ref.so, and the conversion with its flags made of them."""

    def __init__(self):
        lib = ctypes.CDLL(LIB)
        self.dp = dp = ctypes.POINTER(ctypes.c_double)
        ci, cd = ctypes.c_int, ctypes.c_double
        self._mgc2mgc = getattr(lib, symbol("mgc2mgc"))
        self._mgc2mgc.restype = None
        self._mgc2mgc.argtypes = [dp, ci, cd, cd, dp, ci, cd, cd]
        self._gnorm = getattr(lib, symbol("gnorm"))
        self._ignorm = getattr(lib, symbol("ignorm"))
        for f in (self._gnorm, self._ignorm):
            f.restype = None
            f.argtypes = [dp, dp, ci, cd]

    def mgc2mgc(self, c, m1, a1, g1, m2, a2, g2):
        src, dst = np.ascontiguousarray(c, dtype=np.float64), np.zeros(m2 + 1)
        self._mgc2mgc(src.ctypes.data_as(self.dp), m1, a1, g1, dst.ctypes.data_as(self.dp), m2, a2, g2)
        return dst

    def _norm(self, f, c, m, g):
        src, dst = np.ascontiguousarray(c, dtype=np.float64), np.zeros(m + 1)
        f(src.ctypes.data_as(self.dp), dst.ctypes.data_as(self.dp), m, g)
        return dst

    def gnorm(self, c, m, g):
        return self._norm(self._gnorm, c, m, g)

    def ignorm(self, c, m, g):
        return self._norm(self._ignorm, c, m, g)

    def flagged_input(self, plain, opt):
        """The row a caller holds under -n / -u whose plain form is `plain`."""
        m1, _, g1, n, u = opt[:5]
        c = plain.copy()
        if n:
            c = self.gnorm(c, m1, g1)
        elif u:
            c[0] = c[0] * g1 + 1.0
        if u:
            c[1:] = c[1:] * g1
        return c

    def convert(self, c, opt):
        m1, a1, g1, n, u, m2, a2, g2, N, U = opt
        c = np.array(c, dtype=np.float64)
        if n:
            c = self.ignorm(c, m1, g1)
        elif u:
            c[0] = (c[0] - 1.0) / g1
        if u:
            c[1:] = c[1:] / g1
        c = self.mgc2mgc(c, m1, a1, g1, m2, a2, g2)
        if N:
            c = self.gnorm(c, m2, g2)
        elif U:
            c[0] = c[0] * g2 + 1.0
        if U:
            c[1:] = c[1:] * g2
        return c

    def convert_rows(self, rows, opt):
        return np.stack([self.convert(r, opt) for r in rows])


def child(spec_path, out_path):
    z = np.load(spec_path, allow_pickle=False)
    opt = R.option(*[z["opt"][i] for i in (0, 1, 2, 5, 6, 7, 3, 4, 8, 9)])
    m1, a1, g1 = opt[:3]
    ref = Compiled()
    res = {}
    if "rows_in" in z.files:
        rows = z["rows_in"].copy()
    else:
        plain = np.stack([ref.mgc2mgc(r, m1, a1, 0.0, m1, a1, g1) if g1 != 0.0 else r.copy() for r in z["base"]])
        res["plain"] = plain
        rows = np.stack([ref.flagged_input(r, opt) for r in plain])
    if "override" in z.files:                                    # the status case: values set after the conversion
        for r, k, v in z["override"]:
            rows[int(r), int(k)] = v
    res["in"] = rows
    res["out"] = ref.convert_rows(rows, opt)
    res["outp"] = ref.convert_rows(perturb(rows), opt)
    n_rate = int(z["rate_rows"])
    if n_rate:
        many = np.tile(rows, (n_rate // len(rows) + 1, 1))[:n_rate]
        t0 = time.perf_counter()
        for r in many:
            ref.convert(r, opt)
        res["secs_per_row"] = (time.perf_counter() - t0) / n_rate
    np.savez(out_path, **res)


def run_child(opt, base=None, rows_in=None, override=None, rate_rows=0):
    with tempfile.TemporaryDirectory() as d:
        spec, out = os.path.join(d, "spec.npz"), os.path.join(d, "out.npz")
        extra = {}
        if base is not None:
            extra["base"] = base
        if rows_in is not None:
            extra["rows_in"] = rows_in
        if override is not None:
            extra["override"] = np.asarray(override, dtype=np.float64)
        np.savez(spec, opt=np.asarray(opt, dtype=np.float64), rate_rows=rate_rows, **extra)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", spec, out], check=True)
        z = np.load(out)
        return {k: z[k] for k in z.files}


def sens_of(r, opt, rows=None):
    """[rows][2]: figures (a) and (b) per row."""
    sel = slice(None) if rows is None else rows
    ld = R.convert_rows(r["in"][sel], opt, R.LD)
    a = np.abs(r["outp"][sel] - r["out"][sel]).max(axis=1)
    b = np.abs(r["out"][sel] - ld).max(axis=1).astype(np.float64)
    return np.stack([a, b], axis=1)


def main():
    assert os.path.exists(LIB), "run `make -C oracle ref` first"
    store = {"perturb_seed": PERTURB_SEED, "keys": np.asarray(sorted(OPTIONS))}
    for key in sorted(OPTIONS):
        opt, rows = OPTIONS[key]
        r = run_child(opt, base=candidates(opt, rows))
        g1 = opt[2]
        assert np.isfinite(r["in"]).all() and np.isfinite(r["out"]).all(), key
        assert (1.0 + g1 * r["plain"][:, 0] > 0).all(), key
        ab = sens_of(r, opt)
        store[key + "/opt"] = np.asarray(opt, dtype=np.float64)
        store[key + "/in"], store[key + "/out"] = r["in"], r["out"]
        store[key + "/sens_ab"], store[key + "/sens"] = ab, ab.max(axis=1)
        peak = np.abs(r["out"]).max(axis=1)
        print("%-24s max|c2| %6.2f  sens (a) %.1e (b) %.1e  worst sens / ulp(max|row|) %.1f" % (
            key, peak.max(), ab[:, 0].max(), ab[:, 1].max(), (ab.max(axis=1) / np.spacing(peak)).max()), flush=True)
    # ---- the status case ----
    base = candidates(STATUS_OPT, 4)
    r = run_child(STATUS_OPT, base=base, override=[(1, 0, 40.0), (3, 5, np.nan)])
    good = np.asarray(STATUS) == 0
    g1 = STATUS_OPT[2]
    assert 1.0 + g1 * r["in"][1, 0] < 0 and np.isnan(r["in"][3, 5]) and np.isfinite(r["in"][good]).all()
    assert not np.isfinite(r["out"][1]).all() and not np.isfinite(r["out"][3]).all() and np.isfinite(r["out"][good]).all()
    ab = np.zeros((4, 2))
    ab[good] = sens_of(r, STATUS_OPT, rows=good)
    out = r["out"].copy()
    out[~good] = 0.0
    store.update({"S/opt": np.asarray(STATUS_OPT, dtype=np.float64), "S/in": r["in"], "S/out": out,
                  "S/status": np.asarray(STATUS, dtype=np.int32), "S/sens_ab": ab, "S/sens": ab.max(axis=1)})
    print("S: status %s  sens %.1e" % (list(STATUS), ab.max()))
    np.savez_compressed(PATH, **store)
    size = os.path.getsize(PATH)
    print("wrote %s (%d bytes)" % (PATH, size))
    assert size < 1 << 20, "over the size limit for a committed file: store fewer rows"
    # ---- the reference's one-thread rate (a record, not a fixture) ----
    for name, opt in RATE_CALLS:
        n = 20000 if opt[5] < 64 else 40
        r = run_child(opt, base=candidates(opt), rate_rows=n)
        print("reference %s %s: %.3e rows/s on one thread (%d rows, the ctypes call included)" % (
            name, opt, 1.0 / float(r["secs_per_row"]), n))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main()

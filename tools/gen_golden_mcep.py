#!/usr/bin/env python3
"""Writes tests/golden/sptk_mcep.npz: inputs and the COMPILED reference's outputs of SPTK's mcep
(test/sptkfunctions.cpp:11-184, built by oracle/Makefile into oracle/_ref/libsptk_ref.so), for
tests/test_mel_cepstrum_host.py and tests/test_gpu_mel_cepstrum.py.

    make -C oracle ref && python tools/gen_golden_mcep.py

mcep keeps static buffers and calls exit() where it fails, so every job runs in a child process (this file with
--child), always with flng = fft_size.  Only data is stored: inputs, their seeds, and what the reference returned.

Per case and option set (`key`):
  <key>/fixed        [4][frames][m+1]  dd = 0: exactly itr2 = 0, 1, 2, 5 Newton steps
  <key>/conv         [frames][m+1]     SPTK's defaults itr1 2, itr2 30, dd 1e-3
  <key>/ret          [frames]          mcep's return value of that run (0 / -1)
  <key>/robust       [frames]          the runs at dd 0.99e-3 and 1.01e-3 return the same row and value
  <key>/sens_fixed   [4], <key>/sens_conv   max |d mc| when the input is multiplied by 1 + 4 * 2^-52 * xi, xi uniform in
                                       [-1, 1] (seeded): the size of last-bit differences between transforms / libm
At least 90 % of the frames of every key must be robust, or this script fails.
The option set A_m8_a42_short runs its convergence mode with itr2 = 4: some frames meet dd by then and some run out of
steps, so -1 is also recorded where dd > 0 decides (in the fixed mode it follows from dd = 0).
Case D holds what makes the reference exit: a row with an exact 0 (status 2) and, with f = 1e6, theq's singular pivot
at the first step of every frame (status 1; a flat spectrum with a large f: found on the CPU, see d_fail below).
D/sens_conv and D/sens_init are its own perturbation figures (the rows differ from case A's).
Also prints the one-thread rate of the compiled reference at F = 1024, m = 24 and 49 (a record for DESIGN.md).
"""
import ctypes
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oracle", "_ref", "libsptk_ref.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXED_ITR = (0, 1, 2, 5)
DD = 1e-3
PERTURB_SEED = 20240
SHORT_ITR2 = 4                                                   # the convergence run of the `_short` option set

# key -> (case, m, alpha, extra options)
OPTIONS = {}
for _m in (1, 8, 24):
    for _a in (0.0, 0.42, 0.55):
        OPTIONS["A_m%d_a%02d" % (_m, round(_a * 100))] = ("A", _m, _a, {})
OPTIONS["B_cli"] = ("B", 24, 0.55, {"etype": 1, "e": 1e-8})      # analysis.cpp:340-342 with a usable flng / itr2
OPTIONS["B_m49"] = ("B", 49, 0.42, {})
OPTIONS["B_m49_pow"] = ("B2", 49, 0.42, {"itype": 4})            # the same rows squared, as periodograms
OPTIONS["C_m63"] = ("C", 63, 0.55, {})
OPTIONS["A_m8_a42_short"] = ("A", 8, 0.42, {"itr2": SHORT_ITR2})  # dd 1e-3 met by some frames only: -1 under dd > 0
CASE_SEEDS = {"A": 11, "C": 5}
CASE_SHAPE = {"A": (512, 24), "B": (1024, 24), "B2": (1024, 24), "C": (2048, 8), "D": (512, 4)}
A_UTTERANCES = (1, 6, 17)
B_SP_ROWS = (0, 2, 4, 6, 8, 10, 12, 14)                          # of world_16k_short.npz's sp_sub; then all of 1e4 * ap_sub


def smooth_spectra(seed, frames, fft_size):
    """Smooth positive amplitude spectra: exp of six random low-order cosines, dynamic range 60 dB."""
    rs = np.random.RandomState(seed)
    k = np.arange(fft_size // 2 + 1) / (fft_size // 2)
    out = np.empty((frames, fft_size // 2 + 1))
    for f in range(frames):
        w = rs.randn(6) / (1.0 + np.arange(6))
        lg = sum(w[i] * np.cos(np.pi * (i + 1) * k) for i in range(6))
        lg *= (60.0 / 20.0 * np.log(10.0)) / (lg.max() - lg.min())
        out[f] = np.exp(lg + rs.uniform(-2.0, 2.0))
    return out


def case_b_rows():
    z = np.load(os.path.join(GOLDEN, "world_16k_short.npz"))
    return np.concatenate([z["sp_sub"][list(B_SP_ROWS)], 1e4 * z["ap_sub"]])


def case_d_rows():
    x = smooth_spectra(3, 4, 512)
    x[1, 5] = 0.0                                                # status 2
    return x


def case_input(case):
    if case in ("A", "C"):
        F, n = CASE_SHAPE[case]
        return smooth_spectra(CASE_SEEDS[case], n, F)
    if case == "B":
        return case_b_rows()
    if case == "B2":
        return case_b_rows() ** 2
    return case_d_rows()


def perturb(x):
    xi = np.random.RandomState(PERTURB_SEED).uniform(-1.0, 1.0, x.shape)
    return x * (1.0 + 4.0 * 2.0 ** -52 * xi)


def mcep_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = [ln.split()[-1] for ln in out.splitlines() if ln.split() and "mcep" in ln.split()[-1]]
    assert len(names) == 1, names
    return names[0]


def child(spec_path, out_path):
    """Runs the jobs of spec_path in this process; a failing mcep ends it with the reference's exit status."""
    z = np.load(spec_path, allow_pickle=False)
    x, jobs = z["x"], z["jobs"]                                  # jobs: [itr1, itr2, dd, m, alpha, etype, e, f, itype]
    F = int(z["fft_size"])
    lib = ctypes.CDLL(LIB)
    fn = getattr(lib, mcep_symbol())
    dp = ctypes.POINTER(ctypes.c_double)
    fn.restype = ctypes.c_int
    fn.argtypes = [dp, ctypes.c_int, dp, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                   ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int]
    m_max = int(jobs[:, 3].max())
    mc = np.zeros((len(jobs), len(x), m_max + 1))
    ret = np.zeros((len(jobs), len(x)), dtype=np.int32)
    secs = np.zeros(len(jobs))
    buf = np.zeros(F)
    for j, (itr1, itr2, dd, m, alpha, etype, e, f, itype) in enumerate(jobs):
        t0 = time.perf_counter()
        for i, row in enumerate(x):
            buf[:] = 0.0
            buf[:F // 2 + 1] = row
            o = np.zeros(int(m) + 1)
            ret[j, i] = fn(buf.ctypes.data_as(dp), F, o.ctypes.data_as(dp), int(m), float(alpha), int(itr1), int(itr2),
                           float(dd), int(etype), float(e), float(f), int(itype))
            mc[j, i, :int(m) + 1] = o
        secs[j] = time.perf_counter() - t0
    np.savez(out_path, mc=mc, ret=ret, secs=secs)


def run_child(x, F, jobs):
    """(mc [jobs][frames][m+1], ret, secs), or (None, exit status, stderr) when the reference exits."""
    with tempfile.TemporaryDirectory() as d:
        spec, out = os.path.join(d, "spec.npz"), os.path.join(d, "out.npz")
        np.savez(spec, x=x, jobs=np.asarray(jobs, dtype=np.float64), fft_size=F)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", spec, out], capture_output=True,
                           text=True)
        if r.returncode != 0:
            return None, r.returncode, r.stderr
        z = np.load(out)
        return z["mc"], z["ret"], z["secs"]


def job(m, alpha, extra, itr1, itr2, dd):
    o = {"etype": 0, "e": 0.0, "f": 1e-6, "itype": 3}
    o.update({k: v for k, v in extra.items() if k != "itr2"})   # itr2 belongs to the convergence run alone
    return [itr1, itr2, dd, m, alpha, o["etype"], o["e"], o["f"], o["itype"]]


def main():
    assert os.path.exists(LIB), "run `make -C oracle ref` first"
    store = {"fixed_itr": np.asarray(FIXED_ITR), "dd": DD, "perturb_seed": PERTURB_SEED,
             "a_utterances": np.asarray(A_UTTERANCES), "b_sp_rows": np.asarray(B_SP_ROWS)}
    for case in ("A", "C"):
        store["seed_" + case] = CASE_SEEDS[case]
        store["x_" + case] = case_input(case)
    store["x_D"] = case_d_rows()
    for key, (case, m, alpha, extra) in OPTIONS.items():
        F, frames = CASE_SHAPE[case]
        x = case_input(case)
        assert x.shape == (frames, F // 2 + 1)
        jobs = [job(m, alpha, extra, 2, k, 0.0) for k in FIXED_ITR]
        itr2 = extra.get("itr2", 30)
        jobs += [job(m, alpha, extra, 2, itr2, dd) for dd in (DD, DD * 0.99, DD * 1.01)]
        mc, ret, _ = run_child(x, F, jobs)
        assert mc is not None, (key, ret, _)
        mcp, retp, _ = run_child(perturb(x), F, jobs[:5])
        assert mcp is not None, key
        robust = np.ones(frames, dtype=bool)
        for v in (5, 6):
            robust &= (mc[v] == mc[4]).all(axis=1) & (ret[v] == ret[4])
        share = robust.mean()
        print("%-12s F %4d m %2d a %.2f  robust %.0f %%  ret0 %2d/%d  sens fixed %s  conv %.2e" % (
            key, F, m, alpha, 100 * share, (ret[4] == 0).sum(), frames,
            " ".join("%.1e" % np.abs(mcp[k] - mc[k]).max() for k in range(4)),
            np.abs(mcp[4] - mc[4])[robust].max()))
        assert share >= 0.9, "%s: only %.0f %% of the frames are robust: choose another seed" % (key, 100 * share)
        assert (ret[:4] == -1).all()
        if "itr2" in extra:                                      # frames that run out of steps, and frames that do not
            assert (ret[4][robust] == -1).sum() >= 4 and (ret[4][robust] == 0).sum() >= 4, (key, ret[4])
        store[key + "/opt"] = np.asarray(job(m, alpha, extra, 2, itr2, DD))
        store[key + "/fixed"] = mc[:4, :, :m + 1]
        store[key + "/conv"] = mc[4, :, :m + 1]
        store[key + "/ret"] = ret[4]
        store[key + "/robust"] = robust
        store[key + "/sens_fixed"] = np.asarray([np.abs(mcp[k] - mc[k]).max() for k in range(4)])
        store[key + "/sens_conv"] = np.abs(mcp[4] - mc[4])[robust].max()
    # ---- case D: what makes the reference exit (one child per frame) ----
    xd = case_d_rows()
    d_conv = np.zeros((4, 9))
    d_init = np.zeros((4, 9))
    d_status = np.zeros(4, dtype=np.int32)
    d_fail = np.zeros(4, dtype=np.int32)
    d_sens = np.zeros((4, 2))                                    # of the convergence run, of the initial estimate
    for i in range(4):
        mc, ret, err = run_child(xd[i:i + 1], 512, [job(8, 0.42, {}, 2, 30, DD), job(8, 0.42, {}, 2, 0, DD)])
        if mc is None:
            assert "periodogram has '0'" in err, err
            d_status[i] = 2
        else:
            d_conv[i], d_init[i], d_status[i] = mc[0, 0], mc[1, 0], ret[0, 0]
            mcp, _, _ = run_child(perturb(xd)[i:i + 1], 512, [job(8, 0.42, {}, 2, 30, DD), job(8, 0.42, {}, 2, 0, DD)])
            d_sens[i] = np.abs(mcp[:, 0] - mc[:, 0]).max(axis=1)
        mc2, ret2, err2 = run_child(xd[i:i + 1], 512, [job(8, 0.42, {"f": 1e6}, 2, 30, DD)])
        assert mc2 is None
        d_fail[i] = 1 if "Error in theq() at 1th iteration" in err2 else 2
    print("D: status", d_status, "with f = 1e6", d_fail, "sens conv %.1e init %.1e" % tuple(d_sens.max(axis=0)))
    assert list(d_status) == [d_status[0], 2, d_status[2], d_status[3]] and list(d_fail) == [1, 2, 1, 1]
    store.update({"D/conv": d_conv, "D/init": d_init, "D/status": d_status, "D/status_f1e6": d_fail,
                  "D/sens_conv": d_sens[:, 0].max(), "D/sens_init": d_sens[:, 1].max()})
    path = os.path.join(GOLDEN, "sptk_mcep.npz")
    np.savez_compressed(path, **store)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    # ---- the reference's one-thread rate (a record, not a fixture) ----
    xb = np.tile(case_b_rows(), (8, 1))
    for m, alpha in ((24, 0.55), (49, 0.42)):
        _, _, secs = run_child(xb, 1024, [job(m, alpha, {}, 2, 30, DD)])
        print("reference mcep, F 1024, m %d, defaults: %.0f frames/s on one thread" % (m, len(xb) / secs[0]))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main()

#!/usr/bin/env python3
"""Writes tests/golden/sptk_mgcep.npz: integer-valued waveforms, option sets and the COMPILED reference's outputs of SPTK's
mcep with itype 0 (test/sptkfunctions.cpp:11-184, built by oracle/Makefile into oracle/_ref/libsptk_ref.so) on their
windowed frames, for tests/test_mgcep_host.py and tests/test_gpu_mgcep.py.

    make -C oracle ref && python tools/gen_golden_mgcep.py

The frames are tests/mgcep_reference.py's (SPTK's frame and window are not in the reference tree), windowed with the
LIBRARY's table (WorldMi355SptkWindow, host only: libworld_mi355.so must be built).  mcep keeps static buffers and calls
exit() where it fails, so every job runs in a child process (this file with --child), always with flng = fft_size.  A
frame whose windowed samples are all zero makes the reference exit at etype 0 and 2 (:119-124); such frames are found
here, recorded in <key>/exits and not handed to it.  Only data is stored.

Per option set (`key`), over the batch's frames:
  <key>/fixed        [4][frames][m+1]  dd = 0: exactly itr2 = 0, 1, 2, 5 Newton steps
  <key>/conv         [frames][m+1]     SPTK's stop rule: itr1 2, itr2 30, dd 1e-3
  <key>/ret          [frames]          mcep's return value of that run (0 / -1)
  <key>/robust       [frames]          the runs at dd 0.99e-3 and 1.01e-3 return the same row and value
  <key>/exits        [frames]          the reference exits on the frame (rows of zeros above)
  <key>/sens_fixed   [4], <key>/sens_conv   max |d mc| when the windowed frame is multiplied by 1 + 4 * 2^-52 * xi, xi uniform
                                       in [-1, 1] (seeded), as gen_golden_mcep.perturb does
At least 90 % of the frames the reference takes must be robust in every set, or this script fails.
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_mcep as base  # noqa: E402
import mgcep_reference as ref  # noqa: E402

LIB = base.LIB
GOLDEN = base.GOLDEN
FIXED_ITR = base.FIXED_ITR
DD = base.DD

WAVE_T = (1, 37, 199, 200, 201, 1000, 1203)          # the waveform sets' utterances, one batch
ROWS_T = (1500,)                                     # the rows sets' utterance: L 400, P 100, Hamming, power-normalised
ROWS_FRAME = (400, 100, 1, 1)
RECIPE_T = (9000,)                                   # 40 frames at the recipe's shape

# key -> (utterances, F, L, P, window, norm, pipe_float32, m, alpha, extra options)
SETS = {}
for _i, (_m, _a, _e) in enumerate(((12, 0.0, 0), (12, 0.42, 1), (12, 0.55, 2), (49, 0.0, 1), (49, 0.42, 2), (49, 0.55, 0),
                                   (63, 0.0, 2), (63, 0.42, 0), (63, 0.55, 1))):
    _x = {0: {}, 1: {"etype": 1, "e": 1e-8}, 2: {"etype": 2, "e": -60.0}}[_e]
    SETS["R_m%d_a%02d_e%d" % (_m, round(_a * 100), _e)] = ("rows", 512) + ROWS_FRAME + (False, _m, _a, _x)
# every L, P, window, norm and pipe mode, each pair of (L, P) and (window, norm) once
for _i, (_L, _P, _w, _n, _f) in enumerate(((400, 80, 0, 0, False), (400, 400, 1, 1, True), (401, 80, 2, 2, True),
                                           (401, 401, 5, 0, False), (512, 80, 1, 2, False), (512, 512, 0, 1, True),
                                           (400, 80, 2, 1, False), (401, 401, 0, 2, True), (512, 80, 5, 1, True),
                                           (400, 400, 2, 0, True), (401, 80, 1, 0, True), (512, 512, 5, 2, False))):
    SETS["W_L%d_P%d_w%d_n%d_f%d" % (_L, _P, _w, _n, int(_f))] = ("wave", 512, _L, _P, _w, _n, _f, 12, 0.42,
                                                                 {"etype": 1, "e": 1e-8} if _i % 2 else {})
SETS["recipe"] = ("recipe", 2048, 1200, 240, 1, 1, True, 49, 0.55, {"etype": 1, "e": 1e-8})
UTTERANCES = {"rows": ROWS_T, "wave": WAVE_T, "recipe": RECIPE_T}
SEEDS = {"rows": 31, "wave": 47, "recipe": 59}


def make_wave(seed, T, fs=16000.0):
    """Integer-valued, speech-like: twelve harmonics under a slow envelope plus noise, peak about 8000; the first and the
    last sample are not zero."""
    rs = np.random.RandomState(seed)
    t = np.arange(T) / fs
    f0 = 110.0 + 60.0 * rs.rand()
    x = sum(rs.rand() / h * np.sin(2 * np.pi * h * f0 * t + 2 * np.pi * rs.rand()) for h in range(1, 13))
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t + rs.rand())) + 0.02 * rs.randn(T)
    x = np.rint(8000.0 * x / max(np.abs(x).max(), 1e-9))
    x[x == 0] = 1.0
    return x


def waves(group):
    return [make_wave(SEEDS[group] + 101 * k, T) for k, T in enumerate(UTTERANCES[group])]


def library_window(kind, norm, L):
    pkg = __import__("importlib").import_module("hts-train-world_amd")
    return pkg.world.sptk_window(kind, norm, L)


def set_frames(key, table=None):
    """(rows [frames][F], frame counts) of the option set."""
    group, F, L, P, kind, norm, f32 = SETS[key][:7]
    w = library_window(kind, norm, L) if table is None else table
    return ref.windowed_batch(waves(group), w, P, F, f32)


def child(spec_path, out_path):
    """Runs the jobs of spec_path in this process; a failing mcep ends it with the reference's exit status."""
    z = np.load(spec_path, allow_pickle=False)
    x, jobs = z["x"], z["jobs"]                                  # jobs: [itr1, itr2, dd, m, alpha, etype, e, f, itype]
    F = int(z["fft_size"])
    lib = ctypes.CDLL(LIB)
    fn = getattr(lib, base.mcep_symbol())
    dp = ctypes.POINTER(ctypes.c_double)
    fn.restype = ctypes.c_int
    fn.argtypes = [dp, ctypes.c_int, dp, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                   ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int]
    m_max = int(jobs[:, 3].max())
    mc = np.zeros((len(jobs), len(x), m_max + 1))
    ret = np.zeros((len(jobs), len(x)), dtype=np.int32)
    buf = np.zeros(F)
    for j, (itr1, itr2, dd, m, alpha, etype, e, f, itype) in enumerate(jobs):
        for i, row in enumerate(x):
            buf[:] = row
            o = np.zeros(int(m) + 1)
            ret[j, i] = fn(buf.ctypes.data_as(dp), F, o.ctypes.data_as(dp), int(m), float(alpha), int(itr1), int(itr2),
                           float(dd), int(etype), float(e), float(f), int(itype))
            mc[j, i, :int(m) + 1] = o
    np.savez(out_path, mc=mc, ret=ret)


def run_child(x, F, jobs):
    with tempfile.TemporaryDirectory() as d:
        spec, out = os.path.join(d, "spec.npz"), os.path.join(d, "out.npz")
        np.savez(spec, x=x, jobs=np.asarray(jobs, dtype=np.float64), fft_size=F)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", spec, out], capture_output=True,
                           text=True)
        assert r.returncode == 0, (r.returncode, r.stderr)
        z = np.load(out)
        return z["mc"], z["ret"]


def job(m, alpha, extra, itr1, itr2, dd):
    o = {"etype": 0, "e": 0.0, "f": 1e-6, "itype": 0}
    o.update(extra)
    return [itr1, itr2, dd, m, alpha, o["etype"], o["e"], o["f"], o["itype"]]


def exits_on(rows, extra):
    """Frames the reference exits on: all samples zero and nothing added to the periodogram (etype 0; at etype 2 the floor
    of a zero maximum is zero)."""
    if extra.get("etype", 0) == 1 and extra.get("e", 0.0) > 0.0:
        return np.zeros(len(rows), dtype=bool)
    return ~rows.any(axis=1)


def reference_of(key, rows):
    """The fixture's entries of one option set from the compiled reference."""
    F, m, alpha, extra = SETS[key][1], SETS[key][7], SETS[key][8], SETS[key][9]
    exits = exits_on(rows, extra)
    live = np.nonzero(~exits)[0]
    jobs = [job(m, alpha, extra, 2, k, 0.0) for k in FIXED_ITR]
    jobs += [job(m, alpha, extra, 2, 30, dd) for dd in (DD, DD * 0.99, DD * 1.01)]
    mc_l, ret_l = run_child(rows[live], F, jobs)
    mcp_l, _ = run_child(base.perturb(rows[live]), F, jobs[:5])
    n = len(rows)
    mc = np.zeros((7, n, m + 1))
    ret = np.zeros((7, n), dtype=np.int32)
    mc[:, live], ret[:, live] = mc_l[:, :, :m + 1], ret_l
    robust = np.zeros(n, dtype=bool)
    rb = np.ones(len(live), dtype=bool)
    for v in (5, 6):
        rb &= (mc_l[v] == mc_l[4]).all(axis=1) & (ret_l[v] == ret_l[4])
    robust[live] = rb
    assert (ret_l[:4] == -1).all()
    return {"fixed": mc[:4], "conv": mc[4], "ret": ret[4], "robust": robust, "exits": exits,
            "sens_fixed": np.asarray([np.abs(mcp_l[k] - mc_l[k]).max() for k in range(4)]),
            "sens_conv": np.abs(mcp_l[4] - mc_l[4])[rb].max()}


def main():
    assert os.path.exists(LIB), "run `make -C oracle ref` first"
    store = {"fixed_itr": np.asarray(FIXED_ITR), "dd": DD, "perturb_seed": base.PERTURB_SEED}
    for group in UTTERANCES:
        ws = waves(group)
        assert all((w == np.rint(w)).all() and np.abs(w).max() < 32768 for w in ws)
        store["x_" + group] = np.concatenate(ws).astype(np.int16)
        store["T_" + group] = np.asarray(UTTERANCES[group])
    for key in SETS:
        rows, counts = set_frames(key)
        r = reference_of(key, rows)
        taken = ~r["exits"]
        share = r["robust"][taken].mean()
        print("%-22s frames %3d exits %d  robust %.0f %%  ret0 %3d  sens fixed %s  conv %.2e" % (
            key, len(rows), r["exits"].sum(), 100 * share, (r["ret"][taken] == 0).sum(),
            " ".join("%.1e" % s for s in r["sens_fixed"]), r["sens_conv"]))
        assert share >= 0.9, "%s: only %.0f %% of the frames are robust: choose another seed" % (key, 100 * share)
        store[key + "/counts"] = np.asarray(counts)
        for name, v in r.items():
            store[key + "/" + name] = v
    path = os.path.join(GOLDEN, "sptk_mgcep.npz")
    np.savez_compressed(path, **store)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main()

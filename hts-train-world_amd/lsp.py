"""MGC-LSP rows back to LPC and MGC rows, and the recipe's LSP postfilter, on the device (csrc/lsp.hip).

With GAMMA != 0 the recipe's `mgc` stream holds MGC-LSP rows [gain, lsp_1 .. lsp_m]; gen_wave and postfiltering_lsp
(scripts/Training.pl:2690-2752, :2846-2868) take them back by `lspcheck -c -r 0.1 -g -G 1e-10 | lsp2lpc | mgc2mgc -n -u`.
include/world_mi355.h defines every step (parity with SPTK's lspcheck and lsp2lpc is unpinned: the commands are not in
the reference tree); here are the three calls on the frames of a WorldBatch:

    lsp_to_lpc(batch, lsp, ...)                          lspcheck | lsp2lpc: rows [K, a_1 .. a_m]
    lsp_to_mel_generalized_cepstrum(batch, lsp, ...)     ... | mgc2mgc -n -u: plain MGC rows at (out_alpha, out_gamma)
    postfilter_lsp(batch, lsp, ...)                      postfiltering_lsp: rows [gain', p]

Every tensor is float64 on the batch's device, [total_frames][order+1]; the order is the rows' width less one.  status is
int32 [total_frames], bits: 1 the check changed an LSP, 2 the gain was raised to min_gain, 4 a non-finite input value,
8 a non-finite result (4 and 8: zeros), 16 the checked LSPs are not strictly increasing inside (0, pi).  Refused options
raise RuntimeError("... bad argument"), refused tensors ValueError, both before anything is launched.  Asynchronous on the
context's stream.
"""
from __future__ import annotations

import ctypes as C

from .world import LspOption, LspPostfilterOption, _check, _option, _ptr, load_library, torch  # noqa: F401


def _rows(batch, where, lsp):
    return batch._f64(where, "lsp", lsp, batch.total_frames, None)


def _lsp_option(where, cols, alpha, gamma, log_gain, min_distance, min_gain):
    return _option(where, LspOption, "WorldMi355DefaultLspOption",
                   dict(order=cols - 1, alpha=float(alpha), gamma=float(gamma), log_gain=int(bool(log_gain)),
                        min_distance=float(min_distance), min_gain=float(min_gain)))


def lsp_to_lpc(batch, lsp, alpha=0.35, gamma=-1.0, log_gain=False, min_distance=0.1, min_gain=1e-10, checked=False):
    """`lspcheck -c -r min_distance -g -G min_gain [-L] | lsp2lpc` per frame.  Returns (lpc, status), with checked=True
    (lpc, checked rows, status).  K = lpc[:, 0] is linear whatever log_gain is; the checked rows keep the gain's form.
    alpha and gamma are checked as the other two calls check them and otherwise unused."""
    where = "lsp_to_lpc"
    lp, cols = _rows(batch, where, lsp)
    o = _lsp_option(where, cols, alpha, gamma, log_gain, min_distance, min_gain)
    lpc = batch._new(batch.total_frames, cols)
    chk = batch._new(batch.total_frames, cols) if checked else None
    status = batch._new(batch.total_frames, dtype=torch.int32)
    _check(load_library().WorldMi355LspToLpc(batch.handle, lp, C.byref(o), _ptr(lpc), _ptr(chk), _ptr(status)),
           "LspToLpc")
    return (lpc, chk, status) if checked else (lpc, status)


def lsp_to_mel_generalized_cepstrum(batch, lsp, alpha, gamma, out_order=None, out_alpha=None, out_gamma=None,
                                    log_gain=False, min_distance=0.1, min_gain=1e-10):
    """lsp_to_lpc, then WorldBatch.convert_mel_generalized_cepstrum(..., normalized=True, multiplied=True) of the LPC rows
    at (alpha, gamma), -1 <= gamma < 0, towards (out_order, out_alpha, out_gamma): None means the input's own, which is
    gen_wave's call.  Returns (out [total_frames][out_order+1], status); a row the conversion flags is bit 8."""
    where = "lsp_to_mel_generalized_cepstrum"
    lp, cols = _rows(batch, where, lsp)
    o = _lsp_option(where, cols, alpha, gamma, log_gain, min_distance, min_gain)
    out_order = cols - 1 if out_order is None else int(out_order)
    out_alpha = float(alpha if out_alpha is None else out_alpha)
    out_gamma = float(gamma if out_gamma is None else out_gamma)
    out = batch._new(batch.total_frames, max(out_order, 0) + 1)
    status = batch._new(batch.total_frames, dtype=torch.int32)
    _check(load_library().WorldMi355LspToMelGeneralizedCepstrum(batch.handle, lp, C.byref(o), out_order, out_alpha,
                                                                out_gamma, _ptr(out), _ptr(status)),
           "LspToMelGeneralizedCepstrum")
    return out, status


def postfilter_lsp(batch, lsp, alpha, gamma, beta=0.7, length=4096, compensation=False, log_gain=False, min_distance=0.1,
                   min_gain=1e-10, energies=False, out=None):
    """postfiltering_lsp per frame: the filtered LSPs p (from the row as it is, ends untouched) beside the gain.
    compensation=False is the script as written, gain' = gain bit for bit; True puts the energy difference of the
    impulse responses over `length` samples into it: gain + (ene1 - ene2) under log_gain, else gain exp(ene1 - ene2).
    out: None for a fresh tensor, or the tensor to write, which may be `lsp` itself.  Returns (out, status), with
    energies=True (out, ene1, ene2, status).  beta == 1 or order <= 2 copies the rows."""
    where = "postfilter_lsp"
    lp, cols = _rows(batch, where, lsp)
    o = _option(where, LspPostfilterOption, "WorldMi355DefaultLspPostfilterOption",
                dict(order=cols - 1, alpha=float(alpha), gamma=float(gamma), log_gain=int(bool(log_gain)),
                     min_distance=float(min_distance), min_gain=float(min_gain), beta=float(beta), length=int(length),
                     compensation=int(bool(compensation))))
    out, op = batch._out(where, out, batch.total_frames, cols)
    e1 = batch._new(batch.total_frames) if energies else None
    e2 = batch._new(batch.total_frames) if energies else None
    status = batch._new(batch.total_frames, dtype=torch.int32)
    _check(load_library().WorldMi355LspPostfilter(batch.handle, lp, C.byref(o), op, _ptr(e1), _ptr(e2), _ptr(status)),
           "LspPostfilter")
    return (out, e1, e2, status) if energies else (out, status)

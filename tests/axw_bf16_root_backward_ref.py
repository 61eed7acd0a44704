"""float64 references and bounds of flex_axw_backward_root_bf16 (include/flex_axw.h) for tests/test_gpu_axw_bf16_root_backward.py, composed of
those of tests/axw_bf16_root_ref.py (the dual-source dense stage) and tests/axw_bf16_backward_ref.py (dW); every input is an fp32 array of
bf16 numbers.  The dX kernel alone is axw_bf16_root_ref.dense_reference(G, Wt, dOut, Rt) on the arrays padded to cp."""
import numpy as np

import f64ref
from attention_bf16_ref import bound_bf16
from axw_bf16_backward_ref import dw_reference
from backward_ref import transpose
from f64ref import P, TINY, gamma, gemm_f64, spmm64


def db_reference(dOut, slices):
    """(ref, bound) of db = 1^T dOut in fp32: L = rows per slice + slices roundings, as dw_reference; no bf16 rounding"""
    L = (-(-dOut.shape[0] // slices) + 63) // 64 * 64 + slices
    with np.errstate(invalid="ignore", over="ignore"):
        return dOut.astype(np.float64).sum(axis=0), gamma(L) * np.abs(dOut.astype(np.float64)).sum(axis=0) + L * TINY


def check_db(r, bound, got, what=""):
    """(message or None, worst err / bound) of the fp32 db against db_reference"""
    got = got.astype(np.float64)
    fin = np.isfinite(r)
    if f64ref._class_mismatch(r, got).any():
        return f"[{what}] db has entries of the wrong class: got {got!r}, reference {r!r}", np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        ratio = np.where(fin, np.abs(got - r) / bound, 0.0)
    j = int(np.argmax(ratio))
    return (f"[{what}] db[{j}] = {got[j]!r}, reference {r[j]!r}: err/bound {ratio[j]:.3g}" if ratio[j] > 1 else None), float(ratio[j])


def backward_reference(a, X, W, R, dOut, cp, slices):
    """((ref, bound) of dGradX, of dGradW, of dGradR, of dGradBias): G64 = A^T dOut and eG as axw_bf16_backward_ref.backward_reference; dX is
    one chain of length 2 cp over [G W^T; dOut R^T]"""
    at = transpose(a)
    nr = (np.diff(at.rowPtr.astype(np.int64)) + P)[:, None]
    absWt, absRt = np.abs(W.astype(np.float64)).T, np.abs(R.astype(np.float64)).T
    with np.errstate(invalid="ignore", over="ignore"):
        G = spmm64(at, dOut)
        eG = bound_bf16(G, gamma(nr) * spmm64(at, dOut, absolute=True) + nr * TINY)
        dx = (gemm_f64(G, W.T) + gemm_f64(dOut, R.T),
              gemm_f64(eG, absWt) + gamma(2 * cp + 2) * (gemm_f64(np.abs(G) + eG, absWt) + gemm_f64(np.abs(dOut), absRt)) + 2 * cp * TINY)
    return dx, dw_reference(X, G, slices, eG), dw_reference(X, dOut, slices), db_reference(dOut, slices)

"""float64 references and bounds of flex_axw_backward_bf16 (include/flex_axw.h) for tests/test_gpu_axw_bf16_backward.py; every input is an
fp32 array of bf16 numbers.  Each returns (R, E1 + b2) for axw_bf16_ref.check: |out - R| <= bound_bf16(R, E1 + b2)."""
import numpy as np

from attention_bf16_ref import bound_bf16
from axw_bf16_ref import M
from backward_ref import transpose
from f64ref import P, TINY, gamma, gemm_f64, spmm64


def dw_reference(X, G, slices, eG=0.0):
    """dW = X^T G; L = rows per slice + slices, rows = ceil(n / slices) rounded up to the kernel's 64-row stage (never below its own)"""
    L = (-(-X.shape[0] // slices) + 63) // 64 * 64 + slices
    absX = np.abs(X.astype(np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        b2 = gamma(M * L) * gemm_f64(absX.T, np.abs(G) + eG) + L * TINY * (1.0 + absX.sum(axis=0)[:, None])
        return gemm_f64(X.T, G), gemm_f64(absX.T, np.zeros_like(G, np.float64) + eG) + b2


def backward_reference(a, X, W, dOut, cp, slices):
    """((R, bound) of dGradX, (R, bound) of dGradW): G64 = A^T dOut [n x c], eG flex_spmm_bf16's bound for it on the rows of A^T; dX = G W^T
    is a dot product of length cp (G and W^T zero-padded)"""
    at = transpose(a)
    nr = (np.diff(at.rowPtr.astype(np.int64)) + P)[:, None]
    absWt = np.abs(W.astype(np.float64)).T
    with np.errstate(invalid="ignore", over="ignore"):
        G = spmm64(at, dOut)
        eG = bound_bf16(G, gamma(nr) * spmm64(at, dOut, absolute=True) + nr * TINY)
        dx = gemm_f64(G, W.T), gemm_f64(eG, absWt) + gamma(M * cp) * gemm_f64(np.abs(G) + eG, absWt) + cp * TINY
    return dx, dw_reference(X, G, slices, eG)

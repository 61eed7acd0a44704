"""float64 references and bounds of the bf16 layer with a root-weight term (include/flex_axw.h: flex_axw_run_root_bf16) and of its dense
stage Out = rn_bf16(L1 W1 + L2 W2 + Cin + b), for tests/test_gpu_axw_bf16_root.py.  Inputs are fp32 arrays of bf16 numbers (the bias: any
fp32).  Dense stage: the products are exact in fp32 and the chain is d1 + d2 + 1 additions of one rounding each, so |x32 - ref64| <= g =
gamma(d1 + d2 + 2) (|L1||W1| + |L2||W2| + |Cin| + |b|) + (d1 + d2) 2^-149; rn_bf16(x32) lies within bound_bf16(ref64, g).  The layer bounds
compose it with flex_spmm_bf16's and the GCN layer's as flex_axw.h states.  check is axw_bf16_ref.check."""
import numpy as np

import f64ref
from axw_bf16_ref import bound_bf16, check, gemm_bound, rounded  # noqa: F401  (check, rounded: for the tests)
from f64ref import A_XW, TINY, gamma, gemm_f64, spmm64


def dense_reference(L1, W1, L2=None, W2=None, Cin=None, bias=None):
    """(ref64, g) of the dense stage; absent terms are None."""
    d = L1.shape[1] + (0 if L2 is None else L2.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        ref, mag = gemm_f64(L1, W1), gemm_f64(np.abs(L1), np.abs(W1))
        if L2 is not None:
            ref, mag = ref + gemm_f64(L2, W2), mag + gemm_f64(np.abs(L2), np.abs(W2))
        for t in (Cin, None if bias is None else bias[None, :]):
            if t is not None:
                ref, mag = ref + t.astype(np.float64), mag + np.abs(t.astype(np.float64))
        return ref, gamma(d + 2) * mag + d * TINY


def layer_reference(a, X, W, R, bias, order):
    """(ref, E) of flex_axw_run_root_bf16 in `order`: |Out - ref| <= bound_bf16(ref, E)."""
    dim = X.shape[1]
    nr = (np.diff(a.rowPtr.astype(np.int64)) + f64ref.P)[:, None]
    b = np.zeros(W.shape[1]) if bias is None else bias.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        root, root_abs = gemm_f64(X, R), gemm_f64(np.abs(X), np.abs(R))
        if order == A_XW:
            U = gemm_f64(X, W)
            eU = bound_bf16(U, gemm_bound(X, W))
            S = spmm64(a, U)
            eS = bound_bf16(S, spmm64(a, eU, absolute=True) + gamma(nr) * spmm64(a, np.abs(U) + eU, absolute=True) + nr * TINY)
            return S + root + b, eS + gamma(dim + 2) * (root_abs + np.abs(S) + eS + np.abs(b)) + dim * TINY
        T = spmm64(a, X)
        e1 = bound_bf16(T, gamma(nr) * spmm64(a, X, absolute=True) + nr * TINY)
        absW = np.abs(W.astype(np.float64))
        return (gemm_f64(T, W) + root + b,
                gemm_f64(e1, absW) + gamma(2 * dim + 2) * (gemm_f64(np.abs(T) + e1, absW) + root_abs + np.abs(b)) + 2 * dim * TINY)


def operands(rng, n, d1, d2, c, cp, cin, bias, cancel=False):
    """(L1, W1, L2, W2, Cin [n x cp], bias [c]) of bf16 numbers (the bias: fp32), magnitudes 2^U(-4, 4); None for what is absent.  Cin's
    padding columns hold 3.0.  cancel (d1 = d2): L2 = L1 and W2 = -W1 (1 + 2^-7): the products cancel across the seam, |L||W| >> |L W|."""
    lu = lambda *shape: rounded(f64ref._logu(rng, -4, 4, shape))  # noqa: E731
    L1, W1 = lu(n, d1), lu(d1, c)
    L2, W2 = (lu(n, d2), lu(d2, c)) if d2 else (None, None)
    if cancel:
        L2, W2 = L1.copy(), rounded(-(W1 * np.float32(1 + 2.0 ** -7)))
    Cin = np.pad(lu(n, c), ((0, 0), (0, cp - c)), constant_values=3.0) if cin else None
    return L1, W1, L2, W2, Cin, (f64ref._logu(rng, -4, 4, c).astype(np.float32) if bias else None)

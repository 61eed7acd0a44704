"""float64 references and bounds of the backward pass (include/flex_axw.h, flex_axw_backward; FLEX_PLAN_TRANSPOSE), on top of f64ref.

G = A^T dOut first, then dGradX = G W^T and dGradW = X^T G.  dGradX is flex_axw_run's order AX_W for (A^T, dOut, W^T), so its check is
check_axw's.  dGradW gets its own: |dGradW - ref| <= gamma(M) |X|^T (|A|^T |dOut|) + 2^-149 M (1 + sum_r |X_ri|), M = max_r n_r + L,
n_r = nnz(column r of A) + 32 and L the longest chain of the X^T G product (L_dW of the kernel; n for rocBLAS), with exact classes."""
import numpy as np

from f64ref import (AX_W, NORMAL_MIN, P, S_LIMIT, TINY, _class_mismatch, _finite, axw_range_guard, axw_scenario, check_axw, gamma,
                    gemm_f64, spmm64)
from f64ref import ROUTES
from flex_amd.binding import HostCsr


def _flex():
    import flex_amd
    return flex_amd


def transpose(a):
    """The CSR of A^T (n x m): rows of A ascending inside each row of A^T, duplicates in CSR order (what FLEX_PLAN_TRANSPOSE plans)."""
    rp = a.rowPtr.astype(np.int64)
    rows = np.repeat(np.arange(a.m, dtype=np.int64), np.diff(rp))
    perm = np.argsort(a.col.astype(np.int64), kind="stable")
    counts = np.bincount(a.col.astype(np.int64), minlength=a.n)
    rpT = np.zeros(a.n + 1, dtype=np.int64)
    np.cumsum(counts, out=rpT[1:])
    return HostCsr(rpT.astype(np.uint32), rows[perm].astype(np.uint32), a.vals[perm], n=a.m)


def _directed(m=300, n=None, seed=0, dup=False, empty=True):
    """A random directed m x n CSR: skewed in- and out-degrees, empty rows and columns, optional duplicate entries."""
    n = m if n is None else n
    rng = np.random.default_rng([seed, m, n])
    deg = rng.poisson(5, size=m)
    if empty:
        deg[rng.random(m) < 0.15] = 0
    deg[m // 2] = min(3 * n, 150)
    hot = rng.integers(0, n, size=3)  # columns of high in-degree: long rows of A^T
    cols = []
    for d in deg:
        c = np.where(rng.random(d) < 0.2, rng.choice(hot, d), rng.integers(0, max(1, n - n // 10), d))  # the last tenth: empty columns
        cols.append(c if dup else np.unique(c)[rng.permutation(len(np.unique(c)))])
    deg = np.array([len(c) for c in cols])
    rp = np.zeros(m + 1, np.int64)
    np.cumsum(deg, out=rp[1:])
    col = np.concatenate(cols) if rp[-1] else np.zeros(0, np.int64)
    vals = rng.uniform(-1, 1, rp[-1]).astype(np.float32)
    return HostCsr(rp.astype(np.uint32), col.astype(np.uint32), vals, n=n)


def route_plans(route, a, t):
    """plan_for_route (tests/f64ref.py) with the plans made from A with FLEX_PLAN_TRANSPOSE (t) or from the explicit A^T."""
    spec = ROUTES[route]
    k, tn = spec["k"], spec["tuning"]
    if spec.get("mapped"):
        vo, ap = _flex().perm_csr(a, _flex().order_rcm(a))
        return [_flex().Plan(ap if t else transpose(ap), k, vo_mp=vo, tuning=tn, transpose=t)]
    src = a if t else transpose(a)
    if spec.get("shards"):
        b = _flex().shard_rows(transpose(a), k, spec["shards"])
        return [_flex().Plan(src, k, rows=(int(b[i]), int(b[i + 1])), tuning=tn, transpose=t) for i in range(spec["shards"])]
    ldb, ldc = spec.get("ld", (None, None))
    return [_flex().Plan(src, k, order=spec.get("order", 0), ldb=ldb, ldc=ldc, tuning=tn, transpose=t)]


def dw_slices(n, n_cus):
    """flex_axw_dw_slices: the n-slices of the X^T G kernel."""
    return max(1, min(n_cus, (n + 255) // 256))


def dw_chain(n, n_cus):
    """L_dW(n): ceil(n / S) + S roundings."""
    s = dw_slices(n, n_cus)
    return -(-n // s) + s


def backward_case(name, n, dim, c, seed=0):
    """(A, X, W, dOut [n x c]) of AXW scenario `name`: dOut takes the X values of the same scenario at width c."""
    a, X, W = axw_scenario(name, n, dim, c, seed)
    _, D, _ = axw_scenario(name, n, c, c, seed + 1)
    # dOut scaled by a power of two so that |A^T| |dOut| |W^T| and |X|^T |A^T| |dOut| stay below 2^120 ("huge": with the largest near it)
    t = transpose(a)
    g = spmm64(HostCsr(t.rowPtr, t.col, _finite(t.vals).astype(np.float32), n=t.n), _finite(D))
    s = max(gemm_f64(g, _finite(W).T).max(initial=0), gemm_f64(_finite(X).T, g).max(initial=0))
    if s > 0 and (name == "huge" or s >= 2.0 ** 119):
        D = (D.astype(np.float64) * 2.0 ** (118 - int(np.floor(np.log2(s))))).astype(np.float32)
    return a, X, W, np.ascontiguousarray(D, np.float32)


def dw_range_guard(aT, X, D, extra=P):
    """None if X^T (A^T D) stays in the checked range (no stage sum reaches 2^120; no finite G entry that fp32 may round to zero or
    to the other sign meets an inf / NaN of X), else why not."""
    af = HostCsr(aT.rowPtr, aT.col, np.where(np.isfinite(aT.vals), np.abs(aT.vals), 0).astype(np.float32), n=aT.n)
    sg = spmm64(af, _finite(D))
    s = gemm_f64(_finite(X).T, sg)
    for what, v in (("|A|^T |dOut|", sg), ("|X|^T |A|^T |dOut|", s)):
        if v.size and v.max() >= S_LIMIT:
            return f"stage sum {what} reaches {v.max():g} >= 2^120"
    with np.errstate(invalid="ignore", over="ignore"):
        g, s1 = spmm64(aT, D), spmm64(aT, D, absolute=True)
        nr = (np.diff(aT.rowPtr.astype(np.int64)) + extra)[:, None]
        b1 = gamma(nr) * s1 + nr * TINY
        ag = np.abs(g)
        unsafe = np.isfinite(g) & (s1 > 0) & ~((ag > b1) & (ag >= NORMAL_MIN))
    bad_r = ~np.isfinite(X).all(axis=1)
    if unsafe[bad_r].any():
        return "a G entry fp32 may flush or flip meets an inf / NaN row of X"
    return None


def check_dw(aT, X, D, got, chain, extra=P):
    """None if got (dim x c) passes the dGradW bound with exact classes, else a message.  chain: L of the X^T G product."""
    guard = dw_range_guard(aT, X, D, extra)
    assert guard is None, f"case leaves the checked range: {guard}"
    with np.errstate(invalid="ignore", over="ignore"):
        ref = gemm_f64(np.asarray(X, np.float64).T, spmm64(aT, D))
        S = gemm_f64(np.abs(np.asarray(X, np.float64)).T, spmm64(aT, D, absolute=True))
    M = float(np.diff(aT.rowPtr.astype(np.int64)).max(initial=0) + extra + chain)
    bound = gamma(M) * S + TINY * M * (1.0 + np.abs(np.asarray(X, np.float64)).sum(axis=0))[:, None]
    got = np.asarray(got, np.float32).astype(np.float64)
    bad = _class_mismatch(ref, got)
    if bad.any():
        i, j = np.argwhere(bad)[0]
        return f"dGradW: {int(bad.sum())} entries of the wrong class; first ({i}, {j}): got {got[i, j]!r}, reference {ref[i, j]!r}"
    with np.errstate(invalid="ignore"):
        ratio = np.where(np.isfinite(ref), np.abs(got - ref) / bound, 0.0)
    if ratio.size and ratio.max() > 1.0:
        i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        return f"dGradW: {int((ratio > 1).sum())} entries beyond the bound; worst err/bound {ratio[i, j]:.3g} at ({i}, {j})"
    return None


def check_dx(aT, D, W, got, extra=P):
    """None if got (n x dim) passes flex_axw_run's AX_W bound for (A^T, dOut, W^T) with exact classes, else a message."""
    Wt = np.ascontiguousarray(np.asarray(W, np.float32).T)
    guard = axw_range_guard(aT, D, Wt, AX_W, extra)
    assert guard is None, f"case leaves the checked range: {guard}"
    return check_axw(aT, D, Wt, got, AX_W, "dGradX", extra)

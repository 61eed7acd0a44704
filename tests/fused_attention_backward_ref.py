"""float64 reference, bounds, graphs and checker of the fused attention backward (include/flex_spmm.h: flex_attention_backward), shared by
tests/test_fused_attention_backward_host.py and tests/test_gpu_fused_attention_backward.py.

The reference is float64 numpy on the SAME fp32 Q, K, V, p and g with the header's definitions (entries e of row r in CSR order, src(e)
the entry's column):
    da_e    = <g[r], V[src(e)]>
    delta_r = sum_j p_j da_j
    ds_e    = scale p_e (da_e - delta_r)
    gQ[r]   = sum_{e in row r}      ds_e K[src(e)]
    gK[c]   = sum_{e: src(e) == c}  ds_e Q[row(e)]
    gV[c]   = sum_{e: src(e) == c}  p_e  g[row(e)]
Bounds, verbatim (u = 2^-24, gamma(n) = n u / (1 - n u), n_r = entries of the row, n_c = entries of the column, a = 3, b = 0):
    dda_e    = gamma(k) sum_j |g V| + k 2^-149                                             (flex_sddmm's bound)
    dds_e    = gamma(n_r + a) scale p_e (|da_e| + sum_j |p_j da_j|) + scale p_e (dda_e + sum_j p_j dda_j) + max(1, scale) n_r 2^-149
    |gQ - gQ64| <= sum_{e in r} (gamma(n_r + b) |ds_e| + dds_e) |K[src]| + 2^-126
    |gK - gK64| <= sum_{e in c} (gamma(n_c + b) |ds_e| + dds_e) |Q[row]| + 2^-126
    |gV - gV64| <= sum_{e in c}  gamma(n_c + b) p_e |g[row]|            + 2^-126
a: ds = fl(fl(scale p) fl(da - delta)) is one subtraction and two products, and delta is summed by fma (no rounding of p_j da_j) in a
tree of depth <= n_r.  b: the three gradients are summed by fma in trees of depth <= n_r (n_c) and nothing else rounds."""
import numpy as np

from flex_amd.binding import HostCsr
from fused_attention_ref import coo
from softmax_ref import gamma

A_ROUNDINGS, B_ROUNDINGS = 3, 0


def both_sides(a):
    """The lift [[0, A], [A^T, 0]] of an m x n graph to (m + n) x (m + n): rows AND columns take a's row lengths (and its column counts),
    so the classes and thresholds a test graph has in its rows appear in the columns too."""
    row, col, rp = coo(a)
    order = np.argsort(col, kind="stable")
    cp = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=a.n))])
    rowptr = np.concatenate([rp, rp[-1] + cp[1:]]).astype(np.uint32)
    cols = np.concatenate([col + a.m, row[order]]).astype(np.uint32)
    vals = np.concatenate([a.vals, a.vals[order]]).astype(np.float32)
    return HostCsr(rowptr, cols, vals, n=a.m + a.n)


def _sum_by(x, seg, n):
    out = np.zeros((n,) + x.shape[1:])
    np.add.at(out, seg, x)
    return out


def reference(a, Q, K, V, p, g, scale, a_r=A_ROUNDINGS, b_r=B_ROUNDINGS):
    """dict(gq, gk, gv, ds and their bounds gq_bound, ...): float64 on the fp32 operands, with the header's bounds.  a_r = 4 and
    b_r = 32 give the bounds of the chain of engine calls on the same p instead (flex_edge_softmax_backward rounds its products, flex_spmm
    pads its rows: the header's n_r + 4 and nnz(row) + 32)."""
    row, col, rp = coo(a)
    k = Q.shape[1]
    Q64, K64, V64, g64, p64 = (np.asarray(x, np.float32).astype(np.float64) for x in (Q, K, V, g, p))
    sc = np.float64(np.float32(scale))
    n_r, n_c = np.diff(rp)[row], np.bincount(col, minlength=a.n)[col]
    with np.errstate(invalid="ignore", over="ignore"):
        da = (g64[row] * V64[col]).sum(1)
        dda = gamma(k) * (np.abs(g64[row]) * np.abs(V64[col])).sum(1) + k * 2.0 ** -149
        delta = _sum_by(p64 * da, row, a.m)
        ds = sc * p64 * (da - delta[row])
        ap = np.abs(p64)
        dds = (gamma(n_r + a_r) * sc * ap * (np.abs(da) + _sum_by(np.abs(p64 * da), row, a.m)[row])
               + sc * ap * (dda + _sum_by(ap * dda, row, a.m)[row]) + max(1.0, float(sc)) * n_r * 2.0 ** -149)
        gq = _sum_by(ds[:, None] * K64[col], row, a.m)
        gk = _sum_by(ds[:, None] * Q64[row], col, a.n)
        gv = _sum_by(p64[:, None] * g64[row], col, a.n)
        gq_b = _sum_by((gamma(n_r + b_r) * np.abs(ds) + dds)[:, None] * np.abs(K64[col]), row, a.m) + 2.0 ** -126
        gk_b = _sum_by((gamma(n_c + b_r) * np.abs(ds) + dds)[:, None] * np.abs(Q64[row]), col, a.n) + 2.0 ** -126
        gv_b = _sum_by((gamma(n_c + b_r) * ap)[:, None] * np.abs(g64[row]), col, a.n) + 2.0 ** -126
    return dict(gq=gq, gk=gk, gv=gv, ds=ds, gq_bound=gq_b, gk_bound=gk_b, gv_bound=gv_b, ds_bound=dds)


def fp32_result(a, Q, K, V, p, g, scale, drop_entry=None, unweighted_delta=False, no_scale=False):
    """(gQ, gK, gV, ds) as float32 from a float64 evaluation: what a right kernel returns up to roundings.  The faults the checker must
    catch: drop_entry = e: entry e is left out of its column's sums; unweighted_delta: delta is taken without the p weights; no_scale:
    scale is left out."""
    row, col, _ = coo(a)
    Q64, K64, V64, g64, p64 = (np.asarray(x, np.float64) for x in (Q, K, V, g, p))
    sc = 1.0 if no_scale else float(np.float32(scale))
    da = (g64[row] * V64[col]).sum(1)
    delta = _sum_by(da if unweighted_delta else p64 * da, row, a.m)
    ds = sc * p64 * (da - delta[row])
    keep = np.ones(len(ds))
    if drop_entry is not None:
        keep[drop_entry] = 0.0
    gq = _sum_by(ds[:, None] * K64[col], row, a.m)
    gk = _sum_by((keep * ds)[:, None] * Q64[row], col, a.n)
    gv = _sum_by((keep * p64)[:, None] * g64[row], col, a.n)
    return tuple(x.astype(np.float32) for x in (gq, gk, gv, ds))


def check(a, Q, K, V, p, g, scale, gQ=None, gK=None, gV=None, ds=None, what="", ratios=None):
    """Asserts, for every output given, the classes exactly (+0 rows without entries, NaN and infinities where float64 has them) and the
    bound on every other element; returns the worst err / bound (ratios, a dict: the worst of each output is kept in it)."""
    ref = reference(a, Q, K, V, p, g, scale)
    row, col, rp = coo(a)
    empty = {"gq": np.diff(rp) == 0, "gk": np.bincount(col, minlength=a.n) == 0}
    empty["gv"] = empty["gk"]
    worst = 0.0
    for key, got in (("gq", gQ), ("gk", gK), ("gv", gV), ("ds", ds)):
        if got is None:
            continue
        got, want, bound = np.asarray(got, np.float32), ref[key], ref[key + "_bound"]
        assert got.shape == want.shape, (what, key, got.shape, want.shape)
        if key in empty:
            assert np.all(got[empty[key]].view(np.uint32) == 0), f"{what}: a row of {key} without entries is not +0 in every column"
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: {key} is NaN where float64 is, and nowhere else ({int((np.isnan(got) != np.isnan(want)).sum())} differ)"
        inf = np.isinf(want)
        assert np.array_equal(got[inf].astype(np.float64), want[inf]) and not np.isinf(got[~inf]).any(), f"{what}: {key}: infinities as float64 gives them"
        fin = np.isfinite(want)
        ratio = np.abs(got[fin].astype(np.float64) - want[fin]) / bound[fin]
        w = float(ratio.max()) if ratio.size else 0.0
        assert w <= 1.0, f"{what}: {int((ratio > 1).sum())} elements of {key} beyond the bound, worst err / bound {w:.3g}"
        worst = max(worst, w)
        if ratios is not None:
            ratios[key] = max(w, ratios.get(key, 0.0))
    return worst

"""float64 reference, bounds, operands and checkers of the multi-head fused attention (include/flex_spmm.h: flex_attention_heads,
flex_attention_heads_backward), shared by tests/test_multihead_attention_host.py and tests/test_gpu_multihead_attention.py.

k = H d.  Head h is columns [h d, (h + 1) d) of Q, K, V, Out, g, gQ, gK and gV, and is the single-head definition at width d on those
columns: the reference is fused_attention_ref.reference and fused_attention_backward_ref.reference called per head on the head's column
slice and stacked, and the bounds are theirs with k = d (they take k from the slice's width).  The edge arrays P and ds are
[entries, H], entry-major: column h is head h's vector in CSR order."""
import numpy as np

import fused_attention_backward_ref as backward
import fused_attention_ref as forward
from fused_attention_ref import QKV_SCENARIOS, coo


def head_columns(k, heads, h):
    assert k % heads == 0, (k, heads)
    d = k // heads
    return slice(h * d, (h + 1) * d)


def scenarios_of(heads, shift=0):
    """One score scenario per head, so that the heads of one call differ: uniform4, spread80, masked30, rows_masked, poisoned in turn."""
    return [QKV_SCENARIOS[(h + shift) % len(QKV_SCENARIOS)] for h in range(heads)]


def operands(names, a, k, seed=0):
    """(Q [m, k], K [n, k], V [n, k]) fp32: head h holds fused_attention_ref.operands(names[h], a, d) under a seed of its own."""
    heads = len(names)
    parts = [forward.operands(name, a, k // heads, seed=100 * seed + h) for h, name in enumerate(names)]
    return tuple(np.ascontiguousarray(np.concatenate([p[i] for p in parts], axis=1)) for i in range(3))


def reference(a, Q, K, V, scale, heads, rows=None):
    """dict(out, out_bound [rows, k]; p, p_bound, s [entries, H]): the single-head reference per head, stacked."""
    k = Q.shape[1]
    refs = [forward.reference(a, *(x[:, head_columns(k, heads, h)] for x in (Q, K, V)), scale, rows) for h in range(heads)]
    res = {key: np.concatenate([r[key] for r in refs], axis=1) for key in ("out", "out_bound")}
    res.update({key: np.stack([r[key] for r in refs], axis=1) for key in ("p", "p_bound", "s")})
    return res


def check(a, Q, K, V, scale, heads, out, p=None, rows=None, what=""):
    """fused_attention_ref.check per head on the head's columns of Out and, where given, column h of P [entries, H]: the classes exactly
    (+0 rows, NaN rows, masked p = +0 bit for bit -- per head) and the per-head bound on every element; the worst err / bound."""
    k = Q.shape[1]
    out = np.asarray(out, np.float32)
    assert out.ndim == 2 and out.shape[1] == k, (what, out.shape, k)
    if p is not None:
        p = np.asarray(p, np.float32)
        assert p.ndim == 2 and p.shape[1] == heads, f"{what}: P is [entries, heads], entry-major; got {p.shape}"
    worst = 0.0
    for h in range(heads):
        c = head_columns(k, heads, h)
        worst = max(worst, forward.check(a, Q[:, c], K[:, c], V[:, c], scale, out[:, c], None if p is None else p[:, h], rows, what=f"{what} head {h}"))
    return worst


def backward_reference(a, Q, K, V, p, g, scale, heads):
    """dict(gq, gk, gv [., k]; ds [nnz, H] and their bounds): the single-head backward reference per head on p[:, h], stacked."""
    k = Q.shape[1]
    refs = [backward.reference(a, *(x[:, head_columns(k, heads, h)] for x in (Q, K, V)), p[:, h], g[:, head_columns(k, heads, h)], scale)
            for h in range(heads)]
    res = {key: np.concatenate([r[key] for r in refs], axis=1) for key in ("gq", "gk", "gv", "gq_bound", "gk_bound", "gv_bound")}
    res.update({key: np.stack([r[key] for r in refs], axis=1) for key in ("ds", "ds_bound")})
    return res


def check_backward(a, Q, K, V, p, g, scale, heads, gQ=None, gK=None, gV=None, ds=None, what="", ratios=None):
    """fused_attention_backward_ref.check per head; ds is [nnz, H].  The worst err / bound (ratios: the worst of each output)."""
    k = Q.shape[1]
    p = np.asarray(p, np.float32)
    assert p.shape == (a.nnz, heads), (what, p.shape)
    if ds is not None:
        assert np.asarray(ds).shape == (a.nnz, heads), f"{what}: ds is [nnz, heads], entry-major; got {np.asarray(ds).shape}"
    worst = 0.0
    for h in range(heads):
        c = head_columns(k, heads, h)
        worst = max(worst, backward.check(a, Q[:, c], K[:, c], V[:, c], p[:, h], g[:, c], scale, *(None if x is None else np.asarray(x)[:, c] for x in (gQ, gK, gV)),
                                          None if ds is None else np.asarray(ds)[:, h], what=f"{what} head {h}", ratios=ratios))
    return worst


def fp32_result(a, Q, K, V, scale, heads, joint_softmax=False, head_major=False, poison_spreads=False, next_heads_sum=False):
    """(Out [m, k], P [nnz, H]) as float32 from a float64 evaluation: what a right kernel returns up to roundings.  The faults the checker
    must catch: joint_softmax: one softmax over all heads' scores of a row; head_major: P delivered as [H, nnz] in the same memory;
    poison_spreads: a row that one head poisons is NaN in every head's columns; next_heads_sum: head h divides by head h + 1's sum.
    joint_softmax and next_heads_sum are evaluated here and want finite scores with every row live (uniform4, spread80)."""
    k = Q.shape[1]
    if not (joint_softmax or next_heads_sum):
        ref = reference(a, Q, K, V, scale, heads)
        with np.errstate(invalid="ignore", over="ignore"):
            out, p = ref["out"].astype(np.float32), ref["p"].astype(np.float32)
        if poison_spreads:
            out[np.isnan(out).any(1)] = np.nan
        if head_major:
            p = np.ascontiguousarray(p.T).reshape(p.shape)
        return out, p
    row, col, rp = coo(a)
    Q64, K64, V64 = (np.asarray(x, np.float64) for x in (Q, K, V))
    sc, m = float(np.float32(scale)), len(rp) - 1
    s = np.stack([(Q64[row][:, head_columns(k, heads, h)] * K64[col][:, head_columns(k, heads, h)]).sum(1) for h in range(heads)], axis=1)
    M = np.full((m, heads), -np.inf)
    np.maximum.at(M, row, s)
    if joint_softmax:
        M = np.repeat(M.max(1, keepdims=True), heads, axis=1)
    t = np.exp(sc * (s - M[row]))
    L = np.zeros((m, heads))
    np.add.at(L, row, t)
    if joint_softmax:
        L = np.repeat(L.sum(1, keepdims=True), heads, axis=1)
    if next_heads_sum:
        L = np.roll(L, -1, axis=1)
    p = t / L[row]
    out = np.zeros((m, k))
    for h in range(heads):
        c = head_columns(k, heads, h)
        np.add.at(out[:, c], row, p[:, h, None] * V64[col][:, c])
    return out.astype(np.float32), p.astype(np.float32)

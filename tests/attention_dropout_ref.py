"""The mask, float64 reference, bounds, checkers and planted faults of the attention dropout in the fused multi-head attention
(include/flex_spmm.h: flex_attention_dropout, flex_attention_dropout_backward and their bf16 forms, with or without the per-edge bias),
shared by tests/test_attention_dropout_host.py and tests/test_gpu_attention_dropout.py.

The mask is the header's, restated in numpy: mix on wrapping uint32, i = e H + h as uint64 (e the entry's index in a's CSR, also on a
row-range shard), r = mix(mix(lo32(i) + lo32(seed) + 0x9E3779B9) ^ (hi32(i) + hi32(seed))), kept iff r < thr(p).  The factor of an entry
and head is w = kept ? c : 0 with c = 1.0f / (1.0f - p) in fp32.

The reference is attention_bias_ref's (multihead_attention_ref's without a bias) with w inserted at three places, and a dropped entry
SELECTED OUT, not multiplied by zero:
    Out[r, head h] = sum_e alpha w V         alpha (P), the scores, the masks and the poison rules are the undropped reference's
    da_e = w <g, V>,  delta, ds, gBias, gQ, gK from da as before,  gV[c] = sum_e (p w) g
Bounds: the undropped ones, with every rounding count that now includes the product by c grown by one:
    Out     |Out - Out64| <= sum_{e kept} (gamma(n_r + 4) alpha_e + dalpha_e) c |V| + 2^-126
    da      dda_e = c (gamma(d + 1) sum_j |g V| + d 2^-149) + 2^-149 on a kept entry (the product by c >= 1 of a subnormal sum is inexact
            by at most 2^-150), 0 on a dropped one: its da is exactly +0
    ds, gBias, gQ, gK   fused_attention_backward_ref's and attention_bias_ref's lines on this da and dda (a = 3, b = 0)
    gV      |gV - gV64| <= sum_{e kept} gamma(n_c + 1) p_e c |g| + 2^-126       (p c >= p: no new underflow, p being 0 or normal)
No free multiplier: every element must have err <= bound.  bf16 rows: attention_bf16_ref's bound on Out, gQ, gK, gV; P, ds and gBias
keep the fp32 bounds."""
import numpy as np

import attention_bf16_ref as bf
import attention_bias_ref as ab
import fused_attention_backward_ref as backward
import multihead_attention_ref as mh
from fused_attention_ref import coo
from multihead_attention_ref import head_columns
from softmax_ref import gamma

M32 = np.uint64(0xFFFFFFFF)


# ---- the mask

def mix(x):
    """The mixer on wrapping uint32 arithmetic (x: uint64 holding 32-bit values)."""
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def bits(seed, i):
    """r(seed, i) for i an array of uint64 indices e H + h."""
    i = np.asarray(i, np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    first = mix(((i & M32) + lo + np.uint64(0x9E3779B9)) & M32)
    return mix(first ^ (((i >> np.uint64(32)) + hi) & M32))


def threshold(p):
    """thr = min(floor((1 - (double)p) 2^32), 2^32 - 1) for the fp32 value of p."""
    return min(int(np.floor((1.0 - float(np.float32(p))) * 4294967296.0)), 0xFFFFFFFF)


def keep(seed, p, i):
    """The keep bits (bool) of the indices i under seed and p."""
    return bits(seed, i) < np.uint64(threshold(p))


def factor(p):
    """c = 1.0f / (1.0f - p) as the float64 of its fp32 value."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def kept_entries(a, heads, p, seed, rows=None, fault=None):
    """keep [entries of the rows, H] (bool).  fault: a wrong index or test, as fp32_result lists them."""
    r0, r1 = (0, a.m) if rows is None else rows
    e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
    e = np.arange(0 if fault == "shard_local" else e0, (e1 - e0) if fault == "shard_local" else e1, dtype=np.uint64)[:, None]
    h = np.arange(heads, dtype=np.uint64)[None, :]
    if fault == "next_head":
        h = (h + np.uint64(1)) % np.uint64(heads)
    i = h * np.uint64(a.nnz) + e if fault == "head_major" else e * np.uint64(heads) + h
    kp = keep(int(seed) & 0xFFFFFFFF if fault == "seed_high_ignored" else seed, p, i)
    return ~kp if fault == "inverted" else kp


# ---- the reference

def _sum_by(x, seg, n):
    out = np.zeros((n,) + x.shape[1:])
    np.add.at(out, seg, x)
    return out


def _undropped(a, Q, K, V, bias, scale, heads, rows):
    return mh.reference(a, Q, K, V, scale, heads, rows) if bias is None else ab.reference(a, Q, K, V, bias, scale, heads, rows)


def reference(a, Q, K, V, bias, scale, heads, p, seed, rows=None):
    """dict(out, out_bound [rows, k]; p, p_bound, s, keep [entries of the rows, H]): p, p_bound and s are the undropped reference's."""
    k = Q.shape[1]
    res = _undropped(a, Q, K, V, bias, scale, heads, rows)
    row, col, rp = coo(a, rows)
    m = len(rp) - 1
    kp, c = kept_entries(a, heads, p, seed, rows), factor(p)
    V64 = np.asarray(V, np.float32).astype(np.float64)
    n_r = np.diff(rp)[row]
    out, ob = np.zeros((m, k)), np.zeros((m, k))
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(heads):
            cs, sel = head_columns(k, heads, h), kp[:, h]
            al = res["p"][sel, h]
            al0 = np.where(np.isnan(al), 0.0, al)
            np.add.at(out[:, cs], row[sel], (al * c)[:, None] * V64[col[sel]][:, cs])
            np.add.at(ob[:, cs], row[sel], ((gamma(n_r[sel] + 4) * al0 + res["p_bound"][sel, h]) * c)[:, None] * np.abs(V64[col[sel]][:, cs]))
            poisoned = np.zeros(m, bool)
            poisoned[row[np.isnan(res["p"][:, h])]] = True
            out[poisoned, cs] = np.nan  # a poisoned head is NaN whether or not its entries are kept
    res.update(out=out, out_bound=ob + 2.0 ** -126, keep=kp)
    return res


def _check_rows(got, want, bound, what, key, bf16, zero_rows=None):
    """One row-shaped output (fp32, or bf16 bits) against float64: +0 bits on zero_rows, NaN and infinities where float64 has them,
    the bound on every other element.  Returns the worst err / bound."""
    got = np.ascontiguousarray(got)
    assert got.dtype == (np.uint16 if bf16 else np.float32) and got.shape == want.shape, f"{what}: {key} is {got.dtype} {got.shape}"
    bits_ = got if bf16 else got.view(np.uint32)
    val = bf.from_bf16(got) if bf16 else got
    if zero_rows is not None:
        assert np.all(bits_[zero_rows] == 0), f"{what}: {key} is not +0 where nothing is summed"
    assert np.array_equal(np.isnan(val), np.isnan(want)), f"{what}: {key} is NaN where float64 is, and nowhere else ({int((np.isnan(val) != np.isnan(want)).sum())} differ)"
    inf = np.isinf(want)
    assert np.array_equal(val[inf].astype(np.float64), want[inf]), f"{what}: {key}: infinities as float64 gives them"
    fin = np.isfinite(want)
    assert np.isfinite(val[fin]).all(), f"{what}: {key} is not finite where float64 is"
    b = bf.bound_bf16(want[fin], bound[fin]) if bf16 else bound[fin]
    ratio = np.abs(val[fin].astype(np.float64) - want[fin]) / b
    w = float(ratio.max()) if ratio.size else 0.0
    assert w <= 1.0, f"{what}: {int((ratio > 1).sum())} elements of {key} beyond the bound, worst err / bound {w:.3g}"
    return w


def _check_edge(got, want, bound, what, key, shape):
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == shape, f"{what}: {key} is fp32 [entries, heads], entry-major; got {got.dtype} {got.shape}"
    return _check_rows(got, want, bound, what, key, False)


def check(a, Q, K, V, bias, scale, heads, p, seed, out, probs=None, rows=None, what="", ratios=None, bf16=False):
    """Out ([rows, k]: fp32, or bf16 bits with bf16=True) against the reference -- NaN in a poisoned head's columns and nowhere else, +0
    bits in a head of a row with no kept live entry (where the kept V rows are finite), non-finite values where float64 has them, the
    bound on every other element -- and, where given, P (fp32 [entries, H]) under the UNDROPPED checker.  Returns the worst err / bound."""
    ref = reference(a, Q, K, V, bias, scale, heads, p, seed, rows)
    k = Q.shape[1]
    row, col, rp = coo(a, rows)
    m = len(rp) - 1
    zero = np.zeros((m, k), bool)
    for h in range(heads):
        cs, sel = head_columns(k, heads, h), ref["keep"][:, h]
        busy = np.zeros(m, bool)  # a kept entry that is live (p > 0 or NaN) or whose V is not finite
        al = ref["p"][sel, h]
        busy[row[sel][~(al == 0) | ~np.isfinite(np.asarray(V, np.float64)[col[sel]][:, cs]).all(1)]] = True
        busy[row[np.isnan(ref["p"][:, h])]] = True  # a poisoned head is NaN even where none of its entries is kept
        zero[:, cs] = ~busy[:, None]
    worst = _check_rows(out, ref["out"], ref["out_bound"], what, "Out", bf16, zero_rows=zero)
    if ratios is not None:
        ratios["out"] = max(worst, ratios.get("out", 0.0))
    if probs is not None:  # the UNDROPPED alpha, under the undropped reference's classes and bound
        probs = np.asarray(probs)
        assert probs.dtype == np.float32 and probs.shape == ref["p"].shape, f"{what}: P is fp32 [entries, heads], entry-major; got {probs.dtype} {probs.shape}"
        nan_ref = np.isnan(ref["p"])
        assert np.array_equal(np.isnan(probs), nan_ref), f"{what}: P is NaN exactly on the poisoned rows of each head"
        masked = ~nan_ref & (ref["s"] == -np.inf)
        assert np.all(probs[masked].view(np.uint32) == 0), f"{what}: a masked entry is not +0 bit for bit"
        r = np.abs(probs[~nan_ref].astype(np.float64) - ref["p"][~nan_ref]) / ref["p_bound"][~nan_ref]
        wp = float(r.max()) if r.size else 0.0
        assert wp <= 1.0, f"{what}: {int((r > 1).sum())} entries of P beyond the bound (P holds the UNDROPPED alpha), worst err / bound {wp:.3g}"
        if ratios is not None:
            ratios["p"] = max(wp, ratios.get("p", 0.0))
        worst = max(worst, wp)
    return worst


def backward_reference(a, Q, K, V, probs, g, scale, heads, p, seed, da_unmasked=False, gv_unmasked=False):
    """dict(gq, gk, gv [., k]; ds, gb [nnz, H] and their bounds): float64 on the fp32 Q, K, V and g and on probs AS GIVEN (the kernel's
    fp32 undropped probabilities, or float64 ones for a comparison in float64)."""
    row, col, rp = coo(a)
    k = Q.shape[1]
    d = k // heads
    Q64, K64, V64, g64 = (np.asarray(x, np.float32).astype(np.float64) for x in (Q, K, V, g))
    p64 = np.asarray(probs, np.float64)
    assert p64.shape == (a.nnz, heads), (p64.shape, (a.nnz, heads))
    sc, c = np.float64(np.float32(scale)), factor(p)
    kp = kept_entries(a, heads, p, seed)
    n_r, n_c = np.diff(rp)[row], np.bincount(col, minlength=a.n)[col]
    res = {key: [] for key in ("gq", "gk", "gv", "ds", "gb", "gq_bound", "gk_bound", "gv_bound", "ds_bound", "gb_bound")}
    A = backward.A_ROUNDINGS
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(heads):
            cs, sel = head_columns(k, heads, h), kp[:, h]
            ph, ap = p64[:, h], np.abs(p64[:, h])
            gv_, Vv = g64[row][:, cs], V64[col][:, cs]
            dot = (gv_ * Vv).sum(1)
            da = dot if da_unmasked else np.where(sel, c * np.where(sel, dot, 0.0), 0.0)
            dda = np.where(sel, c * (gamma(d + 1) * np.where(sel, (np.abs(gv_) * np.abs(Vv)).sum(1), 0.0) + d * 2.0 ** -149) + 2.0 ** -149, 0.0)
            delta = _sum_by(ph * da, row, a.m)
            spread = np.abs(da) + _sum_by(np.abs(ph * da), row, a.m)[row]
            gb = ph * (da - delta[row])
            ds = sc * gb
            gbb = gamma(n_r + A) * ap * spread + ap * (dda + _sum_by(ap * dda, row, a.m)[row]) + n_r * 2.0 ** -149
            dds = gamma(n_r + A) * sc * ap * spread + sc * ap * (dda + _sum_by(ap * dda, row, a.m)[row]) + max(1.0, float(sc)) * n_r * 2.0 ** -149
            use = np.ones_like(sel) if gv_unmasked else sel  # the entries that add to gV
            pw = ph if gv_unmasked else c * ph
            res["gb"].append(gb), res["gb_bound"].append(gbb), res["ds"].append(ds), res["ds_bound"].append(dds)
            res["gq"].append(_sum_by(ds[:, None] * K64[col][:, cs], row, a.m))
            res["gk"].append(_sum_by(ds[:, None] * Q64[row][:, cs], col, a.n))
            res["gv"].append(_sum_by(pw[use, None] * gv_[use], col[use], a.n))
            res["gq_bound"].append(_sum_by((gamma(n_r) * np.abs(ds) + dds)[:, None] * np.abs(K64[col][:, cs]), row, a.m) + 2.0 ** -126)
            res["gk_bound"].append(_sum_by((gamma(n_c) * np.abs(ds) + dds)[:, None] * np.abs(Q64[row][:, cs]), col, a.n) + 2.0 ** -126)
            res["gv_bound"].append(_sum_by((gamma(n_c[use] + 1) * np.abs(pw[use]))[:, None] * np.abs(gv_[use]), col[use], a.n) + 2.0 ** -126)
    return {key: np.concatenate(v, axis=1) if key[:2] in ("gq", "gk", "gv") else np.stack(v, axis=1) for key, v in res.items()}


def check_backward(a, Q, K, V, probs, g, scale, heads, p, seed, gQ=None, gK=None, gV=None, gB=None, ds=None, what="", ratios=None, bf16=False):
    """For every output given (gQ, gK, gV: fp32, or bf16 bits with bf16=True; gB, ds: fp32 [nnz, H]): +0 bits on rows (columns) without
    entries and, in gV, in a head of a column without a kept entry; NaN and infinities where float64 has them; the bound on every other
    element.  Returns the worst err / bound (ratios: the worst of each output, gBias as "gb")."""
    probs = np.asarray(probs, np.float32)
    ref = backward_reference(a, Q, K, V, probs, g, scale, heads, p, seed)
    row, col, rp = coo(a)
    k = Q.shape[1]
    kp = kept_entries(a, heads, p, seed)
    empty_r = np.repeat((np.diff(rp) == 0)[:, None], k, 1)
    empty_c = np.repeat((np.bincount(col, minlength=a.n) == 0)[:, None], k, 1)
    none_kept = np.zeros((a.n, k), bool)
    for h in range(heads):
        any_kept = np.zeros(a.n, bool)
        any_kept[col[kp[:, h]]] = True
        none_kept[:, head_columns(k, heads, h)] = ~any_kept[:, None]
    worst = 0.0
    for key, got, zero in (("gq", gQ, empty_r), ("gk", gK, empty_c), ("gv", gV, none_kept)):
        if got is not None:
            w = _check_rows(got, ref[key], ref[key + "_bound"], what, key, bf16, zero_rows=zero)
            worst = max(worst, w)
            if ratios is not None:
                ratios[key] = max(w, ratios.get(key, 0.0))
    for key, got in (("ds", ds), ("gb", gB)):
        if got is not None:
            w = _check_edge(got, ref[key], ref[key + "_bound"], what, "gBias" if key == "gb" else "ds", (a.nnz, heads))
            worst = max(worst, w)
            if ratios is not None:
                ratios[key] = max(w, ratios.get(key, 0.0))
    return worst


# ---- what a right kernel returns up to roundings, and the faults the checkers must reject

FORWARD_FAULTS = ("shard_local", "head_major", "next_head", "inverted", "no_rescale", "c_over_p", "mask_before_norm", "seed_high_ignored",
                  "multiply_by_zero")
BACKWARD_FAULTS = ("gv_unmasked", "da_unmasked")
FAULTS = FORWARD_FAULTS + BACKWARD_FAULTS


def fp32_result(a, Q, K, V, bias, scale, heads, p, seed, g=None, probs=None, rows=None, fault=None):
    """dict(out [rows, k], p [entries, H]; with g also gq, gk, gv [., k], gb, ds [nnz, H]) as float32 from a float64 evaluation; the
    backward starts from `probs` (default: this forward's).  Faults:
      shard_local        on rows = (r0, r1): the mask is indexed from the shard's first entry
      head_major         the mask is taken at h nnz + e
      next_head          head h takes the bit of head h + 1 (the last head the first's)
      inverted           the keep test is inverted
      no_rescale         c = 1
      c_over_p           c = 1 / p
      mask_before_norm   the mask is applied before the normalisation: l sums the kept entries only, and P holds the dropped alpha
      seed_high_ignored  the seed's high word is ignored
      multiply_by_zero   a dropped entry is multiplied by zero instead of selected out (an inf V row behind it then reaches Out)
      gv_unmasked        gV = sum p g
      da_unmasked        da = <g, V>"""
    assert fault in (None,) + FAULTS, fault
    k = Q.shape[1]
    row, col, rp = coo(a, rows)
    m = len(rp) - 1
    res = _undropped(a, Q, K, V, bias, scale, heads, rows)
    kp = kept_entries(a, heads, p, seed, rows, fault if fault in ("shard_local", "head_major", "next_head", "inverted", "seed_high_ignored") else None)
    c = 1.0 if fault == "no_rescale" else 1.0 / float(np.float32(p)) if fault == "c_over_p" else factor(p)
    V64 = np.asarray(V, np.float32).astype(np.float64)
    pr = res["p"].copy()
    out = np.zeros((m, k))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if fault == "mask_before_norm":
            pr = np.where(kp, pr, 0.0)
            pr = pr / _sum_by(pr, row, m)[row]
        for h in range(heads):
            cs, sel = head_columns(k, heads, h), kp[:, h]
            if fault == "multiply_by_zero":
                np.add.at(out[:, cs], row, (pr[:, h] * np.where(sel, c, 0.0))[:, None] * V64[col][:, cs])
            else:
                np.add.at(out[:, cs], row[sel], (pr[sel, h] * c)[:, None] * V64[col[sel]][:, cs])
            poisoned = np.zeros(m, bool)
            poisoned[row[np.isnan(res["p"][:, h])]] = True
            out[poisoned, cs] = np.nan
        got = dict(out=out.astype(np.float32), p=pr.astype(np.float32))
    if g is None:
        return got
    assert rows is None, "the backward is not defined on shards"
    pin = got["p"] if probs is None else np.asarray(probs, np.float32)
    ref = backward_reference(a, Q, K, V, pin, g, scale, heads, p, seed, da_unmasked=fault == "da_unmasked", gv_unmasked=fault == "gv_unmasked")
    with np.errstate(invalid="ignore", over="ignore"):
        got.update({key: ref[key].astype(np.float32) for key in ("gq", "gk", "gv", "gb", "ds")})
    return got


def torch_float64(a, Q, K, V, bias, scale, heads, g, kp, c):
    """(Out, gQ, gK, gV, gBias) by torch autograd in float64 on the fp32 inputs with the mask kp [nnz, H] put in as a constant tensor
    (w = kp c), independent of the reference above; finite scores only.  bias may be None (gBias is then None)."""
    import torch
    row, col, _ = coo(a)
    k = Q.shape[1]
    d = k // heads
    row_t, col_t = torch.from_numpy(row), torch.from_numpy(col)
    Qt, Kt, Vt = (torch.from_numpy(np.ascontiguousarray(x, np.float32)).double().requires_grad_() for x in (Q, K, V))
    bt = None if bias is None else torch.from_numpy(np.ascontiguousarray(np.asarray(bias).reshape(a.nnz, heads), np.float32)).double().requires_grad_()
    s = (Qt.view(a.m, heads, d)[row_t] * Kt.view(a.n, heads, d)[col_t]).sum(2)
    t = float(np.float32(scale)) * s + (0.0 if bt is None else bt)
    M = torch.full((a.m, heads), -np.inf, dtype=torch.float64).scatter_reduce(0, row_t[:, None].expand(-1, heads), t.detach(), "amax")
    e = torch.exp(t - M[row_t])
    pr = e / torch.zeros((a.m, heads), dtype=torch.float64).index_add_(0, row_t, e)[row_t]
    w = torch.from_numpy(np.asarray(kp, np.float64) * c)
    out = torch.zeros((a.m, heads, d), dtype=torch.float64).index_add_(0, row_t, (pr * w)[:, :, None] * Vt.view(a.n, heads, d)[col_t]).reshape(a.m, k)
    out.backward(torch.from_numpy(np.ascontiguousarray(g, np.float32)).double())
    return tuple(None if x is None else x.numpy() for x in (out.detach(), Qt.grad, Kt.grad, Vt.grad, None if bt is None else bt.grad))

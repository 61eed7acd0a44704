"""The float64 reference, bounds, checkers and planted faults of the attention dropout in the fused GAT attention (include/flex_spmm.h:
flex_gat_attention_dropout, flex_gat_attention_dropout_backward), shared by tests/test_gat_dropout_host.py and
tests/test_gpu_gat_dropout.py.

The mask is attention_dropout_ref's (keep / kept_entries / factor: the header's hash of i = e H + h, e the entry's index in a's CSR, also
on a row-range shard), not a second copy.  The reference is gat_attention_ref's with w = kept ? c : 0 inserted at three places, and a
dropped entry SELECTED OUT, not multiplied by zero:
    Out[r, head h] = sum_e alpha w V         alpha (P), the scores, the masks and the poison rules are the undropped reference's
    da_e = w <g, V>,  delta, dz, dx, gEl, gEr from da as before (dx holds the mask through da: gEl and gEr do not see it again),
    gV[c] = sum_e (p w) g
Bounds: gat_attention_ref's, with every rounding count that now includes the product by c grown by one:
    Out     |Out - Out64| <= sum_{e kept} (gamma(n_r + 4) alpha_e + dalpha_e) c |V| + 2^-126
    da      dda_e = c (gamma(d + 1) sum_j |g V| + d 2^-149) + 2^-149 on a kept entry (the product by c >= 1 of a subnormal sum is inexact
            by at most 2^-150), 0 on a dropped one: its da is exactly +0
    dz, dx, gEl, gEr    gat_attention_ref's lines on this da and dda (a = 3, b = 0)
    gV      |gV - gV64| <= sum_{e kept} gamma(n_c + 1) p_e c |g| + 2^-126       (p c >= p: no new underflow, p being 0 or normal)
No free multiplier: every element must have err <= bound."""
import numpy as np

import attention_dropout_ref as ad
import gat_attention_ref as gat
from attention_dropout_ref import _check_edge, _check_rows, _sum_by, factor, kept_entries  # noqa: F401
from fused_attention_ref import coo
from multihead_attention_ref import head_columns
from softmax_ref import U, gamma

SLOPE = gat.SLOPE


# ---- the reference

def reference(a, el, er, V, slope, p, seed, rows=None):
    """dict(out, out_bound [rows, k]; p, p_bound, s, keep [entries of the rows, H]): p, p_bound and s are the undropped reference's."""
    k, heads = V.shape[1], el.shape[1]
    res = gat.reference(a, el, er, V, slope, rows)
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


def check(a, el, er, V, slope, p, seed, out, probs=None, rows=None, what="", ratios=None):
    """Out [rows, k] against the reference -- NaN in a poisoned head's columns and nowhere else, +0 bits in a head of a row with no kept
    live entry (where the kept V rows are finite), non-finite values where float64 has them, the bound on every other element -- and,
    where given, P (fp32 [entries, H]) under the UNDROPPED reference's classes and bound.  Returns the worst err / bound."""
    ref = reference(a, el, er, V, slope, p, seed, rows)
    k, heads = V.shape[1], el.shape[1]
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
    worst = _check_rows(out, ref["out"], ref["out_bound"], what, "Out", False, zero_rows=zero)
    if ratios is not None:
        ratios["out"] = max(worst, ratios.get("out", 0.0))
    if probs is not None:  # the UNDROPPED alpha
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


def backward_reference(a, el, er, V, probs, g, slope, p, seed, fault=None):
    """dict(gel [m, H], ger [n, H], gv [n, k], dx [nnz, H] and their bounds): float64 on the fp32 el, er, V and g and on probs AS GIVEN
    (the kernel's fp32 undropped probabilities, or float64 ones for a comparison in float64).  fault: one of BACKWARD_FAULTS."""
    row, col, rp = coo(a)
    k, heads = V.shape[1], el.shape[1]
    d = k // heads
    V64, g64 = (np.asarray(x, np.float32).astype(np.float64) for x in (V, g))
    p64 = np.asarray(probs, np.float64)
    assert p64.shape == (a.nnz, heads), (p64.shape, (a.nnz, heads))
    sl, c = np.float64(np.float32(slope)), factor(p)
    _, pos = gat.scores(a, el, er, slope)
    kp = kept_entries(a, heads, p, seed)
    n_r, n_c = np.diff(rp)[row], np.bincount(col, minlength=a.n)[col]
    res = {key: [] for key in ("gel", "ger", "gv", "dx", "gel_bound", "ger_bound", "gv_bound", "dx_bound")}
    A, B = gat.A_ROUNDINGS, gat.B_ROUNDINGS
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(heads):
            cs, sel = head_columns(k, heads, h), kp[:, h]
            ph, ap = p64[:, h], np.abs(p64[:, h])
            gv_, Vv = g64[row][:, cs], V64[col][:, cs]
            dot = (gv_ * Vv).sum(1)
            da = dot if fault == "da_unmasked" else np.where(sel, c * np.where(sel, dot, 0.0), 0.0)
            dda = np.where(sel, c * (gamma(d + 1) * np.where(sel, (np.abs(gv_) * np.abs(Vv)).sum(1), 0.0) + d * 2.0 ** -149) + 2.0 ** -149, 0.0)
            delta = _sum_by(ph * da, row, a.m)
            f = np.where(pos[:, h], 1.0, sl)
            dx = f * (ph * (da - delta[row]))
            ddz = gamma(n_r + A) * ap * (np.abs(da) + _sum_by(np.abs(ph * da), row, a.m)[row]) + ap * (dda + _sum_by(ap * dda, row, a.m)[row]) + n_r * 2.0 ** -149
            ddx = f * ddz + U * np.abs(dx) + 2.0 ** -149
            use = np.ones_like(sel) if fault == "gv_unmasked" else sel  # the entries that add to gV
            pw = ph if fault == "gv_unmasked" else c * ph
            res["dx"].append(dx), res["dx_bound"].append(ddx)
            res["gel"].append(_sum_by(np.where(sel, dx, 0.0) if fault == "gel_masked_twice" else dx, row, a.m))
            res["ger"].append(_sum_by(np.where(sel, dx, 0.0) if fault == "ger_masked_twice" else dx, col, a.n))
            res["gel_bound"].append(_sum_by(gamma(n_r + B) * np.abs(dx) + ddx, row, a.m) + 2.0 ** -126)
            res["ger_bound"].append(_sum_by(gamma(n_c + B) * np.abs(dx) + ddx, col, a.n) + 2.0 ** -126)
            res["gv"].append(_sum_by(pw[use, None] * gv_[use], col[use], a.n))
            res["gv_bound"].append(_sum_by((gamma(n_c[use] + 1) * np.abs(pw[use]))[:, None] * np.abs(gv_[use]), col[use], a.n) + 2.0 ** -126)
    return {key: np.concatenate(v, axis=1) if key.startswith("gv") else np.stack(v, axis=1) for key, v in res.items()}


def check_backward(a, el, er, V, probs, g, slope, p, seed, gEl=None, gEr=None, gV=None, dx=None, what="", ratios=None):
    """For every output given (fp32): +0 bits on rows of gEl and of gEr / gV without entries and, in gV, in a head of a column without a
    kept entry; NaN and infinities where float64 has them; the bound on every other element.  Returns the worst err / bound (ratios:
    the worst of each output)."""
    probs = np.asarray(probs, np.float32)
    ref = backward_reference(a, el, er, V, probs, g, slope, p, seed)
    row, col, rp = coo(a)
    k, heads = V.shape[1], el.shape[1]
    kp = kept_entries(a, heads, p, seed)
    empty_r = np.repeat((np.diff(rp) == 0)[:, None], heads, 1)
    empty_c = np.repeat((np.bincount(col, minlength=a.n) == 0)[:, None], heads, 1)
    none_kept = np.zeros((a.n, k), bool)
    for h in range(heads):
        any_kept = np.zeros(a.n, bool)
        any_kept[col[kp[:, h]]] = True
        none_kept[:, head_columns(k, heads, h)] = ~any_kept[:, None]
    worst = 0.0
    for key, got, zero in (("gel", gEl, empty_r), ("ger", gEr, empty_c), ("gv", gV, none_kept)):
        if got is not None:
            w = _check_rows(np.asarray(got), ref[key], ref[key + "_bound"], what, key, False, zero_rows=zero)
            worst = max(worst, w)
            if ratios is not None:
                ratios[key] = max(w, ratios.get(key, 0.0))
    if dx is not None:
        w = _check_edge(dx, ref["dx"], ref["dx_bound"], what, "dx", (a.nnz, heads))
        worst = max(worst, w)
        if ratios is not None:
            ratios["dx"] = max(w, ratios.get("dx", 0.0))
    return worst


# ---- what a right kernel returns up to roundings, and the faults the checkers must reject

FORWARD_FAULTS = ad.FORWARD_FAULTS
BACKWARD_FAULTS = ("gv_unmasked", "da_unmasked", "ger_masked_twice", "gel_masked_twice")
FAULTS = FORWARD_FAULTS + BACKWARD_FAULTS


def fp32_result(a, el, er, V, slope, p, seed, g=None, probs=None, rows=None, fault=None):
    """dict(out [rows, k], p [entries, H]; with g also gel [m, H], ger [n, H], gv [n, k], dx [nnz, H]) as float32 from a float64
    evaluation; the backward starts from `probs` (default: this forward's).  Faults:
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
      da_unmasked        da = <g, V>
      ger_masked_twice   gEr sums dx over the kept entries only (dx already holds the mask through da)
      gel_masked_twice   gEl likewise"""
    assert fault in (None,) + FAULTS, fault
    k, heads = V.shape[1], el.shape[1]
    row, col, rp = coo(a, rows)
    m = len(rp) - 1
    res = gat.reference(a, el, er, V, slope, rows)
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
    ref = backward_reference(a, el, er, V, pin, g, slope, p, seed, fault=fault if fault in BACKWARD_FAULTS else None)
    with np.errstate(invalid="ignore", over="ignore"):
        got.update({key: ref[key].astype(np.float32) for key in ("gel", "ger", "gv", "dx")})
    return got


def torch_float64(a, el, er, V, slope, g, kp, c):
    """(Out, gEl, gEr, gV) by torch autograd in float64 on the fp32 inputs with the mask kp [nnz, H] put in as a constant tensor
    (w = kp c), independent of the reference above; finite scores only."""
    import torch
    row, col, _ = coo(a)
    k, heads = V.shape[1], el.shape[1]
    d = k // heads
    row_t, col_t = torch.from_numpy(row), torch.from_numpy(col)
    el_t, er_t, V_t = (torch.from_numpy(np.ascontiguousarray(x, np.float32)).double().requires_grad_() for x in (el, er, V))
    s = torch.nn.functional.leaky_relu(el_t[row_t] + er_t[col_t], float(np.float32(slope)))
    M = torch.full((a.m, heads), -np.inf, dtype=torch.float64).scatter_reduce(0, row_t[:, None].expand(-1, heads), s.detach(), "amax")
    t = torch.exp(s - M[row_t])
    pr = t / torch.zeros((a.m, heads), dtype=torch.float64).index_add_(0, row_t, t)[row_t]
    w = torch.from_numpy(np.asarray(kp, np.float64) * c)
    out = torch.zeros((a.m, heads, d), dtype=torch.float64).index_add_(0, row_t, (pr * w)[:, :, None] * V_t.view(a.n, heads, d)[col_t]).reshape(a.m, k)
    out.backward(torch.from_numpy(np.ascontiguousarray(g, np.float32)).double())
    return out.detach().numpy(), el_t.grad.numpy(), er_t.grad.numpy(), V_t.grad.numpy()

"""The float64 reference, bounds, checkers, an fp32 evaluation and planted faults of the attention dropout in the fused GATv2 attention
(include/flex_spmm.h: flex_dropout_gatv2_attention, flex_dropout_gatv2_attention_backward), shared by
tests/test_gatv2_dropout_host.py and tests/test_gpu_gatv2_dropout.py.

The mask is attention_dropout_ref's (keep / kept_entries / factor: the header's hash of i = e H + h, e the entry's index in a's CSR, also
on a row-range shard), not a second copy.  The reference is gatv2_attention_ref's with w = kept ? c : 0 at three places, and a dropped
entry SELECTED OUT, not multiplied by zero.  x, s, alpha, f, L and w_ej = att_j f_ej are gatv2_attention_ref's:
    Out[r, head h] = sum_e alpha w Xs        alpha (P), the scores and the poison rules are the undropped reference's: a dropped entry
                                             is gathered all the same and stays in the softmax
    da_e = w <g, Xs>,  delta, dz from da as before
    gXt[r] = sum dz att f,  gAtt = sum dz L                  (the mask is in dz: they do not see it again)
    gXs[c] = sum_{e in c} dz att f  +  sum_{e in c, kept} (p c) g[row]          (the score term runs over ALL entries)
Bounds: gatv2_attention_ref's, with every rounding count that now includes the product by c grown by one (u, gamma, n_r, n_c, d as
there; C_ROUNDINGS = 3):
    Out     |Out - Out64| <= sum_{e kept} (gamma(n_r + C_ROUNDINGS + 1) alpha_e + dalpha_e) c |Xs| + 2^-126
    da      dda_e = c (gamma(d + 1) sum_j |g Xs| + d 2^-149) + 2^-149 on a kept entry (the product by c >= 1 of a subnormal sum is
            inexact by at most 2^-150), 0 on a dropped one: its da is exactly +0
    ddz, gXt, gAtt    gatv2_attention_ref's lines on this da and dda
    gXs     |gXs - gXs64| <= sum_{e in c} [(gamma(2 n_c + 1) |dz_e| + ddz_e) |w_ej| + |dz_e| 2^-149]
                             + sum_{e in c, kept} gamma(2 n_c + 1) p_e c |g[row]| + 2^-126
            (the kernel multiplies p by c, one rounding, and adds the product by one fma into the row of depth <= 2 n_c)
No free multiplier: every element must have err <= bound."""
import numpy as np

import attention_dropout_ref as ad
import gatv2_attention_ref as v2
from attention_dropout_ref import _check_edge, _check_rows, factor, kept_entries  # noqa: F401
from fused_attention_ref import coo
from gatv2_attention_ref import SUB, TINY, _dot32, _fma, _seg_fma, _sum_by
from multihead_attention_ref import head_columns
from softmax_ref import gamma

SLOPE = v2.SLOPE
F32 = np.float32


# ---- the reference

def reference(a, xt, xs, att, slope, p, seed, rows=None):
    """dict(out, out_bound [rows, k]; p, p_bound, s, keep [entries of the rows, H]): p, p_bound and s are the undropped reference's."""
    k, heads = xs.shape[1], att.shape[0]
    res = v2.reference(a, xt, xs, att, slope, rows)
    row, col, rp = coo(a, rows)
    m = len(rp) - 1
    kp, c = kept_entries(a, heads, p, seed, rows), factor(p)
    V64 = np.asarray(xs, np.float32).astype(np.float64)
    n_r = np.diff(rp)[row]
    out, ob = np.zeros((m, k)), np.zeros((m, k))
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(heads):
            cs, sel = head_columns(k, heads, h), kp[:, h]
            al = res["p"][sel, h]
            al0 = np.where(np.isnan(al), 0.0, al)
            np.add.at(out[:, cs], row[sel], (al * c)[:, None] * V64[col[sel]][:, cs])
            np.add.at(ob[:, cs], row[sel], ((gamma(n_r[sel] + v2.C_ROUNDINGS + 1) * al0 + res["p_bound"][sel, h]) * c)[:, None] * np.abs(V64[col[sel]][:, cs]))
            poisoned = np.zeros(m, bool)
            poisoned[row[np.isnan(res["p"][:, h])]] = True
            out[poisoned, cs] = np.nan  # a poisoned head is NaN whether or not its entries are kept
    res.update(out=out, out_bound=ob + TINY, keep=kp)
    return res


def check(a, xt, xs, att, slope, p, seed, out, probs=None, rows=None, what="", ratios=None):
    """Out [rows, k] against the reference -- NaN in a poisoned head's columns and where a kept entry with alpha = 0 meets an infinite
    Xs, +0 bits in a head of a row with no kept live entry (where the kept Xs rows are finite), non-finite values where float64 has
    them, the bound on every other element -- and, where given, P (fp32 [entries, H]) under the UNDROPPED reference's classes and
    bound.  Returns the worst err / bound."""
    ref = reference(a, xt, xs, att, slope, p, seed, rows)
    k, heads = xs.shape[1], att.shape[0]
    row, col, rp = coo(a, rows)
    m = len(rp) - 1
    zero = np.zeros((m, k), bool)
    for h in range(heads):
        cs, sel = head_columns(k, heads, h), ref["keep"][:, h]
        busy = np.zeros(m, bool)  # a kept entry that is live (p > 0 or NaN) or whose Xs is not finite
        al = ref["p"][sel, h]
        busy[row[sel][~(al == 0) | ~np.isfinite(np.asarray(xs, np.float64)[col[sel]][:, cs]).all(1)]] = True
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
        assert np.all(probs[masked].view(np.uint32) == 0), f"{what}: a masked entry of P is not +0 bit for bit"
        r = np.abs(probs[~nan_ref].astype(np.float64) - ref["p"][~nan_ref]) / ref["p_bound"][~nan_ref]
        wp = float(r.max()) if r.size else 0.0
        assert wp <= 1.0, f"{what}: {int((r > 1).sum())} entries of P beyond the bound (P holds the UNDROPPED alpha), worst err / bound {wp:.3g}"
        if ratios is not None:
            ratios["p"] = max(wp, ratios.get("p", 0.0))
        worst = max(worst, wp)
    return worst


def dz_lines(ph, da, dda, row, m, n_r):
    """(dz, ddz) of one head from its probabilities, da and dda [entries]: gatv2_attention_ref's lines."""
    ap = np.abs(ph)
    dz = ph * (da - _sum_by(ph * da, row, m)[row])
    ddz = gamma(n_r + v2.A_ROUNDINGS) * ap * (np.abs(da) + _sum_by(np.abs(ph * da), row, m)[row]) + ap * (dda + _sum_by(ap * dda, row, m)[row]) + n_r * SUB
    return dz, ddz


def backward_reference(a, xt, xs, att, probs, g, slope, p, seed, fault=None):
    """dict(gxt [m, k], gxs [n, k], gatt [H, d], dz [nnz, H] and their bounds): float64 on the fp32 xt, xs, att and g and on probs AS
    GIVEN (the kernel's fp32 undropped probabilities, or float64 ones for a comparison in float64).  fault: one of BACKWARD_FAULTS."""
    row, col, rp = coo(a)
    k, heads = xs.shape[1], att.shape[0]
    d = k // heads
    V64, g64 = (np.asarray(x, np.float32).astype(np.float64) for x in (xs, g))
    p64 = np.asarray(probs, np.float64)
    assert p64.shape == (a.nnz, heads), (p64.shape, (a.nnz, heads))
    c = factor(p)
    kp = kept_entries(a, heads, p, seed)
    n_r, n_c = np.diff(rp)[row], np.bincount(col, minlength=a.n)[col]
    T = v2.att_depth(a)
    res = {key: [] for key in ("gxt", "gxs", "gatt", "dz", "gxt_bound", "gxs_bound", "gatt_bound", "dz_bound")}
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(heads):
            cs, sel = head_columns(k, heads, h), kp[:, h]
            _, _, L, w = v2.head_terms(a, xt, xs, att, slope, h)
            ph, ap = p64[:, h], np.abs(p64[:, h])
            gr, vc = g64[row][:, cs], V64[col][:, cs]
            dot = np.where(sel[:, None], gr * vc, 0.0).sum(1)
            da = (gr * vc).sum(1) if fault == "da_unmasked" else np.where(sel, c * dot, 0.0)
            dda = np.where(sel, c * (gamma(d + 1) * np.where(sel[:, None], np.abs(gr) * np.abs(vc), 0.0).sum(1) + d * SUB) + SUB, 0.0)
            dz, ddz = dz_lines(ph, da, dda, row, a.m, n_r)
            adz = np.abs(dz)[:, None]
            twice = np.where(sel, dz, 0.0)  # what a sum that applies the mask again adds
            use = np.ones_like(sel) if fault == "gxs_value_unmasked" else sel  # the entries whose value term adds to gXs
            pw = ph if fault == "gxs_value_unmasked" else c * ph
            res["dz"].append(dz)
            res["dz_bound"].append(ddz)
            res["gxt"].append(_sum_by((twice if fault == "gxt_masked_twice" else dz)[:, None] * w, row, a.m))
            res["gxt_bound"].append(_sum_by((gamma(n_r + 1)[:, None] * adz + ddz[:, None]) * np.abs(w) + adz * SUB, row, a.m) + TINY)
            res["gxs"].append(_sum_by((twice if fault == "gxs_score_masked" else dz)[:, None] * w, col, a.n) + _sum_by(pw[use, None] * gr[use], col[use], a.n))
            res["gxs_bound"].append(_sum_by((gamma(2 * n_c + 1)[:, None] * adz + ddz[:, None]) * np.abs(w) + adz * SUB, col, a.n)
                                    + _sum_by((gamma(2 * n_c[use] + 1) * np.abs(pw[use]))[:, None] * np.abs(gr[use]), col[use], a.n) + TINY)
            res["gatt"].append(((twice if fault == "gatt_masked_twice" else dz)[:, None] * L).sum(0))
            res["gatt_bound"].append(((gamma(T + 3) * adz + ddz[:, None]) * np.abs(L) + adz * SUB).sum(0) + TINY)
    return {key: np.stack(v, axis=0 if key.startswith("gatt") else 1) if key.startswith(("gatt", "dz")) else np.concatenate(v, axis=1) for key, v in res.items()}


def check_backward(a, xt, xs, att, probs, g, slope, p, seed, gXt=None, gXs=None, gAtt=None, dz=None, what="", ratios=None):
    """For every output given (fp32): +0 bits on rows of gXt without entries and on rows of gXs whose column has no entry (NOT on a
    head of a column without a kept entry: the score term remains); NaN and infinities where float64 has them; the bound on every
    other element.  Returns the worst err / bound (ratios: the worst of each output)."""
    probs = np.asarray(probs, np.float32)
    ref = backward_reference(a, xt, xs, att, probs, g, slope, p, seed)
    _, col, rp = coo(a)
    k, heads = xs.shape[1], att.shape[0]
    empty_r = np.repeat((np.diff(rp) == 0)[:, None], k, 1)
    empty_c = np.repeat((np.bincount(col, minlength=a.n) == 0)[:, None], k, 1)
    worst = 0.0
    for key, got, zero in (("gxt", gXt, empty_r), ("gxs", gXs, empty_c), ("gatt", gAtt, None)):
        if got is not None:
            w = _check_rows(np.asarray(got), ref[key], ref[key + "_bound"], what, key, False, zero_rows=zero)
            worst = max(worst, w)
            if ratios is not None:
                ratios[key] = max(w, ratios.get(key, 0.0))
    if dz is not None:
        w = _check_edge(dz, ref["dz"], ref["dz_bound"], what, "dz", (a.nnz, heads))
        worst = max(worst, w)
        if ratios is not None:
            ratios["dz"] = max(w, ratios.get("dz", 0.0))
    return worst


# ---- an evaluation in fp32 arithmetic, and the faults the checkers must reject

FORWARD_FAULTS = ad.FORWARD_FAULTS + ("gather_skipped",)
BACKWARD_FAULTS = ("gxs_score_masked", "gxt_masked_twice", "gatt_masked_twice", "gxs_value_unmasked", "da_unmasked")
FAULTS = FORWARD_FAULTS + BACKWARD_FAULTS
_MASK_FAULTS = ("shard_local", "head_major", "next_head", "inverted", "seed_high_ignored")


def fp32_result(a, xt, xs, att, slope, p, seed, g=None, probs=None, rows=None, fault=None, partials=None):
    """dict(out [rows, k], p [entries, H]; with g also gxt [m, k], gxs [n, k], gatt [H, d], dz [nnz, H]) evaluated in fp32 arithmetic
    with numpy, as gatv2_attention_ref.fp32_result (fmas where the kernels use them, chains where they use trees): what a right kernel
    returns up to the order of its additions.  The backward starts from `probs` (default: this forward's).  Faults:
      shard_local        on rows = (r0, r1): the mask is indexed from the shard's first entry
      head_major         the mask is taken at h nnz + e
      next_head          head h takes the bit of head h + 1 (the last head the first's)
      inverted           the keep test is inverted
      no_rescale         c = 1
      c_over_p           c = 1 / p
      mask_before_norm   the mask is applied before the normalisation: l sums the kept entries only, and P holds the dropped alpha
      seed_high_ignored  the seed's high word is ignored
      multiply_by_zero   a dropped entry is multiplied by zero instead of selected out (an inf Xs row behind it then reaches Out)
      gather_skipped     GATv2's own: a dropped entry's Xs row is not gathered, so its score is formed from a zero row
      gxs_score_masked   the score term of gXs sums over the kept entries only (dz already holds the mask through da)
      gxt_masked_twice   gXt likewise
      gatt_masked_twice  gAtt likewise
      gxs_value_unmasked the value term of gXs is sum p g
      da_unmasked        da = <g, Xs>
    partials = gatv2_attention_ref.att_work_layout(...): with g, also att_work [rows, k], every row of dAttWork as a chain of fmas over
    its entries in entry order, and gatt is then att_reduce32 of these rows."""
    assert fault in (None,) + FAULTS, fault
    row, col, rp = coo(a, rows)
    m, k, heads = len(rp) - 1, xs.shape[1], att.shape[0]
    d = k // heads
    sl = F32(slope)
    xt, xs, att = (np.asarray(x, F32) for x in (xt, xs, att))
    kp = kept_entries(a, heads, p, seed, rows, fault if fault in _MASK_FAULTS else None)
    c = F32(1.0) if fault == "no_rescale" else F32(1.0) / F32(p) if fault == "c_over_p" else F32(factor(p))
    S, Ls, Ws = [], [], []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for h in range(heads):
            cs = head_columns(k, heads, h)
            xsr = xs[col][:, cs]
            if fault == "gather_skipped":
                xsr = np.where(kp[:, h, None], xsr, F32(0))
            x = xt[row][:, cs] + xsr
            pos = x > 0
            L = np.where(pos, x, sl * x).astype(F32)
            S.append(_dot32(att[h], L))
            Ls.append(L)
            Ws.append(np.where(pos, att[h], att[h] * sl).astype(F32))
        s = np.stack(S, 1)
        key = np.where(np.isnan(s) | (s == np.inf), np.inf, s).astype(F32)
        M = np.full((m, heads), -np.inf, F32)
        np.maximum.at(M, row, key)
        poisoned, dead = M == np.inf, M == -np.inf
        Mf = np.where(poisoned | dead, F32(0), M)
        t = np.where(s == -np.inf, F32(0), np.exp((s - Mf[row]).astype(F32))).astype(F32)
        t = np.where(poisoned[row] | dead[row], F32(0), t)
        if fault == "mask_before_norm":
            t = np.where(kp, t, F32(0))
        Lsum = np.zeros((m, heads), F32)
        np.add.at(Lsum, row, t)
        pr = np.where(dead[row], F32(0), t / np.where(dead, F32(1), Lsum)[row]).astype(F32)
        pr[poisoned[row]] = np.nan
        out = np.zeros((m, k), F32)
        for h in range(heads):
            cs, sel = head_columns(k, heads, h), kp[:, h]
            if fault == "multiply_by_zero":
                o = _seg_fma([(np.where(sel, (t[:, h] * c).astype(F32), F32(0)), xs[col][:, cs])], row, m, d)
            else:
                o = _seg_fma([((t[sel, h] * c).astype(F32), xs[col[sel]][:, cs])], row[sel], m, d)
            o = np.where(dead[:, h, None], o, o / np.where(dead[:, h], F32(1), Lsum[:, h])[:, None]).astype(F32)
            o[poisoned[:, h]] = np.nan
            out[:, cs] = o
    res = dict(out=out, p=pr)
    if g is None:
        return res
    assert rows is None, "the backward is not defined on shards"
    pin = res["p"] if probs is None else np.asarray(probs, F32)
    g = np.asarray(g, F32)
    gxt, gxs, gatt, dzs = np.zeros((a.m, k), F32), np.zeros((a.n, k), F32), np.zeros((heads, d), F32), []
    chunk = 512
    rows32 = None if partials is None else np.zeros((partials[1], k), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(heads):
            cs, sel = head_columns(k, heads, h), kp[:, h]
            ph = pin[:, h]
            dot = _dot32(g[row][:, cs], xs[col][:, cs])
            da = dot if fault == "da_unmasked" else np.where(sel, (c * dot).astype(F32), F32(0))
            delta = _seg_fma([(ph, da[:, None])], row, a.m, 1)[:, 0]
            dz = (ph * (da - delta[row]).astype(F32)).astype(F32)
            dzs.append(dz)
            twice = np.where(sel, dz, F32(0))
            gxt[:, cs] = _seg_fma([(twice if fault == "gxt_masked_twice" else dz, Ws[h])], row, a.m, d)
            if fault == "gxs_value_unmasked":
                pe, gg = ph, g[row][:, cs]
            else:  # a dropped entry's g row is not gathered: its term is 0 x 0
                pe, gg = np.where(sel, (ph * c).astype(F32), F32(0)), np.where(sel[:, None], g[row][:, cs], F32(0))
            gxs[:, cs] = _seg_fma([(twice if fault == "gxs_score_masked" else dz, Ws[h]), (pe, gg)], col, a.n, d)
            part = _seg_fma([(twice if fault == "gatt_masked_twice" else dz, Ls[h])], np.arange(a.nnz) // chunk, -(-a.nnz // chunk), d)
            tot = np.zeros(d, F32)
            for r in range(part.shape[0]):
                tot = (tot + part[r]).astype(F32)
            gatt[h] = tot
            if partials is not None:
                rows32[:, cs] = _seg_fma([(twice if fault == "gatt_masked_twice" else dz, Ls[h])], partials[0], partials[1], d)
    res.update(gxt=gxt, gxs=gxs, gatt=gatt, dz=np.stack(dzs, 1))
    if partials is not None:
        res.update(att_work=rows32, gatt=v2.att_reduce32(rows32).reshape(heads, d))
    return res


def torch_float64(a, xt, xs, att, slope, g, kp, c):
    """(Out, P, gXt, gXs, gAtt) by torch autograd in float64 on the fp32 inputs with the mask kp [nnz, H] put in as a constant tensor
    (w = kp c) behind a plain softmax per row, independent of the reference above; finite scores only."""
    import torch
    row, col, _ = coo(a)
    k, heads = xs.shape[1], att.shape[0]
    d = k // heads
    row_t, col_t = torch.from_numpy(row.astype(np.int64)), torch.from_numpy(col.astype(np.int64))
    xt_t, xs_t, att_t = (torch.from_numpy(np.ascontiguousarray(x, np.float32)).double().requires_grad_() for x in (xt, xs, att))
    x = (xt_t[row_t] + xs_t[col_t]).view(-1, heads, d)
    s = (torch.nn.functional.leaky_relu(x, float(np.float32(slope))) * att_t).sum(-1)
    pr = torch.cat([torch.softmax(s[int(a.rowPtr[r]):int(a.rowPtr[r + 1])], 0) for r in range(a.m)], 0)
    w = torch.from_numpy(np.asarray(kp, np.float64) * c)
    out = torch.zeros((a.m, heads, d), dtype=torch.float64).index_add_(0, row_t, (pr * w)[:, :, None] * xs_t.view(a.n, heads, d)[col_t]).reshape(a.m, k)
    out.backward(torch.from_numpy(np.ascontiguousarray(g, np.float32)).double())
    return out.detach().numpy(), pr.detach().numpy(), xt_t.grad.numpy(), xs_t.grad.numpy(), att_t.grad.numpy()


def propagated_bounds(a, xt, xs, att, slope, g, p, seed):
    """(Out, gXt, gXs, gAtt) bounds of a forward and backward step against float64 THROUGHOUT, for finite scores:
    gatv2_attention_ref.propagated_bounds with this module's da and dda (c <g, Xs> and its bound on a kept entry, 0 on a dropped one),
    this module's Out bound, and (gamma(2 n_c + 1) alpha_e + dalpha_e) c |g| over the kept entries for the value term of gXs.  First
    order, 0.1 % spare."""
    ref = reference(a, xt, xs, att, slope, p, seed)
    row, col, rp = coo(a)
    k, heads = xs.shape[1], att.shape[0]
    d = k // heads
    V64, g64 = (np.asarray(x, np.float64) for x in (xs, g))
    n_r, n_c = np.diff(rp)[row], np.bincount(col, minlength=a.n)[col]
    T, c = v2.att_depth(a), factor(p)
    gxt, gxs, gatt = [], [], []
    for h in range(heads):
        cs, sel = head_columns(k, heads, h), ref["keep"][:, h]
        _, _, L, w = v2.head_terms(a, xt, xs, att, slope, h)
        al, dal = ref["p"][:, h], ref["p_bound"][:, h]
        gr, vc = g64[row][:, cs], V64[col][:, cs]
        da = np.where(sel, c * (gr * vc).sum(1), 0.0)
        ada = np.abs(da)
        dda = np.where(sel, c * (gamma(d + 1) * (np.abs(gr) * np.abs(vc)).sum(1) + d * SUB) + SUB, 0.0)
        spread = ada + _sum_by(al * ada, row, a.m)[row]
        ddz = (gamma(n_r + v2.A_ROUNDINGS) * al * spread + n_r * SUB + dal * spread + al * (dda + _sum_by(dal * ada + al * dda, row, a.m)[row]))[:, None]
        adz = np.abs(al * (da - _sum_by(al * da, row, a.m)[row]))[:, None]
        gxt.append(_sum_by((gamma(n_r + 1)[:, None] * adz + ddz) * np.abs(w) + adz * SUB, row, a.m) + TINY)
        gxs.append(_sum_by((gamma(2 * n_c + 1)[:, None] * adz + ddz) * np.abs(w) + adz * SUB, col, a.n)
                   + _sum_by(((gamma(2 * n_c[sel] + 1) * al[sel] + dal[sel]) * c)[:, None] * np.abs(gr[sel]), col[sel], a.n) + TINY)
        gatt.append(((gamma(T + 3) * adz + ddz) * np.abs(L) + adz * SUB).sum(0) + TINY)
    return tuple(1.001 * t for t in (ref["out_bound"], np.concatenate(gxt, 1), np.concatenate(gxs, 1), np.stack(gatt, 0)))

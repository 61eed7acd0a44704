"""float64 reference, bounds, operands, checkers and planted faults of the fused attention with a per-edge bias (include/flex_spmm.h:
flex_attention_bias, flex_attention_bias_backward and their bf16 forms), shared by tests/test_attention_bias_host.py and
tests/test_gpu_attention_bias.py.

k = H d; head h is columns [h d, (h + 1) d) of the row operands and column h of the edge arrays bias, P, gBias and ds, all [nnz, H],
entry-major, in CSR order.  Forward, float64 on the fp32 inputs (the fp32 value of scale, the fp32 bias):
    s_eh = <Q[r, head h], K[src(e), head h]>,  t_eh = scale s_eh + bias[e, h],  alpha = flex_edge_softmax's softmax of t rounded to fp32,
    scale 1 (softmax_ref.forward_ref: -inf is a masked entry, a row of -inf is +0, a +inf or NaN poisons the row),  Out = sum alpha V.
Bounds, verbatim (u = 2^-24, gamma(n) = n u / (1 - n u), n_r = entries of the row, E = softmax_ref.E_ULP, R_r = ceil(n_r / 4) + 8):
    score   dt_e     = scale (gamma(d) sum_j |Q K| + d 2^-149) + u |t_e| + 2^-149
    alpha   dalpha_e = alpha_e [gamma(n_r + 4 D_r + (E + 3) R_r + 2 E + 4) + expm1(2 max_row dt)] + 2^-126,  D_r = min(104, spread of finite t)
    Out     |Out - Out64| <= sum_e (gamma(n_r + 3) alpha_e + dalpha_e) |V| + 2^-126
The backward never sees the bias: gQ, gK, gV and ds are multihead_attention_ref.backward_reference on the same p (its checkers are used
as they are), and gBias = p (da - delta) is that reference's ds at scale 1, whose bound at scale 1 (a = 3) is the header's gBias line:
    gBias   |gB - gB64| <= gamma(n_r + 3) p_e (|da_e| + sum_j |p_j da_j|) + p_e (dda_e + sum_j p_j dda_j) + n_r 2^-149
bf16 rows: attention_bf16_ref's bound on Out, gQ, gK, gV; P, ds and gBias keep the fp32 bounds."""
import numpy as np

import attention_bf16_ref as bf
import fused_attention_backward_ref as backward
import multihead_attention_ref as mh
from fused_attention_ref import coo
from multihead_attention_ref import head_columns
from softmax_ref import E_ULP, U, _per_row, _segments, forward_ref, gamma

BIAS_SCENARIOS = ["zero", "uniform4", "spread80", "masked30", "rows_masked", "poisoned", "opposed"]


def scenarios_of(heads, shift=0):
    """One bias scenario per head, rotating as multihead_attention_ref.scenarios_of does."""
    return [BIAS_SCENARIOS[(h + shift) % len(BIAS_SCENARIOS)] for h in range(heads)]


def _sum_by(x, seg, n):
    out = np.zeros((n,) + x.shape[1:])
    np.add.at(out, seg, x)
    return out


def _chosen_rows(rp, rng):
    """Rows with entries: the first, the longest and a tenth of the rest, without the middle one (it stays live)."""
    deg = np.diff(rp)
    ne = np.flatnonzero(deg > 0)
    return sorted({int(ne[0]), int(ne[np.argmax(deg[ne])]), *rng.choice(ne, max(1, len(ne) // 10)).tolist()} - {int(ne[len(ne) // 2])})


def operands(names, a, k, seed=0, bf16=False):
    """(Q [m, k], K [n, k], V [n, k], bias [nnz, H]) fp32, head h under the bias scenario names[h].  Q and K are finite with scores within
    +-4 in every head (multihead_attention_ref's uniform4), so what masks, poisons and decides a row is the bias alone:
    zero; uniform4: +-4; spread80: +-39, so that with the scale of 1 / 4 of the table (scale s within +-1) the t of a row are spread by
    up to 80 and the bias decides the row; masked30: 30 % of the entries -inf; rows_masked: 10 % -inf and every entry of some chosen rows;
    poisoned: masks, one +inf and one NaN in two rows.  The spread stops at 80 so that every p > 0 is a NORMAL number on rows of up to
    513 entries (p >= e^-80 / 513 > 2^-126): flex_attention_heads_backward's bound on ds, which holds here unchanged, grants products
    below 2^-126 n_r 2^-149 and so does not cover fl(scale p) of a SUBNORMAL p -- off by up to 2^-150 -- multiplied by a da - delta
    beyond n_r.  With a bias of +-80 such p arise (p = 2 x 2^-149, scale 1 / 4, da - delta = -5.2 on a row of two entries: err / bound
    1.29 on the GPU, and the same figure from the fp32 expressions on the host); the unbiased call has the same limit.  opposed: a few K rows hold +inf in the head's first column, so an entry into one
    of them scores +inf or -inf by the sign of Q there, and the bias of every such entry is -inf: +inf against -inf is a NaN t, which
    poisons the row, where a kernel that applied the mask before the score would leave it live.  bf16: Q, K, V are bf16 numbers."""
    heads = len(names)
    Q, K, V = mh.operands(["uniform4"] * heads, a, k, seed=seed)
    if bf16:
        Q, K, V = (bf.rounded(x) for x in (Q, K, V))
    row, col, rp = coo(a)
    bias = np.zeros((a.nnz, heads), np.float32)
    for h, name in enumerate(names):
        rng = np.random.default_rng([seed, BIAS_SCENARIOS.index(name), k, h])
        b = bias[:, h]
        if name != "zero":
            b[:] = rng.uniform(-39 if name == "spread80" else -4, 39 if name == "spread80" else 4, a.nnz)
        if a.nnz == 0:
            continue
        if name in ("masked30", "rows_masked", "poisoned"):
            b[rng.random(a.nnz) < (0.3 if name == "masked30" else 0.1)] = -np.inf
        if name == "rows_masked":
            for r in _chosen_rows(rp, rng):
                b[rp[r]:rp[r + 1]] = -np.inf
        if name == "poisoned":
            deg = np.diff(rp)
            ne = np.flatnonzero(deg > 0)
            b[rp[ne[0]]] = np.inf
            b[rp[ne[np.argmax(deg[ne])] + 1] - 1] = np.nan
        if name == "opposed":
            c0 = head_columns(k, heads, h).start
            hot = np.unique(col[rng.integers(0, a.nnz, 3)])
            K[hot, c0] = np.inf
            b[np.isin(col, hot)] = -np.inf
    return Q, K, V, bias


def _bias_of(a, bias, heads, rows):
    bias = np.asarray(bias, np.float32)
    if bias.ndim == 1 and heads == 1:
        bias = bias[:, None]
    assert bias.shape == (a.nnz, heads), f"bias is [nnz, heads] over ALL of a's entries, entry-major; got {bias.shape}"
    r0, r1 = (0, a.m) if rows is None else rows
    return bias[int(a.rowPtr[r0]):int(a.rowPtr[r1])].astype(np.float64)


def _head_reference(row, col, rp, Q64, K64, V64, b64, sc):
    m, d = len(rp) - 1, Q64.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        s = (Q64[row] * K64[col]).sum(1)
        T = (np.abs(Q64[row]) * np.abs(K64[col])).sum(1)
        t = sc * s + b64
    if t.size == 0:
        z = np.zeros((m, d))
        return dict(out=z, out_bound=z + 2.0 ** -126, p=t, p_bound=t, s=t)
    with np.errstate(over="ignore"):
        t32 = t.astype(np.float32)
    p, _ = forward_ref(rp, t32, 1.0)
    starts, seg, n_r = _segments(rp)
    fin = np.isfinite(t)
    dt = np.where(fin, sc * (gamma(d) * np.where(fin, T, 0.0) + d * 2.0 ** -149) + U * np.abs(np.where(fin, t, 0.0)) + 2.0 ** -149, 0.0)
    dt_row = _per_row(np.maximum, dt, starts, seg)
    hi = _per_row(np.maximum, np.where(fin, t32.astype(np.float64), -np.inf), starts, seg)
    lo = _per_row(np.minimum, np.where(fin, t32.astype(np.float64), np.inf), starts, seg)
    with np.errstate(invalid="ignore"):
        D = np.where(hi == -np.inf, 0.0, np.minimum(104.0, hi - lo))
    R = np.ceil(n_r / 4.0) + 8
    p0 = np.where(np.isnan(p), 0.0, p)
    p_bound = p0 * (gamma(n_r + 4 * D + (E_ULP + 3) * R + 2 * E_ULP + 4) + np.expm1(2 * dt_row)) + 2.0 ** -126
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.zeros((m, d))
        np.add.at(out, row, p[:, None] * V64[col])
        ob = np.zeros((m, d))
        np.add.at(ob, row, (gamma(n_r + 3) * p0 + p_bound)[:, None] * np.abs(V64[col]))
    return dict(out=out, out_bound=ob + 2.0 ** -126, p=p, p_bound=p_bound, s=t32)


def reference(a, Q, K, V, bias, scale, heads, rows=None):
    """dict(out, out_bound [rows, k]; p, p_bound, s [entries of the rows, H], s being t rounded to fp32).  rows = (r0, r1): Q holds the
    shard's rows, bias ALL of a's entries (the shard's are read at a's indices)."""
    k = Q.shape[1]
    row, col, rp = coo(a, rows)
    b = _bias_of(a, bias, heads, rows)
    Q64, K64, V64 = (np.asarray(x, np.float32).astype(np.float64) for x in (Q, K, V))
    sc = np.float64(np.float32(scale))
    refs = [_head_reference(row, col, rp, *(x[:, head_columns(k, heads, h)] for x in (Q64, K64, V64)), b[:, h], sc) for h in range(heads)]
    res = {key: np.concatenate([r[key] for r in refs], axis=1) for key in ("out", "out_bound")}
    res.update({key: np.stack([r[key] for r in refs], axis=1) for key in ("p", "p_bound", "s")})
    return res


def check(a, Q, K, V, bias, scale, heads, out, p=None, rows=None, what="", ratios=None, bf16=False):
    """Out ([rows, k]: fp32, or bf16 bits as uint16 with bf16=True) and, where given, P (fp32 [entries, H]) against the reference: per
    head the classes exactly (NaN in a poisoned head's d columns and nowhere else, +0 bits on a row without a live entry, non-finite
    values where float64 has them, masked p = +0 bit for bit) and the bound on every element.  Returns the worst err / bound (ratios, a
    dict: the worst of "out" and "p")."""
    ref = reference(a, Q, K, V, bias, scale, heads, rows)
    k = Q.shape[1]
    out = np.ascontiguousarray(out)
    assert out.dtype == (np.uint16 if bf16 else np.float32) and out.shape == ref["out"].shape, f"{what}: Out is {out.dtype} {out.shape}"
    bits = out if bf16 else out.view(np.uint32)
    val = bf.from_bf16(out) if bf16 else out
    row, col, rp = coo(a, rows)
    m = len(rp) - 1
    for h in range(heads):
        c = head_columns(k, heads, h)
        poisoned, live, vfin = np.zeros(m, bool), np.zeros(m, bool), np.ones(m, bool)
        if row.size:
            poisoned[row[np.isnan(ref["p"][:, h])]] = True
            live[row[np.nan_to_num(ref["p"][:, h]) > 0]] = True
            vfin[row[~np.isfinite(np.asarray(V, np.float64)[col][:, c]).all(1)]] = False
        assert np.all(np.isnan(val[poisoned][:, c])), f"{what} head {h}: a row with a +inf or NaN score is not NaN in every column of the head"
        zero = ~poisoned & ~live & vfin
        assert np.all(bits[zero][:, c] == 0), f"{what} head {h}: a row without a live entry is not +0 in every column"
        want, got = ref["out"][~poisoned][:, c], val[~poisoned][:, c]
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), f"{what} head {h}: non-finite values not exactly where float64 has them"
    ok = np.isfinite(ref["out"])
    bound = bf.bound_bf16(ref["out"][ok], ref["out_bound"][ok]) if bf16 else ref["out_bound"][ok]
    ratio = np.abs(val[ok].astype(np.float64) - ref["out"][ok]) / bound
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} elements of Out beyond the bound, worst err / bound {worst:.3g}"
    if ratios is not None:
        ratios["out"] = max(worst, ratios.get("out", 0.0))
    if p is not None:
        p = np.asarray(p)
        assert p.dtype == np.float32 and p.shape == ref["p"].shape, f"{what}: P is fp32 [entries, heads], entry-major; got {p.dtype} {p.shape}"
        nan_ref = np.isnan(ref["p"])
        assert np.array_equal(np.isnan(p), nan_ref), f"{what}: P is NaN exactly on the poisoned rows of each head"
        masked = ~nan_ref & (ref["s"] == -np.inf)
        assert np.all(p[masked].view(np.uint32) == 0), f"{what}: a masked entry is not +0 bit for bit"
        r = np.abs(p[~nan_ref].astype(np.float64) - ref["p"][~nan_ref]) / ref["p_bound"][~nan_ref]
        wp = float(r.max()) if r.size else 0.0
        assert wp <= 1.0, f"{what}: {int((r > 1).sum())} entries of P beyond the bound, worst err / bound {wp:.3g}"
        if ratios is not None:
            ratios["p"] = max(wp, ratios.get("p", 0.0))
        worst = max(worst, wp)
    return worst


def backward_reference(a, Q, K, V, p, g, scale, heads):
    """dict(gq, gk, gv [., k]; ds, gb, gb_bound [nnz, H]): float64 on the fp32 Q, K, V and g and on p AS GIVEN -- the kernel's fp32
    probabilities, where gq, gk, gv and ds are multihead_attention_ref.backward_reference's to the last bit (whose bounds check_backward
    uses), or float64 ones for a comparison in float64.  gb = p (da - delta); gb_bound is the header's gBias line, which is
    fused_attention_backward_ref's dds at scale 1."""
    row, col, rp = coo(a)
    k = Q.shape[1]
    d = k // heads
    Q64, K64, V64, g64 = (np.asarray(x, np.float32).astype(np.float64) for x in (Q, K, V, g))
    p64 = np.asarray(p, np.float64)
    assert p64.shape == (a.nnz, heads), (p64.shape, (a.nnz, heads))
    sc = np.float64(np.float32(scale))
    n_r = np.diff(rp)[row]
    res = {key: [] for key in ("gq", "gk", "gv", "ds", "gb", "gb_bound")}
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(heads):
            c = head_columns(k, heads, h)
            ph, ap = p64[:, h], np.abs(p64[:, h])
            da = (g64[row][:, c] * V64[col][:, c]).sum(1)
            dda = gamma(d) * (np.abs(g64[row][:, c]) * np.abs(V64[col][:, c])).sum(1) + d * 2.0 ** -149
            delta = _sum_by(ph * da, row, a.m)
            ds = sc * ph * (da - delta[row])
            res["gb"].append(ph * (da - delta[row]))
            res["gb_bound"].append(gamma(n_r + backward.A_ROUNDINGS) * ap * (np.abs(da) + _sum_by(np.abs(ph * da), row, a.m)[row])
                                   + ap * (dda + _sum_by(ap * dda, row, a.m)[row]) + n_r * 2.0 ** -149)
            res["ds"].append(ds)
            res["gq"].append(_sum_by(ds[:, None] * K64[col][:, c], row, a.m))
            res["gk"].append(_sum_by(ds[:, None] * Q64[row][:, c], col, a.n))
            res["gv"].append(_sum_by(ph[:, None] * g64[row][:, c], col, a.n))
    return {key: np.concatenate(v, axis=1) if key in ("gq", "gk", "gv") else np.stack(v, axis=1) for key, v in res.items()}


def check_backward(a, Q, K, V, p, g, scale, heads, gQ=None, gK=None, gV=None, gB=None, ds=None, what="", ratios=None, bf16=False):
    """gQ, gK, gV (fp32, or bf16 bits with bf16=True) and ds (fp32 [nnz, H]) under the unbiased checkers unchanged (the backward does not
    see the bias), and gB (fp32 [nnz, H]) against p (da - delta): NaN and infinities where float64 has them, the bound on every other
    element.  Returns the worst err / bound (ratios: the worst of each output, gBias as "gb")."""
    p = np.asarray(p, np.float32)
    worst = (bf if bf16 else mh).check_backward(a, Q, K, V, p, g, scale, heads, gQ, gK, gV, ds, what=what, ratios=ratios)
    if gB is not None:
        gB = np.asarray(gB)
        assert gB.dtype == np.float32 and gB.shape == (a.nnz, heads), f"{what}: gBias is fp32 [nnz, heads], entry-major; got {gB.dtype} {gB.shape}"
        ref = backward_reference(a, Q, K, V, p, g, scale, heads)
        want, bound = ref["gb"], ref["gb_bound"]
        assert np.array_equal(np.isnan(gB), np.isnan(want)), f"{what}: gBias is NaN where float64 is, and nowhere else ({int((np.isnan(gB) != np.isnan(want)).sum())} differ)"
        inf = np.isinf(want)
        assert np.array_equal(gB[inf].astype(np.float64), want[inf]) and not np.isinf(gB[~inf]).any(), f"{what}: gBias: infinities as float64 gives them"
        fin = np.isfinite(want)
        ratio = np.abs(gB[fin].astype(np.float64) - want[fin]) / bound[fin]
        w = float(ratio.max()) if ratio.size else 0.0
        assert w <= 1.0, f"{what}: {int((ratio > 1).sum())} elements of gBias beyond the bound, worst err / bound {w:.3g}"
        worst = max(worst, w)
        if ratios is not None:
            ratios["gb"] = max(w, ratios.get("gb", 0.0))
    return worst


# ---- what a right kernel returns up to roundings, and the faults the checkers must reject

FORWARD_FAULTS = ("no_bias", "bias_in_scale", "max_before_bias", "next_head", "head_major", "shard_local")
BACKWARD_FAULTS = ("gb_scaled", "gb_no_delta", "gb_unweighted_delta", "work_holds_gb")
FAULTS = FORWARD_FAULTS + BACKWARD_FAULTS


def fp32_result(a, Q, K, V, bias, scale, heads, g=None, p=None, rows=None, fault=None):
    """dict(out [rows, k], p [entries, H]; with g also gq, gk, gv [., k], gb, ds [nnz, H]) as float32 from a float64 evaluation; the
    backward starts from `p` (default: this forward's).  Faults:
      no_bias               the bias is left out
      bias_in_scale         t = scale (s + b)
      max_before_bias       the row maximum is taken over scale s, the bias is added afterwards: a row masked through the bias alone
                            divides 0 by 0, and a +inf bias is no longer seen by the maximum
      next_head             head h reads bias[e H + h + 1] (the last head the first)
      head_major            the bias is read at h nnz + e
      shard_local           on rows = (r0, r1): the bias is indexed from the shard's first entry
      gb_scaled             gBias = ds
      gb_no_delta           gBias = p da
      gb_unweighted_delta   gBias = p (da - sum_j da_j)
      work_holds_gb         dWork holds gBias"""
    assert fault in (None,) + FAULTS, fault
    k = Q.shape[1]
    row, col, rp = coo(a, rows)
    m = len(rp) - 1
    Q64, K64, V64 = (np.asarray(x, np.float32).astype(np.float64) for x in (Q, K, V))
    sc = float(np.float32(scale))
    full = np.asarray(bias, np.float32).reshape(a.nnz, heads).astype(np.float64)
    if fault == "next_head":
        full = np.roll(full, -1, axis=1)
    if fault == "head_major":
        full = np.ascontiguousarray(full.reshape(heads, a.nnz).T)
    b = full[: len(row)] if fault == "shard_local" else full[int(rp[0]):int(rp[-1])]
    if fault is None or fault in BACKWARD_FAULTS or fault in ("next_head", "head_major", "shard_local"):
        refs = [_head_reference(row, col, rp, *(x[:, head_columns(k, heads, h)] for x in (Q64, K64, V64)), b[:, h], np.float64(sc)) for h in range(heads)]
        out, pr = np.concatenate([r["out"] for r in refs], axis=1), np.stack([r["p"] for r in refs], axis=1)
    else:
        out, pr = np.zeros((m, k)), np.zeros((len(row), heads))
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for h in range(heads):
                c = head_columns(k, heads, h)
                s = (Q64[row][:, c] * K64[col][:, c]).sum(1)
                t = sc * s if fault == "no_bias" else sc * (s + b[:, h]) if fault == "bias_in_scale" else sc * s + b[:, h]
                M = np.full(m, -np.inf)
                np.maximum.at(M, row, sc * s if fault == "max_before_bias" else t)
                e = np.exp(t - M[row])
                pr[:, h] = e / _sum_by(e, row, m)[row]
                np.add.at(out[:, c], row, pr[:, h, None] * V64[col][:, c])
    with np.errstate(invalid="ignore", over="ignore"):
        res = dict(out=out.astype(np.float32), p=pr.astype(np.float32))
    if g is None:
        return res
    assert rows is None, "the backward is not defined on shards"
    pin = res["p"] if p is None else np.asarray(p, np.float32)
    ref = backward_reference(a, Q, K, V, pin, g, scale, heads)
    g64, p64 = np.asarray(g, np.float32).astype(np.float64), pin.astype(np.float64)
    gb, ds = ref["gb"], ref["ds"]
    if fault == "gb_scaled":
        gb = ds
    if fault in ("gb_no_delta", "gb_unweighted_delta"):
        da = np.stack([(g64[row][:, head_columns(k, heads, h)] * V64[col][:, head_columns(k, heads, h)]).sum(1) for h in range(heads)], axis=1)
        gb = p64 * da if fault == "gb_no_delta" else p64 * (da - _sum_by(da, row, a.m)[row])
    if fault == "work_holds_gb":
        ds = gb
    with np.errstate(invalid="ignore", over="ignore"):
        res.update(gq=ref["gq"].astype(np.float32), gk=ref["gk"].astype(np.float32), gv=ref["gv"].astype(np.float32), gb=gb.astype(np.float32),
                   ds=ds.astype(np.float32))
    return res


# ---- a forward and backward step against float64 throughout

def propagated_bounds(a, Q, K, V, bias, scale, heads, g, composition=False):
    """(Out, gQ, gK, gV [., k], gBias [nnz, H]) bounds of a forward and backward step against float64 THROUGHOUT, for finite t: the
    backward starts from the forward's fp32 alpha, so alpha's own bound dalpha enters every gradient beside the backward's bounds (first
    order, 0.1 % spare), as in tests/test_gpu_fused_attention_backward.py (_fused_backward_tolerances), per head at width d:
        dgt_e = gamma(n_r + 3) alpha_e (|da_e| + sum_j alpha_j |da_j|) + n_r 2^-149
                + dalpha_e (|da_e| + sum_j alpha_j |da_j|) + alpha_e (dda_e + sum_j (dalpha_j |da_j| + alpha_j dda_j))          -> gBias
        dds_e = scale dgt_e + max(1, scale) n_r 2^-149                                                                      -> gQ, gK
    composition=True: the bounds of the chain flex_sddmm, t = fl(fl(scale s) + b) in torch, flex_edge_softmax at scale 1, flex_spmm and
    their backward calls instead, as tests/test_gpu_attention.py propagates them (_attention_tolerances: P = 32 for flex_spmm's padding,
    n_r + 4 for flex_edge_softmax_backward, gamma(8) on alpha), with one more rounding in t (u scale |s|, through the softmax) and one in
    gS = fl(scale gt) (u |ds|)."""
    ref = reference(a, Q, K, V, bias, scale, heads)
    row, col, rp = coo(a)
    k = Q.shape[1]
    d = k // heads
    sc = float(np.float32(scale))
    Q64, K64, V64, g64 = (np.asarray(x, np.float32).astype(np.float64) for x in (Q, K, V, g))
    n_r, n_c = np.diff(rp)[row], np.bincount(col, minlength=a.n)[col]
    P, a_r = (32, 4) if composition else (0, 3)
    outb, gq, gk, gv, gb = [], [], [], [], []
    for h in range(heads):
        c = head_columns(k, heads, h)
        al, dal = ref["p"][:, h], ref["p_bound"][:, h]
        if composition:
            dal = dal + al * (np.expm1(2 * U * _sum_by_max(sc * np.abs((Q64[row][:, c] * K64[col][:, c]).sum(1)), row, a.m)[row]) + gamma(8))
            outb.append(_sum_by((gamma(n_r + P) * al + dal)[:, None] * np.abs(V64[col][:, c]), row, a.m) + 2.0 ** -126)
        da = (g64[row][:, c] * V64[col][:, c]).sum(1)
        ada = np.abs(da)
        dda = gamma(d) * (np.abs(g64[row][:, c]) * np.abs(V64[col][:, c])).sum(1) + d * 2.0 ** -149
        spread = ada + _sum_by(al * ada, row, a.m)[row]
        dgt = gamma(n_r + a_r) * al * spread + n_r * 2.0 ** -149 + dal * spread + al * (dda + _sum_by(dal * ada + al * dda, row, a.m)[row])
        ds = np.abs(sc * al * (da - _sum_by(al * da, row, a.m)[row]))
        dds = sc * dgt + (U * ds if composition else 0.0) + max(1.0, sc) * n_r * 2.0 ** -149
        gb.append(dgt)
        gq.append(_sum_by((gamma(n_r + P) * ds + dds)[:, None] * np.abs(K64[col][:, c]), row, a.m) + 2.0 ** -126)
        gk.append(_sum_by((gamma(n_c + P) * ds + dds)[:, None] * np.abs(Q64[row][:, c]), col, a.n) + 2.0 ** -126)
        gv.append(_sum_by((gamma(n_c + P) * al + dal)[:, None] * np.abs(g64[row][:, c]), col, a.n) + 2.0 ** -126)
    out_bound = np.concatenate(outb, 1) if composition else ref["out_bound"]
    return tuple(1.001 * t for t in (out_bound, np.concatenate(gq, 1), np.concatenate(gk, 1), np.concatenate(gv, 1), np.stack(gb, 1)))


def _sum_by_max(x, seg, n):
    out = np.zeros(n)
    np.maximum.at(out, seg, x)
    return out


def torch_float64(a, Q, K, V, bias, scale, heads, g):
    """(Out, gQ, gK, gV, gBias) by torch autograd in float64 on the fp32 inputs, independent of the reference above; finite t only."""
    import torch
    row, col, _ = coo(a)
    k = Q.shape[1]
    d = k // heads
    row_t, col_t = torch.from_numpy(row), torch.from_numpy(col)
    Qt, Kt, Vt, bt = (torch.from_numpy(np.ascontiguousarray(x, np.float32)).double().requires_grad_() for x in (Q, K, V, np.asarray(bias).reshape(a.nnz, heads)))
    s = (Qt.view(a.m, heads, d)[row_t] * Kt.view(a.n, heads, d)[col_t]).sum(2)
    t = float(np.float32(scale)) * s + bt
    M = torch.full((a.m, heads), -np.inf, dtype=torch.float64).scatter_reduce(0, row_t[:, None].expand(-1, heads), t.detach(), "amax")
    e = torch.exp(t - M[row_t])
    p = e / torch.zeros((a.m, heads), dtype=torch.float64).index_add_(0, row_t, e)[row_t]
    out = torch.zeros((a.m, heads, d), dtype=torch.float64).index_add_(0, row_t, p[:, :, None] * Vt.view(a.n, heads, d)[col_t]).reshape(a.m, k)
    out.backward(torch.from_numpy(np.ascontiguousarray(g, np.float32)).double())
    return tuple(x.numpy() for x in (out.detach(), Qt.grad, Kt.grad, Vt.grad, bt.grad))

"""float64 reference, bounds, operands and checkers of the fused GAT attention (include/flex_spmm.h: flex_gat_attention,
flex_gat_attention_backward), shared by tests/test_gat_attention_host.py and tests/test_gpu_gat_attention.py.

k = H d.  Head h is columns [h d, (h + 1) d) of V, Out, g and gV; el is [rows, H], er is [n, H]; the edge arrays P and dx are
[entries, H], entry-major.  For row r, entry e in CSR order, src(e) the entry's column, head h:
    x_eh     = el[r, h] + er[src(e), h]
    s_eh     = x_eh > 0 ? x_eh : slope x_eh
    alpha_eh = flex_edge_softmax's softmax of s_.h over the row, scale 1      (softmax_ref.forward_ref on the score rounded to fp32)
    Out[r, head h] = sum_e alpha_eh V[src(e), head h]
    da_eh    = <g[r, head h], V[src(e), head h]>
    delta_rh = sum_j p_jh da_jh
    dz_eh    = p_eh (da_eh - delta_rh)
    dx_eh    = x_eh > 0 ? dz_eh : slope dz_eh
    gEl[r, h] = sum_{e in row r} dx_eh      gEr[c, h] = sum_{src(e) == c} dx_eh      gV[c, head h] = sum_{src(e) == c} p_eh g[row(e), head h]
The reference is float64 numpy on the fp32 inputs; it takes the branch of the leaky ReLU from the sign of the fp32 sum fl(el + er), which is
what the kernel sees, and uses the fp32 value of slope.  Bounds, verbatim (u = 2^-24, gamma(n) = n u / (1 - n u), n_r = entries of the
row, n_c = entries of the column, D_r = min(104, the spread of the row's finite scores), E = softmax_ref.E_ULP, R_r = ceil(n_r / 4) + 8):
    score   ds_e     = gamma(2) |s_e| + 2^-149
    alpha   dalpha_e = alpha_e [gamma(n_r + 4 D_r + (E + 3) R_r + 2 E + 4) + expm1(2 max_row(ds + |s| u))] + 2^-126
    Out     |Out - Out64| <= sum_e (gamma(n_r + 3) alpha_e + dalpha_e) |V| + 2^-126
    dda_e    = gamma(d) sum_j |g V| + d 2^-149
    ddz_e    = gamma(n_r + 3) p_e (|da_e| + sum_j |p_j da_j|) + p_e (dda_e + sum_j p_j dda_j) + n_r 2^-149
    ddx_e    = f_e ddz_e + u |dx_e| + 2^-149,   f_e = 1 where x_e > 0, else slope
    |gEl - gEl64| <= sum_{e in r} (gamma(n_r) |dx_e| + ddx_e) + 2^-126
    |gEr - gEr64| <= sum_{e in c} (gamma(n_c) |dx_e| + ddx_e) + 2^-126
    |gV  - gV64|  <= sum_{e in c}  gamma(n_c) p_e |g[row]|    + 2^-126"""
import numpy as np

from fused_attention_backward_ref import both_sides  # noqa: F401  (the tests take the lifted graph from here)
from fused_attention_ref import coo, threshold_graph  # noqa: F401
from multihead_attention_ref import head_columns
from softmax_ref import E_ULP, U, _per_row, _segments, forward_ref, gamma

SLOPE = 0.2
SCENARIOS = ["uniform4", "spread80", "masked30", "rows_masked", "poisoned", "zero"]


def scenarios_of(heads, shift=0):
    """One scenario per head, in turn, so that the heads of one call differ."""
    return [SCENARIOS[(h + shift) % len(SCENARIOS)] for h in range(heads)]


def _head_operands(name, a, seed):
    """(el [m], er [n]) fp32 of one head.  uniform4 / spread80: x = el + er spans +-4 / +-80, both signs in most rows.  masked30:
    er = -inf on 30 % of the columns.  rows_masked: 10 %, every column some chosen rows touch, and el = -inf on other chosen rows.
    poisoned: masks, and a NaN in el for three rows, the longest among them.  zero: for the first entry of every third row with
    entries el[r] = -er[c] exactly, so x = +0 there."""
    rng = np.random.default_rng([seed, SCENARIOS.index(name)])
    half = 40.0 if name == "spread80" else 2.0
    el, er = (rng.uniform(-half, half, r).astype(np.float32) for r in (a.m, a.n))
    _, col, rp = coo(a)
    deg = np.diff(rp)
    ne = np.flatnonzero(deg > 0)
    if name in ("masked30", "rows_masked", "poisoned"):
        masked = rng.random(a.n) < (0.3 if name == "masked30" else 0.1)
        if name == "rows_masked" and len(ne):
            chosen = {int(ne[0]), int(ne[np.argmax(deg[ne])]), *rng.choice(ne, max(1, len(ne) // 10)).tolist()} - {int(ne[len(ne) // 2])}
            for r in chosen:
                masked[col[rp[r]:rp[r + 1]]] = True
            el[[int(r) for r in rng.choice(ne, max(1, len(ne) // 10)) if int(r) != int(ne[len(ne) // 2])]] = -np.inf
        er[masked] = -np.inf
        if name == "poisoned" and len(ne):
            el[sorted({int(ne[0]), int(ne[np.argmax(deg[ne])]), int(ne[len(ne) // 2])})] = np.nan
    if name == "zero":
        for r in ne[::3]:
            el[r] = -er[col[rp[r]]]
    return el, er


def operands(names, a, k, seed=0):
    """(el [m, H], er [n, H], V [n, k]) fp32: head h holds scenario names[h] under a seed of its own."""
    heads = len(names)
    assert k % heads == 0
    parts = [_head_operands(name, a, 100 * seed + h) for h, name in enumerate(names)]
    el, er = (np.ascontiguousarray(np.stack([p[i] for p in parts], axis=1)) for i in range(2))
    V = np.random.default_rng([seed, k, 7]).uniform(-1, 1, (a.n, k)).astype(np.float32)
    return el, er, V


def _sum_by(x, seg, n):
    out = np.zeros((n,) + x.shape[1:])
    np.add.at(out, seg, x)
    return out


def scores(a, el, er, slope, rows=None):
    """(s64 [entries, H], positive [entries, H]): the float64 score with the branch taken from the fp32 sum's sign."""
    row, col, _ = coo(a, rows)
    el32, er32 = np.asarray(el, np.float32), np.asarray(er, np.float32)
    sl = np.float64(np.float32(slope))
    with np.errstate(invalid="ignore", over="ignore"):
        pos = (el32[row] + er32[col]) > 0
        x = el32.astype(np.float64)[row] + er32.astype(np.float64)[col]
        s = np.where(pos, x, sl * x)
    return s, pos


C_ROUNDINGS, A_ROUNDINGS, B_ROUNDINGS = 3, 3, 0


def reference(a, el, er, V, slope, rows=None, c_r=C_ROUNDINGS):
    """dict(out, out_bound [rows, k]; p, p_bound, s [entries, H]) of the rows [r0, r1) (el holds those rows only).  c_r = 32 gives the
    bound of the composition of engine calls instead (flex_spmm pads its rows: the header's nnz(row) + 32)."""
    row, col, rp = coo(a, rows)
    m, k, heads = len(rp) - 1, V.shape[1], el.shape[1]
    assert el.shape[0] == m and er.shape == (a.n, heads), (el.shape, er.shape)
    V64 = np.asarray(V, np.float32).astype(np.float64)
    if len(row) == 0:
        z, e = np.zeros((m, k)), np.zeros((0, heads))
        return dict(out=z, out_bound=z + 2.0 ** -126, p=e, p_bound=e, s=e)
    s, _ = scores(a, el, er, slope, rows)
    with np.errstate(over="ignore"):
        s32 = s.astype(np.float32)
    starts, seg, n_r = _segments(rp)
    R = np.ceil(n_r / 4.0) + 8
    out, ob = np.zeros((m, k)), np.zeros((m, k))
    ps, pbs = [], []
    for h in range(heads):
        p, _ = forward_ref(rp, s32[:, h], 1.0)
        fin = np.isfinite(s[:, h])
        # ds_e + |s_e| u, the argument of max_row in dalpha: the header's ds with the |s| u of the expm1 term folded in, as
        # fused_attention_ref.reference does -- not a raised constant
        ds = np.where(fin, (gamma(2) + U) * np.abs(np.where(fin, s[:, h], 0.0)) + 2.0 ** -149, 0.0)
        ds_row = _per_row(np.maximum, ds, starts, seg)
        hi = _per_row(np.maximum, np.where(fin, s32[:, h].astype(np.float64), -np.inf), starts, seg)
        lo = _per_row(np.minimum, np.where(fin, s32[:, h].astype(np.float64), np.inf), starts, seg)
        with np.errstate(invalid="ignore"):
            D = np.where(hi == -np.inf, 0.0, np.minimum(104.0, hi - lo))
        p0 = np.where(np.isnan(p), 0.0, p)
        pb = p0 * (gamma(n_r + 4 * D + (E_ULP + 3) * R + 2 * E_ULP + 4) + np.expm1(2 * ds_row)) + 2.0 ** -126
        c = head_columns(k, heads, h)
        with np.errstate(invalid="ignore", over="ignore"):
            np.add.at(out[:, c], row, p[:, None] * V64[col][:, c])
            np.add.at(ob[:, c], row, (gamma(n_r + c_r) * p0 + pb)[:, None] * np.abs(V64[col][:, c]))
        ps.append(p)
        pbs.append(pb)
    return dict(out=out, out_bound=ob + 2.0 ** -126, p=np.stack(ps, 1), p_bound=np.stack(pbs, 1), s=s32)


def check(a, el, er, V, slope, out, p=None, rows=None, what=""):
    """Asserts per head the classes exactly (+0 rows, NaN rows, masked p = +0 bit for bit, non-finite values exactly where float64 has
    them) and the bound on every element of Out and, where given, of P [entries of the rows, H]; returns the worst err / bound."""
    ref = reference(a, el, er, V, slope, rows)
    heads, k = el.shape[1], V.shape[1]
    out = np.asarray(out, np.float32)
    assert out.shape == ref["out"].shape, (what, out.shape, ref["out"].shape)
    if p is not None:
        p = np.asarray(p, np.float32)
        assert p.shape == ref["p"].shape, f"{what}: P is [entries, heads], entry-major; got {p.shape}, want {ref['p'].shape}"
    row, col, rp = coo(a, rows)
    deg = np.diff(rp)
    worst = 0.0
    for h in range(heads):
        c, w = head_columns(k, heads, h), f"{what} head {h}"
        rp_h, o, ro, rb = ref["p"][:, h], out[:, c], ref["out"][:, c], ref["out_bound"][:, c]
        poisoned = np.zeros(len(deg), bool)
        poisoned[row[np.isnan(rp_h)]] = True
        assert np.all(np.isnan(o[poisoned])), f"{w}: a row with a +inf or NaN score is not NaN in every column of its head"
        live = np.zeros(len(deg), bool)
        live[row[np.nan_to_num(rp_h) > 0]] = True
        vfin = np.ones(len(deg), bool)
        vfin[row[~np.isfinite(np.asarray(V, np.float64)[col][:, c]).all(1)]] = False
        zero = ~poisoned & ~live & vfin
        assert np.all(o[zero].view(np.uint32) == 0), f"{w}: a row without a live entry is not +0 in every column"
        rest = ~poisoned[:, None] & np.ones_like(ro, bool)
        assert np.array_equal(np.isfinite(o)[rest], np.isfinite(ro)[rest]), f"{w}: non-finite values not exactly where float64 has them"
        ok = rest & np.isfinite(ro)
        ratio = np.abs(o[ok].astype(np.float64) - ro[ok]) / rb[ok]
        wo = float(ratio.max()) if ratio.size else 0.0
        assert wo <= 1.0, f"{w}: {int((ratio > 1).sum())} elements of Out beyond the bound, worst err / bound {wo:.3g}"
        worst = max(worst, wo)
        if p is not None:
            ph, nan_ref = p[:, h], np.isnan(rp_h)
            assert np.array_equal(np.isnan(ph), nan_ref), f"{w}: P is NaN exactly on the poisoned rows"
            masked = ~nan_ref & (ref["s"][:, h] == -np.inf)
            assert np.all(ph[masked].view(np.uint32) == 0), f"{w}: a masked entry is not +0 bit for bit"
            r = np.abs(ph[~nan_ref].astype(np.float64) - rp_h[~nan_ref]) / ref["p_bound"][:, h][~nan_ref]
            wp = float(r.max()) if r.size else 0.0
            assert wp <= 1.0, f"{w}: {int((r > 1).sum())} entries of P beyond the bound, worst err / bound {wp:.3g}"
            worst = max(worst, wp)
    return worst


def backward_reference(a, el, er, V, p, g, slope, a_r=A_ROUNDINGS, b_r=B_ROUNDINGS):
    """dict(gel [m, H], ger [n, H], gv [n, k], dx [nnz, H] and their bounds gel_bound, ...): float64 on the operands as given (p is
    taken as it is: the kernel's fp32 probabilities, or float64 ones for a comparison in float64).  a_r = 4 and b_r = 32 give the
    bounds of the chain of engine calls on the same p instead (flex_edge_softmax_backward rounds its products, flex_spmm pads its rows)."""
    row, col, rp = coo(a)
    k, heads = V.shape[1], el.shape[1]
    d = k // heads
    V64, g64 = (np.asarray(x, np.float32).astype(np.float64) for x in (V, g))
    p64 = np.asarray(p, np.float64)
    assert p64.shape == (a.nnz, heads), (p64.shape, (a.nnz, heads))
    sl = np.float64(np.float32(slope))
    _, pos = scores(a, el, er, slope)
    n_r, n_c = np.diff(rp)[row], np.bincount(col, minlength=a.n)[col]
    res = {key: [] for key in ("gel", "ger", "gv", "dx", "gel_bound", "ger_bound", "gv_bound", "dx_bound")}
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(heads):
            c = head_columns(k, heads, h)
            ph, ap = p64[:, h], np.abs(p64[:, h])
            da = (g64[row][:, c] * V64[col][:, c]).sum(1)
            dda = gamma(d) * (np.abs(g64[row][:, c]) * np.abs(V64[col][:, c])).sum(1) + d * 2.0 ** -149
            delta = _sum_by(ph * da, row, a.m)
            f = np.where(pos[:, h], 1.0, sl)
            dx = f * (ph * (da - delta[row]))
            ddz = gamma(n_r + a_r) * ap * (np.abs(da) + _sum_by(np.abs(ph * da), row, a.m)[row]) + ap * (dda + _sum_by(ap * dda, row, a.m)[row]) + n_r * 2.0 ** -149
            ddx = f * ddz + U * np.abs(dx) + 2.0 ** -149
            res["dx"].append(dx)
            res["dx_bound"].append(ddx)
            res["gel"].append(_sum_by(dx, row, a.m))
            res["ger"].append(_sum_by(dx, col, a.n))
            res["gel_bound"].append(_sum_by(gamma(n_r + b_r) * np.abs(dx) + ddx, row, a.m) + 2.0 ** -126)
            res["ger_bound"].append(_sum_by(gamma(n_c + b_r) * np.abs(dx) + ddx, col, a.n) + 2.0 ** -126)
            res["gv"].append(_sum_by(ph[:, None] * g64[row][:, c], col, a.n))
            res["gv_bound"].append(_sum_by((gamma(n_c + b_r) * ap)[:, None] * np.abs(g64[row][:, c]), col, a.n) + 2.0 ** -126)
    return {key: np.concatenate(v, axis=1) if key.startswith("gv") else np.stack(v, axis=1) for key, v in res.items()}


def check_backward(a, el, er, V, p, g, slope, gEl=None, gEr=None, gV=None, dx=None, what="", ratios=None):
    """Asserts, for every output given, the classes exactly (+0 rows without entries, NaN and infinities where float64 has them) and the
    bound on every other element; returns the worst err / bound (ratios, a dict: the worst of each output is kept in it)."""
    ref = backward_reference(a, el, er, V, np.asarray(p, np.float32), g, slope)
    row, col, rp = coo(a)
    empty = {"gel": np.diff(rp) == 0, "ger": np.bincount(col, minlength=a.n) == 0}
    empty["gv"] = empty["ger"]
    worst = 0.0
    for key, got in (("gel", gEl), ("ger", gEr), ("gv", gV), ("dx", dx)):
        if got is None:
            continue
        got, want, bound = np.asarray(got, np.float32), ref[key], ref[key + "_bound"]
        assert got.shape == want.shape, f"{what}: {key} has shape {got.shape}, want {want.shape}"
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


FAULTS = ("no_slope", "slope_on_positive", "branch_from_s", "next_heads_el", "head_major", "joint_softmax", "ger_by_row", "poison_spreads")


def fp32_result(a, el, er, V, slope, g=None, p=None, fault=None):
    """dict(out, p) -- and, with g, dict(gel, ger, gv, dx) from the p given (default: this forward's) -- as float32 from a float64
    evaluation: what a right kernel returns up to roundings.  The faults the checkers must catch: no_slope: the slope left out
    (identity); slope_on_positive: the slope applied where x > 0; branch_from_s: the backward takes the branch from s's sign with the
    derivative 1 at x = 0; next_heads_el: el of head h + 1 used for head h; head_major: P and dx delivered as [H, nnz] in the same
    memory; joint_softmax: one softmax over all heads' scores of a row; ger_by_row: gEr summed by row; poison_spreads: a row that one
    head poisons is NaN in every head's columns of Out.  joint_softmax is evaluated here and wants finite scores with every row live."""
    assert fault is None or fault in FAULTS, fault
    row, col, rp = coo(a)
    k, heads = V.shape[1], el.shape[1]
    sl = float(np.float32(slope))
    el_used = np.roll(el, -1, axis=1) if fault == "next_heads_el" else el
    if fault in ("no_slope", "slope_on_positive", "joint_softmax"):
        x = np.asarray(el_used, np.float64)[row] + np.asarray(er, np.float64)[col]
        s = x if fault == "no_slope" else np.where(x > 0, sl * x, x) if fault == "slope_on_positive" else np.where(x > 0, x, sl * x)
        M = np.full((a.m, heads), -np.inf)
        np.maximum.at(M, row, s)
        if fault == "joint_softmax":
            M = np.repeat(M.max(1, keepdims=True), heads, axis=1)
        t = np.exp(s - M[row])
        L = _sum_by(t, row, a.m)
        if fault == "joint_softmax":
            L = np.repeat(L.sum(1, keepdims=True), heads, axis=1)
        p64 = t / L[row]
        out = np.zeros((a.m, k))
        for h in range(heads):
            c = head_columns(k, heads, h)
            np.add.at(out[:, c], row, p64[:, h, None] * np.asarray(V, np.float64)[col][:, c])
    else:
        ref = reference(a, el_used, er, V, slope)
        out, p64 = ref["out"], ref["p"]
    with np.errstate(invalid="ignore", over="ignore"):
        res = dict(out=out.astype(np.float32), p=p64.astype(np.float32))
    if fault == "poison_spreads":
        res["out"][np.isnan(res["out"]).any(1)] = np.nan
    if g is not None:
        pin = res["p"] if p is None else np.asarray(p, np.float32)
        b = backward_reference(a, el_used, er, V, pin, g, slope)
        if fault == "branch_from_s":
            s, pos = scores(a, el, er, slope)
            with np.errstate(invalid="ignore"):
                b["dx"] = np.where(~pos & (s >= 0), b["dx"] / sl, b["dx"])
            b["gel"], b["ger"] = _sum_by(b["dx"], row, a.m), _sum_by(b["dx"], col, a.n)
        if fault == "ger_by_row":
            b["ger"] = _sum_by(b["dx"], row % a.n, a.n)
        with np.errstate(invalid="ignore", over="ignore"):
            res.update({key: b[key].astype(np.float32) for key in ("gel", "ger", "gv", "dx")})
    if fault == "head_major":
        for key in ("p", "dx"):
            if key in res:
                res[key] = np.ascontiguousarray(res[key].T).reshape(res[key].shape)
    return res


def propagated_bounds(a, el, er, V, slope, g):
    """(Out, gEl, gEr, gV) bounds of a forward and backward step against float64 THROUGHOUT, for finite scores: the backward starts from
    the forward's fp32 alpha, so alpha's own bound dalpha enters every gradient beside the backward's bounds (first order, 0.1 % spare):
        ddz_e = gamma(n_r + 3) alpha_e (|da_e| + sum_j alpha_j |da_j|) + n_r 2^-149
                + dalpha_e (|da_e| + sum_j alpha_j |da_j|) + alpha_e (dda_e + sum_j (dalpha_j |da_j| + alpha_j dda_j))
    and ddx, gEl, gEr as in the module's head; gV <= sum_{e in c} (gamma(n_c) alpha_e + dalpha_e) |g| + 2^-126."""
    ref = reference(a, el, er, V, slope)
    row, col, rp = coo(a)
    k, heads = V.shape[1], el.shape[1]
    d = k // heads
    V64, g64 = (np.asarray(x, np.float64) for x in (V, g))
    sl = np.float64(np.float32(slope))
    _, pos = scores(a, el, er, slope)
    n_r, n_c = np.diff(rp)[row], np.bincount(col, minlength=a.n)[col]
    gel, ger, gv = [], [], []
    for h in range(heads):
        c = head_columns(k, heads, h)
        al, dal = ref["p"][:, h], ref["p_bound"][:, h]
        da = (g64[row][:, c] * V64[col][:, c]).sum(1)
        ada = np.abs(da)
        dda = gamma(d) * (np.abs(g64[row][:, c]) * np.abs(V64[col][:, c])).sum(1) + d * 2.0 ** -149
        spread = ada + _sum_by(al * ada, row, a.m)[row]
        ddz = gamma(n_r + 3) * al * spread + n_r * 2.0 ** -149 + dal * spread + al * (dda + _sum_by(dal * ada + al * dda, row, a.m)[row])
        f = np.where(pos[:, h], 1.0, sl)
        dx = np.abs(f * al * (da - _sum_by(al * da, row, a.m)[row]))
        ddx = f * ddz + U * dx + 2.0 ** -149
        gel.append(_sum_by(gamma(n_r) * dx + ddx, row, a.m) + 2.0 ** -126)
        ger.append(_sum_by(gamma(n_c) * dx + ddx, col, a.n) + 2.0 ** -126)
        gv.append(_sum_by((gamma(n_c) * al + dal)[:, None] * np.abs(g64[row][:, c]), col, a.n) + 2.0 ** -126)
    return tuple(1.001 * t for t in (ref["out_bound"], np.stack(gel, 1), np.stack(ger, 1), np.concatenate(gv, 1)))

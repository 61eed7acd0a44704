"""The float64 reference, bounds, operands, checkers and planted faults of the per-edge score term of the fused GAT attention
(include/flex_spmm.h: flex_edge_gat_attention, flex_edge_gat_attention_backward), shared by tests/test_gat_edge_host.py and
tests/test_gpu_gat_edge.py.

Everything is gat_attention_ref's and gat_dropout_ref's except one line:
    x_eh = fl(fl(el[r, h] + er[src(e), h]) + ee[e, h])      (fp32, in this order)
ee is [nnz, H] fp32, entry-major, in a's CSR order (on a row-range shard: the whole matrix's array, of which the shard's entries are
read).  s, alpha, Out, da, delta, dz, dx = x > 0 ? dz : slope dz, gEl, gEr, gV and the mask of (seed, e H + h) are unchanged, and
gEe[e, h] = dx_eh.  The softmax (softmax_ref.forward_ref on the score rounded to fp32), the mask (attention_dropout_ref.kept_entries,
factor), the row and edge checkers (attention_dropout_ref._check_rows, _check_edge) and the el / er scenarios (gat_attention_ref) are
the existing ones; drop_p == 0 is the undropped call (every entry kept, c = 1, the undropped rounding counts).

The float64 reference uses the exact x = el + er + ee on the fp32 inputs and takes the LeakyReLU branch from the sign of the fp32 x
formed in the order above.  The only new bound is the score's.  Two rounded additions, where the first sum may cancel against ee, give
    |x^ - x| <= u (1 + u) |el + er| + u |x|
so with f_e = 1 or slope:
    ds_e = gamma(2) f_e |el + er| + gamma(3) |s_e| + 2^-149
in place of gamma(2) |s_e| + 2^-149.  Derivation: a = fl(el + er) = (el + er)(1 + d1) and x^ = fl(a + ee) = (x + (el + er) d1)(1 + d2) with
|d1|, |d2| <= u, which is the first line; s^ = x^ or fl(slope x^), one more rounding that may be subnormal, so
|s^ - s| <= f u (1 + u)^2 |el + er| + (u (1 + u) + u) |s| + 2^-149, inside the second line.  Where x^ and x differ in sign, |x| is below
u (1 + u) |el + er| and either branch of the reference is within the same line.  alpha, Out, dda, ddz, ddx, gEl, gEr and gV keep
gat_attention_ref's (with dropout: gat_dropout_ref's) formulas with this ds; gEe is held to ddx."""
import numpy as np

import gat_attention_ref as gat
from attention_dropout_ref import _check_edge, _check_rows, _sum_by, factor, kept_entries
from fused_attention_ref import coo
from multihead_attention_ref import head_columns
from softmax_ref import E_ULP, U, _per_row, _segments, forward_ref, gamma

SLOPE = gat.SLOPE
EDGE_SCENARIOS = ["zero_edge", "spread", "cancel", "near_cancel", "edge_masked", "edge_poison"]


def edge_scenarios_of(heads, shift=0):
    """One ee scenario per head, in turn."""
    return [EDGE_SCENARIOS[(h + shift) % len(EDGE_SCENARIOS)] for h in range(heads)]


def _head_edge(name, a, el, er, seed):
    """ee [nnz] fp32 of one head over that head's el [m], er [n].  zero_edge: all +0.  spread: uniform +-40.  cancel: +-2, and
    ee = -fl(el + er) exactly on the first entry of every third row with entries (where that sum is finite), so x = +0 and the slope
    branch is taken while the float64 x is a rounding residue.  near_cancel: the same, times (1 + 2^-20).  edge_masked: -inf on 30 % of
    the entries and on every entry of some chosen rows.  edge_poison: a NaN on one entry each of three rows, the longest among them,
    and a +inf on an entry of another row.  No element is -0."""
    rng = np.random.default_rng([seed, 50 + EDGE_SCENARIOS.index(name)])
    row, col, rp = coo(a)
    deg = np.diff(rp)
    ne = np.flatnonzero(deg > 0)
    if name == "zero_edge":
        return np.zeros(a.nnz, np.float32)
    half = 40.0 if name == "spread" else 2.0
    ee = rng.uniform(-half, half, a.nnz).astype(np.float32)
    if name in ("cancel", "near_cancel"):
        first = rp[:-1][ne[::3]].astype(np.int64)
        with np.errstate(invalid="ignore"):
            s = (el[row[first]] + er[col[first]]).astype(np.float32)
        ok = np.isfinite(s)
        v = -s[ok] if name == "cancel" else (-s[ok] * np.float32(1 + 2.0 ** -20)).astype(np.float32)
        ee[first[ok]] = v + np.float32(0)  # -0 + 0 = +0
    if name == "edge_masked":
        ee[rng.random(a.nnz) < 0.3] = -np.inf
        if len(ne):
            for r in {int(ne[0]), int(ne[np.argmax(deg[ne])]), *rng.choice(ne, max(1, len(ne) // 10)).tolist()} - {int(ne[len(ne) // 2])}:
                ee[rp[r]:rp[r + 1]] = -np.inf
    if name == "edge_poison" and len(ne):
        rows = sorted({int(ne[0]), int(ne[np.argmax(deg[ne])]), int(ne[len(ne) // 2])})
        for r in rows:
            ee[int(rp[r]) + int(rng.integers(deg[r]))] = np.nan
        other = [int(r) for r in ne if int(r) not in rows]
        if other:
            r = other[len(other) // 3]
            ee[int(rp[r]) + int(rng.integers(deg[r]))] = np.inf
    ee[ee == 0] = 0.0
    return ee


def operands(names, edge_names, a, k, seed=0):
    """(el [m, H], er [n, H], ee [nnz, H], V [n, k]) fp32: head h holds gat_attention_ref's scenario names[h] in el and er and the ee
    scenario edge_names[h] on top of it."""
    el, er, V = gat.operands(names, a, k, seed=seed)
    ee = np.stack([_head_edge(name, a, el[:, h], er[:, h], 100 * seed + h) for h, name in enumerate(edge_names)], axis=1)
    for x in (el, er, ee):  # the +0 identity of the ee = 0 case relies on it
        assert not np.any((x == 0) & np.signbit(x))
    return el, er, np.ascontiguousarray(ee), V


# ---- the reference

def _entries(a, rows):
    r0, r1 = (0, a.m) if rows is None else rows
    return int(a.rowPtr[r0]), int(a.rowPtr[r1])


def scores(a, el, er, ee, slope, rows=None, fault=None):
    """(s64, positive, |el + er| in float64), each [entries of the rows, H]: the float64 score of the exact x = el + er + ee with the
    branch taken from the sign of the fp32 x = fl(fl(el + er) + ee).  ee is the whole matrix's array.  fault: a score fault of FAULTS."""
    row, col, _ = coo(a, rows)
    e0, e1 = _entries(a, rows)
    el32, er32, ee32 = (np.asarray(x, np.float32) for x in (el, er, ee))
    assert ee32.shape == (a.nnz, el32.shape[1]), f"ee is [nnz, heads] = {(a.nnz, el32.shape[1])}, entry-major; got {ee32.shape}"
    if fault == "next_heads_ee":
        ee32 = np.roll(ee32, -1, axis=1)
    if fault == "head_major_ee":
        ee32 = np.ascontiguousarray(ee32).reshape(ee32.shape[1], a.nnz).T
    if fault == "mask_spreads":
        ee32 = np.where((ee32 == -np.inf).any(1, keepdims=True), np.float32(-np.inf), ee32)
    ee32 = ee32[e0:e1]
    if fault == "ee_left_out":
        ee32 = np.zeros_like(ee32)
    sl = np.float64(np.float32(slope))
    with np.errstate(invalid="ignore", over="ignore"):
        a32 = el32[row] + er32[col]
        a64 = el32.astype(np.float64)[row] + er32.astype(np.float64)[col]
        if fault == "ee_after_leaky":
            pos = a32 > 0
            s = np.where(pos, a64, sl * a64) + ee32.astype(np.float64)
        else:
            pos = (a32 > 0) if fault == "branch_from_el_er" else ((a32 + ee32) > 0)
            x = a64 + ee32.astype(np.float64)
            s = np.where(pos, x, sl * x)
    return s, pos, np.abs(a64)


def reference(a, el, er, ee, V, slope, p=0.0, seed=0, rows=None, fault=None, c_r=None):
    """dict(out, out_bound [rows, k]; p, p_bound, s, keep [entries of the rows, H]) of the rows [r0, r1) (el holds those rows only, ee
    the whole matrix's entries): p, p_bound and s are the undropped ones; p = 0 keeps every entry.  c_r = 32 gives the bound of the
    composition of engine calls instead, as in gat_attention_ref.reference."""
    row, col, rp = coo(a, rows)
    m, k, heads = len(rp) - 1, V.shape[1], el.shape[1]
    assert el.shape[0] == m and er.shape == (a.n, heads), (el.shape, er.shape)
    V64 = np.asarray(V, np.float32).astype(np.float64)
    if len(row) == 0:
        z, e = np.zeros((m, k)), np.zeros((0, heads))
        return dict(out=z, out_bound=z + 2.0 ** -126, p=e, p_bound=e, s=e, keep=e.astype(bool))
    s, pos, aab = scores(a, el, er, ee, slope, rows, fault)
    with np.errstate(over="ignore"):
        s32 = s.astype(np.float32)
    kp = kept_entries(a, heads, p, seed, rows) if p else np.ones(s.shape, bool)
    c, c_r = (factor(p), c_r or 4) if p else (1.0, c_r or gat.C_ROUNDINGS)
    starts, seg, n_r = _segments(rp)
    R = np.ceil(n_r / 4.0) + 8
    sl = np.float64(np.float32(slope))
    out, ob = np.zeros((m, k)), np.zeros((m, k))
    ps, pbs = [], []
    for h in range(heads):
        pr, _ = forward_ref(rp, s32[:, h], 1.0)
        fin = np.isfinite(s[:, h])
        f = np.where(pos[:, h], 1.0, sl)
        # ds_e + |s_e| u, the argument of max_row in dalpha, as gat_attention_ref.reference folds it
        ds = np.where(fin, gamma(2) * f * np.where(fin, aab[:, h], 0.0) + (gamma(3) + U) * np.abs(np.where(fin, s[:, h], 0.0)) + 2.0 ** -149, 0.0)
        ds_row = _per_row(np.maximum, ds, starts, seg)
        hi = _per_row(np.maximum, np.where(fin, s32[:, h].astype(np.float64), -np.inf), starts, seg)
        lo = _per_row(np.minimum, np.where(fin, s32[:, h].astype(np.float64), np.inf), starts, seg)
        with np.errstate(invalid="ignore"):
            D = np.where(hi == -np.inf, 0.0, np.minimum(104.0, hi - lo))
        p0 = np.where(np.isnan(pr), 0.0, pr)
        pb = p0 * (gamma(n_r + 4 * D + (E_ULP + 3) * R + 2 * E_ULP + 4) + np.expm1(2 * ds_row)) + 2.0 ** -126
        cs, sel = head_columns(k, heads, h), kp[:, h]
        with np.errstate(invalid="ignore", over="ignore"):
            np.add.at(out[:, cs], row[sel], (pr[sel] * c)[:, None] * V64[col[sel]][:, cs])
            np.add.at(ob[:, cs], row[sel], ((gamma(n_r[sel] + c_r) * p0[sel] + pb[sel]) * c)[:, None] * np.abs(V64[col[sel]][:, cs]))
        poisoned = np.zeros(m, bool)
        poisoned[row[np.isnan(pr)]] = True
        out[poisoned, cs] = np.nan  # a poisoned head is NaN whether or not its entries are kept
        ps.append(pr)
        pbs.append(pb)
    return dict(out=out, out_bound=ob + 2.0 ** -126, p=np.stack(ps, 1), p_bound=np.stack(pbs, 1), s=s32, keep=kp)


def check(a, el, er, ee, V, slope, p, seed, out, probs=None, rows=None, what="", ratios=None):
    """gat_dropout_ref.check on this reference: Out [rows, k] -- NaN in a poisoned head's columns and nowhere else, +0 bits in a head of
    a row with no kept live entry (where the kept V rows are finite), non-finite values where float64 has them, the bound on every other
    element -- and, where given, P (fp32 [entries, H], the UNDROPPED alpha): NaN exactly on the poisoned heads of rows, +0 bits on
    masked entries, the bound elsewhere.  Returns the worst err / bound (ratios: the worst of each output)."""
    ref = reference(a, el, er, ee, V, slope, p, seed, rows)
    k, heads = V.shape[1], el.shape[1]
    row, col, rp = coo(a, rows)
    m = len(rp) - 1
    zero = np.zeros((m, k), bool)
    for h in range(heads):
        cs, sel = head_columns(k, heads, h), ref["keep"][:, h]
        busy = np.zeros(m, bool)
        al = ref["p"][sel, h]
        busy[row[sel][~(al == 0) | ~np.isfinite(np.asarray(V, np.float64)[col[sel]][:, cs]).all(1)]] = True
        busy[row[np.isnan(ref["p"][:, h])]] = True
        zero[:, cs] = ~busy[:, None]
    worst = _check_rows(out, ref["out"], ref["out_bound"], what, "Out", False, zero_rows=zero)
    if ratios is not None:
        ratios["out"] = max(worst, ratios.get("out", 0.0))
    if probs is not None:
        probs = np.asarray(probs)
        assert probs.dtype == np.float32 and probs.shape == ref["p"].shape, f"{what}: P is fp32 [entries, heads], entry-major; got {probs.dtype} {probs.shape}"
        nan_ref = np.isnan(ref["p"])
        assert np.array_equal(np.isnan(probs), nan_ref), f"{what}: P is NaN exactly on the poisoned rows of each head"
        masked = ~nan_ref & (ref["s"] == -np.inf)
        assert np.all(probs[masked].view(np.uint32) == 0), f"{what}: a masked entry of P is not +0 bit for bit"
        r = np.abs(probs[~nan_ref].astype(np.float64) - ref["p"][~nan_ref]) / ref["p_bound"][~nan_ref]
        wp = float(r.max()) if r.size else 0.0
        assert wp <= 1.0, f"{what}: {int((r > 1).sum())} entries of P beyond the bound, worst err / bound {wp:.3g}"
        if ratios is not None:
            ratios["p"] = max(wp, ratios.get("p", 0.0))
        worst = max(worst, wp)
    return worst


def backward_reference(a, el, er, ee, V, probs, g, slope, p=0.0, seed=0, fault=None, a_r=gat.A_ROUNDINGS, b_r=gat.B_ROUNDINGS):
    """dict(gel [m, H], ger [n, H], gee [nnz, H], gv [n, k] and their bounds; gee is dx): float64 on the fp32 el, er, ee, V and g and on
    probs AS GIVEN.  gat_dropout_ref.backward_reference with the branch of this score (p = 0: gat_attention_ref's counts).  a_r = 4
    and b_r = 32 give the bounds of the chain of engine calls on the same probs, as in gat_attention_ref.backward_reference."""
    row, col, rp = coo(a)
    k, heads = V.shape[1], el.shape[1]
    d = k // heads
    V64, g64 = (np.asarray(x, np.float32).astype(np.float64) for x in (V, g))
    p64 = np.asarray(probs, np.float64)
    assert p64.shape == (a.nnz, heads), (p64.shape, (a.nnz, heads))
    sl = np.float64(np.float32(slope))
    _, pos, _ = scores(a, el, er, ee, slope, fault=fault if fault in SCORE_FAULTS else None)
    masked = bool(p) and fault != "gee_unmasked"
    kp = kept_entries(a, heads, p, seed) if p else np.ones(p64.shape, bool)
    c, one = (factor(p), 1) if p else (1.0, 0)
    n_r, n_c = np.diff(rp)[row], np.bincount(col, minlength=a.n)[col]
    res = {key: [] for key in ("gel", "ger", "gv", "gee", "gel_bound", "ger_bound", "gv_bound", "gee_bound")}
    A, B = a_r, b_r
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(heads):
            cs, sel = head_columns(k, heads, h), kp[:, h]
            ph, ap = p64[:, h], np.abs(p64[:, h])
            gv_, Vv = g64[row][:, cs], V64[col][:, cs]
            dot = (gv_ * Vv).sum(1)
            da = np.where(sel, c * np.where(sel, dot, 0.0), 0.0) if masked else c * dot
            dda = np.where(sel, c * (gamma(d + one) * np.where(sel, (np.abs(gv_) * np.abs(Vv)).sum(1), 0.0) + d * 2.0 ** -149) + one * 2.0 ** -149, 0.0)
            delta = _sum_by(ph * da, row, a.m)
            f = np.where(pos[:, h], 1.0, sl)
            dz = ph * (da - delta[row])
            dx = f * dz
            ddz = gamma(n_r + A) * ap * (np.abs(da) + _sum_by(np.abs(ph * da), row, a.m)[row]) + ap * (dda + _sum_by(ap * dda, row, a.m)[row]) + n_r * 2.0 ** -149
            ddx = f * ddz + U * np.abs(dx) + 2.0 ** -149
            res["gee"].append(dz if fault == "gee_from_dz" else dx), res["gee_bound"].append(ddx)
            res["gel"].append(_sum_by(dx, row, a.m))
            res["ger"].append(_sum_by(dx, col, a.n))
            res["gel_bound"].append(_sum_by(gamma(n_r + B) * np.abs(dx) + ddx, row, a.m) + 2.0 ** -126)
            res["ger_bound"].append(_sum_by(gamma(n_c + B) * np.abs(dx) + ddx, col, a.n) + 2.0 ** -126)
            res["gv"].append(_sum_by((c * ph)[sel, None] * gv_[sel], col[sel], a.n))
            res["gv_bound"].append(_sum_by((gamma(n_c[sel] + B + one) * np.abs(c * ph[sel]))[:, None] * np.abs(gv_[sel]), col[sel], a.n) + 2.0 ** -126)
    return {key: np.concatenate(v, axis=1) if key.startswith("gv") else np.stack(v, axis=1) for key, v in res.items()}


def check_backward(a, el, er, ee, V, probs, g, slope, p, seed, gEl=None, gEr=None, gEe=None, gV=None, what="", ratios=None):
    """gat_dropout_ref.check_backward on this reference, gEe [nnz, H] in dx's place and under its bound ddx.  For every output given
    (fp32): +0 bits on rows of gEl and of gEr / gV without entries and, in gV, in a head of a column without a kept entry; NaN and
    infinities where float64 has them; the bound on every other element.  Returns the worst err / bound."""
    probs = np.asarray(probs, np.float32)
    ref = backward_reference(a, el, er, ee, V, probs, g, slope, p, seed)
    row, col, rp = coo(a)
    k, heads = V.shape[1], el.shape[1]
    kp = kept_entries(a, heads, p, seed) if p else np.ones((a.nnz, heads), bool)
    empty_r = np.repeat((np.diff(rp) == 0)[:, None], heads, 1)
    empty_c = np.repeat((np.bincount(col, minlength=a.n) == 0)[:, None], heads, 1)
    none_kept = np.zeros((a.n, k), bool)
    for h in range(heads):
        any_kept = np.zeros(a.n, bool)
        any_kept[col[kp[:, h]]] = True
        none_kept[:, head_columns(k, heads, h)] = ~any_kept[:, None]
    worst = 0.0
    for key, got, zero in (("gel", gEl, empty_r), ("ger", gEr, empty_c), ("gv", gV, none_kept), ("gee", gEe, None)):
        if got is None:
            continue
        if key == "gee":
            w = _check_edge(got, ref["gee"], ref["gee_bound"], what, "gee", (a.nnz, heads))
        else:
            w = _check_rows(np.asarray(got), ref[key], ref[key + "_bound"], what, key, False, zero_rows=zero)
        worst = max(worst, w)
        if ratios is not None:
            ratios[key] = max(w, ratios.get(key, 0.0))
    return worst


# ---- what a right kernel returns up to roundings, and the faults the checkers must reject

SCORE_FAULTS = ("ee_left_out", "ee_after_leaky", "next_heads_ee", "head_major_ee", "branch_from_el_er", "mask_spreads")
BACKWARD_FAULTS = ("gee_from_dz", "gee_unmasked")
FAULTS = SCORE_FAULTS + BACKWARD_FAULTS


def fp32_result(a, el, er, ee, V, slope, p=0.0, seed=0, g=None, probs=None, rows=None, fault=None):
    """dict(out [rows, k], p [entries, H]; with g also gel [m, H], ger [n, H], gee [nnz, H], gv [n, k]) as float32 from a float64
    evaluation; the backward starts from `probs` (default: this forward's).  Faults:
      ee_left_out        x = el + er
      ee_after_leaky     s = leaky(el + er) + ee
      next_heads_ee      head h takes ee of head h + 1 (the last head the first's)
      head_major_ee      ee is read as [H, nnz] in the same memory
      branch_from_el_er  the branch of the LeakyReLU, forward and backward, from the sign of el + er alone
      mask_spreads       a -inf in ee of one head masks the entry for every head
      gee_from_dz        gEe = dz, the slope left out
      gee_unmasked       under dropout: gEe from the da of every entry, dropped ones included"""
    assert fault in (None,) + FAULTS, fault
    sf = fault if fault in SCORE_FAULTS else None
    ref = reference(a, el, er, ee, V, slope, p, seed, rows, fault=sf)
    with np.errstate(invalid="ignore", over="ignore"):
        got = dict(out=ref["out"].astype(np.float32), p=ref["p"].astype(np.float32))
    if g is None:
        return got
    assert rows is None, "the backward is not defined on shards"
    pin = got["p"] if probs is None else np.asarray(probs, np.float32)
    b = backward_reference(a, el, er, ee, V, pin, g, slope, p, seed, fault=fault)
    if fault == "gee_unmasked":  # the other gradients are the right ones
        right = backward_reference(a, el, er, ee, V, pin, g, slope, p, seed)
        b = {**right, "gee": b["gee"]}
    with np.errstate(invalid="ignore", over="ignore"):
        got.update({key: b[key].astype(np.float32) for key in ("gel", "ger", "gee", "gv")})
    return got


def fp32_evaluation(a, el, er, ee, V, slope, p=0.0, seed=0, g=None):
    """What the kernel's arithmetic gives in a plain order, in fp32 numpy: x by the two fp32 additions, the LeakyReLU product, the
    exponential of the fp32 difference to the row's maximum, the sum and the quotient in fp32, Out by fmas in entry order; with g the
    backward from this P: da and delta by fmas, dz = p (da - delta), dx, and plain fp32 sums for gEl, gEr and gV by fma.  An fma is
    emulated as the float64 product and sum rounded once to fp32 (the product of two fp32 numbers is exact in float64).  The evidence
    that the bounds are not too tight: tests/test_gat_edge_host.py holds it to both checkers on every scenario."""
    f32 = np.float32
    row, col, rp = coo(a)
    k, heads = V.shape[1], el.shape[1]
    el, er, ee, V = (np.asarray(x, f32) for x in (el, er, ee, V))
    sl = f32(slope)
    kp = kept_entries(a, heads, p, seed) if p else np.ones((a.nnz, heads), bool)
    c = f32(factor(p)) if p else f32(1)

    def fma(x, y, z):
        return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(f32)

    def chain(n, seg, shape, term):
        """acc[seg[e]] = fma-or-sum over the entries in order: term(e, acc) -> new acc, one entry of every segment at a time"""
        acc = np.zeros(shape, f32)
        order = np.argsort(seg, kind="stable")
        pos_in = np.arange(len(seg)) - np.searchsorted(seg[order], seg[order])
        for j in range(int(pos_in.max()) + 1 if len(seg) else 0):
            e = order[pos_in == j]
            acc[seg[e]] = term(e, acc[seg[e]])
        return acc

    with np.errstate(invalid="ignore", over="ignore"):
        x = (el[row] + er[col]) + ee
        s = np.where(x > 0, x, sl * x).astype(f32)
        M = np.full((a.m, heads), -np.inf, f32)
        np.maximum.at(M, row, np.where(np.isnan(s), f32(np.inf), s))  # a NaN score poisons as +inf does
        Mr = M[row]
        t = np.where(Mr == -np.inf, f32(0), np.exp((s - Mr).astype(f32)).astype(f32))
        t = np.where(np.isnan(s) | (Mr == np.inf), f32(np.nan), t).astype(f32)
        L = chain(a.nnz, row, (a.m, heads), lambda e, acc: acc + t[e])
        P = np.where(L[row] > 0, t / L[row], np.where(np.isnan(L[row]), f32(np.nan), f32(0))).astype(f32)
        w = np.where(kp, c, f32(0)).astype(f32)
        Pk = np.repeat(P, k // heads, axis=1)
        keepk = np.repeat(kp, k // heads, axis=1)
        wk = np.repeat((P * w).astype(f32), k // heads, axis=1)
        out = chain(a.nnz, row, (a.m, k), lambda e, acc: np.where(keepk[e], fma(wk[e], V[col[e]], acc), acc))
        bad = np.repeat(np.isnan(L), k // heads, axis=1)
        out[bad] = np.nan
        res = dict(out=out, p=P)
        if g is None:
            return res
        g = np.asarray(g, f32)
        da = np.zeros((a.nnz, heads), f32)
        d = k // heads
        for h in range(heads):
            acc = np.zeros(a.nnz, f32)
            for j in range(h * d, (h + 1) * d):
                acc = fma(g[row][:, j], np.where(kp[:, h], V[col][:, j], f32(0)), acc)
            da[:, h] = np.where(kp[:, h], c * acc, f32(0))
        delta = chain(a.nnz, row, (a.m, heads), lambda e, acc: fma(P[e], da[e], acc))
        dz = (P * (da - delta[row]).astype(f32)).astype(f32)
        dx = np.where(x > 0, dz, sl * dz).astype(f32)
        gel = chain(a.nnz, row, (a.m, heads), lambda e, acc: acc + dx[e])
        ger = chain(a.nnz, col, (a.n, heads), lambda e, acc: acc + dx[e])
        gv = chain(a.nnz, col, (a.n, k), lambda e, acc: np.where(keepk[e], fma(wk[e], g[row[e]], acc), acc))
        res.update(gel=gel, ger=ger, gee=dx, gv=gv)
    return res


def torch_float64(a, el, er, ee, V, slope, g, kp=None, c=1.0):
    """(Out, P, gEl, gEr, gEe, gV) by torch autograd in float64 on the fp32 inputs -- index arithmetic for the scores, leaky_relu, a
    plain softmax per row by index_add_ -- with the mask kp [nnz, H] as a constant tensor (None: no mask); finite scores only."""
    import torch
    row, col, _ = coo(a)
    k, heads = V.shape[1], el.shape[1]
    d = k // heads
    row_t, col_t = torch.from_numpy(row.astype(np.int64)), torch.from_numpy(col.astype(np.int64))
    el_t, er_t, ee_t, V_t = (torch.from_numpy(np.ascontiguousarray(x, np.float32)).double().requires_grad_() for x in (el, er, ee, V))
    s = torch.nn.functional.leaky_relu(el_t[row_t] + er_t[col_t] + ee_t, float(np.float32(slope)))
    M = torch.full((a.m, heads), -np.inf, dtype=torch.float64).scatter_reduce(0, row_t[:, None].expand(-1, heads), s.detach(), "amax")
    t = torch.exp(s - M[row_t])
    pr = t / torch.zeros((a.m, heads), dtype=torch.float64).index_add_(0, row_t, t)[row_t]
    w = torch.ones((a.nnz, heads), dtype=torch.float64) if kp is None else torch.from_numpy(np.asarray(kp, np.float64) * c)
    out = torch.zeros((a.m, heads, d), dtype=torch.float64).index_add_(0, row_t, (pr * w)[:, :, None] * V_t.view(a.n, heads, d)[col_t]).reshape(a.m, k)
    out.backward(torch.from_numpy(np.ascontiguousarray(g, np.float32)).double())
    return out.detach().numpy(), pr.detach().numpy(), el_t.grad.numpy(), er_t.grad.numpy(), ee_t.grad.numpy(), V_t.grad.numpy()


def propagated_bounds(a, el, er, ee, V, slope, g):
    """(Out, gEl, gEr, gEe, gV) bounds of a forward and backward step against float64 THROUGHOUT, for finite scores and no dropout:
    gat_attention_ref.propagated_bounds on this reference's alpha and dalpha (the backward starts from the forward's fp32 alpha), with
    gEe under the ddx of that derivation; first order, 0.1 % spare."""
    ref = reference(a, el, er, ee, V, slope)
    row, col, rp = coo(a)
    k, heads = V.shape[1], el.shape[1]
    d = k // heads
    V64, g64 = (np.asarray(x, np.float64) for x in (V, g))
    sl = np.float64(np.float32(slope))
    _, pos, _ = scores(a, el, er, ee, slope)
    n_r, n_c = np.diff(rp)[row], np.bincount(col, minlength=a.n)[col]
    gel, ger, gee, gv = [], [], [], []
    for h in range(heads):
        cs = head_columns(k, heads, h)
        al, dal = ref["p"][:, h], ref["p_bound"][:, h]
        da = (g64[row][:, cs] * V64[col][:, cs]).sum(1)
        ada = np.abs(da)
        dda = gamma(d) * (np.abs(g64[row][:, cs]) * np.abs(V64[col][:, cs])).sum(1) + d * 2.0 ** -149
        spread = ada + _sum_by(al * ada, row, a.m)[row]
        ddz = gamma(n_r + 3) * al * spread + n_r * 2.0 ** -149 + dal * spread + al * (dda + _sum_by(dal * ada + al * dda, row, a.m)[row])
        f = np.where(pos[:, h], 1.0, sl)
        dx = np.abs(f * al * (da - _sum_by(al * da, row, a.m)[row]))
        ddx = f * ddz + U * dx + 2.0 ** -149
        gee.append(ddx)
        gel.append(_sum_by(gamma(n_r) * dx + ddx, row, a.m) + 2.0 ** -126)
        ger.append(_sum_by(gamma(n_c) * dx + ddx, col, a.n) + 2.0 ** -126)
        gv.append(_sum_by((gamma(n_c) * al + dal)[:, None] * np.abs(g64[row][:, cs]), col, a.n) + 2.0 ** -126)
    return tuple(1.001 * t for t in (ref["out_bound"], np.stack(gel, 1), np.stack(ger, 1), np.stack(gee, 1), np.concatenate(gv, 1)))

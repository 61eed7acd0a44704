"""float64 reference, bounds, operands and checker of the fused attention forward (include/flex_spmm.h: flex_attention), shared by
tests/test_fused_attention_host.py and tests/test_gpu_fused_attention.py.

The reference is float64 numpy on the fp32 inputs with the header's definitions: s_e = <Q[r], K[col(e)]>, alpha = flex_edge_softmax's
softmax of the scores rounded to fp32 (softmax_ref.forward_ref: a -inf score is a masked edge, a row of -inf is +0 everywhere, a row
with a +inf or NaN score is NaN everywhere), Out[r] = sum_e alpha_e V[col(e)].  Bounds, verbatim (u = 2^-24, gamma(n) = n u / (1 - n u),
n_r = entries of the row, D_r = min(104, scale x the spread of the row's finite scores), E = softmax_ref.E_ULP, R_r = ceil(n_r / 4) + 8):
    score   ds_e     = gamma(k) sum_j |Q K| + k 2^-149
    alpha   dalpha_e = alpha_e [gamma(n_r + 4 D_r + (E + 3) R_r + 2 E + 4) + expm1(2 scale max_row(ds + |s| u))] + 2^-126
    Out     |Out - Out64| <= sum_e (gamma(n_r + 3) alpha_e + dalpha_e) |V| + 2^-126"""
import numpy as np

from softmax_ref import E_ULP, U, _per_row, _segments, csr_from_degrees, forward_ref, gamma

SLOT_ROW, WAVE_ROW = 32, 512  # internal.h: kAtSlotRow, kAtWaveRow


def lanes(k):
    """internal.h, sddmm_lanes: the lanes of a slot."""
    w = 4
    while 4 * w < k and w < 64:
        w <<= 1
    return w


def expected_classes(rp):
    """(empty, slot, wave, block) rows by the rule of internal.h (attention_row_class)."""
    deg = np.diff(np.asarray(rp, np.int64))
    return (int((deg == 0).sum()), int(((deg > 0) & (deg <= SLOT_ROW)).sum()), int(((deg > SLOT_ROW) & (deg <= WAVE_ROW)).sum()),
            int((deg > WAVE_ROW).sum()))


def threshold_graph():
    """Rows one below, at and one above both class thresholds, each kind twice, with short and empty rows between them."""
    deg = np.random.default_rng(11).poisson(4, 90)
    deg[[3, 4, 5, 40, 41, 42]] = [SLOT_ROW - 1, SLOT_ROW, SLOT_ROW + 1, SLOT_ROW + 1, SLOT_ROW, SLOT_ROW - 1]
    deg[[20, 21, 22, 70, 71, 72]] = [WAVE_ROW - 1, WAVE_ROW, WAVE_ROW + 1, WAVE_ROW + 1, WAVE_ROW, WAVE_ROW - 1]
    deg[[0, 10, 89]] = 0
    return csr_from_degrees(deg, 800, seed=11)


def coo(a, rows=None):
    """(row of every entry, column of every entry, row pointer slice) of rows [r0, r1) of a; rows are slice-local."""
    r0, r1 = (0, a.m) if rows is None else rows
    rp = a.rowPtr.astype(np.int64)[r0:r1 + 1]
    return np.repeat(np.arange(r1 - r0), np.diff(rp)), a.col.astype(np.int64)[rp[0]:rp[-1]], rp


def reference(a, Q, K, V, scale, rows=None):
    """dict(out, out_bound, p, p_bound, s): Out64 [rows, k] and alpha64 [entries of the rows] with the header's bounds."""
    row, col, rp = coo(a, rows)
    m, k = len(rp) - 1, Q.shape[1]
    Q64, K64, V64 = (np.asarray(x, np.float32).astype(np.float64) for x in (Q, K, V))
    sc = np.float64(np.float32(scale))
    with np.errstate(invalid="ignore", over="ignore"):
        s = (Q64[row] * K64[col]).sum(1)
        T = (np.abs(Q64[row]) * np.abs(K64[col])).sum(1)
    if s.size == 0:
        z = np.zeros((m, k))
        return dict(out=z, out_bound=z + 2.0 ** -126, p=s, p_bound=s, s=s)
    with np.errstate(over="ignore"):
        s32 = s.astype(np.float32)
    p, _ = forward_ref(rp, s32, scale)
    starts, seg, n_r = _segments(rp)
    fin = np.isfinite(s)
    ds = np.where(fin, gamma(k) * np.where(fin, T, 0.0) + k * 2.0 ** -149 + np.abs(np.where(fin, s, 0.0)) * U, 0.0)
    ds_row = _per_row(np.maximum, ds, starts, seg)
    hi = _per_row(np.maximum, np.where(fin, s32.astype(np.float64), -np.inf), starts, seg)
    lo = _per_row(np.minimum, np.where(fin, s32.astype(np.float64), np.inf), starts, seg)
    with np.errstate(invalid="ignore"):
        D = np.where(hi == -np.inf, 0.0, np.minimum(104.0, sc * (hi - lo)))
    R = np.ceil(n_r / 4.0) + 8
    p0 = np.where(np.isnan(p), 0.0, p)
    p_bound = p0 * (gamma(n_r + 4 * D + (E_ULP + 3) * R + 2 * E_ULP + 4) + np.expm1(2 * sc * ds_row)) + 2.0 ** -126
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.zeros((m, k))
        np.add.at(out, row, p[:, None] * V64[col])
        ob = np.zeros((m, k))
        np.add.at(ob, row, (gamma(n_r + 3) * p0 + p_bound)[:, None] * np.abs(V64[col]))
    return dict(out=out, out_bound=ob + 2.0 ** -126, p=p, p_bound=p_bound, s=s32)


def fp32_result(a, Q, K, V, scale, rows=None, drop_entry=None, no_scale=False, wrong_sum=None):
    """(Out, P) as float32 from a float64 evaluation: what a right kernel returns up to roundings.  The faults the checker must catch:
    drop_entry = e: entry e is left out of its row; no_scale: scale is left out; wrong_sum = (r, r2): row r divides by row r2's sum."""
    row, col, rp = coo(a, rows)
    Q64, K64, V64 = (np.asarray(x, np.float64) for x in (Q, K, V))
    s = (Q64[row] * K64[col]).sum(1)
    keep = np.ones(len(s), bool)
    if drop_entry is not None:
        keep[drop_entry] = False
    sc = 1.0 if no_scale else float(np.float32(scale))
    m = len(rp) - 1
    M = np.full(m, -np.inf)
    np.maximum.at(M, row[keep], s[keep])
    t = np.where(keep, np.exp(sc * (s - M[row])), 0.0)
    L = np.zeros(m)
    np.add.at(L, row, t)
    if wrong_sum is not None:
        L[wrong_sum[0]] = L[wrong_sum[1]]
    p = t / L[row]
    out = np.zeros((m, Q.shape[1]))
    np.add.at(out, row, p[:, None] * V64[col])
    return out.astype(np.float32), p.astype(np.float32)


def check(a, Q, K, V, scale, out, p=None, rows=None, what=""):
    """Asserts the classes exactly (+0 rows, NaN rows, masked p = +0 bit for bit) and the bound on every element of Out and, where given,
    of P (the entries of the rows, in CSR order); returns the worst err / bound."""
    ref = reference(a, Q, K, V, scale, rows)
    out = np.asarray(out, np.float32)
    assert out.shape == ref["out"].shape, (what, out.shape, ref["out"].shape)
    row, col, rp = coo(a, rows)
    deg = np.diff(rp)
    poisoned = np.zeros(len(deg), bool)
    poisoned[row[np.isnan(ref["p"])]] = True
    assert np.all(np.isnan(out[poisoned])), f"{what}: a row with a +inf or NaN score is not NaN in every column"
    live = np.zeros(len(deg), bool)
    live[row[np.nan_to_num(ref["p"]) > 0]] = True
    vfin = np.ones(len(deg), bool)
    vfin[row[~np.isfinite(np.asarray(V, np.float64)[col]).all(1)]] = False
    zero = ~poisoned & ~live & vfin  # without entries, or fully masked, and no non-finite V row to multiply
    assert np.all(out[zero].view(np.uint32) == 0), f"{what}: a row without a live entry is not +0 in every column"
    rest = ~poisoned[:, None] & np.ones_like(ref["out"], bool)
    assert np.array_equal(np.isfinite(out)[rest], np.isfinite(ref["out"])[rest]), f"{what}: non-finite values not exactly where float64 has them"
    ok = rest & np.isfinite(ref["out"])
    ratio = np.abs(out[ok].astype(np.float64) - ref["out"][ok]) / ref["out_bound"][ok]
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} elements of Out beyond the bound, worst err / bound {worst:.3g}"
    if p is not None:
        p = np.asarray(p, np.float32)
        assert p.shape == ref["p"].shape, (what, p.shape, ref["p"].shape)
        nan_ref = np.isnan(ref["p"])
        assert np.array_equal(np.isnan(p), nan_ref), f"{what}: P is NaN exactly on the poisoned rows"
        masked = ~nan_ref & (ref["s"] == -np.inf)
        assert np.all(p[masked].view(np.uint32) == 0), f"{what}: a masked entry is not +0 bit for bit"
        r = np.abs(p[~nan_ref].astype(np.float64) - ref["p"][~nan_ref]) / ref["p_bound"][~nan_ref]
        wp = float(r.max()) if r.size else 0.0
        assert wp <= 1.0, f"{what}: {int((r > 1).sum())} entries of P beyond the bound, worst err / bound {wp:.3g}"
        worst = max(worst, wp)
    return worst


# ---- operands whose scores reproduce the score scenarios of softmax_ref

QKV_SCENARIOS = ["uniform4", "spread80", "masked30", "rows_masked", "poisoned"]


def operands(name, a, k, seed=0):
    """(Q [m, k], K [n, k], V [n, k]) fp32.  uniform4 / spread80: the scores span +-4 / +-80.  Masks: column 0 of Q is negative and a
    masked K row holds +inf there, so every edge into it scores -inf (masked30: 30 % of the K rows; rows_masked: 10 % and every K row
    some chosen rows touch, which masks those rows entirely).  poisoned: masks, and a NaN in Q for three rows."""
    rng = np.random.default_rng([seed, QKV_SCENARIOS.index(name), k])
    Q, K, V = (rng.uniform(-1, 1, (r, k)).astype(np.float32) for r in (a.m, a.n, a.n))
    row, col, rp = coo(a)
    if a.nnz:
        span = 80.0 if name == "spread80" else 4.0
        Q *= np.float32(span / max(1e-30, np.abs((Q.astype(np.float64)[row] * K.astype(np.float64)[col]).sum(1)).max()))
    if name in ("masked30", "rows_masked", "poisoned"):
        Q[:, 0] = -np.abs(Q[:, 0]) - np.float32(2.0 ** -20)
        masked = rng.random(a.n) < (0.3 if name == "masked30" else 0.1)
        if name == "rows_masked" and a.nnz:
            deg = np.diff(rp)
            ne = np.flatnonzero(deg > 0)
            for r in {int(ne[0]), int(ne[np.argmax(deg[ne])]), *rng.choice(ne, max(1, len(ne) // 10)).tolist()} - {int(ne[len(ne) // 2])}:
                masked[col[rp[r]:rp[r + 1]]] = True
        K[masked, 0] = np.inf
        if name == "poisoned" and a.nnz:
            deg = np.diff(rp)
            ne = np.flatnonzero(deg > 0)
            for i, r in enumerate(sorted({int(ne[0]), int(ne[np.argmax(deg[ne])]), int(ne[len(ne) // 2])})):
                Q[r, (i * 5) % k] = np.nan
    return Q, K, V

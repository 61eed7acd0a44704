"""float64 reference, bounds, operands, checkers and an fp32 emulation of the fused GATv2 attention (include/flex_spmm.h:
flex_gatv2_attention, flex_gatv2_attention_backward), shared by tests/test_gatv2_attention_host.py and tests/test_gpu_gatv2_attention.py.

k = H d.  Head h is columns [h d, (h + 1) d) of Xt, Xs, Out, g, gXt and gXs; att is [H, d]; the edge arrays P and dz are [entries, H],
entry-major.  For entry e of row r with source c = src(e), head h, column j of the head:
    x_ej    = Xt[r, hd + j] + Xs[c, hd + j]
    s_eh    = sum_j att[hd + j] * (x_ej > 0 ? x_ej : slope * x_ej)
    alpha_.h = flex_edge_softmax's softmax over the row, scale 1              (softmax_ref.forward_ref on the score rounded to fp32)
    Out[r, head h] = sum_e alpha_eh Xs[c, head h]
    da_eh   = <g[r, head h], Xs[c, head h]>     delta_rh = sum_e p_eh da_eh     dz_eh = p_eh (da_eh - delta_rh)
    f_ej    = x_ej > 0 ? 1 : slope
    gXt[r, hd + j] = sum_{e in r}       dz_eh att[hd + j] f_ej
    gXs[c, hd + j] = sum_{src(e) = c}  (dz_eh att[hd + j] f_ej  +  p_eh g[row(e), hd + j])
    gAtt[hd + j]   = sum_{all e}        dz_eh leaky(x_ej)
The reference is float64 numpy on the fp32 inputs; it takes the branch of the leaky ReLU from the sign of the fp32 sum fl(Xt + Xs),
which is what the kernel sees, and uses the fp32 value of slope.  Bounds, verbatim from the header (u = 2^-24, gamma(n) = n u / (1 - n u),
n_r / n_c = entries of the row / column, D_r = min(104, the spread of the row's finite scores), E = softmax_ref.E_ULP,
R_r = ceil(n_r / 4) + 8, L_ej = leaky(x_ej), w_ej = att_j f_ej):
    score   ds_e     = gamma(d + 2) sum_j |att_j| |L_ej| + (d + sum_j |att_j|) 2^-149
    alpha   dalpha_e = alpha_e [gamma(n_r + 4 D_r + (E + 3) R_r + 2 E + 4) + expm1(2 max_row(ds + |s| u))] + 2^-126
    Out     |Out - Out64| <= sum_e (gamma(n_r + 3) alpha_e + dalpha_e) |Xs| + 2^-126
    dda_e    = gamma(d) sum_j |g Xs| + d 2^-149
    ddz_e    = gamma(n_r + 3) p_e (|da_e| + sum_j |p_j da_j|) + p_e (dda_e + sum_j p_j dda_j) + n_r 2^-149
    |gXt - gXt64|   <= sum_{e in r} [(gamma(n_r + 1) |dz_e| + ddz_e) |w_ej| + |dz_e| 2^-149] + 2^-126
    |gXs - gXs64|   <= sum_{e in c} [(gamma(2 n_c + 1) |dz_e| + ddz_e) |w_ej| + gamma(2 n_c) p_e |g[row]| + |dz_e| 2^-149] + 2^-126
    |gAtt - gAtt64| <= sum_{all e}  [(gamma(T + 3) |dz_e| + ddz_e) |L_ej| + |dz_e| 2^-149] + 2^-126
    T = min(nnz, 2048 + ceil(max_r n_r / 4) + ceil(m / 4) + 24)
ds replaces flex_gat_attention's gamma(2) |s|: x is one rounding, L at most one more (subnormal: 2^-149, times |att_j|), the dot with
att a chain of four fmas per lane and a tree over the d / 4 lanes, d roundings at most.  ddz is flex_gat_attention's; it goes through
w = att f (one rounding) into gXt (one fma per entry, depth <= n_r) and gXs (two fmas per entry, depth <= 2 n_c), and through L into
gAtt, whose T is the depth of the tree the kernels use: a lane's chain over its wave's group (at most the group budget of 2048
entries, or a quarter of a block row), the slots (4), the waves (3), the chain of every fourth partial row (one row per workgroup, at
most ceil(m / 4) + 2 to a chain) and the four chains (3); never more than nnz, additions of zeros being exact.

The whole-graph line of gAtt is an A PRIORI bound, not the check of gAtt: gamma(T + 3) sum |dz| |L| over every entry of the graph exceeds
|gAtt| itself on large graphs (up to 7 |gAtt| on 7 copies of walk_graph(1) and 31 |gAtt| on 30, DESIGN.md section 3.23: gAtt = 0 would
pass), and a kernel that loses whole items of its groups stays within it in most columns.  check_backward keeps it, for small graphs and for the comparison with the composition of engine calls.  The
check of gAtt is check_att, in the two stages of the kernels:
    partial rows   row w of dAttWork is the sum of dz_e leaky(x_ej) over the entries of ONE workgroup of the row launch
                   (att_work_layout restates which), held to float64 under
                       sum_{e in w} [(gamma(n_w + 3) |dz_e| + ddz_e) |L_ej| + |dz_e| 2^-149] + 2^-126,    n_w = the entries of w
                   (any order of n fma terms is within gamma(n), so no model of the tree's depth enters; + 3 as in the line above); a row
                   without entries is +0 bit for bit
    the reduction  gAtt has the BITS of att_reduce32 of the rows the kernel wrote: four chains of every fourth row from 0.f, then
                   ((c0 + c1) + c2) + c3, plain fp32 additions in a fixed order"""
import numpy as np

from fused_attention_backward_ref import both_sides  # noqa: F401  (the tests take the lifted graph from here)
from fused_attention_ref import coo, threshold_graph  # noqa: F401
from multihead_attention_ref import head_columns
from softmax_ref import E_ULP, U, _per_row, _segments, forward_ref, gamma

SLOPE = 0.2
SCENARIOS = ["uniform4", "spread80", "zero", "poisoned", "att_signs", "x_zero"]
TINY, SUB = 2.0 ** -126, 2.0 ** -149


def scenarios_of(heads, shift=0):
    """One scenario per head, in turn, so that the heads of one call differ."""
    return [SCENARIOS[(h + shift) % len(SCENARIOS)] for h in range(heads)]


def _head_operands(name, a, d, seed):
    """(xt [m, d], xs [n, d], att [d]) fp32 of one head.  uniform4: x = xt + xs spans +-4, att +-1.  spread80: att scaled so that the
    scores of a row spread over tens.  zero: Xt and Xs are zero in the head's columns (every score +0 or -0, alpha uniform, Out and
    every gradient but gAtt's share zero).  x_zero: for the first entry of every third row with entries Xt[r] = -Xs[c] exactly, so
    x = +0 in every column there (the slope branch).  poisoned: a NaN in Xt for three rows, the longest among them.  att_signs: att alternates
    in sign and is exactly 0 in every third column."""
    rng = np.random.default_rng([seed, SCENARIOS.index(name)])
    xt, xs = (rng.uniform(-2, 2, (r, d)).astype(np.float32) for r in (a.m, a.n))
    att = rng.uniform(-1, 1, d).astype(np.float32)
    _, col, rp = coo(a)
    deg = np.diff(rp)
    ne = np.flatnonzero(deg > 0)
    if name == "spread80":
        att = (att * np.float32(40.0 / np.sqrt(d))).astype(np.float32)
    if name == "zero":
        xt[:], xs[:] = 0, 0
    if name == "x_zero":
        for r in ne[::3]:
            xt[r] = -xs[col[rp[r]]]
    if name == "poisoned" and len(ne):
        xt[sorted({int(ne[0]), int(ne[np.argmax(deg[ne])]), int(ne[len(ne) // 2])}), 0] = np.nan
    if name == "att_signs":
        att = (np.abs(att) * np.where(np.arange(d) % 2 == 0, 1, -1)).astype(np.float32)
        att[::3] = 0
    return xt, xs, att


def operands(names, a, k, seed=0):
    """(xt [m, k], xs [n, k], att [H, d]) fp32: head h holds scenario names[h] under a seed of its own."""
    heads = len(names)
    assert k % heads == 0
    parts = [_head_operands(name, a, k // heads, 100 * seed + h) for h, name in enumerate(names)]
    xt, xs = (np.ascontiguousarray(np.concatenate([p[i] for p in parts], axis=1)) for i in range(2))
    return xt, xs, np.ascontiguousarray(np.stack([p[2] for p in parts], axis=0))


def _sum_by(x, seg, n):
    out = np.zeros((n,) + x.shape[1:])
    np.add.at(out, seg, x)
    return out


def head_terms(a, xt, xs, att, slope, h, rows=None):
    """(s64 [entries], A [entries] = sum_j |att_j| |L_j|, L64 [entries, d], w64 [entries, d]) of head h: the float64 score with the
    branch of every column taken from the fp32 sum's sign."""
    row, col, _ = coo(a, rows)
    k, heads = xs.shape[1], att.shape[0]
    c = head_columns(k, heads, h)
    t32, s32 = np.asarray(xt, np.float32)[:, c], np.asarray(xs, np.float32)[:, c]
    a64 = np.asarray(att, np.float32).astype(np.float64)[h]
    sl = np.float64(np.float32(slope))
    with np.errstate(invalid="ignore", over="ignore"):
        pos = (t32[row] + s32[col]) > 0
        x = t32.astype(np.float64)[row] + s32.astype(np.float64)[col]
        L = np.where(pos, x, sl * x)
        return (a64 * L).sum(1), (np.abs(a64) * np.abs(L)).sum(1), L, a64 * np.where(pos, 1.0, sl)


C_ROUNDINGS, A_ROUNDINGS, B_ROUNDINGS = 3, 3, 0


def reference(a, xt, xs, att, slope, rows=None, c_r=C_ROUNDINGS):
    """dict(out, out_bound [rows, k]; p, p_bound, s [entries, H]) of the rows [r0, r1) (xt holds those rows only).  c_r = 32 gives the
    bound of the composition of engine calls instead (flex_spmm pads its rows: the header's nnz(row) + 32)."""
    row, col, rp = coo(a, rows)
    m, k, heads = len(rp) - 1, xs.shape[1], att.shape[0]
    d = k // heads
    assert xt.shape == (m, k) and xs.shape == (a.n, k) and att.shape == (heads, d), (xt.shape, xs.shape, att.shape)
    V64 = np.asarray(xs, np.float32).astype(np.float64)
    if len(row) == 0:
        z, e = np.zeros((m, k)), np.zeros((0, heads))
        return dict(out=z, out_bound=z + TINY, p=e, p_bound=e, s=e)
    starts, seg, n_r = _segments(rp)
    R = np.ceil(n_r / 4.0) + 8
    out, ob = np.zeros((m, k)), np.zeros((m, k))
    ps, pbs, ss = [], [], []
    for h in range(heads):
        s, A, _, _ = head_terms(a, xt, xs, att, slope, h, rows)
        with np.errstate(over="ignore"):
            s32 = s.astype(np.float32)
        p, _ = forward_ref(rp, s32, 1.0)
        fin = np.isfinite(s)
        sub = (d + np.abs(np.asarray(att, np.float64)[h]).sum()) * SUB
        # ds_e + |s_e| u, the argument of max_row in dalpha (|s| u: the reference's own rounding of the score to fp32)
        ds = np.where(fin, gamma(d + 2) * np.where(fin, A, 0.0) + sub + U * np.abs(np.where(fin, s, 0.0)), 0.0)
        ds_row = _per_row(np.maximum, ds, starts, seg)
        hi = _per_row(np.maximum, np.where(fin, s32.astype(np.float64), -np.inf), starts, seg)
        lo = _per_row(np.minimum, np.where(fin, s32.astype(np.float64), np.inf), starts, seg)
        with np.errstate(invalid="ignore"):
            D = np.where(hi == -np.inf, 0.0, np.minimum(104.0, hi - lo))
        p0 = np.where(np.isnan(p), 0.0, p)
        pb = p0 * (gamma(n_r + 4 * D + (E_ULP + 3) * R + 2 * E_ULP + 4) + np.expm1(2 * ds_row)) + TINY
        c = head_columns(k, heads, h)
        with np.errstate(invalid="ignore", over="ignore"):
            np.add.at(out[:, c], row, p[:, None] * V64[col][:, c])
            np.add.at(ob[:, c], row, (gamma(n_r + c_r) * p0 + pb)[:, None] * np.abs(V64[col][:, c]))
        ps.append(p)
        pbs.append(pb)
        ss.append(s32)
    return dict(out=out, out_bound=ob + TINY, p=np.stack(ps, 1), p_bound=np.stack(pbs, 1), s=np.stack(ss, 1))


def check(a, xt, xs, att, slope, out, p=None, rows=None, what=""):
    """Asserts per head the classes exactly (+0 rows, NaN rows, masked p = +0 bit for bit, non-finite values exactly where float64 has
    them) and the bound on every element of Out and, where given, of P [entries of the rows, H]; returns the worst err / bound."""
    ref = reference(a, xt, xs, att, slope, rows)
    heads, k = att.shape[0], xs.shape[1]
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
        vfin[row[~np.isfinite(np.asarray(xs, np.float64)[col][:, c]).all(1)]] = False
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


def att_depth(a):
    """T of the gAtt bound: the depth of the tree in which the kernels add the nnz terms of a column of gAtt."""
    _, _, rp = coo(a)
    deg = np.diff(rp)
    return int(min(a.nnz, 2048 + -(-int(deg.max(initial=0)) // 4) + -(-a.m // 4) + 24))


def backward_reference(a, xt, xs, att, p, g, slope, a_r=A_ROUNDINGS, b_r=B_ROUNDINGS, depth=None):
    """dict(gxt [m, k], gxs [n, k], gatt [H, d], dz [nnz, H] and their bounds gxt_bound, ...): float64 on the operands as given (p is
    taken as it is: the kernel's fp32 probabilities, or float64 ones for a comparison in float64).  a_r = 4, b_r = 32 and depth = nnz
    give the bounds of the composition on the same p instead (flex_edge_softmax_backward rounds its products, flex_spmm pads its rows,
    torch adds the terms of a gradient in an order of its own)."""
    row, col, rp = coo(a)
    k, heads = xs.shape[1], att.shape[0]
    d = k // heads
    V64, g64 = (np.asarray(x, np.float32).astype(np.float64) for x in (xs, g))
    p64 = np.asarray(p, np.float64)
    assert p64.shape == (a.nnz, heads), (p64.shape, (a.nnz, heads))
    n_r, n_c = np.diff(rp)[row], np.bincount(col, minlength=a.n)[col]
    T = att_depth(a) if depth is None else depth
    res = {key: [] for key in ("gxt", "gxs", "gatt", "dz", "gxt_bound", "gxs_bound", "gatt_bound", "dz_bound")}
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(heads):
            c = head_columns(k, heads, h)
            _, _, L, w = head_terms(a, xt, xs, att, slope, h)
            ph, ap = p64[:, h], np.abs(p64[:, h])
            gr, vc = g64[row][:, c], V64[col][:, c]
            da = (gr * vc).sum(1)
            dda = gamma(d) * (np.abs(gr) * np.abs(vc)).sum(1) + d * SUB
            delta = _sum_by(ph * da, row, a.m)
            dz = ph * (da - delta[row])
            adz = np.abs(dz)[:, None]
            ddz = gamma(n_r + a_r) * ap * (np.abs(da) + _sum_by(np.abs(ph * da), row, a.m)[row]) + ap * (dda + _sum_by(ap * dda, row, a.m)[row]) + n_r * SUB
            res["dz"].append(dz)
            res["dz_bound"].append(ddz)
            res["gxt"].append(_sum_by(dz[:, None] * w, row, a.m))
            res["gxt_bound"].append(_sum_by((gamma(n_r + 1 + b_r)[:, None] * adz + ddz[:, None]) * np.abs(w) + adz * SUB, row, a.m) + TINY)
            res["gxs"].append(_sum_by(dz[:, None] * w + ph[:, None] * gr, col, a.n))
            res["gxs_bound"].append(_sum_by((gamma(2 * n_c + 1 + b_r)[:, None] * adz + ddz[:, None]) * np.abs(w)
                                            + (gamma(2 * n_c + b_r) * ap)[:, None] * np.abs(gr) + adz * SUB, col, a.n) + TINY)
            res["gatt"].append((dz[:, None] * L).sum(0))
            res["gatt_bound"].append(((gamma(T + 3) * adz + ddz[:, None]) * np.abs(L) + adz * SUB).sum(0) + TINY)
    return {key: np.stack(v, axis=0 if key.startswith("gatt") else 1) if key.startswith(("gatt", "dz")) else np.concatenate(v, axis=1) for key, v in res.items()}


def check_backward(a, xt, xs, att, p, g, slope, gXt=None, gXs=None, gAtt=None, dz=None, what="", ratios=None):
    """Asserts, for every output given, the classes exactly (+0 rows without entries, NaN and infinities where float64 has them) and the
    bound on every other element; returns the worst err / bound (ratios, a dict: the worst of each output is kept in it)."""
    ref = backward_reference(a, xt, xs, att, np.asarray(p, np.float32), g, slope)
    row, col, rp = coo(a)
    empty = {"gxt": np.diff(rp) == 0, "gxs": np.bincount(col, minlength=a.n) == 0}
    worst = 0.0
    for key, got in (("gxt", gXt), ("gxs", gXs), ("gatt", gAtt), ("dz", dz)):
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


# ---- gAtt in the two stages of the kernels: the partial row of every workgroup of the row launch, then gatt_reduce

KXCDS, WAVES = 8, 4  # internal.h: kXcds, kWavesPerBlock


def att_work_layout(rowptr, k, budget, remap):
    """(row [nnz]: the row of dAttWork that receives the term of every entry, the row count): rows_backward restated.  The block rows
    come first, a workgroup and a row each, in the order of walk_model's blocks; group g of the walk is run by wave g % 4 of workgroup
    g // 4, and a workgroup stores at its blockIdx.x.  Under the remap the grid of the grouped items is padded to a multiple of 8
    workgroups and the kernel runs workgroup wg = (x % 8) * per + x // 8 at id x (per = padded / 8): wg is stored at
    x = (wg % per) * 8 + wg // per, and the ids that no workgroup with a group maps to hold rows without entries."""
    from attention_walk_graphs import walk_model
    items, grp, blocks = walk_model(rowptr, k, budget)
    nnz = int(np.asarray(rowptr, np.int64)[-1] - np.asarray(rowptr, np.int64)[0])
    wgs = -(-(len(grp) - 1) // WAVES) if len(items) else 0
    if remap:
        wgs = -(-wgs // KXCDS) * KXCDS
    row = np.full(nnz, -1, np.int64)
    first = int(np.asarray(rowptr, np.int64)[0])
    for b, (e0, cnt, _, _) in enumerate(blocks.tolist()):
        row[e0 - first:e0 - first + cnt] = b
    wg = (np.searchsorted(grp, np.arange(len(items)), side="right") - 1) // WAVES
    if remap and wgs:
        per = wgs // KXCDS
        wg = (wg % per) * KXCDS + wg // per
    at = np.repeat(items[:, 0] - first, items[:, 1]) + (np.arange(int(items[:, 1].sum())) - np.repeat(np.cumsum(items[:, 1]) - items[:, 1], items[:, 1]))
    row[at] = np.repeat(len(blocks) + wg, items[:, 1])
    assert (row >= 0).all() and (row < len(blocks) + wgs).all()
    return row, len(blocks) + wgs


def att_line_terms(a, xt, xs, att, p, g, slope, drop=None):
    """(w, s1, s2), each [m, k] in float64: per line (row) of a the sums over its entries of dz_e L_ej, of |dz_e| |L_ej| and of
    ddz_e |L_ej| + |dz_e| 2^-149, dz and its bound ddz backward_reference's on the probabilities given -- gatv2_dropout_ref's under
    drop = (p, seed).  A line's entries all belong to one workgroup of the row launch, so the rows of dAttWork are sums of lines."""
    if drop is None:
        ref = backward_reference(a, xt, xs, att, p, g, slope)
    else:
        import gatv2_dropout_ref
        ref = gatv2_dropout_ref.backward_reference(a, xt, xs, att, p, g, slope, *drop)
    row, _, _ = coo(a)
    k, heads = xs.shape[1], att.shape[0]
    d = k // heads
    w, s1, s2 = (np.zeros((a.m, k)) for _ in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(heads):
            _, _, L, _ = head_terms(a, xt, xs, att, slope, h)
            dz, adz, ddz = ref["dz"][:, h], np.abs(ref["dz"][:, h]), ref["dz_bound"][:, h]
            for j in range(d):
                aL = np.abs(L[:, j])
                w[:, h * d + j] = np.bincount(row, weights=dz * L[:, j], minlength=a.m)
                s1[:, h * d + j] = np.bincount(row, weights=adz * aL, minlength=a.m)
                s2[:, h * d + j] = np.bincount(row, weights=ddz * aL + adz * SUB, minlength=a.m)
    return w, s1, s2


def att_partials_reference(a, xt, xs, att, p, g, slope, layout, drop=None, copies=1, lines=None):
    """(want [rows, k], bound [rows, k]) in float64 of the rows of dAttWork under layout = att_work_layout(...), from the probabilities
    given (the kernel's own fp32 P): want = sum over the row's entries of dz_e leaky(x_ej), bound = gamma(n_w + 3) sum |dz_e| |L_ej|
    + sum (ddz_e |L_ej| + |dz_e| 2^-149) + 2^-126, n_w the entries of the row; a row without entries is 0 (the checker asks it +0 bit
    for bit).  copies = T: the layout is that of the block-diagonal graph of T copies of a with the operands repeated (no dropout:
    its mask differs from copy to copy), and a row of dAttWork is a sum of whole lines of known copies, each taken from the one-copy
    terms.  lines: att_line_terms(...) computed before."""
    row_of, n_rows = layout
    assert drop is None or copies == 1
    w, s1, s2 = att_line_terms(a, xt, xs, att, p, g, slope, drop) if lines is None else lines
    rp = np.asarray(a.rowPtr, np.int64)
    assert row_of.shape == (copies * a.nnz,)
    first = (rp[:-1][None, :] + a.nnz * np.arange(copies)[:, None]).reshape(-1)  # the first entry of every line of every copy
    full = np.tile(np.diff(rp) > 0, copies)
    line_row = row_of[first[full]]
    n_w = np.bincount(row_of, minlength=n_rows)
    assert np.array_equal(np.bincount(line_row, weights=np.tile(np.diff(rp), copies)[full], minlength=n_rows), n_w)  # whole lines
    k = xs.shape[1]
    want, bound = np.zeros((n_rows, k)), np.zeros((n_rows, k))
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(k):
            t = [np.bincount(line_row, weights=np.tile(x[:, c], copies)[full], minlength=n_rows) for x in (w, s1, s2)]
            want[:, c], bound[:, c] = t[0], gamma(n_w + 3) * t[1] + t[2]
    return want, bound + TINY


def att_reduce32(att_work):
    """gatt_reduce on the rows [rows, k] in fp32 numpy: chain w takes rows w, w + 4, ... from 0.f, then ((c0 + c1) + c2) + c3.  [k]."""
    x = np.asarray(att_work, np.float32)
    chains = np.zeros((WAVES, x.shape[1]), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(x.shape[0]):
            chains[r % WAVES] += x[r]
        tot = chains[0]
        for w in range(1, WAVES):
            tot = tot + chains[w]
    return tot.astype(np.float32)


def check_att_reduce(att_work, gatt, what=""):
    """gatt [H, d] has the bits of att_reduce32 of att_work [rows, k], the rows the kernel itself wrote (NaN for NaN, whatever the
    payload)."""
    gatt = np.asarray(gatt, np.float32).reshape(-1)
    red = att_reduce32(att_work)
    assert gatt.shape == red.shape, f"{what}: gAtt has {gatt.size} elements, want {red.size}"
    assert np.array_equal(np.isnan(gatt), np.isnan(red)), f"{what}: gAtt is NaN exactly where the sum of the rows of dAttWork is"
    ok = ~np.isnan(red)
    differ = gatt[ok].view(np.uint32) != red[ok].view(np.uint32)
    assert not differ.any(), f"{what}: gAtt has not the bits of gatt_reduce on the rows of dAttWork in {int(differ.sum())} of {red.size} columns"


def check_att(a, xt, xs, att, p, g, slope, att_work, gatt, layout, drop=None, what="", ratios=None, copies=1, lines=None):
    """gAtt in two stages.  att_work: what the kernel left in dAttWork, [rows of the layout, k] (or flat); gatt [H, d].  Asserts that
    every element of every partial row is within its bound, a row without entries +0 bit for bit, NaN and infinities exactly where
    float64 has them; and that gatt has the bits of att_reduce32(att_work).  copies, lines: att_partials_reference's.  Returns the
    worst err / bound of the partial rows (ratios["att_work"] keeps it)."""
    row_of, n_rows = layout
    k = xs.shape[1]
    got = np.asarray(att_work, np.float32)
    assert got.size == n_rows * k, f"{what}: dAttWork holds {got.size} floats, the layout has {n_rows} rows of {k}"
    got = got.reshape(n_rows, k)
    want, bound = att_partials_reference(a, xt, xs, att, np.asarray(p, np.float32), g, slope, layout, drop, copies, lines)
    idle = np.bincount(row_of, minlength=n_rows) == 0
    assert np.all(got[idle].view(np.uint32) == 0), f"{what}: {int((got[idle].view(np.uint32) != 0).any(1).sum())} rows of dAttWork without entries are not +0 in every column"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: dAttWork is NaN where float64 is, and nowhere else ({int((np.isnan(got) != np.isnan(want)).sum())} differ)"
    inf = np.isinf(want)
    assert np.array_equal(got[inf].astype(np.float64), want[inf]) and not np.isinf(got[~inf]).any(), f"{what}: dAttWork: infinities as float64 gives them"
    fin = np.isfinite(want)
    ratio = np.zeros(want.shape)
    ratio[fin] = np.abs(got[fin].astype(np.float64) - want[fin]) / bound[fin]
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, (f"{what}: {int((ratio > 1).sum())} elements in {int((ratio > 1).any(1).sum())} rows of dAttWork beyond the bound, worst err / bound {worst:.3g}, "
                          f"median of the rows beyond it {float(np.median(ratio.max(1)[(ratio > 1).any(1)])):.3g}")
    check_att_reduce(got, gatt, what)
    if ratios is not None:
        ratios["att_work"] = max(worst, ratios.get("att_work", 0.0))
    return worst


# ---- an evaluation in fp32 arithmetic

FAULTS = ("no_att", "leaky_after_dot", "slope_on_positive", "next_heads_att", "head_major", "joint_softmax", "gxs_no_value", "gxt_no_f",
          "gatt_from_x", "poison_spreads")
F32 = np.float32


def _fma(x, y, z):
    """fl(x y + z) on fp32 arrays: the product of two floats is exact in float64"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(x, F32).astype(np.float64) * np.asarray(y, F32).astype(np.float64) + np.asarray(z, F32).astype(np.float64)).astype(F32)


def _dot32(x, y):
    """sum_j x_j y_j over the last axis as a chain of fmas in fp32"""
    x, y = np.broadcast_arrays(x, y)
    acc = np.zeros(x.shape[:-1], F32)
    for j in range(x.shape[-1]):
        acc = _fma(x[..., j], y[..., j], acc)
    return acc


def _seg_fma(terms, seg, n, d):
    """[n, d] fp32: for every segment, in entry order, acc = fl(a B + acc) for each (a [E], B [E, d]) of terms: one fma per term"""
    order = np.argsort(seg, kind="stable")
    counts = np.bincount(seg, minlength=n)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    acc = np.zeros((n, d), F32)
    for t in range(int(counts.max(initial=0))):
        live = np.flatnonzero(counts > t)
        e = order[starts[live] + t]
        for x, B in terms:
            acc[live] = _fma(np.asarray(x, F32)[e][:, None], np.asarray(B, F32)[e], acc[live])
    return acc


def fp32_result(a, xt, xs, att, slope, g=None, p=None, fault=None, partials=None):
    """dict(out, p) -- and, with g, dict(gxt, gxs, gatt, dz) from the p given (default: this forward's) -- evaluated in fp32 arithmetic
    with numpy (fmas where the kernels use them, chains where they use trees): what a right kernel returns up to the order of its
    additions.  The faults the checkers must catch: no_att: att left out (all ones); leaky_after_dot: the leaky ReLU applied after the
    dot with att (GAT's order); slope_on_positive: the slope applied where x > 0; next_heads_att: att of head h + 1 used for head h;
    head_major: P and dz delivered as [H, nnz] in the same memory; joint_softmax: one softmax over all heads' scores of a row;
    gxs_no_value: gXs without its term p g; gxt_no_f: gXt without f; gatt_from_x: gAtt from dz x in place of dz leaky(x);
    poison_spreads: a row that one head poisons is NaN in every head's columns of Out.
    partials = att_work_layout(...): with g, also att_work [rows, k], every row of dAttWork as a chain of fmas over its entries in entry
    order, and gatt is then att_reduce32 of these rows: the two stages of the kernels."""
    assert fault is None or fault in FAULTS, fault
    row, col, rp = coo(a)
    k, heads = xs.shape[1], att.shape[0]
    d = k // heads
    sl = F32(slope)
    xt, xs, att = (np.asarray(x, F32) for x in (xt, xs, att))
    att_used = np.ones_like(att) if fault == "no_att" else np.roll(att, -1, axis=0) if fault == "next_heads_att" else att
    S, Ls, Xs_, Ws = [], [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(heads):
            c = head_columns(k, heads, h)
            x = xt[row][:, c] + xs[col][:, c]
            pos = x <= 0 if fault == "slope_on_positive" else x > 0
            L = np.where(pos, x, sl * x).astype(F32)
            if fault == "leaky_after_dot":
                t = _dot32(att_used[h], x)
                s = np.where(t > 0, t, sl * t).astype(F32)
            else:
                s = _dot32(att_used[h], L)
            S.append(s)
            Ls.append(L)
            Xs_.append(x)
            Ws.append(np.where(pos, att_used[h], att_used[h] * sl).astype(F32))
        s = np.stack(S, 1)
        key = np.where(np.isnan(s) | (s == np.inf), np.inf, s).astype(F32)
        M = np.full((a.m, heads), -np.inf, F32)
        np.maximum.at(M, row, key)
        if fault == "joint_softmax":
            M = np.repeat(M.max(1, keepdims=True), heads, axis=1)
        poisoned, dead = M == np.inf, M == -np.inf
        Mf = np.where(poisoned | dead, F32(0), M)
        t = np.where(s == -np.inf, F32(0), np.exp((s - Mf[row]).astype(F32))).astype(F32)
        t = np.where(poisoned[row] | dead[row], F32(0), t)
        Lsum = np.zeros((a.m, heads), F32)
        np.add.at(Lsum, row, t)
        if fault == "joint_softmax":
            Lsum = np.repeat(Lsum.sum(1, keepdims=True), heads, axis=1).astype(F32)
        pr = np.where(dead[row], F32(0), t / np.where(dead, F32(1), Lsum)[row]).astype(F32)
        pr[poisoned[row]] = np.nan
        out = np.zeros((a.m, k), F32)
        for h in range(heads):
            c = head_columns(k, heads, h)
            o = _seg_fma([(t[:, h], xs[col][:, c])], row, a.m, d)
            o = np.where(dead[:, h, None], o, o / np.where(dead[:, h], F32(1), Lsum[:, h])[:, None]).astype(F32)
            o[poisoned[:, h]] = np.nan
            out[:, c] = o
    res = dict(out=out, p=pr)
    if fault == "poison_spreads":
        res["out"][np.isnan(res["out"]).any(1)] = np.nan
    if g is not None:
        pin = res["p"] if p is None else np.asarray(p, F32)
        g = np.asarray(g, F32)
        gxt, gxs, gatt, dzs = np.zeros((a.m, k), F32), np.zeros((a.n, k), F32), np.zeros((heads, d), F32), []
        chunk = 512
        rows32 = None if partials is None else np.zeros((partials[1], k), F32)
        with np.errstate(invalid="ignore", over="ignore"):
            for h in range(heads):
                c = head_columns(k, heads, h)
                ph = pin[:, h]
                da = _dot32(g[row][:, c], xs[col][:, c])
                delta = _seg_fma([(ph, da[:, None])], row, a.m, 1)[:, 0]
                dz = (ph * (da - delta[row]).astype(F32)).astype(F32)
                dzs.append(dz)
                w = np.broadcast_to(att_used[h], Ws[h].shape) if fault == "gxt_no_f" else Ws[h]
                gxt[:, c] = _seg_fma([(dz, w)], row, a.m, d)
                gxs[:, c] = _seg_fma([(dz, Ws[h])] + ([] if fault == "gxs_no_value" else [(ph, g[row][:, c])]), col, a.n, d)
                # chains of `chunk` entries, then a chain over the chunks: depth chunk + chunks <= T
                src = Xs_[h] if fault == "gatt_from_x" else Ls[h]
                part = _seg_fma([(dz, src)], np.arange(a.nnz) // chunk, -(-a.nnz // chunk), d)
                tot = np.zeros(d, F32)
                for r in range(part.shape[0]):
                    tot = (tot + part[r]).astype(F32)
                gatt[h] = tot
                if partials is not None:
                    rows32[:, c] = _seg_fma([(dz, src)], partials[0], partials[1], d)
        res.update(gxt=gxt, gxs=gxs, gatt=gatt, dz=np.stack(dzs, 1))
        if partials is not None:
            res.update(att_work=rows32, gatt=att_reduce32(rows32).reshape(heads, d))
    if fault == "head_major":
        for key in ("p", "dz"):
            if key in res:
                res[key] = np.ascontiguousarray(res[key].T).reshape(res[key].shape)
    return res


def propagated_bounds(a, xt, xs, att, slope, g, c_r=C_ROUNDINGS, a_r=A_ROUNDINGS, b_r=B_ROUNDINGS, depth=None, with_dz=False):
    """(Out, gXt, gXs, gAtt) bounds of a forward and backward step against float64 THROUGHOUT, for finite scores: the backward starts
    from the forward's fp32 alpha, so alpha's own bound dalpha enters every gradient beside the backward's bounds (first order, 0.1 %
    spare):
        ddz_e = gamma(n_r + 3) alpha_e (|da_e| + sum_j alpha_j |da_j|) + n_r 2^-149
                + dalpha_e (|da_e| + sum_j alpha_j |da_j|) + alpha_e (dda_e + sum_j (dalpha_j |da_j| + alpha_j dda_j))
    and gXt, gXs, gAtt as in the module's head on this ddz, with (gamma(2 n_c) alpha_e + dalpha_e) |g| for the value term of gXs.
    c_r, a_r, b_r, depth: as in reference() and backward_reference(), for a composition of other calls; with_dz: the bound ddz [nnz, H]
    and the bound of alpha come fifth and sixth."""
    ref = reference(a, xt, xs, att, slope, c_r=c_r)
    row, col, rp = coo(a)
    k, heads = xs.shape[1], att.shape[0]
    d = k // heads
    V64, g64 = (np.asarray(x, np.float64) for x in (xs, g))
    n_r, n_c = np.diff(rp)[row], np.bincount(col, minlength=a.n)[col]
    T = att_depth(a) if depth is None else depth
    gxt, gxs, gatt, dzb = [], [], [], []
    for h in range(heads):
        c = head_columns(k, heads, h)
        _, _, L, w = head_terms(a, xt, xs, att, slope, h)
        al, dal = ref["p"][:, h], ref["p_bound"][:, h]
        gr, vc = g64[row][:, c], V64[col][:, c]
        da = (gr * vc).sum(1)
        ada = np.abs(da)
        dda = gamma(d) * (np.abs(gr) * np.abs(vc)).sum(1) + d * SUB
        spread = ada + _sum_by(al * ada, row, a.m)[row]
        ddz = (gamma(n_r + a_r) * al * spread + n_r * SUB + dal * spread + al * (dda + _sum_by(dal * ada + al * dda, row, a.m)[row]))[:, None]
        dzb.append(ddz[:, 0])
        adz = np.abs(al * (da - _sum_by(al * da, row, a.m)[row]))[:, None]
        gxt.append(_sum_by((gamma(n_r + 1 + b_r)[:, None] * adz + ddz) * np.abs(w) + adz * SUB, row, a.m) + TINY)
        gxs.append(_sum_by((gamma(2 * n_c + 1 + b_r)[:, None] * adz + ddz) * np.abs(w) + (gamma(2 * n_c + b_r) * al + dal)[:, None] * np.abs(gr) + adz * SUB, col, a.n) + TINY)
        gatt.append(((gamma(T + 3) * adz + ddz) * np.abs(L) + adz * SUB).sum(0) + TINY)
    res = (ref["out_bound"], np.concatenate(gxt, 1), np.concatenate(gxs, 1), np.stack(gatt, 0)) + ((np.stack(dzb, 1), ref["p_bound"]) if with_dz else ())
    return tuple(1.001 * t for t in res)

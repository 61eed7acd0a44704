"""The attention dropout of the fused GAT attention on the GPU (flex_gat_attention_dropout, flex_gat_attention_dropout_backward): Out,
P, gEl, gEr, gV and dWork against float64 on every element under the bounds of tests/gat_dropout_ref.py over the table of
tests/test_gat_dropout_host.py (every (W, NS) form in all three kernels); P and p = 0 against the undropped calls bit for bit; one mask
in all three launches, equal to flex_dropout_mask; non-finite V and g rows behind dropped entries; the output invariants (no P, the
subsets of the gradients, run to run, a captured graph, another seed, padded rows); the refusals; a row-range shard; and
SparseOperator.gat_attention(..., dropout=p) with its gradients against a float64 torch evaluation."""
import numpy as np
import pytest

import attention_dropout_ref as ad
import flex_amd
import gat_attention_ref as gat
import gat_dropout_ref as gd
from backward_ref import _directed
from flex_amd import binding
from softmax_ref import gamma
from test_gat_dropout_host import CASES, SEED, SLOPE, case_id, case_operands, grad, graph

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = -12345.5
_plans, _runs = {}, {}


def plan(name, k, **kw):
    key = (name, k, tuple(sorted(kw.items())))
    if key not in _plans:
        kw.setdefault("attention_backward", True)
        _plans[key] = flex_amd.Plan(graph(name), k, attention=True, **kw)
        _plans[key].self_check()
    return _plans[key]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _filled(shape):
    return torch.full(shape, SENTINEL, device="cuda")


def _is_fill(x):
    return bool(np.all(x == np.float32(SENTINEL)))


def _same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and bool(np.array_equal(x.view(np.uint8), y.view(np.uint8)))


def _forward(p, a, el, er, V, drop, seed=SEED, slope=SLOPE, with_p=True):
    """(Out, P [nnz, H]) on the host; both start at the sentinel."""
    H = el.shape[1]
    pd = _filled((a.nnz, H)) if with_p else None
    out = p.gat_attention_dropout(_dev(el), _dev(er), _dev(V), slope, drop, seed, out=_filled((a.m, V.shape[1])), probs=pd)
    return _host(out), (_host(pd) if with_p else None)


def _backward(p, a, el, er, V, pr, g, drop, seed=SEED, slope=SLOPE, want=(True, True, True)):
    """(gEl, gEr, gV, dx) on the host; an output that is not wanted is None, dx is what dWork holds afterwards."""
    work = _filled((a.nnz, el.shape[1]))
    outs = p.gat_attention_dropout_backward(_dev(el), _dev(er), _dev(V), _dev(pr), _dev(g), slope, drop, seed, work=work, want=want)
    return tuple(None if t is None else _host(t) for t in outs) + (_host(work),)


def _run(c):
    """The forward and backward of a case of the table, run once and shared by the tests below; nothing changes it.
    (Out, P, gEl, gEr, gV, dx)."""
    if c not in _runs:
        name, k, H, drop = c
        a, el, er, V, g = case_operands(name, k, H)
        p = plan(name, k)
        out, pr = _forward(p, a, el, er, V, drop)
        _runs[c] = (out, pr) + _backward(p, a, el, er, V, pr, g, drop)
    return _runs[c]


KEYS = ("out", "p", "gel", "ger", "gv", "dx")


# ---- 1. against float64

@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_every_output_against_float64(c):
    name, k, H, drop = c
    a, el, er, V, g = case_operands(name, k, H)
    out, pr, gel, ger, gv, dx = _run(c)
    each, what = {}, case_id(c)
    gd.check(a, el, er, V, SLOPE, drop, SEED, out, pr, what=what, ratios=each)
    gd.check_backward(a, el, er, V, pr, g, SLOPE, drop, SEED, gel, ger, gv, dx, what=what, ratios=each)
    print(f"{what}: worst err / bound " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))


# ---- 2. P is the undropped call's, and p = 0 is the undropped call

def _undropped(p, a, el, er, V, g):
    """(Out, P, gEl, gEr, gV, dx) of the undropped entry points on the same operands."""
    H = el.shape[1]
    eld, erd, Vd, gd_ = (_dev(x) for x in (el, er, V, g))
    pd, work = _filled((a.nnz, H)), _filled((a.nnz, H))
    o = p.gat_attention(eld, erd, Vd, SLOPE, out=_filled((a.m, V.shape[1])), p=pd)
    grads = p.gat_attention_backward(eld, erd, Vd, pd, gd_, SLOPE, work=work)
    return (_host(o), _host(pd)) + tuple(_host(t) for t in grads) + (_host(work),)


@pytest.mark.parametrize("name,k,H", [("thresholds_lifted", 48, 3), ("long_rows", 64, 8), ("directed_empty", 128, 1), ("thresholds_lifted", 1024, 64)])
def test_p_is_the_undropped_calls_and_p_zero_is_the_undropped_call(name, k, H):
    a, el, er, V, g = case_operands(name, k, H)
    p = plan(name, k)
    plain = _undropped(p, a, el, er, V, g)
    pr = _run((name, k, H, 0.5))[1]
    assert _same_bits(pr, plain[1]), f"P differs from gat_attention's in {int((pr.view(np.uint32) != plain[1].view(np.uint32)).sum())} entries"
    out0, p0 = _forward(p, a, el, er, V, 0.0)
    zero = (out0, p0) + _backward(p, a, el, er, V, p0, g, 0.0)
    for key, x, y in zip(KEYS, zero, plain):
        assert _same_bits(x, y), f"p = 0: {key} differs from the undropped entry point's"


# ---- 3. one mask in all three launches, and it is flex_dropout_mask

def test_the_three_launches_and_flex_dropout_mask_agree_on_every_bit():
    """Every column has exactly one entry (col(e) = e) and row r has r + 1 entries, r < d: slot rows and wave rows, four slabs.
    el = er = 0, so x = +0 takes the slope branch and alpha is 1 / len; V is one-hot: entry e, the j-th of its row, holds 1 at column j
    of every head, so Out[r, h d + j] is alpha w of that entry and head alone; g = 1, so gV[e, head h] is alpha w in every column of
    the head and da = w exactly."""
    k, H = 1024, 4
    d = k // H
    lens = np.arange(1, d + 1)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    nnz = int(rp[-1])
    a = binding.HostCsr(rp, np.arange(nnz, dtype=np.uint32), np.ones(nnz, np.float32), n=nnz)
    p = flex_amd.Plan(a, k, attention=True, attention_backward=True)
    row = np.repeat(np.arange(d), lens)
    j = np.arange(nnz) - rp[:-1].astype(np.int64)[row]
    Vd = torch.zeros((nnz, k), device="cuda")
    e_t, j_t = torch.arange(nnz, device="cuda"), torch.from_numpy(j).cuda()
    for h in range(H):
        Vd[e_t, h * d + j_t] = 1
    eld, erd, gd_ = torch.zeros((d, H), device="cuda"), torch.zeros((nnz, H), device="cuda"), torch.ones((d, k), device="cuda")
    pd = torch.empty((nnz, H), device="cuda")
    for drop in (0.5, 0.9):
        out = p.gat_attention_dropout(eld, erd, Vd, SLOPE, drop, SEED, probs=pd)
        _, _, gv = p.gat_attention_dropout_backward(eld, erd, Vd, pd, gd_, SLOPE, drop, SEED, want=(False, False, True))
        torch.cuda.synchronize()
        want = binding.dropout_mask(SEED, drop, 0, nnz * H).astype(bool).reshape(nnz, H)
        assert np.array_equal(want, ad.keep(SEED, drop, np.arange(nnz * H, dtype=np.uint64)).reshape(nnz, H))
        out_nz = (out != 0).cpu().numpy().reshape(d, H, d)
        gv_nz = (gv != 0).view(nnz, H, d)
        assert bool((gv_nz.all(2) == gv_nz.any(2)).all()), "gV: a head of an entry is zero in all of its columns or in none"
        gv_keep = gv_nz.any(2).cpu().numpy()
        fwd_keep = out_nz[row, :, j]
        tail = np.arange(d)[None, :] >= lens[:, None]  # columns past the row's entries stay 0
        assert not out_nz.transpose(0, 2, 1)[tail].any()
        assert np.array_equal(fwd_keep, want), f"p={drop}: the forward's mask differs from flex_dropout_mask in {int((fwd_keep != want).sum())} bits"
        assert np.array_equal(gv_keep, want), f"p={drop}: the column launch's mask differs from flex_dropout_mask in {int((gv_keep != want).sum())} bits"
        # the row backward: dx = slope p (da - delta) with da = w (g = 1, V one-hot: <g, V> = 1, and c x 1 is exact).  Tolerance: delta is
        # n_r fmas, then one subtraction and two products, on a p that is 1 / len within a few roundings (the exponential of 0 is 1, the
        # sum is exact): gamma(n_r + 8) on slope p (|da| + |delta|) <= 2 slope p c
        work = torch.empty((nnz, H), device="cuda")
        p.gat_attention_dropout_backward(eld, erd, Vd, pd, gd_, SLOPE, drop, SEED, work=work, want=(True, False, False))
        dx = _host(work).astype(np.float64)
        al, c = 1.0 / lens[row], ad.factor(drop)
        da = want * c
        delta = np.zeros((d, H))
        np.add.at(delta, row, al[:, None] * da)
        sl = float(np.float32(SLOPE))
        ref = sl * al[:, None] * (da - delta[row])
        tol = gamma(lens[row] + 8)[:, None] * 2 * sl * al[:, None] * c
        assert np.all(np.abs(dx - ref) <= tol), f"p={drop}: dWork is not the dx of that mask (worst err / tolerance {float((np.abs(dx - ref) / tol).max()):.3g})"
    p.destroy()


# ---- 4. non-finite V and g behind dropped entries, and fully dropped heads

@pytest.mark.parametrize("name,k,H,drop", [("thresholds_lifted", 32, 4, 0.5), ("directed_empty", 128, 1, 0.6), ("long_rows", 32, 4, 0.9)])
def test_non_finite_rows_behind_dropped_entries_reach_nothing_and_a_fully_dropped_head_is_zero(name, k, H, drop):
    a = graph(name)
    d = k // H
    el, er, V = gat.operands(["uniform4"] * H, a, k, seed=12)
    g = grad(a, k, 12)
    p = plan(name, k)
    row, col, rp = gat.coo(a)
    kp = ad.kept_entries(a, H, drop, SEED)
    Vbad, gbad, hit_v, hit_g = V.copy(), g.copy(), 0, 0
    dead_rows = []
    for h in range(H):
        any_kept = np.zeros(a.n, bool)
        any_kept[col[kp[:, h]]] = True
        cols = np.flatnonzero(~any_kept & (np.bincount(col, minlength=a.n) > 0))  # columns with entries, all of them dropped in head h
        Vbad[cols[0::2], h * d:(h + 1) * d] = np.inf
        Vbad[cols[1::2], h * d:(h + 1) * d] = np.nan
        hit_v += len(cols)
        any_kept = np.zeros(a.m, bool)
        any_kept[row[kp[:, h]]] = True
        rows = np.flatnonzero(~any_kept & (np.diff(rp) > 0))  # non-empty rows, every entry dropped in head h
        gbad[rows[0::2], h * d:(h + 1) * d] = np.inf
        gbad[rows[1::2], h * d:(h + 1) * d] = np.nan
        hit_g += len(rows)
        dead_rows.append(rows)
    assert hit_v >= 8 and hit_g >= 8, (hit_v, hit_g)  # the input has such columns and such heads

    def run(Vx, gx):
        out, pr = _forward(p, a, el, er, Vx, drop)
        return (out, pr) + _backward(p, a, el, er, Vx, pr, gx, drop)

    clean, dirty = run(V, g), run(Vbad, gbad)
    for key, x, y in zip(KEYS, clean, dirty):
        assert np.isfinite(y).all(), f"{key} is not finite"
        assert _same_bits(x, y), f"{key} changed with the V and g rows behind dropped entries"
    for h, rows in enumerate(dead_rows):  # a head of a non-empty row whose entries are all dropped is +0 bits in Out
        assert not np.ascontiguousarray(clean[0][rows, h * d:(h + 1) * d]).view(np.uint8).any()
    gd.check(a, el, er, Vbad, SLOPE, drop, SEED, dirty[0], dirty[1], what="non-finite V")


# ---- 5. output invariants

def test_without_p_the_same_out_and_every_gradient_has_the_same_bits_whichever_others_are_asked_for():
    c = ("thresholds_lifted", 48, 3, 0.5)
    name, k, H, drop = c
    a, el, er, V, g = case_operands(name, k, H)
    p = plan(name, k)
    out, pr, *full = _run(c)
    assert _same_bits(_forward(p, a, el, er, V, drop, with_p=False)[0], out)
    for mask in range(1, 8):
        want = tuple(bool(mask >> i & 1) for i in range(3))
        got = _backward(p, a, el, er, V, pr, g, drop, want=want)
        for i in range(3):
            assert (got[i] is None) if not want[i] else _same_bits(got[i], full[i]), (want, i)
        if want[0] or want[1]:
            assert _same_bits(got[3], full[3]), want
        else:
            assert _is_fill(got[3]), want  # gV alone: the rows' launch is skipped and dWork is not written
    other = _forward(p, a, el, er, V, drop, seed=SEED + 1)
    assert not _same_bits(other[0], out) and _same_bits(other[1], pr)  # another seed: another Out, the same P


def test_two_runs_and_a_captured_graph_give_the_same_bits():
    c = ("long_rows", 64, 8, 0.5)
    name, k, H, drop = c
    a, el, er, V, g = case_operands(name, k, H)
    p = plan(name, k)
    first = _run(c)
    out2, pr2 = _forward(p, a, el, er, V, drop)
    again = (out2, pr2) + _backward(p, a, el, er, V, pr2, g, drop)
    for x, y in zip(first, again):
        assert _same_bits(x, y)
    eld, erd, Vd, gd_ = (_dev(x) for x in (el, er, V, g))
    o, pd, work = _filled((a.m, k)), torch.empty((a.nnz, H), device="cuda"), torch.empty((a.nnz, H), device="cuda")
    gel, ger, gv = _filled((a.m, H)), _filled((a.n, H)), _filled((a.n, k))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=side):  # one stream: the three launches are a chain
        p.gat_attention_dropout(eld, erd, Vd, SLOPE, drop, SEED, out=o, probs=pd)
        p.gat_attention_dropout_backward(eld, erd, Vd, pd, gd_, SLOPE, drop, SEED, grad_el=gel, grad_er=ger, grad_v=gv, work=work)
    for t in (o, pd, gel, ger, gv, work):
        t.fill_(SENTINEL)
    graph_.replay()
    for x, t in zip(first, (o, pd, gel, ger, gv, work)):
        assert _same_bits(x, _host(t))


def test_padded_leading_dimensions_give_the_same_bits_and_leave_the_padding_untouched():
    c = ("thresholds_lifted", 48, 3, 0.5)
    name, k, H, drop = c
    a, el, er, V, g = case_operands(name, k, H)
    ldb, ldc = k + 4, k + 8
    p = plan(name, k, ldb=ldb, ldc=ldc)
    dense = _run(c)
    s = torch.cuda.current_stream().cuda_stream
    Vp, gp = _filled((a.n, ldb)), _filled((a.m, ldc))
    Vp[:, :k], gp[:, :k] = _dev(V), _dev(g)
    eld, erd = _dev(el), _dev(er)
    o, gv = _filled((a.m, ldc)), _filled((a.n, ldb))
    pd, work, gel, ger = _filled((a.nnz, H)), _filled((a.nnz, H)), _filled((a.m, H)), _filled((a.n, H))
    p.gat_attention_dropout_ptr(H, eld.data_ptr(), erd.data_ptr(), Vp.data_ptr(), SLOPE, drop, SEED, o.data_ptr(), pd.data_ptr(), s)
    p.gat_attention_dropout_backward_ptr(H, eld.data_ptr(), erd.data_ptr(), Vp.data_ptr(), pd.data_ptr(), gp.data_ptr(), SLOPE, drop, SEED, gel.data_ptr(),
                                         ger.data_ptr(), gv.data_ptr(), work.data_ptr(), s)
    o, gv = _host(o), _host(gv)
    assert _is_fill(o[:, k:]) and _is_fill(gv[:, k:])
    for key, x, y in zip(KEYS, dense, (o[:, :k], _host(pd), _host(gel), _host(ger), gv[:, :k], _host(work))):
        assert _same_bits(x, y), key


# ---- 6. refusals

def test_refused_calls_leave_the_outputs_untouched():
    name, k = "directed_empty", 32
    a, p = graph(name), plan(name, k)
    s = torch.cuda.current_stream().cuda_stream

    def calls(pl, H, kk, drop=0.5, shift=0, work=1, grad_shift=0, slope=SLOPE):
        """(forward, backward, untouched) through the pointer forms; edge arrays: 0 = P, 1 = Work."""
        hh = max(H, 1)
        eld, erd = torch.zeros((a.m, hh), device="cuda"), torch.zeros((a.n, hh), device="cuda")
        Vd, gd_ = torch.zeros((a.n * kk + 8,), device="cuda"), torch.zeros((a.m, kk), device="cuda")
        outs = [_filled((r * c + 8,)) for r, c in ((a.m, kk), (a.m, hh), (a.n, hh), (a.n, kk))]
        edge = [_filled((a.nnz * hh + 2,)) for _ in range(2)]
        fwd = lambda: pl.gat_attention_dropout_ptr(H, eld.data_ptr(), erd.data_ptr(), Vd.data_ptr() + shift, slope, drop, SEED, outs[0].data_ptr(),
                                                   edge[0].data_ptr(), s)
        bwd = lambda: pl.gat_attention_dropout_backward_ptr(H, eld.data_ptr(), erd.data_ptr(), Vd.data_ptr() + shift, edge[0].data_ptr(), gd_.data_ptr(), slope,
                                                            drop, SEED, outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr() + grad_shift,
                                                            edge[work].data_ptr(), s)
        untouched = lambda: all(_is_fill(_host(t)) for t in outs) and all(_is_fill(_host(t)) for t in edge)
        return fwd, bwd, untouched

    def refused(pl, H, kk, match, **kw):
        fwd, bwd, untouched = calls(pl, H, kk, **kw)
        for f in (fwd, bwd):
            with pytest.raises(binding.FlexError, match=match):
                f()
        assert untouched()

    for bad in (1.0, -0.25, 1.5, float("nan"), float("inf"), -float("inf")):     # p outside [0, 1)
        refused(p, 4, k, "invalid", drop=bad)
    for bad in (0.0, -1.0, 1.5, float("inf"), float("nan")):                     # the slope check beside it, at p > 0 and at p = 0
        refused(p, 4, k, "invalid", slope=bad)
        refused(p, 4, k, "invalid", slope=bad, drop=0.0)
    refused(p, 0, k, "invalid")
    refused(p, 3, k, "not supported")                                             # 3 does not divide 32
    refused(plan(name, 24), 2, 24, "not supported")                               # d = 12
    refused(plan(name, 1024), 2, 1024, "not supported")                           # d = 512
    refused(plan(name, 48), 1, 48, "not supported")                               # one head: d = 48 is no power of two
    refused(plan(name, 48), 1, 48, "not supported", drop=0.0)                     # and p = 0 refuses what p > 0 refuses
    refused(plan(name, k, ldb=34, ldc=36), 4, 36, "not supported")                # an odd stride: ldb % 4 != 0
    refused(p, 4, k, "not supported", shift=4)                                    # V aligned as one float only
    refused(p, 4, k, "not supported", shift=8, drop=0.0)                          # half the vector, at p = 0 as well
    for drop in (0.5, 0.0):
        fwd, bwd, untouched = calls(p, 4, k, grad_shift=8, drop=drop)            # an output of the backward misaligned
        with pytest.raises(binding.FlexError, match="not supported"):
            bwd()
        assert untouched()
    refused(flex_amd.Plan(a, k), 4, k, "invalid")                                 # the wrong kind of plan: no FLEX_PLAN_ATTENTION
    refused(flex_amd.Plan(a, k), 4, k, "invalid", drop=0.0)
    for drop in (0.5, 0.0):
        fwd, bwd, untouched = calls(plan(name, k, attention_backward=False), 4, k, drop=drop)  # the forward's flag alone
        fwd()
        with pytest.raises(binding.FlexError, match="invalid"):
            bwd()
        fwd, bwd, untouched = calls(p, 4, k, work=0, drop=drop)                   # dWork == dP
        with pytest.raises(binding.FlexError, match="invalid"):
            bwd()
        assert untouched()
        shard = flex_amd.Plan(a, k, rows=(10, 90), attention=True, attention_backward=False)
        fwd, bwd, untouched = calls(shard, 4, k, drop=drop)                       # the backward on a row-range shard
        with pytest.raises(binding.FlexError, match="invalid"):
            bwd()
        assert untouched()
        shard.destroy()
    empty = binding.HostCsr(np.zeros(41, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=17)
    pe = flex_amd.Plan(empty, k, attention=True, attention_backward=True)
    pe.gat_attention_dropout_ptr(4, None, None, None, SLOPE, 0.5, SEED, None)  # no entries: no launch, nothing read
    pe.gat_attention_dropout_backward_ptr(4, None, None, None, None, None, SLOPE, 0.5, SEED, None, None, None, None)


# ---- 7. a row-range shard, forward

def test_a_shard_takes_the_mask_at_the_entries_of_the_whole_matrix():
    name, k, H, drop = "long_rows", 32, 4, 0.5
    a = graph(name)
    el, er, V = gat.operands(gat.scenarios_of(H, shift=3), a, k, seed=9)
    whole, whole_p = _forward(plan(name, k), a, el, er, V, drop)
    eld, erd, Vd = _dev(el), _dev(er), _dev(V)
    s = torch.cuda.current_stream().cuda_stream
    cuts = [0, 17, 18, 18, 101, 260, a.m]
    union, union_p = np.full((a.m, k), np.float32(SENTINEL)), np.full((a.nnz, H), np.float32(SENTINEL))
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        shard = flex_amd.Plan(a, k, rows=(r0, r1), attention=True)
        shard.self_check()
        e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
        out, pd = _filled((a.m, k)), _filled((a.nnz, H))
        shard.gat_attention_dropout_ptr(H, eld.data_ptr() + 4 * H * r0, erd.data_ptr(), Vd.data_ptr(), SLOPE, drop, SEED, out.data_ptr() + 4 * k * r0,
                                        pd.data_ptr(), s)
        out, pd = _host(out), _host(pd)
        assert _is_fill(out[:r0]) and _is_fill(out[r1:]), (r0, r1)
        assert _is_fill(pd[:e0]) and _is_fill(pd[e1:]), (r0, r1)
        if r1 > r0:
            gd.check(a, el[r0:r1], er, V, SLOPE, drop, SEED, out[r0:r1], pd[e0:e1], rows=(r0, r1), what=f"rows [{r0}, {r1})")
        union[r0:r1], union_p[e0:e1] = out[r0:r1], pd[e0:e1]
        shard.destroy()
    assert _same_bits(union, whole) and _same_bits(union_p, whole_p)


# ---- 8. autograd

@pytest.mark.parametrize("k,H", [(32, 4), (128, 8)])
def test_the_operator_with_dropout_and_its_gradients_against_float64(k, H):
    """Against float64 torch autograd with the numpy mask as a constant.  Tolerance: gat_attention_ref.propagated_bounds of the
    undropped step (the backward starts from the forward's fp32 alpha) times 2 c: every term of those bounds is linear in |V|, |da| or
    dda of an entry, which dropout multiplies by w <= c, and the one more rounding per count (gamma(n + 1) for gamma(n), n >= 1) at most
    doubles a term.  The operator's outputs are also held to the plan's own calls bit for bit, which test 1 holds to the tight bounds."""
    a = _directed(300, seed=6, dup=True)
    drop, seed = 0.6, SEED ^ 0x55
    rng = np.random.default_rng([k, H, 25])
    el, er = (rng.uniform(-2, 2, (r, H)).astype(np.float32) for r in (a.m, a.n))
    V, gOut = (rng.uniform(-1, 1, (r, k)).astype(np.float32) for r in (a.n, a.m))
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    eld, erd, Vd = (_dev(x).requires_grad_() for x in (el, er, V))
    plain_before = _host(op.gat_attention(eld.detach(), erd.detach(), Vd.detach()))
    out = op.gat_attention(eld, erd, Vd, dropout=drop, seed=seed)
    out.backward(_dev(gOut))
    got = tuple(_host(t) for t in (out.detach(), eld.grad, erd.grad, Vd.grad))
    kp, c = ad.kept_entries(a, H, drop, seed), ad.factor(drop)
    want = gd.torch_float64(a, el, er, V, SLOPE, gOut, kp, c)
    tols = gat.propagated_bounds(a, el, er, V, SLOPE, gOut)
    worst = 0.0
    for what, x, ref, tol in zip(("Out", "grad_el", "grad_er", "grad_V"), got, want, tols):
        tol = 2 * c * tol
        err = np.abs(x.astype(np.float64) - ref)
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), f"{what} k={k} H={H}: worst err / tolerance {float((err / tol).max()):.3g}"
    print(f"k={k} H={H}: worst err / tolerance {worst:.3g}")
    # the plan's own calls give the same bits
    pd = torch.zeros((a.nnz, H), device="cuda")
    o2 = op.plan.gat_attention_dropout(eld.detach(), erd.detach(), Vd.detach(), SLOPE, drop, seed, probs=pd)
    g2 = op.plan.gat_attention_dropout_backward(eld.detach(), erd.detach(), Vd.detach(), pd, _dev(gOut), SLOPE, drop, seed)
    for x, t in zip(got, (o2,) + tuple(g2)):
        assert _same_bits(x, _host(t))
    # dropout=0 and training=False take the path they took before: the same bits
    for kw in (dict(dropout=0.0), dict(dropout=drop, training=False), dict(dropout=0.0, seed=3)):
        assert _same_bits(_host(op.gat_attention(eld.detach(), erd.detach(), Vd.detach(), **kw)), plain_before)
    # seed=None draws from torch's default generator: torch.manual_seed reproduces a run, and the next draw differs
    torch.manual_seed(11)
    x1 = _host(op.gat_attention(eld.detach(), erd.detach(), Vd.detach(), dropout=drop))
    x2 = _host(op.gat_attention(eld.detach(), erd.detach(), Vd.detach(), dropout=drop))
    torch.manual_seed(11)
    assert _same_bits(_host(op.gat_attention(eld.detach(), erd.detach(), Vd.detach(), dropout=drop)), x1) and not _same_bits(x1, x2)

"""The fused GAT attention on bf16 V rows on the GPU (flex_gat_attention_bf16, flex_gat_attention_bf16_backward and the dropout pair):
Out, P, gEl, gEr, gV and dWork against float64 on every element under the bounds of tests/gat_bf16_ref.py over the table of
tests/test_gat_bf16_host.py (every (W, NS) form in all three kernels, DROP off and on); every output against the fp32 kernels on the
widened operands bit for bit; with dropout P and p = 0 against the undropped calls, one mask in all three launches equal to
flex_dropout_mask, non-finite V and g rows behind dropped entries; the output invariants (no P, the subsets of the gradients, run to
run, a captured graph, padded rows); the refusals; a row-range shard; and SparseOperator.gat_attention on bfloat16 leaves with its
gradients against a float64 torch evaluation.  The smallest shapes that reach every form, not a workload."""
import numpy as np
import pytest

import attention_dropout_ref as ad
import flex_amd
import gat_attention_ref as gat
import gat_bf16_ref as gb
import gat_dropout_ref as gd
from attention_bf16_ref import bound_bf16
from backward_ref import _directed
from flex_amd import binding
from softmax_ref import gamma
from test_gat_bf16_host import CASES, SEED, SLOPE, case_id, case_operands, drop_of, graph

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = -12345.5    # fp32 outputs
SENTINEL_BF16 = -12288.0  # bf16 outputs: a bf16 number
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


def _dev16(x):
    """An fp32 array of bf16 numbers as a bfloat16 cuda tensor (exact)."""
    bits = gb.to_bf16(x)
    assert np.array_equal(gb.from_bf16(bits), np.asarray(x, np.float32), equal_nan=True)
    return torch.from_numpy(bits.view(np.int16)).cuda().view(torch.bfloat16)


def _host(t):
    torch.cuda.synchronize()
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.cpu().numpy()


def _filled(shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL_BF16 if dtype == torch.bfloat16 else SENTINEL, device="cuda", dtype=dtype)


def _filled16(shape):
    return _filled(shape, torch.bfloat16)


def _is_fill(x):
    return bool(np.all(x == gb.to_bf16(np.float32(SENTINEL_BF16)))) if x.dtype == np.uint16 else bool(np.all(x == np.float32(SENTINEL)))


def _same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and bool(np.array_equal(x.view(np.uint8), y.view(np.uint8)))


def _forward(p, a, el, er, V, drop, slope=SLOPE, with_p=True):
    """(Out bits, P [nnz, H]) on the host; both start at the sentinel.  drop: None, or (p, seed)."""
    pd = _filled((a.nnz, el.shape[1])) if with_p else None
    out = _filled16((a.m, V.shape[1]))
    if drop is None:
        p.gat_attention_bf16(_dev(el), _dev(er), _dev16(V), slope, out=out, p=pd)
    else:
        p.gat_attention_bf16_dropout(_dev(el), _dev(er), _dev16(V), slope, drop[0], drop[1], out=out, probs=pd)
    return _host(out), (_host(pd) if with_p else None)


def _backward(p, a, el, er, V, pr, g, drop, slope=SLOPE, want=(True, True, True)):
    """(gEl, gEr, gV bits, dx) on the host; an output that is not wanted is None, dx is what dWork holds afterwards."""
    work = _filled((a.nnz, el.shape[1]))
    if drop is None:
        outs = p.gat_attention_bf16_backward(_dev(el), _dev(er), _dev16(V), _dev(pr), _dev16(g), slope, work=work, want=want)
    else:
        outs = p.gat_attention_bf16_dropout_backward(_dev(el), _dev(er), _dev16(V), _dev(pr), _dev16(g), slope, drop[0], drop[1], work=work, want=want)
    return tuple(None if t is None else _host(t) for t in outs) + (_host(work),)


def _run(c):
    """The forward and backward of a case of the table, run once and shared by the tests below; nothing changes it.
    (Out, P, gEl, gEr, gV, dx)."""
    if c not in _runs:
        name, k, H, _ = c
        a, el, er, V, g = case_operands(name, k, H)
        p = plan(name, k)
        out, pr = _forward(p, a, el, er, V, drop_of(c))
        _runs[c] = (out, pr) + _backward(p, a, el, er, V, pr, g, drop_of(c))
    return _runs[c]


def _fp32(p, a, el, er, V, g, drop):
    """(Out, P, gEl, gEr, gV, dx) of the fp32 entry points on the widened operands."""
    H = el.shape[1]
    eld, erd, Vd, gd_ = (_dev(x) for x in (el, er, V, g))
    pd, work = _filled((a.nnz, H)), _filled((a.nnz, H))
    if drop is None:
        o = p.gat_attention(eld, erd, Vd, SLOPE, out=_filled((a.m, V.shape[1])), p=pd)
        grads = p.gat_attention_backward(eld, erd, Vd, pd, gd_, SLOPE, work=work)
    else:
        o = p.gat_attention_dropout(eld, erd, Vd, SLOPE, drop[0], drop[1], out=_filled((a.m, V.shape[1])), probs=pd)
        grads = p.gat_attention_dropout_backward(eld, erd, Vd, pd, gd_, SLOPE, drop[0], drop[1], work=work)
    return (_host(o), _host(pd)) + tuple(_host(t) for t in grads) + (_host(work),)


KEYS = ("out", "p", "gel", "ger", "gv", "dx")


# ---- 1. against float64

@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_every_output_against_float64(c):
    name, k, H, _ = c
    a, el, er, V, g = case_operands(name, k, H)
    out, pr, gel, ger, gv, dx = _run(c)
    each, what = {}, case_id(c)
    gb.check(a, el, er, V, SLOPE, out, pr, drop=drop_of(c), what=what, ratios=each)
    gb.check_backward(a, el, er, V, pr, g, SLOPE, gel, ger, gv, dx, drop=drop_of(c), what=what, ratios=each)
    print(f"{what}: worst err / bound " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))


# ---- 2. against the fp32 kernels on the widened operands

@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_the_fp32_kernels_on_the_widened_operands_give_the_same_bits(c):
    """The walk and the source expressions are the same, so P, dWork, gEl and gEr are the fp32 calls' bits and Out and gV the bf16
    roundings of theirs: what catches a sweep that diverged."""
    name, k, H, _ = c
    a, el, er, V, g = case_operands(name, k, H)
    wide = dict(zip(KEYS, _fp32(plan(name, k), a, el, er, V, g, drop_of(c))))
    got = dict(zip(KEYS, _run(c)))
    for key in ("p", "dx", "gel", "ger"):
        assert _same_bits(got[key], wide[key]), f"{case_id(c)}: {key} differs from the fp32 call's in {int((got[key].view(np.uint32) != wide[key].view(np.uint32)).sum())} elements"
    for key in ("out", "gv"):
        nan = np.isnan(wide[key])
        assert np.array_equal(np.isnan(gb.from_bf16(got[key])), nan), f"{case_id(c)}: {key} is not NaN exactly where the fp32 call's is"
        want = gb.to_bf16(wide[key])
        assert np.array_equal(got[key][~nan], want[~nan]), f"{case_id(c)}: {key} is not the bf16 rounding of the fp32 call's in {int((got[key] != want)[~nan].sum())} elements"


# ---- 3. dropout: P and p = 0 are the undropped call's, one mask in all three launches, dropped entries are selected out

@pytest.mark.parametrize("name,k,H", [("thresholds_lifted", 48, 3), ("long_rows", 64, 8), ("directed_empty", 128, 1), ("thresholds_lifted", 1024, 64)])
def test_p_is_the_undropped_calls_and_p_zero_is_the_undropped_call(name, k, H):
    a, el, er, V, g = case_operands(name, k, H)
    p = plan(name, k)
    plain = _run((name, k, H, None))
    pr = _run((name, k, H, 0.5))[1]
    assert _same_bits(pr, plain[1]), f"P differs from gat_attention_bf16's in {int((pr.view(np.uint32) != plain[1].view(np.uint32)).sum())} entries"
    out0, p0 = _forward(p, a, el, er, V, (0.0, SEED))
    zero = (out0, p0) + _backward(p, a, el, er, V, p0, g, (0.0, SEED))
    for key, x, y in zip(KEYS, zero, plain):
        assert _same_bits(x, y), f"p = 0: {key} differs from the undropped entry point's"


def test_the_three_launches_and_flex_dropout_mask_agree_on_every_bit():
    """tests/test_gpu_gat_dropout.py's construction on bf16 rows: every column has exactly one entry (col(e) = e) and row r has r + 1
    entries, r < d.  el = er = 0, so alpha is 1 / len; V is one-hot and g = 1, both bf16 numbers: Out[r, h d + j] is rn_bf16(alpha w) of
    entry j of the row and head h alone -- not zero iff kept -- gV[e, head h] is rn_bf16(alpha w) in every column of the head, and
    da = w exactly."""
    k, H = 1024, 4
    d = k // H
    lens = np.arange(1, d + 1)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    nnz = int(rp[-1])
    a = binding.HostCsr(rp, np.arange(nnz, dtype=np.uint32), np.ones(nnz, np.float32), n=nnz)
    p = flex_amd.Plan(a, k, attention=True, attention_backward=True)
    row = np.repeat(np.arange(d), lens)
    j = np.arange(nnz) - rp[:-1].astype(np.int64)[row]
    Vd = torch.zeros((nnz, k), device="cuda", dtype=torch.bfloat16)
    e_t, j_t = torch.arange(nnz, device="cuda"), torch.from_numpy(j).cuda()
    for h in range(H):
        Vd[e_t, h * d + j_t] = 1
    eld, erd = torch.zeros((d, H), device="cuda"), torch.zeros((nnz, H), device="cuda")
    gd_ = torch.ones((d, k), device="cuda", dtype=torch.bfloat16)
    pd = torch.empty((nnz, H), device="cuda")
    for drop in (0.5, 0.9):
        out = p.gat_attention_bf16_dropout(eld, erd, Vd, SLOPE, drop, SEED, probs=pd)
        _, _, gv = p.gat_attention_bf16_dropout_backward(eld, erd, Vd, pd, gd_, SLOPE, drop, SEED, want=(False, False, True))
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
        # the row backward: dWork is fp32, and the tolerance is tests/test_gpu_gat_dropout.py's: gamma(n_r + 8) on slope p (|da| + |delta|)
        work = torch.empty((nnz, H), device="cuda")
        p.gat_attention_bf16_dropout_backward(eld, erd, Vd, pd, gd_, SLOPE, drop, SEED, work=work, want=(True, False, False))
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


@pytest.mark.parametrize("name,k,H,drop", [("thresholds_lifted", 32, 4, 0.5), ("directed_empty", 128, 1, 0.6), ("long_rows", 32, 4, 0.9)])
def test_non_finite_rows_behind_dropped_entries_reach_nothing_and_a_fully_dropped_head_is_zero(name, k, H, drop):
    a = graph(name)
    d = k // H
    el, er, V = gb.operands(["uniform4"] * H, a, k, seed=12)
    g = gb.rounded(np.random.default_rng([12, k, 81]).uniform(-1, 1, (a.m, k)).astype(np.float32))
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
        out, pr = _forward(p, a, el, er, Vx, (drop, SEED))
        return (out, pr) + _backward(p, a, el, er, Vx, pr, gx, (drop, SEED))

    clean, dirty = run(V, g), run(Vbad, gbad)
    for key, x, y in zip(KEYS, clean, dirty):
        assert np.isfinite(gb.from_bf16(y) if y.dtype == np.uint16 else y).all(), f"{key} is not finite"
        assert _same_bits(x, y), f"{key} changed with the V and g rows behind dropped entries"
    for h, rows in enumerate(dead_rows):  # a head of a non-empty row whose entries are all dropped is +0 bits in Out
        assert not clean[0][rows, h * d:(h + 1) * d].any()
    gb.check(a, el, er, Vbad, SLOPE, dirty[0], dirty[1], drop=(drop, SEED), what="non-finite V")


# ---- 4. output invariants

@pytest.mark.parametrize("drop", [None, 0.5], ids=["plain", "p0.5"])
def test_without_p_the_same_out_and_every_gradient_has_the_same_bits_whichever_others_are_asked_for(drop):
    c = ("thresholds_lifted", 48, 3, drop)
    name, k, H, _ = c
    a, el, er, V, g = case_operands(name, k, H)
    p = plan(name, k)
    out, pr, *full = _run(c)
    assert _same_bits(_forward(p, a, el, er, V, drop_of(c), with_p=False)[0], out)
    for mask in range(1, 8):
        want = tuple(bool(mask >> i & 1) for i in range(3))
        got = _backward(p, a, el, er, V, pr, g, drop_of(c), want=want)
        for i in range(3):
            assert (got[i] is None) if not want[i] else _same_bits(got[i], full[i]), (want, i)
        if want[0] or want[1]:
            assert _same_bits(got[3], full[3]), want
        else:
            assert _is_fill(got[3]), want  # gV alone: the rows' launch is skipped and dWork is not written
    if drop is not None:
        other = _forward(p, a, el, er, V, (drop, SEED + 1))
        assert not _same_bits(other[0], out) and _same_bits(other[1], pr)  # another seed: another Out, the same P


# ---- 5. run to run, and a captured graph

@pytest.mark.parametrize("drop", [None, 0.5], ids=["plain", "p0.5"])
def test_two_runs_and_a_captured_graph_give_the_same_bits(drop):
    c = ("long_rows", 64, 8, drop)
    name, k, H, _ = c
    a, el, er, V, g = case_operands(name, k, H)
    p = plan(name, k)
    first = _run(c)
    out2, pr2 = _forward(p, a, el, er, V, drop_of(c))
    again = (out2, pr2) + _backward(p, a, el, er, V, pr2, g, drop_of(c))
    for x, y in zip(first, again):
        assert _same_bits(x, y)
    eld, erd, Vd, gd_ = _dev(el), _dev(er), _dev16(V), _dev16(g)
    o, pd, work = _filled16((a.m, k)), torch.empty((a.nnz, H), device="cuda"), torch.empty((a.nnz, H), device="cuda")
    gel, ger, gv = _filled((a.m, H)), _filled((a.n, H)), _filled16((a.n, k))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=side):  # one stream: the three launches are a chain
        if drop is None:
            p.gat_attention_bf16(eld, erd, Vd, SLOPE, out=o, p=pd)
            p.gat_attention_bf16_backward(eld, erd, Vd, pd, gd_, SLOPE, grad_el=gel, grad_er=ger, grad_v=gv, work=work)
        else:
            p.gat_attention_bf16_dropout(eld, erd, Vd, SLOPE, drop, SEED, out=o, probs=pd)
            p.gat_attention_bf16_dropout_backward(eld, erd, Vd, pd, gd_, SLOPE, drop, SEED, grad_el=gel, grad_er=ger, grad_v=gv, work=work)
    for t in (o, pd, gel, ger, gv, work):
        t.fill_(SENTINEL_BF16)
    graph_.replay()
    for x, t in zip(first, (o, pd, gel, ger, gv, work)):
        assert _same_bits(x, _host(t))


# ---- 6. padded rows

@pytest.mark.parametrize("drop", [None, 0.5], ids=["plain", "p0.5"])
def test_padded_leading_dimensions_give_the_same_bits_and_leave_the_padding_untouched(drop):
    c = ("thresholds_lifted", 48, 3, drop)
    name, k, H, _ = c
    a, el, er, V, g = case_operands(name, k, H)
    ldb, ldc = k + 4, k + 8
    p = plan(name, k, ldb=ldb, ldc=ldc)
    dense = _run(c)
    s = torch.cuda.current_stream().cuda_stream
    Vp, gp = _filled16((a.n, ldb)), _filled16((a.m, ldc))
    Vp[:, :k], gp[:, :k] = _dev16(V), _dev16(g)
    eld, erd = _dev(el), _dev(er)
    o, gv = _filled16((a.m, ldc)), _filled16((a.n, ldb))
    pd, work, gel, ger = _filled((a.nnz, H)), _filled((a.nnz, H)), _filled((a.m, H)), _filled((a.n, H))
    if drop is None:
        p.gat_attention_bf16_ptr(H, eld.data_ptr(), erd.data_ptr(), Vp.data_ptr(), SLOPE, o.data_ptr(), pd.data_ptr(), s)
        p.gat_attention_bf16_backward_ptr(H, eld.data_ptr(), erd.data_ptr(), Vp.data_ptr(), pd.data_ptr(), gp.data_ptr(), SLOPE, gel.data_ptr(), ger.data_ptr(),
                                          gv.data_ptr(), work.data_ptr(), s)
    else:
        p.gat_attention_bf16_dropout_ptr(H, eld.data_ptr(), erd.data_ptr(), Vp.data_ptr(), SLOPE, drop, SEED, o.data_ptr(), pd.data_ptr(), s)
        p.gat_attention_bf16_dropout_backward_ptr(H, eld.data_ptr(), erd.data_ptr(), Vp.data_ptr(), pd.data_ptr(), gp.data_ptr(), SLOPE, drop, SEED,
                                                  gel.data_ptr(), ger.data_ptr(), gv.data_ptr(), work.data_ptr(), s)
    o, gv = _host(o), _host(gv)
    assert _is_fill(o[:, k:]) and _is_fill(gv[:, k:])
    for key, x, y in zip(KEYS, dense, (o[:, :k], _host(pd), _host(gel), _host(ger), gv[:, :k], _host(work))):
        assert _same_bits(x, y), key


# ---- 7. refusals

def test_refused_calls_leave_the_outputs_untouched():
    name, k = "directed_empty", 32
    a, p = graph(name), plan(name, k)
    s = torch.cuda.current_stream().cuda_stream

    def calls(pl, H, kk, drop=None, shift=0, work=1, grad_shift=0, slope=SLOPE, null_f=None, null_b=None):
        """(forward, backward, untouched) through the pointer forms; drop None: the undropped pair; edge arrays: 0 = P, 1 = Work;
        shift and grad_shift in bytes.  null_f: the required operand of the forward passed as NULL (0 El, 1 Er, 2 V, 3 Out); null_b:
        that of the backward (0 El, 1 Er, 2 V, 3 P, 4 GradOut, 5 Work)."""
        hh = max(H, 1)
        eld, erd = torch.zeros((a.m, hh), device="cuda"), torch.zeros((a.n, hh), device="cuda")
        Vd, gd_ = torch.zeros((a.n * kk + 16,), device="cuda", dtype=torch.bfloat16), torch.zeros((a.m, kk), device="cuda", dtype=torch.bfloat16)
        outs = [_filled((r * c + 16,), dt) for r, c, dt in ((a.m, kk, torch.bfloat16), (a.m, hh, torch.float32), (a.n, hh, torch.float32), (a.n, kk, torch.bfloat16))]
        edge = [_filled((a.nnz * hh + 2,)) for _ in range(2)]
        extra = () if drop is None else (drop, SEED)
        f, b = (pl.gat_attention_bf16_ptr, pl.gat_attention_bf16_backward_ptr) if drop is None else (pl.gat_attention_bf16_dropout_ptr, pl.gat_attention_bf16_dropout_backward_ptr)
        fa = [None if i == null_f else x for i, x in enumerate((eld.data_ptr(), erd.data_ptr(), Vd.data_ptr() + shift, outs[0].data_ptr()))]
        ba = [None if i == null_b else x for i, x in enumerate((eld.data_ptr(), erd.data_ptr(), Vd.data_ptr() + shift, edge[0].data_ptr(), gd_.data_ptr(),
                                                                edge[work].data_ptr()))]
        fwd = lambda: f(H, *fa[:3], slope, *extra, fa[3], edge[0].data_ptr(), s)
        bwd = lambda: b(H, *ba[:5], slope, *extra, outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr() + grad_shift, ba[5], s)
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
    for drop in (None, 0.5, 0.0):                                                 # the undropped pair, dropout, and p = 0
        for bad in (0.0, -1.0, 1.5, float("inf"), float("nan")):
            refused(p, 4, k, "invalid", slope=bad, drop=drop)
        refused(p, 0, k, "invalid", drop=drop)
        refused(p, 3, k, "not supported", drop=drop)                              # 3 does not divide 32
        refused(plan(name, 24), 2, 24, "not supported", drop=drop)                # d = 12
        refused(plan(name, 1024), 2, 1024, "not supported", drop=drop)            # d = 512
        refused(plan(name, 2048), 8, 2048, "not supported", drop=drop)            # k > 1024 with a legal d = 256
        refused(plan(name, 48), 1, 48, "not supported", drop=drop)                # one head: d = 48 is no power of two
        for missing in range(4):                                                  # a NULL operand of the forward: El, Er, V, Out
            fwd, bwd, untouched = calls(p, 4, k, drop=drop, null_f=missing)
            with pytest.raises(binding.FlexError, match="invalid"):
                fwd()
            assert untouched()
        for missing in range(6):                                                  # and of the backward: El, Er, V, P, GradOut, Work
            fwd, bwd, untouched = calls(p, 4, k, drop=drop, null_b=missing)
            with pytest.raises(binding.FlexError, match="invalid"):
                bwd()
            assert untouched()
        refused(plan(name, k, ldb=34, ldc=36), 4, 36, "not supported", drop=drop) # an odd stride: ldb % 4 != 0
        refused(p, 4, k, "not supported", shift=4, drop=drop)                     # V 4-byte aligned, not 8-byte
        refused(p, 4, k, "not supported", shift=2, drop=drop)                     # V aligned as one bf16 only
        fwd, bwd, untouched = calls(p, 4, k, grad_shift=4, drop=drop)             # an output of the backward misaligned
        with pytest.raises(binding.FlexError, match="not supported"):
            bwd()
        assert untouched()
        refused(flex_amd.Plan(a, k), 4, k, "invalid", drop=drop)                  # the wrong kind of plan: no FLEX_PLAN_ATTENTION
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
    fwd, bwd, untouched = calls(p, 4, k, shift=8, grad_shift=8)                   # 8-byte aligned rows are served: nothing is refused
    fwd(), bwd()                                                                  # (and compute the aligned run's bits: the test below)
    empty = binding.HostCsr(np.zeros(41, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=17)
    pe = flex_amd.Plan(empty, k, attention=True, attention_backward=True)
    pe.gat_attention_bf16_ptr(4, None, None, None, SLOPE, None)  # no entries: no launch, nothing read
    pe.gat_attention_bf16_backward_ptr(4, None, None, None, None, None, SLOPE, None, None, None, None)
    pe.gat_attention_bf16_dropout_ptr(4, None, None, None, SLOPE, 0.5, SEED, None)
    pe.gat_attention_bf16_dropout_backward_ptr(4, None, None, None, None, None, SLOPE, 0.5, SEED, None, None, None, None)


@pytest.mark.parametrize("drop", [None, 0.5], ids=["plain", "p0.5"])
def test_rows_8_bytes_off_a_16_byte_mark_give_the_bits_of_the_aligned_run(drop):
    """The shift=8, grad_shift=8 call of the refusals on real operands: V and gV four elements into their buffers, then every row operand
    (V, g, Out, gV).  Every output has the aligned run's bits, and the elements before and after the moved rows keep their fill."""
    c = ("directed_empty", 32, 4, drop)
    name, k, H, _ = c
    a, el, er, V, g = case_operands(name, k, H)
    p = plan(name, k)
    aligned = dict(zip(KEYS, _run(c)))
    s = torch.cuda.current_stream().cuda_stream
    eld, erd = _dev(el), _dev(er)
    rows = {"V": a.n, "g": a.m, "out": a.m, "gv": a.n}
    for moved in (("V", "gv"), ("V", "g", "out", "gv")):
        t = {key: _filled16((r * k + 8,)) for key, r in rows.items()}
        at = {key: 4 if key in moved else 0 for key in t}
        for key, x in (("V", V), ("g", g)):
            t[key][at[key]:at[key] + rows[key] * k] = _dev16(x).view(-1)
        ptr = {key: t[key].data_ptr() + 2 * at[key] for key in t}
        assert all((ptr[key] % 16 == 8) == (key in moved) for key in t)
        pd, work, gel, ger = _filled((a.nnz, H)), _filled((a.nnz, H)), _filled((a.m, H)), _filled((a.n, H))
        if drop is None:
            p.gat_attention_bf16_ptr(H, eld.data_ptr(), erd.data_ptr(), ptr["V"], SLOPE, ptr["out"], pd.data_ptr(), s)
            p.gat_attention_bf16_backward_ptr(H, eld.data_ptr(), erd.data_ptr(), ptr["V"], pd.data_ptr(), ptr["g"], SLOPE, gel.data_ptr(), ger.data_ptr(),
                                              ptr["gv"], work.data_ptr(), s)
        else:
            p.gat_attention_bf16_dropout_ptr(H, eld.data_ptr(), erd.data_ptr(), ptr["V"], SLOPE, drop, SEED, ptr["out"], pd.data_ptr(), s)
            p.gat_attention_bf16_dropout_backward_ptr(H, eld.data_ptr(), erd.data_ptr(), ptr["V"], pd.data_ptr(), ptr["g"], SLOPE, drop, SEED,
                                                      gel.data_ptr(), ger.data_ptr(), ptr["gv"], work.data_ptr(), s)
        for key in ("out", "gv"):
            x, lo, hi = _host(t[key]), at[key], at[key] + rows[key] * k
            assert _is_fill(x[:lo]) and _is_fill(x[hi:]), (moved, key)
            assert _same_bits(x[lo:hi].reshape(rows[key], k), aligned[key]), (moved, key)
        for key, x in (("p", pd), ("gel", gel), ("ger", ger), ("dx", work)):
            assert _same_bits(_host(x), aligned[key]), (moved, key)


# ---- 8. a row-range shard, forward

@pytest.mark.parametrize("drop", [None, 0.5], ids=["plain", "p0.5"])
def test_a_shards_forward_with_the_mask_at_the_entries_of_the_whole_matrix(drop):
    name, k, H = "long_rows", 32, 4
    a = graph(name)
    el, er, V = gb.operands(gat.scenarios_of(H, shift=3), a, k, seed=9)
    dr = None if drop is None else (drop, SEED)
    whole, whole_p = _forward(plan(name, k), a, el, er, V, dr)
    eld, erd, Vd = _dev(el), _dev(er), _dev16(V)
    s = torch.cuda.current_stream().cuda_stream
    cuts = [0, 17, 18, 18, 101, 260, a.m]
    union, union_p = np.zeros((a.m, k), np.uint16), np.full((a.nnz, H), np.float32(SENTINEL))
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        shard = flex_amd.Plan(a, k, rows=(r0, r1), attention=True)
        shard.self_check()
        e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
        out, pd = _filled16((a.m, k)), _filled((a.nnz, H))
        if drop is None:
            shard.gat_attention_bf16_ptr(H, eld.data_ptr() + 4 * H * r0, erd.data_ptr(), Vd.data_ptr(), SLOPE, out.data_ptr() + 2 * k * r0, pd.data_ptr(), s)
        else:
            shard.gat_attention_bf16_dropout_ptr(H, eld.data_ptr() + 4 * H * r0, erd.data_ptr(), Vd.data_ptr(), SLOPE, drop, SEED, out.data_ptr() + 2 * k * r0,
                                                 pd.data_ptr(), s)
        out, pd = _host(out), _host(pd)
        assert _is_fill(out[:r0]) and _is_fill(out[r1:]), (r0, r1)
        assert _is_fill(pd[:e0]) and _is_fill(pd[e1:]), (r0, r1)
        if r1 > r0:
            gb.check(a, el[r0:r1], er, V, SLOPE, out[r0:r1], pd[e0:e1], rows=(r0, r1), drop=dr, what=f"rows [{r0}, {r1})")
        union[r0:r1], union_p[e0:e1] = out[r0:r1], pd[e0:e1]
        shard.destroy()
    assert _same_bits(union, whole) and _same_bits(union_p, whole_p)


# ---- 9. autograd

@pytest.mark.parametrize("k,H,drop,narrow", [(32, 4, None, False), (32, 4, 0.6, False), (128, 8, None, False), (128, 8, 0.6, False), (32, 4, 0.6, True)],
                         ids=["k32-h4-plain", "k32-h4-p0.6", "k128-h8-plain", "k128-h8-p0.6", "k32-h4-p0.6-bf16-el-er"])
def test_the_operator_on_bfloat16_leaves_and_its_gradients_against_float64(k, H, drop, narrow):
    """Against float64 torch autograd on the numbers the kernel reads (bf16 V and g; el and er float32, or bf16 numbers when the leaves
    are bfloat16), the numpy mask a constant.  Tolerance: gat_attention_ref.propagated_bounds (the backward starts from the forward's
    fp32 alpha), times 2 c with dropout as in tests/test_gpu_gat_dropout.py, as bound32 of the bf16 bound for every output that is
    rounded to bf16: Out and grad V always, grad el and grad er where the leaves are bfloat16 (torch rounds the float32 gradient once
    more on its way back through .float()).  The operator's outputs are also held to the plan's own calls bit for bit."""
    a = _directed(300, seed=6, dup=True)
    seed = SEED ^ 0x55
    rng = np.random.default_rng([k, H, 25])
    el, er = (rng.uniform(-2, 2, (r, H)).astype(np.float32) for r in (a.m, a.n))
    if narrow:
        el, er = gb.rounded(el), gb.rounded(er)
    V, gOut = (gb.rounded(rng.uniform(-1, 1, (r, k)).astype(np.float32)) for r in (a.n, a.m))
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    eld, erd = ((_dev16(x) if narrow else _dev(x)).requires_grad_() for x in (el, er))
    Vd = _dev16(V).requires_grad_()
    kw = dict() if drop is None else dict(dropout=drop, seed=seed)
    out = op.gat_attention(eld, erd, Vd, **kw)
    assert out.dtype == torch.bfloat16
    out.backward(_dev16(gOut))
    assert Vd.grad.dtype == torch.bfloat16 and eld.grad.dtype == erd.grad.dtype == (torch.bfloat16 if narrow else torch.float32)
    got = tuple(_host(t) for t in (out.detach(), eld.grad, erd.grad, Vd.grad))
    kp = np.ones((a.nnz, H), bool) if drop is None else ad.kept_entries(a, H, drop, seed)
    c = 1.0 if drop is None else ad.factor(drop)
    want = gd.torch_float64(a, el, er, V, SLOPE, gOut, kp, c)
    tols = gat.propagated_bounds(a, el, er, V, SLOPE, gOut)
    worst = 0.0
    for what, x, ref, tol in zip(("Out", "grad_el", "grad_er", "grad_V"), got, want, tols):
        tol = tol if drop is None else 2 * c * tol
        if x.dtype == np.uint16:
            x, tol = gb.from_bf16(x), bound_bf16(ref, tol)
        err = np.abs(x.astype(np.float64) - ref)
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), f"{what} k={k} H={H}: worst err / tolerance {float((err / tol).max()):.3g}"
    print(f"k={k} H={H} drop={drop} bf16 el/er={narrow}: worst err / tolerance {worst:.3g}")
    # the plan's own calls give the same bits (on float32 el and er: what the Function sees)
    e32, r32, pd = _dev(el), _dev(er), torch.zeros((a.nnz, H), device="cuda")
    if drop is None:
        o2 = op.plan.gat_attention_bf16(e32, r32, Vd.detach(), SLOPE, p=pd)
        g2 = op.plan.gat_attention_bf16_backward(e32, r32, Vd.detach(), pd, _dev16(gOut), SLOPE)
    else:
        o2 = op.plan.gat_attention_bf16_dropout(e32, r32, Vd.detach(), SLOPE, drop, seed, probs=pd)
        g2 = op.plan.gat_attention_bf16_dropout_backward(e32, r32, Vd.detach(), pd, _dev16(gOut), SLOPE, drop, seed)
    assert _same_bits(got[0], _host(o2)) and _same_bits(got[3], _host(g2[2]))
    for x, t in zip(got[1:3], g2[:2]):
        assert _same_bits(x, _host(t.bfloat16() if narrow else t))
    if drop is not None:  # training=False takes the undropped bf16 path: the same bits
        assert _same_bits(_host(op.gat_attention(eld.detach(), erd.detach(), Vd.detach(), dropout=drop, training=False)),
                          _host(op.gat_attention(eld.detach(), erd.detach(), Vd.detach())))
    # float32 calls take the path they took: float32 out from the fp32 kernels
    o32 = op.gat_attention(e32, r32, Vd.detach().float())
    assert o32.dtype == torch.float32 and _same_bits(_host(o32), _host(op.plan.gat_attention(e32, r32, Vd.detach().float(), SLOPE)))

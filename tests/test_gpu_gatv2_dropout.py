"""The attention dropout of the fused GATv2 attention on the GPU (flex_dropout_gatv2_attention, flex_dropout_gatv2_attention_backward):
Out, P, gXt, gXs, gAtt and dWork against float64 on every element under the bounds of tests/gatv2_dropout_ref.py over the table of
tests/test_gatv2_dropout_host.py (every (W, NS) form in all three kernels, a scenario per head); P and p = 0 against the undropped
calls bit for bit; one mask in all launches, equal to flex_dropout_mask; selection (non-finite g behind fully dropped heads, -inf
source rows behind dropped entries); the output invariants; the refusal table of tests/gatv2_dropout_entry_table.py on the real
library; row-range shards; and SparseOperator.gatv2_attention(..., dropout=p) with its gradients against a float64 torch evaluation."""
import numpy as np
import pytest

import attention_dropout_ref as ad
import flex_amd
import gatv2_attention_ref as v2
import gatv2_dropout_entry_table as table
import gatv2_dropout_ref as vd
from backward_ref import _directed
from flex_amd import binding
from test_gatv2_dropout_host import (CASES, SEED, SLOPE, case_id, case_operands, dead_row_heads, grad, graph, masked_source_case,
                                     masked_source_rows, one_mask_case)

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


def _forward(p, a, xt, xs, att, drop, seed=SEED, with_p=True, shared=False):
    """(Out, P [nnz, H]) on the host; both start at the sentinel.  shared: Xt and Xs are one buffer."""
    pd = _filled((a.nnz, att.shape[0])) if with_p else None
    xsd = _dev(xs)
    out = p.gatv2_attention_dropout(xsd if shared else _dev(xt), xsd, _dev(att), SLOPE, drop, seed, out=_filled((a.m, xs.shape[1])), probs=pd)
    return _host(out), (_host(pd) if with_p else None)


def _backward(p, a, xt, xs, att, pr, g, drop, seed=SEED, want=(True, True, True), shared=False):
    """(gXt, gXs, gAtt, dz) on the host; an output that is not wanted is None, dz is what dWork holds afterwards."""
    work = _filled((a.nnz, att.shape[0]))
    xsd = _dev(xs)
    outs = p.gatv2_attention_dropout_backward(xsd if shared else _dev(xt), xsd, _dev(att), _dev(pr), _dev(g), SLOPE, drop, seed, work=work, want=want)
    return tuple(None if t is None else _host(t) for t in outs) + (_host(work),)


def _both(p, a, xt, xs, att, g, drop, **kw):
    out, pr = _forward(p, a, xt, xs, att, drop, **kw)
    return (out, pr) + _backward(p, a, xt, xs, att, pr, g, drop, **kw)


def _run(c):
    """The forward and backward of a case of the table, run once and shared by the tests below; nothing changes it.
    (Out, P, gXt, gXs, gAtt, dz)."""
    if c not in _runs:
        name, k, H, drop = c
        a, xt, xs, att, g = case_operands(name, k, H)
        _runs[c] = _both(plan(name, k), a, xt, xs, att, g, drop)
    return _runs[c]


KEYS = ("out", "p", "gxt", "gxs", "gatt", "dz")


# ---- 1. against float64

@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_every_output_against_float64(c):
    name, k, H, drop = c
    a, xt, xs, att, g = case_operands(name, k, H)
    out, pr, gxt, gxs, gatt, dz = _run(c)
    each, what = {}, case_id(c)
    vd.check(a, xt, xs, att, SLOPE, drop, SEED, out, pr, what=what, ratios=each)
    vd.check_backward(a, xt, xs, att, pr, g, SLOPE, drop, SEED, gxt, gxs, gatt, dz, what=what, ratios=each)
    print(f"{what}: worst err / bound " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))


# ---- 2. P is the undropped call's, and p = 0 is the undropped call

def _undropped(p, a, xt, xs, att, g):
    """(Out, P, gXt, gXs, gAtt, dz) of the undropped entry points on the same operands."""
    H = att.shape[0]
    xtd, xsd, attd, gd_ = (_dev(x) for x in (xt, xs, att, g))
    pd, work = _filled((a.nnz, H)), _filled((a.nnz, H))
    o = p.gatv2_attention(xtd, xsd, attd, SLOPE, out=_filled((a.m, xs.shape[1])), p=pd)
    grads = p.gatv2_attention_backward(xtd, xsd, attd, pd, gd_, SLOPE, work=work)
    return (_host(o), _host(pd)) + tuple(_host(t) for t in grads) + (_host(work),)


@pytest.mark.parametrize("name,k,H", [("thresholds_lifted", 48, 3), ("long_rows", 64, 8), ("directed_empty", 128, 1), ("thresholds_lifted", 1024, 64)])
def test_p_is_the_undropped_calls_and_p_zero_is_the_undropped_call(name, k, H):
    a, xt, xs, att, g = case_operands(name, k, H)
    p = plan(name, k)
    plain = _undropped(p, a, xt, xs, att, g)
    pr = _run((name, k, H, 0.5))[1]
    assert _same_bits(pr, plain[1]), f"P differs from gatv2_attention's in {int((pr.view(np.uint32) != plain[1].view(np.uint32)).sum())} entries"
    for key, x, y in zip(KEYS, _both(p, a, xt, xs, att, g, 0.0), plain):
        assert _same_bits(x, y), f"p = 0: {key} differs from the undropped entry point's"


# ---- 3. one mask in all launches, and it is flex_dropout_mask

def test_the_launches_and_flex_dropout_mask_agree_on_every_bit():
    """Every column has exactly one entry (col(e) = e) and row r has r + 1 entries, r < d = 256: slot rows and wave rows, four slabs.
    att = 0, so every score is 0, alpha is 1 / len and the score term of gXs is exactly 0.  Xs is one-hot: column e holds 1 at column
    e mod d of every head (the entries of a row are consecutive, so they differ there), so Out[r, h d + e mod d] is alpha w of that
    entry and head alone; g = 1, so gXs[e, head h] is alpha w in every column of the head and da = w exactly."""
    k, H = 1024, 4
    d = k // H
    a, lens, row, _ = one_mask_case()
    nnz = a.nnz
    p = flex_amd.Plan(a, k, attention=True, attention_backward=True)
    e_t = torch.arange(nnz, device="cuda")
    xsd = torch.zeros((nnz, k), device="cuda")
    for h in range(H):
        xsd[e_t, h * d + e_t % d] = 1
    xtd, attd, gd_ = torch.zeros((d, k), device="cuda"), torch.zeros((H, d), device="cuda"), torch.ones((d, k), device="cuda")
    pd = torch.empty((nnz, H), device="cuda")
    em = np.arange(nnz) % d
    for drop in (0.5, 0.9):
        out = p.gatv2_attention_dropout(xtd, xsd, attd, SLOPE, drop, SEED, probs=pd)
        work = torch.empty((nnz, H), device="cuda")
        _, gxs, _ = p.gatv2_attention_dropout_backward(xtd, xsd, attd, pd, gd_, SLOPE, drop, SEED, work=work, want=(False, True, False))
        torch.cuda.synchronize()
        want = binding.dropout_mask(SEED, drop, 0, nnz * H).astype(bool).reshape(nnz, H)
        assert want.size == 131584 and np.array_equal(want, ad.keep(SEED, drop, np.arange(nnz * H, dtype=np.uint64)).reshape(nnz, H))
        out_nz = (out != 0).cpu().numpy().reshape(d, H, d)
        gxs_nz = (gxs != 0).view(nnz, H, d)
        assert bool((gxs_nz.all(2) == gxs_nz.any(2)).all()), "gXs: a head of an entry is zero in all of its columns or in none"
        fwd_keep = out_nz[row, :, em]
        assert int(out_nz.sum()) == int(fwd_keep.sum()), "Out is non-zero in a column no entry of the row stands at"
        assert np.array_equal(fwd_keep, want), f"p={drop}: the forward's mask differs from flex_dropout_mask in {int((fwd_keep != want).sum())} bits"
        gxs_keep = gxs_nz.any(2).cpu().numpy()
        assert np.array_equal(gxs_keep, want), f"p={drop}: the column launch's mask differs from flex_dropout_mask in {int((gxs_keep != want).sum())} bits"
        # the row launch: dWork is the dz of that mask under the reference's lines, da = w exactly (c x 1), dda the reference's for <g, Xs> = 1
        c = ad.factor(drop)
        n_r = lens[row]
        pr = _host(pd).astype(np.float64)
        dz = _host(work)
        for h in range(H):
            da = want[:, h] * c
            dda = np.where(want[:, h], c * (vd.gamma(d + 1) * 1.0 + d * vd.SUB) + vd.SUB, 0.0)
            ref, bound = vd.dz_lines(pr[:, h], da, dda, row, a.m, n_r)
            ratio = np.abs(dz[:, h].astype(np.float64) - ref) / bound
            assert ratio.max() <= 1.0, f"p={drop} head {h}: dWork is not the dz of that mask (worst err / bound {float(ratio.max()):.3g})"
            assert np.any(ref != 0)
    p.destroy()


# ---- 4. selection

@pytest.mark.parametrize("name,k,H,drop", [("thresholds_lifted", 32, 4, 0.5), ("directed_empty", 128, 1, 0.5), ("long_rows", 64, 8, 0.9),
                                           ("thresholds", 8, 2, 0.9)])
def test_non_finite_g_in_a_fully_dropped_head_reaches_nothing_and_the_head_is_zero(name, k, H, drop):
    """(a): inf or NaN in g[r, head h] of every head of a non-empty row whose entries are all dropped: da is selected to +0, not
    multiplied, and the column launch does not gather that g row: no bit of any output changes."""
    a, p, d = graph(name), plan(name, k), k // H
    xt, xs, att = v2.operands(["uniform4"] * H, a, k, seed=12)
    g = grad(a, k, 12)
    dead = dead_row_heads(a, H, drop)
    assert sum(len(r) for r in dead) >= 11
    gbad = g.copy()
    for h, rows in enumerate(dead):
        gbad[rows[0::2], h * d:(h + 1) * d] = np.inf
        gbad[rows[1::2], h * d:(h + 1) * d] = np.nan
    clean, dirty = _both(p, a, xt, xs, att, g, drop), _both(p, a, xt, xs, att, gbad, drop)
    for key, x, y in zip(KEYS, clean, dirty):
        assert np.isfinite(y).all(), f"{key} is not finite"
        assert _same_bits(x, y), f"{key} changed with g in heads whose entries are all dropped"
    for h, rows in enumerate(dead):  # such a head is +0 bits in Out
        assert not np.ascontiguousarray(clean[0][rows, h * d:(h + 1) * d]).view(np.uint8).any()


@pytest.mark.parametrize("name", ["directed_empty", "thresholds_lifted", "long_rows"])
def test_a_dropped_entry_with_a_minus_inf_source_row_adds_nothing_and_a_kept_one_adds_nan(name):
    """(b), forward only: s = -inf and alpha = +0 for head 1 of an entry from a marked column; a kept one adds 0 x -inf = NaN to
    Out, as the undropped call does, a dropped one nothing: the NaN set of Out is exactly the reference's."""
    k, H, drop = 32, 4, 0.5
    a, xt, xs, att = masked_source_case(name, k, H)
    with_kept, only_dropped = masked_source_rows(a, xs, k, H, drop)
    assert len(with_kept) >= 51 and len(only_dropped) >= 48
    out, pr = _forward(plan(name, k), a, xt, xs, att, drop)
    ref = vd.reference(a, xt, xs, att, SLOPE, drop, SEED)
    assert np.array_equal(np.isnan(out), np.isnan(ref["out"])), "the NaN set of Out is not the reference's"
    assert np.array_equal(np.flatnonzero(np.isnan(out).any(1)), with_kept) and np.isfinite(out[only_dropped]).all()
    vd.check(a, xt, xs, att, SLOPE, drop, SEED, out, pr, what=name)
    plain = _host(plan(name, k).gatv2_attention(_dev(xt), _dev(xs), _dev(att), SLOPE))
    assert np.isnan(plain[np.concatenate([with_kept, only_dropped])]).any(1).all()  # the undropped call is NaN on all of them


# ---- 5. output invariants

def test_without_p_the_same_out_and_every_gradient_has_the_same_bits_whichever_others_are_asked_for():
    c = ("thresholds_lifted", 48, 3, 0.5)
    name, k, H, drop = c
    a, xt, xs, att, g = case_operands(name, k, H)
    p = plan(name, k)
    out, pr, *full = _run(c)
    assert _same_bits(_forward(p, a, xt, xs, att, drop, with_p=False)[0], out)
    devs = [_dev(x) for x in (xt, xs, att, pr, g)]
    need = p.gatv2_attention_work_size()
    for mask in range(8):
        want = tuple(bool(mask >> i & 1) for i in range(3))
        sent = [_filled(shape) for shape in ((a.m, k), (a.n, k), (H, k // H))]
        work, att_work = _filled((a.nnz, H)), _filled((need,))
        p.gatv2_attention_dropout_backward_ptr(H, *(t.data_ptr() for t in devs), SLOPE, drop, SEED, *(t.data_ptr() if w else None for t, w in zip(sent, want)),
                                               work.data_ptr(), att_work.data_ptr(), torch.cuda.current_stream().cuda_stream)
        for i in range(3):
            got = _host(sent[i])
            assert _same_bits(got, full[i]) if want[i] else _is_fill(got), (want, i)
        assert _same_bits(_host(work), full[3]) if any(want) else _is_fill(_host(work)), want  # every gradient needs dz
        assert bool((_host(att_work) != SENTINEL).all()) if want[2] else _is_fill(_host(att_work)), want
    other = _forward(p, a, xt, xs, att, drop, seed=SEED + 1)
    assert not _same_bits(other[0], out) and _same_bits(other[1], pr)  # another seed: another Out, the same P


def test_two_runs_and_a_captured_graph_give_the_same_bits():
    c = ("long_rows", 64, 8, 0.5)
    name, k, H, drop = c
    a, xt, xs, att, g = case_operands(name, k, H)
    p = plan(name, k)
    first = _run(c)
    for x, y in zip(first, _both(p, a, xt, xs, att, g, drop)):
        assert _same_bits(x, y)
    xtd, xsd, attd, gd_ = (_dev(x) for x in (xt, xs, att, g))
    o, pd, work = _filled((a.m, k)), torch.empty((a.nnz, H), device="cuda"), torch.empty((a.nnz, H), device="cuda")
    gxt, gxs, gatt = _filled((a.m, k)), _filled((a.n, k)), _filled((H, k // H))
    att_work = torch.empty(p.gatv2_attention_work_size(), device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=side):  # one stream: the four launches are a chain
        p.gatv2_attention_dropout(xtd, xsd, attd, SLOPE, drop, SEED, out=o, probs=pd)
        p.gatv2_attention_dropout_backward(xtd, xsd, attd, pd, gd_, SLOPE, drop, SEED, grad_xt=gxt, grad_xs=gxs, grad_att=gatt, work=work, att_work=att_work)
    for t in (o, pd, gxt, gxs, gatt, work):
        t.fill_(SENTINEL)
    graph_.replay()
    for x, t in zip(first, (o, pd, gxt, gxs, gatt, work)):
        assert _same_bits(x, _host(t))


@pytest.mark.parametrize("k,H", [(32, 4), (512, 2)])
def test_one_buffer_for_xt_and_xs_gives_the_bits_of_two_copies(k, H):
    name, drop = "thresholds_lifted", 0.5  # square
    a, p = graph(name), plan(name, k)
    _, xs, att = v2.operands(v2.scenarios_of(H, shift=3), a, k, seed=12)
    g = grad(a, k, 12)
    two = _both(p, a, xs.copy(), xs, att, g, drop)
    one = _both(p, a, None, xs, att, g, drop, shared=True)
    for key, x, y in zip(KEYS, two, one):
        assert _same_bits(x, y), key


def test_padded_leading_dimensions_give_the_same_bits_and_leave_the_padding_untouched():
    name, k, H, drop, ldb, ldc = "directed_empty", 32, 4, 0.5, 40, 36
    a, xt, xs, att, g = case_operands(name, k, H)
    p = plan(name, k, ldb=ldb, ldc=ldc)
    dense = _run((name, k, H, drop))
    xtp, xsp, gp = (_filled((r, ld)) for r, ld in ((a.m, ldc), (a.n, ldb), (a.m, ldc)))
    xtp[:, :k], xsp[:, :k], gp[:, :k] = _dev(xt), _dev(xs), _dev(g)
    pad = 8  # floats of sentinel after every array
    need = p.gatv2_attention_work_size()
    arrays = {key: _filled((n + pad,)) for key, n in
              (("out", a.m * ldc), ("p", a.nnz * H), ("gxt", a.m * ldc), ("gxs", a.n * ldb), ("gatt", k), ("dz", a.nnz * H), ("att_work", need))}
    attd = _dev(att)
    s = torch.cuda.current_stream().cuda_stream
    p.gatv2_attention_dropout_ptr(H, xtp.data_ptr(), xsp.data_ptr(), attd.data_ptr(), SLOPE, drop, SEED, arrays["out"].data_ptr(), arrays["p"].data_ptr(), s)
    p.gatv2_attention_dropout_backward_ptr(H, xtp.data_ptr(), xsp.data_ptr(), attd.data_ptr(), arrays["p"].data_ptr(), gp.data_ptr(), SLOPE, drop, SEED,
                                           arrays["gxt"].data_ptr(), arrays["gxs"].data_ptr(), arrays["gatt"].data_ptr(), arrays["dz"].data_ptr(),
                                           arrays["att_work"].data_ptr(), s)
    got = {key: _host(t) for key, t in arrays.items()}
    for key in got:
        assert _is_fill(got[key][-pad:]), f"{key}: written past its end"
    shapes = {"out": (a.m, ldc), "p": (a.nnz, H), "gxt": (a.m, ldc), "gxs": (a.n, ldb), "gatt": (H, k // H), "dz": (a.nnz, H)}
    for key, want in zip(KEYS, dense):
        x = got[key][:-pad].reshape(shapes[key])
        if key in ("out", "gxt", "gxs"):
            assert _is_fill(x[:, k:]), f"{key}: a padded tail was written"
            x = x[:, :k]
        assert _same_bits(x, want), key


# ---- 6. refusals

@pytest.mark.parametrize("drop", [table.DROP, 0.0], ids=["p0.5", "p0"])
def test_the_real_library_answers_the_refusal_table_and_a_refused_row_writes_nothing(drop):
    """Every row of tests/gatv2_dropout_entry_table.py on real plans and real tensors, at p = 0.5 and at p = 0.  A row that expects no
    launch must leave every writable operand as it was; the valid row must write its outputs; the other launching rows run kernels that
    the tests above run on checked operands and are not launched again here."""
    a = v2.both_sides(v2.threshold_graph())
    plans = table.plans(a)
    stream = torch.cuda.current_stream().cuda_stream
    K, H = table.K, table.H
    need = plans["valid"].gatv2_attention_work_size()
    sizes = {"Xt": a.m * K, "Xs": a.n * K, "Att": K, "Out": a.m * K, "P": a.nnz * H, "G": a.m * K, "GXt": a.m * K, "GXs": a.n * K, "GAtt": K,
             "Work": a.nnz * H, "AttWork": need}
    for name in table.ENTRIES:
        fn = binding._values_fn(name)
        written = table.WRITTEN[name]
        t = {x: torch.full((n + 4,), SENTINEL if x in written else 0.25, device="cuda") for x, n in sizes.items()}  # four floats of slack
        ops = {x: t[x].data_ptr() for x in t}
        for row, change, code, launches in table.rows_of(name, drop):
            if launches and row != "valid":
                assert code == table.OK, (name, row)
                continue
            handle, args = table.arguments(name, change, plans, ops, drop)
            assert fn(handle, *args, stream) == code, (name, row)
            torch.cuda.synchronize()
            if not launches:
                assert all(bool((t[x] == SENTINEL).all()) for x in written), f"{name}, row {row}: it wrote something"
            else:
                assert all(bool((t[x][:sizes[x]] != SENTINEL).all()) for x in written), f"{name}, row {row}: an output was not written"
                for x in written:
                    t[x].fill_(SENTINEL)
    for pl in plans.values():
        pl.destroy()


# ---- 7. row-range shards

def test_the_shards_take_the_mask_at_the_entries_of_the_whole_matrix_and_have_no_backward():
    name, k, H, drop = "long_rows", 32, 4, 0.5
    a = graph(name)
    xt, xs, att = v2.operands(v2.scenarios_of(H, shift=3), a, k, seed=9)
    whole, whole_p = _forward(plan(name, k), a, xt, xs, att, drop)
    xtd, xsd, attd = _dev(xt), _dev(xs), _dev(att)
    s = torch.cuda.current_stream().cuda_stream
    cuts = [0, 17, 18, 18, 101, 260, a.m]
    union, union_p = np.full((a.m, k), np.float32(SENTINEL)), np.full((a.nnz, H), np.float32(SENTINEL))
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        shard = flex_amd.Plan(a, k, rows=(r0, r1), attention=True)
        shard.self_check()
        e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
        out, pd = _filled((a.m, k)), _filled((a.nnz, H))
        shard.gatv2_attention_dropout_ptr(H, xtd.data_ptr() + 4 * k * r0, xsd.data_ptr(), attd.data_ptr(), SLOPE, drop, SEED, out.data_ptr() + 4 * k * r0,
                                          pd.data_ptr(), s)
        out, pd = _host(out), _host(pd)
        assert _is_fill(out[:r0]) and _is_fill(out[r1:]), (r0, r1)
        assert _is_fill(pd[:e0]) and _is_fill(pd[e1:]), (r0, r1)
        if r1 > r0:
            vd.check(a, xt[r0:r1], xs, att, SLOPE, drop, SEED, out[r0:r1], pd[e0:e1], rows=(r0, r1), what=f"rows [{r0}, {r1})")
        union[r0:r1], union_p[e0:e1] = out[r0:r1], pd[e0:e1]
        shard.destroy()
    assert _same_bits(union, whole) and _same_bits(union_p, whole_p)
    shard = flex_amd.Plan(a, k, rows=(17, 101), attention=True)  # a shard cannot carry FLEX_PLAN_ATTENTION_BACKWARD: the backward refuses it
    outs = [_filled(shape) for shape in ((a.m, k), (a.n, k), (H, k // H), (a.nnz, H), (4096,))]
    gd_, pd = _dev(grad(a, k, 9)), _dev(whole_p)
    for p_ in (drop, 0.0):
        with pytest.raises(binding.FlexError, match="invalid"):
            shard.gatv2_attention_dropout_backward_ptr(H, xtd.data_ptr(), xsd.data_ptr(), attd.data_ptr(), pd.data_ptr(), gd_.data_ptr(), SLOPE, p_, SEED,
                                                       *(t.data_ptr() for t in outs), s)
    assert all(_is_fill(_host(t)) for t in outs)
    shard.destroy()


# ---- 8. the operator

@pytest.mark.parametrize("k,H", [(32, 4), (128, 8)])
def test_the_operator_with_dropout_and_its_gradients_against_float64(k, H):
    """Against float64 torch autograd with the numpy mask as a constant, within gatv2_dropout_ref.propagated_bounds (the backward
    starts from the forward's fp32 alpha, so alpha's own bound enters every gradient).  The operator's outputs are also held to the
    plan's own calls bit for bit, which test 1 holds to the tight bounds."""
    a = _directed(300, seed=6, dup=True)
    drop, seed = 0.6, SEED ^ 0x55
    xt, xs, att = v2.operands((["uniform4", "x_zero", "spread80", "att_signs"] * 2)[:H], a, k, seed=10)
    gOut = grad(a, k, 10)
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    xtd, xsd, attd = (_dev(x).requires_grad_() for x in (xt, xs, att))
    plain_before = _host(op.gatv2_attention(xtd.detach(), xsd.detach(), attd.detach()))
    out = op.gatv2_attention(xtd, xsd, attd, dropout=drop, seed=seed)
    out.backward(_dev(gOut))
    got = tuple(_host(t) for t in (out.detach(), xtd.grad, xsd.grad, attd.grad))
    kp, c = ad.kept_entries(a, H, drop, seed), ad.factor(drop)
    ref_out, _, ref_gxt, ref_gxs, ref_gatt = vd.torch_float64(a, xt, xs, att, SLOPE, gOut, kp, c)
    tols = vd.propagated_bounds(a, xt, xs, att, SLOPE, gOut, drop, seed)
    worst = 0.0
    for what, x, ref, tol in zip(("Out", "grad_xt", "grad_xs", "grad_att"), got, (ref_out, ref_gxt, ref_gxs, ref_gatt), tols):
        err = np.abs(x.astype(np.float64) - ref)
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), f"{what} k={k} H={H}: worst err / tolerance {float((err / tol).max()):.3g}"
    print(f"k={k} H={H}: worst err / tolerance {worst:.3g}")
    # the plan's own calls give the same bits
    pd = torch.zeros((a.nnz, H), device="cuda")
    o2 = op.plan.gatv2_attention_dropout(xtd.detach(), xsd.detach(), attd.detach(), SLOPE, drop, seed, probs=pd)
    g2 = op.plan.gatv2_attention_dropout_backward(xtd.detach(), xsd.detach(), attd.detach(), pd, _dev(gOut), SLOPE, drop, seed)
    for x, t in zip(got, (o2,) + tuple(g2)):
        assert _same_bits(x, _host(t))
    # dropout=0 and training=False take the path they took before: the same bits
    for kw in (dict(dropout=0.0), dict(dropout=drop, training=False), dict(dropout=0.0, seed=3)):
        assert _same_bits(_host(op.gatv2_attention(xtd.detach(), xsd.detach(), attd.detach(), **kw)), plain_before)
    # seed=None draws from torch's default generator: torch.manual_seed reproduces a run, and the next draw differs
    torch.manual_seed(11)
    x1 = _host(op.gatv2_attention(xtd.detach(), xsd.detach(), attd.detach(), dropout=drop))
    x2 = _host(op.gatv2_attention(xtd.detach(), xsd.detach(), attd.detach(), dropout=drop))
    torch.manual_seed(11)
    assert _same_bits(_host(op.gatv2_attention(xtd.detach(), xsd.detach(), attd.detach(), dropout=drop)), x1) and not _same_bits(x1, x2)

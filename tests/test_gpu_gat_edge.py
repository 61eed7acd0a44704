"""The per-edge score term of the fused GAT attention on the GPU (flex_edge_gat_attention, flex_edge_gat_attention_backward): Out, P,
gEl, gEr, gEe and gV against float64 on every element under the bounds of tests/gat_edge_ref.py over the table of
tests/test_gat_edge_host.py (every (W, NS) form of both kernels, DROP off and on); ee = +0 against the GAT calls bit for bit; P and
drop_p = 0 against the undropped edge call; the output invariants (no P, the subsets of the gradients, either work array, run to run, a
captured graph, padded rows); the refusals of tests/gat_edge_entry_table.py; a row-range shard; a -inf and a NaN in ee; the composition
of engine calls that the fused call replaces; and SparseOperator.gat_attention(..., edge=e) with its gradients against float64 torch."""
import numpy as np
import pytest

import flex_amd
import gat_attention_ref as gat
import gat_edge_entry_table as table
import gat_edge_ref as ge
from backward_ref import _directed
from flex_amd import binding
from test_gat_dropout_host import SEED, grad, graph
from test_gat_edge_host import CASES, SLOPE, case_id, case_operands

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = -12345.5
KEYS = ("out", "p", "gel", "ger", "gee", "gv")
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


def _forward(p, a, el, er, ee, V, drop, seed=SEED, with_p=True):
    """(Out, P [nnz, H]) on the host; both start at the sentinel."""
    pd = _filled((a.nnz, el.shape[1])) if with_p else None
    out = p.gat_edge_attention(_dev(el), _dev(er), _dev(ee), _dev(V), SLOPE, drop, seed, out=_filled((a.m, V.shape[1])), probs=pd)
    return _host(out), (_host(pd) if with_p else None)


def _backward(p, a, el, er, ee, V, pr, g, drop, seed=SEED, want=(True, True, True, True)):
    """(gEl, gEr, gEe, gV, dWork) on the host; an output that is not wanted is None; dWork starts at the sentinel."""
    work = _filled((a.nnz, el.shape[1]))
    outs = p.gat_edge_attention_backward(_dev(el), _dev(er), _dev(ee), _dev(V), _dev(pr), _dev(g), SLOPE, drop, seed, want=want, work=work)
    return tuple(None if t is None else _host(t) for t in outs) + (_host(work),)


def _run(c):
    """The forward and backward of a case of the table, run once and shared by the tests below; nothing changes it.
    (Out, P, gEl, gEr, gEe, gV)."""
    if c not in _runs:
        name, k, H, drop = c
        a, el, er, ee, V, g = case_operands(name, k, H)
        p = plan(name, k)
        out, pr = _forward(p, a, el, er, ee, V, drop)
        *grads, work = _backward(p, a, el, er, ee, V, pr, g, drop)
        assert _is_fill(work), "dWork was written although dGradEe was given"
        _runs[c] = (out, pr, *grads)
    return _runs[c]


# ---- 1. against float64

@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_every_output_against_float64(c):
    name, k, H, drop = c
    a, el, er, ee, V, g = case_operands(name, k, H)
    out, pr, gel, ger, gee, gv = _run(c)
    each, what = {}, case_id(c)
    ge.check(a, el, er, ee, V, SLOPE, drop, SEED, out, pr, what=what, ratios=each)
    ge.check_backward(a, el, er, ee, V, pr, g, SLOPE, drop, SEED, gel, ger, gee, gv, what=what, ratios=each)
    print(f"{what}: worst err / bound " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))


# ---- 2. ee = +0 is the GAT call, bit for bit: what catches a sweep that diverged

def _gat_calls(p, a, el, er, V, g, drop):
    """(Out, P, gEl, gEr, dWork, gV) of flex_gat_attention / flex_gat_attention_dropout and their backward calls."""
    H = el.shape[1]
    eld, erd, Vd, gd_ = (_dev(x) for x in (el, er, V, g))
    pd, work = _filled((a.nnz, H)), _filled((a.nnz, H))
    if drop:
        o = p.gat_attention_dropout(eld, erd, Vd, SLOPE, drop, SEED, out=_filled((a.m, V.shape[1])), probs=pd)
        gel, ger, gv = p.gat_attention_dropout_backward(eld, erd, Vd, pd, gd_, SLOPE, drop, SEED, work=work)
    else:
        o = p.gat_attention(eld, erd, Vd, SLOPE, out=_filled((a.m, V.shape[1])), p=pd)
        gel, ger, gv = p.gat_attention_backward(eld, erd, Vd, pd, gd_, SLOPE, work=work)
    return tuple(_host(t) for t in (o, pd, gel, ger, work, gv))


@pytest.mark.parametrize("drop", [0.0, 0.5])
@pytest.mark.parametrize("name,k,H", [("directed_empty", 8, 2), ("long_rows", 32, 4), ("thresholds_lifted", 48, 3), ("long_rows", 128, 1),
                                      ("thresholds_lifted", 256, 1), ("thresholds_lifted", 512, 2), ("thresholds_lifted", 1024, 64)])
def test_with_a_zero_edge_term_every_output_has_the_bits_of_the_gat_calls(name, k, H, drop):
    """One pair per (W, NS) form.  No operand is -0 (gat_edge_ref.operands), so x + (+0) has the bits of x."""
    a, el, er, ee, V, g = case_operands(name, k, H)
    zero = np.zeros_like(ee)
    p = plan(name, k)
    out, pr = _forward(p, a, el, er, zero, V, drop)
    gel, ger, gee, gv, _ = _backward(p, a, el, er, zero, V, pr, g, drop)
    for key, x, y in zip(("out", "p", "gel", "ger", "gee (dWork)", "gv"), (out, pr, gel, ger, gee, gv), _gat_calls(p, a, el, er, V, g, drop)):
        assert _same_bits(x, y), f"{key} differs from the GAT call's in {int((x.view(np.uint32) != y.view(np.uint32)).sum())} elements"


# ---- 3. P is the undropped edge call's

@pytest.mark.parametrize("name,k,H", [("thresholds_lifted", 48, 3), ("long_rows", 64, 8), ("thresholds_lifted", 1024, 64)])
def test_with_dropout_p_is_the_undropped_calls(name, k, H):
    """drop_p = 0 launches the DROP-off kernels (test 2 holds them to flex_gat_attention's bits); with dropout P keeps those bits."""
    assert _same_bits(_run((name, k, H, 0.5))[1], _run((name, k, H, 0.0))[1])
    assert not _same_bits(_run((name, k, H, 0.5))[0], _run((name, k, H, 0.0))[0])


# ---- 4. output invariants

@pytest.mark.parametrize("drop", [0.0, 0.5])
def test_without_p_the_same_out_and_every_gradient_has_the_same_bits_whichever_others_are_asked_for(drop):
    c = ("thresholds_lifted", 48, 3, drop)
    name, k, H, _ = c
    a, el, er, ee, V, g = case_operands(name, k, H)
    p = plan(name, k)
    out, pr, *full = _run(c)
    assert _same_bits(_forward(p, a, el, er, ee, V, drop, with_p=False)[0], out)
    for mask in range(1, 16):
        want = tuple(bool(mask >> i & 1) for i in range(4))
        *got, work = _backward(p, a, el, er, ee, V, pr, g, drop, want=want)
        for i in range(4):
            assert (got[i] is None) if not want[i] else _same_bits(got[i], full[i]), (want, i)
        if want[2]:
            assert _is_fill(work), want                   # dGradEe is the work array: dWork is untouched
        elif want[0] or want[1]:
            assert _same_bits(work, full[2]), want        # dWork as the work array holds the same dx
        else:
            assert _is_fill(work), want                   # gV alone: the rows' launch is skipped
    if drop:
        other = _forward(p, a, el, er, ee, V, drop, seed=SEED + 1)
        assert not _same_bits(other[0], out) and _same_bits(other[1], pr)  # another seed: another Out, the same P


@pytest.mark.parametrize("drop", [0.0, 0.5])
def test_two_runs_and_a_captured_graph_give_the_same_bits(drop):
    c = ("long_rows", 64, 8, drop)
    name, k, H, _ = c
    a, el, er, ee, V, g = case_operands(name, k, H)
    p = plan(name, k)
    first = _run(c)
    out2, pr2 = _forward(p, a, el, er, ee, V, drop)
    again = (out2, pr2) + _backward(p, a, el, er, ee, V, pr2, g, drop)[:4]
    for x, y in zip(first, again):
        assert _same_bits(x, y)
    eld, erd, eed, Vd, gd_ = (_dev(x) for x in (el, er, ee, V, g))
    o, pd = _filled((a.m, k)), torch.empty((a.nnz, H), device="cuda")
    gel, ger, gee, gv = _filled((a.m, H)), _filled((a.n, H)), _filled((a.nnz, H)), _filled((a.n, k))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=side):  # one stream: the three launches are a chain
        p.gat_edge_attention(eld, erd, eed, Vd, SLOPE, drop, SEED, out=o, probs=pd)
        p.gat_edge_attention_backward(eld, erd, eed, Vd, pd, gd_, SLOPE, drop, SEED, grad_el=gel, grad_er=ger, grad_ee=gee, grad_v=gv)
    for t in (o, pd, gel, ger, gee, gv):
        t.fill_(SENTINEL)
    graph_.replay()
    for x, t in zip(first, (o, pd, gel, ger, gee, gv)):
        assert _same_bits(x, _host(t))


@pytest.mark.parametrize("drop", [0.0, 0.5])
def test_padded_leading_dimensions_give_the_same_bits_and_leave_the_padding_untouched(drop):
    c = ("thresholds_lifted", 48, 3, drop)
    name, k, H, _ = c
    a, el, er, ee, V, g = case_operands(name, k, H)
    ldb, ldc = k + 4, k + 8
    p = plan(name, k, ldb=ldb, ldc=ldc)
    dense = _run(c)
    s = torch.cuda.current_stream().cuda_stream
    Vp, gp = _filled((a.n, ldb)), _filled((a.m, ldc))
    Vp[:, :k], gp[:, :k] = _dev(V), _dev(g)
    eld, erd, eed = _dev(el), _dev(er), _dev(ee)
    o, gv = _filled((a.m, ldc)), _filled((a.n, ldb))
    pd, gee, gel, ger = _filled((a.nnz, H)), _filled((a.nnz, H)), _filled((a.m, H)), _filled((a.n, H))
    p.gat_edge_attention_ptr(H, eld.data_ptr(), erd.data_ptr(), eed.data_ptr(), Vp.data_ptr(), SLOPE, drop, SEED, o.data_ptr(), pd.data_ptr(), s)
    p.gat_edge_attention_backward_ptr(H, eld.data_ptr(), erd.data_ptr(), eed.data_ptr(), Vp.data_ptr(), pd.data_ptr(), gp.data_ptr(), SLOPE, drop, SEED,
                                      gel.data_ptr(), ger.data_ptr(), gee.data_ptr(), gv.data_ptr(), None, s)
    o, gv = _host(o), _host(gv)
    assert _is_fill(o[:, k:]) and _is_fill(gv[:, k:])
    for key, x, y in zip(KEYS, dense, (o[:, :k], _host(pd), _host(gel), _host(ger), _host(gee), gv[:, :k])):
        assert _same_bits(x, y), key


# ---- 5. refusals: every row of the entry table, with all outputs untouched

@pytest.mark.parametrize("drop", [table.DROP, 0.0], ids=["p0.5", "p0"])
def test_every_row_of_the_entry_table_gets_its_code_and_a_refused_call_writes_nothing(drop):
    """The real library on real buffers, each large enough for any operand of the table's shapes (and for a row moved 4 bytes): a NULL
    dEe, both work pointers NULL, the work array equal to dP and the backward on a shard among the rows.  Every call must return the
    table's code; one that launches nothing must leave every output at the sentinel."""
    from fused_attention_backward_ref import both_sides
    from fused_attention_ref import threshold_graph
    a = both_sides(threshold_graph())
    plans_ = table.plans(a)
    size = max(a.m, a.n) * table.K + a.nnz * table.H + 16
    outputs = ("Out", "GEl", "GEr", "GEe", "GV", "Work")
    bufs = {name: _filled((size,)) if name in outputs else torch.zeros((size,), device="cuda") for name in table.OPERANDS}
    ops = {name: t.data_ptr() for name, t in bufs.items()}
    s = torch.cuda.current_stream().cuda_stream
    quiet = 0
    for entry in table.ENTRIES:
        fn = binding._values_fn(entry)
        watched = outputs + (("P",) if entry == table.FORWARD else ())
        for row, change, code, launches in table.rows_of(entry, drop):
            handle, args = table.arguments(entry, change, plans_, ops, drop)
            for name in watched:
                bufs[name].fill_(SENTINEL)
            if entry == table.BACKWARD:
                bufs["P"].fill_(0.25)  # read, not written: finite probabilities
            rc = fn(handle, *args, s)
            torch.cuda.synchronize()
            assert rc == code, f"{entry}, p = {drop}, row {row}: {rc}, want {code}"
            if not launches:
                quiet += 1
                for name in watched:
                    assert _is_fill(_host(bufs[name])), f"{entry}, p = {drop}, row {row}: {name} was written"
    assert quiet >= 50, quiet
    for pl in plans_.values():
        pl.destroy()


# ---- 6. a row-range shard, forward

@pytest.mark.parametrize("drop", [0.0, 0.5])
def test_a_shard_reads_ee_and_writes_p_at_the_entries_of_the_whole_matrix(drop):
    name, k, H = "long_rows", 32, 4
    a = graph(name)
    el, er, ee, V = ge.operands(gat.scenarios_of(H, shift=3), ge.edge_scenarios_of(H, shift=1), a, k, seed=9)
    whole, whole_p = _forward(plan(name, k), a, el, er, ee, V, drop)
    eld, erd, eed, Vd = _dev(el), _dev(er), _dev(ee), _dev(V)
    s = torch.cuda.current_stream().cuda_stream
    cuts = [0, 17, 18, 18, 101, 260, a.m]
    union, union_p = np.full((a.m, k), np.float32(SENTINEL)), np.full((a.nnz, H), np.float32(SENTINEL))
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        shard = flex_amd.Plan(a, k, rows=(r0, r1), attention=True)
        shard.self_check()
        e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
        out, pd = _filled((a.m, k)), _filled((a.nnz, H))
        shard.gat_edge_attention_ptr(H, eld.data_ptr() + 4 * H * r0, erd.data_ptr(), eed.data_ptr(), Vd.data_ptr(), SLOPE, drop, SEED,
                                     out.data_ptr() + 4 * k * r0, pd.data_ptr(), s)
        out, pd = _host(out), _host(pd)
        assert _is_fill(out[:r0]) and _is_fill(out[r1:]), (r0, r1)
        assert _is_fill(pd[:e0]) and _is_fill(pd[e1:]), (r0, r1)
        if r1 > r0:
            ge.check(a, el[r0:r1], er, ee, V, SLOPE, drop, SEED, out[r0:r1], pd[e0:e1], rows=(r0, r1), what=f"rows [{r0}, {r1})")
        union[r0:r1], union_p[e0:e1] = out[r0:r1], pd[e0:e1]
        shard.destroy()
    assert _same_bits(union, whole) and _same_bits(union_p, whole_p)


# ---- 7. one -inf and one NaN in ee

@pytest.mark.parametrize("drop", [0.0, 0.5])
def test_an_infinite_edge_term_masks_one_entry_of_one_head_and_a_nan_poisons_one_head_of_one_row(drop):
    name, k, H = "thresholds_lifted", 32, 4
    d = k // H
    a = graph(name)
    el, er, ee, V = ge.operands(["uniform4"] * H, ["spread", "cancel", "zero_edge", "near_cancel"], a, k, seed=6)
    ee = np.clip(ee, -4, 4) + np.float32(0)
    row, col, rp = gat.coo(a)
    deg = np.diff(rp)
    r_one, r_all, r_nan = (int(r) for r in np.flatnonzero(deg >= 3)[[0, 5, 9]])
    masked = ee.copy()
    e_one = int(rp[r_one]) + 1
    masked[e_one, 1] = -np.inf                       # one entry, head 1
    masked[rp[r_all]:rp[r_all + 1], 2] = -np.inf     # every entry of a row, head 2
    masked[int(rp[r_nan]) + 2, 3] = np.nan           # one NaN, head 3
    p = plan(name, k)
    clean, clean_p = _forward(p, a, el, er, ee, V, 0.0)
    out, pr = _forward(p, a, el, er, masked, V, drop)
    assert pr[e_one, 1].view(np.uint32) == 0 and np.all(pr[e_one, [0, 2, 3]] > 0)
    assert _same_bits(pr[e_one, [0, 2, 3]], clean_p[e_one, [0, 2, 3]])              # the other heads of the entry are left alone
    assert not np.ascontiguousarray(pr[rp[r_all]:rp[r_all + 1], 2]).view(np.uint32).any()
    assert not np.ascontiguousarray(out[r_all, 2 * d:3 * d]).view(np.uint32).any()   # a fully masked head of a row is +0 bits
    assert np.isnan(out[r_nan, 3 * d:]).all() and np.isfinite(out[r_nan, :3 * d]).all()
    assert np.isnan(pr[rp[r_nan]:rp[r_nan + 1], 3]).all() and np.isfinite(pr[rp[r_nan]:rp[r_nan + 1], :3]).all()
    rest = np.ones(a.m, bool)
    rest[r_nan] = False
    assert np.isfinite(out[rest]).all()
    if not drop:  # rows and heads that hold no changed entry keep their bits
        rest[[r_one, r_all]] = False
        assert _same_bits(out[rest], clean[rest])
    ge.check(a, el, er, masked, V, SLOPE, drop, SEED, out, pr, what="masked and poisoned")


# ---- 8. the composition it replaces

@pytest.mark.parametrize("k,H", [(16, 4), (64, 8)])
def test_against_the_composition_of_engine_calls_it_replaces(k, H):
    """What a model with edge features runs on the parent commit, head by head: torch index arithmetic for the scores with ee,
    edge_softmax, set_values and an SpMM on a width-d plan; in the backward the transposed SpMM, an SDDMM, edge_softmax_backward and
    torch sums, from the same probabilities.  Each side is within its own bound of float64 -- the fused call's, and the composition's
    (c_r = 32, a_r = 4, b_r = 32: flex_spmm pads its rows, flex_edge_softmax_backward rounds its products, as
    tests/test_gpu_gat_attention.py takes them) -- so they differ by at most the sum; the non-finite elements must be the same."""
    name = "thresholds_lifted"
    a, p, d = graph(name), plan(name, k), k // H
    single = flex_amd.Plan(a, d, ldb=k, ldc=k, mutable_values=True)
    single_t = flex_amd.Plan(a, d, ldb=k, ldc=k, transpose=True, mutable_values=True)
    el, er, ee, V = ge.operands(gat.scenarios_of(H, shift=1), ge.edge_scenarios_of(H, shift=4), a, k, seed=3)
    g = grad(a, k, 3)
    out, pr = _forward(p, a, el, er, ee, V, 0.0)
    mine = (out, pr) + _backward(p, a, el, er, ee, V, pr, g, 0.0)[:4]
    row, col, _ = gat.coo(a)
    rowd, cold = _dev(row), _dev(col)
    eld, erd, eed, Vd, gd = (_dev(x) for x in (el, er, ee, V, g))
    s = torch.cuda.current_stream().cuda_stream
    o1, gv1 = torch.zeros((a.m, k), device="cuda"), torch.zeros((a.n, k), device="cuda")
    p1, dx1, gel1, ger1 = [], [], [], []
    for h in range(H):
        off = 4 * h * d
        x = (eld[rowd, h] + erd[cold, h]) + eed[:, h]
        alpha = single.edge_softmax(torch.nn.functional.leaky_relu(x, SLOPE).contiguous(), 1.0)
        single.set_values(alpha)
        single.spmm(Vd.data_ptr() + off, o1.data_ptr() + off, s)
        pin = _dev(pr[:, h])  # the backward of both sides starts from the same probabilities
        single_t.set_values(pin)
        single_t.spmm(gd.data_ptr() + off, gv1.data_ptr() + off, s)
        da = torch.zeros(a.nnz, device="cuda")
        single.sddmm_ptr(gd.data_ptr() + off, Vd.data_ptr() + off, da.data_ptr(), s)
        dz = single.edge_softmax_backward(pin, da, 1.0)
        dx = torch.where(x > 0, dz, SLOPE * dz)
        p1.append(_host(alpha))
        dx1.append(_host(dx))
        gel1.append(_host(torch.zeros(a.m, device="cuda").index_add_(0, rowd, dx)))
        ger1.append(_host(torch.zeros(a.n, device="cuda").index_add_(0, cold, dx)))
    theirs = (_host(o1), np.stack(p1, 1), np.stack(gel1, 1), np.stack(ger1, 1), np.stack(dx1, 1), _host(gv1))
    ref, refb = ge.reference(a, el, er, ee, V, SLOPE), ge.backward_reference(a, el, er, ee, V, pr, g, SLOPE)
    ref2, refb2 = ge.reference(a, el, er, ee, V, SLOPE, c_r=32), ge.backward_reference(a, el, er, ee, V, pr, g, SLOPE, a_r=4, b_r=32)
    bounds = [ref["out_bound"] + ref2["out_bound"], ref["p_bound"] + ref2["p_bound"]] + [refb[key + "_bound"] + refb2[key + "_bound"] for key in KEYS[2:]]
    for key, x, y, b in zip(KEYS, mine, theirs, bounds):
        assert np.array_equal(np.isfinite(x), np.isfinite(y)), f"{key}: the non-finite elements differ in {int((np.isfinite(x) != np.isfinite(y)).sum())} places"
        assert np.array_equal(np.isnan(x), np.isnan(y)), key
        fin = np.isfinite(x) & np.isfinite(b)
        ratio = np.abs(x[fin].astype(np.float64) - y[fin]) / b[fin]
        worst = float(ratio.max()) if ratio.size else 0.0
        print(f"k={k} H={H} {key}: against the composition, worst err / (sum of the two bounds) {worst:.3g}; same bits: {_same_bits(x, y)}")
        assert worst <= 1.0, f"k={k} H={H} {key}: {worst:.3g}"
    single.destroy(), single_t.destroy()


# ---- 9. autograd

@pytest.mark.parametrize("drop", [0.0, 0.6])
@pytest.mark.parametrize("k,H", [(32, 4), (128, 8)])
def test_the_operator_with_edge_and_its_gradients_against_float64(k, H, drop):
    """Against float64 torch autograd (with dropout: the numpy mask as a constant).  Tolerance: gat_edge_ref.propagated_bounds of the
    undropped step (the backward starts from the forward's fp32 alpha); with dropout times 2 c, as tests/test_gpu_gat_dropout.py
    derives it: every term is linear in |V|, |da| or dda of an entry, which dropout multiplies by w <= c, and the one more rounding per
    count at most doubles a term.  The operator's outputs are also held to the plan's own calls bit for bit."""
    import attention_dropout_ref as ad
    a = _directed(300, seed=6, dup=True)
    seed = SEED ^ 0x55
    rng = np.random.default_rng([k, H, 26])
    el, er = (rng.uniform(-2, 2, (r, H)).astype(np.float32) for r in (a.m, a.n))
    ee = rng.uniform(-2, 2, (a.nnz, H)).astype(np.float32)
    V, gOut = (rng.uniform(-1, 1, (r, k)).astype(np.float32) for r in (a.n, a.m))
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    eld, erd, eed, Vd = (_dev(x).requires_grad_() for x in (el, er, ee, V))
    out = op.gat_attention(eld, erd, Vd, dropout=drop, seed=seed, edge=eed)
    out.backward(_dev(gOut))
    got = tuple(_host(t) for t in (out.detach(), eld.grad, erd.grad, eed.grad, Vd.grad))
    kp, c = (ad.kept_entries(a, H, drop, seed), ad.factor(drop)) if drop else (None, 1.0)
    want = ge.torch_float64(a, el, er, ee, V, SLOPE, gOut, kp, c)
    want = (want[0],) + want[2:]
    tols = ge.propagated_bounds(a, el, er, ee, V, SLOPE, gOut)
    worst = 0.0
    for what, x, ref, tol in zip(("Out", "grad_el", "grad_er", "grad_edge", "grad_V"), got, want, tols):
        tol = (2 * c if drop else 1.0) * tol
        err = np.abs(x.astype(np.float64) - ref)
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), f"{what} k={k} H={H} p={drop}: worst err / tolerance {float((err / tol).max()):.3g}"
    print(f"k={k} H={H} p={drop}: worst err / tolerance {worst:.3g}")
    # the plan's own calls give the same bits
    pd = torch.zeros((a.nnz, H), device="cuda")
    ops_ = tuple(t.detach() for t in (eld, erd, eed, Vd))
    o2 = op.plan.gat_edge_attention(*ops_, SLOPE, drop, seed, probs=pd)
    g2 = op.plan.gat_edge_attention_backward(*ops_, pd, _dev(gOut), SLOPE, drop, seed)
    for x, t in zip(got, (o2,) + tuple(g2)):
        assert _same_bits(x, _host(t))
    if drop:  # training=False is the undropped call
        off = op.gat_attention(*ops_[:2], ops_[3], dropout=drop, training=False, edge=ops_[2])
        assert _same_bits(_host(off), _host(op.plan.gat_edge_attention(*ops_, SLOPE)))
    plain = op.gat_attention(ops_[0], ops_[1], ops_[3])  # edge=None takes the path it took
    assert _same_bits(_host(plain), _host(op.plan.gat_attention(ops_[0], ops_[1], ops_[3], SLOPE)))

"""The fused GATv2 attention on the GPU (flex_gatv2_attention, flex_gatv2_attention_backward): Out, P, gXt, gXs, gAtt and dz against the
float64 reference and the bounds of tests/gatv2_attention_ref.py on every element, with a different scenario in every head of a call,
over every (k, H) of tests/attention_forms.py's GAT table and every row and column class; against the composition it replaces; head
isolation; the output invariants (dP = NULL, subsets of the gradients, run to run, a captured graph, one buffer for Xt and Xs,
sentinels, padded leading dimensions); the refusal table of tests/gatv2_entry_table.py on the real library; a row-range shard;
SparseOperator.gatv2_attention with its gradients against a float64 torch evaluation; and the census of namespace flex::gatv2.

Graphs: those of tests/test_gpu_gat_attention.py, by import: threshold_graph() (rows of 31 / 32 / 33 and 511 / 512 / 513 entries),
its lift both_sides() (the same classes in the columns), _directed(250, 260, seed=7) (empty rows and columns) and long_rows_graph().
The wide pairs (k >= 256) run on the two threshold graphs alone."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import flex_amd
import gatv2_attention_ref as v2
import gatv2_entry_table as table
from attention_forms import FORM_OF_K, FORMS
from attention_forms import GAT_PAIRS as PAIRS
from backward_ref import _directed
from flex_amd import binding
from test_gpu_gat_attention import GRAPHS, graph

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = [(name, k, H) for k, H in PAIRS for name in (sorted(GRAPHS) if k < 256 else ["thresholds", "thresholds_lifted"])]
SENTINEL = -12345.5
SLOPE = v2.SLOPE
_plans = {}


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


def _same_bits(x, y):
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    return x.shape == y.shape and bool(np.array_equal(x.view(np.uint32), y.view(np.uint32)))


def _grad(a, k, seed):
    return np.random.default_rng([seed, k, 78]).uniform(-1, 1, (a.m, k)).astype(np.float32)


def _forward(p, a, xt, xs, att, with_p=True, shared=False):
    """(Out, P [nnz, H]) on the host; both start at the sentinel.  shared: Xt and Xs are one buffer."""
    pd = torch.full((a.nnz, att.shape[0]), SENTINEL, device="cuda") if with_p else None
    out = torch.full((a.m, xs.shape[1]), SENTINEL, device="cuda")
    xsd = _dev(xs)
    p.gatv2_attention(xsd if shared else _dev(xt), xsd, _dev(att), SLOPE, out=out, p=pd)
    return _host(out), (_host(pd) if with_p else None)


def _backward(p, a, xt, xs, att, pr, g, want=(True, True, True), shared=False):
    """(gXt, gXs, gAtt, dz [nnz, H]) on the host; an output that is not wanted is None, dz is what dWork holds afterwards."""
    work = torch.full((a.nnz, att.shape[0]), SENTINEL, device="cuda")
    xsd = _dev(xs)
    outs = p.gatv2_attention_backward(xsd if shared else _dev(xt), xsd, _dev(att), _dev(pr), _dev(g), SLOPE, work=work, want=want)
    return tuple(None if t is None else _host(t) for t in outs) + (_host(work),)


# ---- 1. against float64

@pytest.mark.parametrize("name,k,H", CASES)
def test_every_output_against_float64_with_a_scenario_per_head(name, k, H):
    a, p = graph(name), plan(name, k)
    names = v2.scenarios_of(H, shift=PAIRS.index((k, H)) + sorted(GRAPHS).index(name))
    xt, xs, att = v2.operands(names, a, k, seed=1)
    g = _grad(a, k, 1)
    out, pr = _forward(p, a, xt, xs, att)
    wf = v2.check(a, xt, xs, att, SLOPE, out, pr, what=f"{name} k={k} H={H}")
    each = {}
    wb = v2.check_backward(a, xt, xs, att, pr, g, SLOPE, *_backward(p, a, xt, xs, att, pr, g), what=f"{name} k={k} H={H}", ratios=each)
    print(f"{name} k={k} H={H} {'/'.join(names[:6])}: worst err / bound forward {wf:.3g}, backward {wb:.3g} (" + " ".join(f"{key} {v:.3g}" for key, v in each.items()) + ")")


# ---- 2. against the composition it replaces

@pytest.mark.parametrize("name,k,H", [("thresholds_lifted", 16, 4), ("long_rows", 64, 8), ("thresholds_lifted", 512, 2)])
def test_agreement_with_the_composition_it_replaces(name, k, H):
    """What a user has without the fused call: the [nnz, k] tensor Xt[row] + Xs[col] and the scores in torch, then per head
    edge_softmax, set_values and the SpMM on a plan of width d; the gradients by torch autograd through its own softmax."""
    a, p, d = graph(name), plan(name, k), k // H
    single = flex_amd.Plan(a, d, ldb=k, ldc=k, mutable_values=True)
    xt, xs, att = v2.operands(v2.scenarios_of(H, shift=1), a, k, seed=3)
    g = _grad(a, k, 3)
    out, pr = _forward(p, a, xt, xs, att)
    mine = (out, pr) + _backward(p, a, xt, xs, att, pr, g)
    row, col, _ = v2.coo(a)
    rowd, cold = _dev(row.astype(np.int64)), _dev(col.astype(np.int64))
    xtd, xsd, attd = (_dev(x).requires_grad_() for x in (xt, xs, att))
    stream = torch.cuda.current_stream().cuda_stream
    s = (torch.nn.functional.leaky_relu((xtd[rowd] + xsd[cold]).view(-1, H, d), SLOPE) * attd).sum(-1)
    s.retain_grad()
    o1, p1 = torch.zeros((a.m, k), device="cuda"), []
    for h in range(H):
        alpha = single.edge_softmax(s.detach()[:, h].contiguous(), 1.0)
        single.set_values(alpha)
        single.spmm(xsd.data_ptr() + 4 * h * d, o1.data_ptr() + 4 * h * d, stream)
        p1.append(_host(alpha))
    M = torch.full((a.m, H), -np.inf, device="cuda").scatter_reduce(0, rowd[:, None].expand(-1, H), s.detach(), "amax")
    t = torch.exp(s - M[rowd])
    al = t / torch.zeros((a.m, H), device="cuda").index_add_(0, rowd, t)[rowd]
    o2 = torch.zeros((a.m, H, d), device="cuda").index_add_(0, rowd, al[:, :, None] * xsd.view(a.n, H, d)[cold]).reshape(a.m, k)
    o2.backward(_dev(g))
    theirs = (_host(o1), np.stack(p1, 1), _host(xtd.grad), _host(xsd.grad), _host(attd.grad), _host(s.grad))
    b1 = v2.propagated_bounds(a, xt, xs, att, SLOPE, g, with_dz=True)
    b2 = v2.propagated_bounds(a, xt, xs, att, SLOPE, g, c_r=32, a_r=4, b_r=32, depth=a.nnz, with_dz=True)
    order = (0, 5, 1, 2, 3, 4)  # out, p, gxt, gxs, gatt, dz
    for key, x, y, i in zip(("out", "p", "gxt", "gxs", "gatt", "dz"), mine, theirs, order):
        b = b1[i] + b2[i]
        assert np.array_equal(np.isfinite(x), np.isfinite(y)), f"{key}: the non-finite elements differ in {int((np.isfinite(x) != np.isfinite(y)).sum())} places"
        fin = np.isfinite(x) & np.isfinite(b)
        ratio = np.abs(x[fin].astype(np.float64) - y[fin]) / b[fin]
        worst = float(ratio.max()) if ratio.size else 0.0
        print(f"{name} k={k} H={H} {key}: against the composition, worst err / (sum of the two bounds) {worst:.3g}")
        assert worst <= 1.0, f"{name} k={k} H={H} {key}: {worst:.3g}"


# ---- 3. head isolation

@pytest.mark.parametrize("k,H", [(8, 2), (48, 3), (512, 2)])
def test_what_one_head_holds_reaches_no_other_head(k, H):
    name = "thresholds_lifted"
    a, p, d = graph(name), plan(name, k), k // H
    xt, xs, att = v2.operands(v2.scenarios_of(H, shift=2), a, k, seed=4)
    g = _grad(a, k, 4)

    def run(xt, xs, att, g):
        out, pr = _forward(p, a, xt, xs, att)
        return (out, pr) + _backward(p, a, xt, xs, att, pr, g)

    base = run(xt, xs, att, g)
    rng = np.random.default_rng(5)
    for j in sorted({0, H - 1}):
        c = v2.head_columns(k, H, j)
        xt2, xs2, att2, g2 = (x.copy() for x in (xt, xs, att, g))
        att2[j] = rng.uniform(-1e30, 1e30, d).astype(np.float32)  # a huge head
        for x in (xt2, xs2, g2):
            x[:, c] = rng.uniform(-3, 3, (x.shape[0], d)).astype(np.float32)
            x[rng.integers(0, x.shape[0], 9), c.start + rng.integers(0, d, 9)] = [np.nan, np.inf, -np.inf] * 3  # and a poisoned one
        other = run(xt2, xs2, att2, g2)
        keep_cols = np.ones(k, bool)
        keep_cols[c] = False
        keep_heads = np.arange(H) != j
        for key, x, y in zip(("out", "p", "gxt", "gxs", "gatt", "dz"), base, other):
            if key == "gatt":
                assert _same_bits(x[keep_heads], y[keep_heads]), f"k={k} H={H}: changing head {j} changed gatt of another head"
                continue
            sel = keep_heads if key in ("p", "dz") else keep_cols
            assert _same_bits(x[:, sel], y[:, sel]), f"k={k} H={H}: changing head {j} changed {key} of another head"
        assert not _same_bits(base[0][:, c], other[0][:, c])


# ---- 4. output invariants

def test_without_p_the_same_out_and_every_gradient_has_the_same_bits_whichever_others_are_asked_for():
    name, k, H = "thresholds_lifted", 48, 3
    a, p = graph(name), plan(name, k)
    xt, xs, att = v2.operands(["spread80", "x_zero", "att_signs"], a, k, seed=6)
    g = _grad(a, k, 6)
    out, pr = _forward(p, a, xt, xs, att)
    assert _same_bits(_forward(p, a, xt, xs, att, with_p=False)[0], out)
    full = _backward(p, a, xt, xs, att, pr, g)
    devs = [_dev(x) for x in (xt, xs, att, pr, g)]
    need = p.gatv2_attention_work_size()
    for mask in range(8):
        want = tuple(bool(mask >> i & 1) for i in range(3))
        sent = [torch.full(shape, SENTINEL, device="cuda") for shape in ((a.m, k), (a.n, k), (H, k // H))]
        work, att_work = torch.full((a.nnz, H), SENTINEL, device="cuda"), torch.full((need,), SENTINEL, device="cuda")
        p.gatv2_attention_backward_ptr(H, *(t.data_ptr() for t in devs), SLOPE, *(t.data_ptr() if w else None for t, w in zip(sent, want)),
                                       work.data_ptr(), att_work.data_ptr(), torch.cuda.current_stream().cuda_stream)
        for i in range(3):
            got = _host(sent[i])
            assert _same_bits(got, full[i]) if want[i] else np.all(got == SENTINEL), (want, i)
        if any(want):
            assert _same_bits(_host(work), full[3]), want  # every gradient needs dz
        else:
            assert np.all(_host(work) == SENTINEL), want
        assert bool((_host(att_work) != SENTINEL).all()) if want[2] else bool((_host(att_work) == SENTINEL).all()), want


def test_two_runs_and_a_captured_graph_give_the_same_bits():
    name, k, H = "long_rows", 128, 8
    a, p = graph(name), plan(name, k)
    xt, xs, att = v2.operands(v2.scenarios_of(H), a, k, seed=7)
    g = _grad(a, k, 7)
    out, pr = _forward(p, a, xt, xs, att)
    first = (out, pr) + _backward(p, a, xt, xs, att, pr, g)
    out2, pr2 = _forward(p, a, xt, xs, att)
    again = (out2, pr2) + _backward(p, a, xt, xs, att, pr2, g)
    for x, y in zip(first, again):
        assert _same_bits(x, y)
    xtd, xsd, attd, gd = (_dev(x) for x in (xt, xs, att, g))
    o, pd, work = torch.empty((a.m, k), device="cuda"), torch.empty((a.nnz, H), device="cuda"), torch.empty((a.nnz, H), device="cuda")
    gxt, gxs, gatt = torch.empty((a.m, k), device="cuda"), torch.empty((a.n, k), device="cuda"), torch.empty((H, k // H), device="cuda")
    att_work = torch.empty(p.gatv2_attention_work_size(), device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=side):  # one stream: the four launches are a chain
        p.gatv2_attention(xtd, xsd, attd, SLOPE, out=o, p=pd)
        p.gatv2_attention_backward(xtd, xsd, attd, pd, gd, SLOPE, grad_xt=gxt, grad_xs=gxs, grad_att=gatt, work=work, att_work=att_work)
    for t in (o, pd, work, gxt, gxs, gatt, att_work):
        t.fill_(SENTINEL)
    graph_.replay()
    for x, t in zip(first, (o, pd, gxt, gxs, gatt, work)):
        assert _same_bits(x, _host(t))


# ---- 5. Xt and Xs in one buffer

@pytest.mark.parametrize("k,H", [(32, 4), (512, 2)])
def test_one_buffer_for_xt_and_xs_gives_the_bits_of_two_copies(k, H):
    name = "thresholds_lifted"  # square
    a, p = graph(name), plan(name, k)
    _, xs, att = v2.operands(v2.scenarios_of(H, shift=3), a, k, seed=12)
    g = _grad(a, k, 12)
    out, pr = _forward(p, a, xs.copy(), xs, att)
    two = (out, pr) + _backward(p, a, xs.copy(), xs, att, pr, g)
    out1, pr1 = _forward(p, a, None, xs, att, shared=True)
    one = (out1, pr1) + _backward(p, a, None, xs, att, pr1, g, shared=True)
    for key, x, y in zip(("out", "p", "gxt", "gxs", "gatt", "dz"), two, one):
        assert _same_bits(x, y), key


# ---- 6. padded leading dimensions

def test_padded_leading_dimensions_and_everything_outside_the_defined_elements_keep_their_fill():
    name, k, H, ldb, ldc = "directed_empty", 16, 4, 24, 20
    a, p = graph(name), plan(name, k, ldb=ldb, ldc=ldc)
    xt, xs, att = v2.operands(v2.scenarios_of(H, shift=4), a, k, seed=8)
    g = _grad(a, k, 8)
    want_out, want_p = _forward(plan(name, k), a, xt, xs, att)
    want_b = _backward(plan(name, k), a, xt, xs, att, want_p, g)
    xtp, xsp, gp = (torch.full((r, ld), SENTINEL, device="cuda") for r, ld in ((a.m, ldc), (a.n, ldb), (a.m, ldc)))
    xtp[:, :k], xsp[:, :k], gp[:, :k] = _dev(xt), _dev(xs), _dev(g)
    pad = 8  # floats of sentinel after every array
    need = p.gatv2_attention_work_size()
    arrays = {key: torch.full((n + pad,), SENTINEL, device="cuda") for key, n in
              (("out", a.m * ldc), ("p", a.nnz * H), ("gxt", a.m * ldc), ("gxs", a.n * ldb), ("gatt", k), ("work", a.nnz * H), ("att_work", need))}
    attd = _dev(att)
    s = torch.cuda.current_stream().cuda_stream
    p.gatv2_attention_ptr(H, xtp.data_ptr(), xsp.data_ptr(), attd.data_ptr(), SLOPE, arrays["out"].data_ptr(), arrays["p"].data_ptr(), s)
    p.gatv2_attention_backward_ptr(H, xtp.data_ptr(), xsp.data_ptr(), attd.data_ptr(), arrays["p"].data_ptr(), gp.data_ptr(), SLOPE,
                                   arrays["gxt"].data_ptr(), arrays["gxs"].data_ptr(), arrays["gatt"].data_ptr(), arrays["work"].data_ptr(),
                                   arrays["att_work"].data_ptr(), s)
    got = {key: _host(t) for key, t in arrays.items()}
    for key in got:
        assert np.all(got[key][-pad:] == SENTINEL), f"{key}: written past its end"  # att_work: past the size the library reports
    out, gxt, gxs = got["out"][:-pad].reshape(a.m, ldc), got["gxt"][:-pad].reshape(a.m, ldc), got["gxs"][:-pad].reshape(a.n, ldb)
    assert np.all(out[:, k:] == SENTINEL) and np.all(gxt[:, k:] == SENTINEL) and np.all(gxs[:, k:] == SENTINEL), "a padded tail was written"
    assert _same_bits(out[:, :k], want_out) and _same_bits(gxt[:, :k], want_b[0]) and _same_bits(gxs[:, :k], want_b[1])
    for key, want, shape in (("p", want_p, (a.nnz, H)), ("gatt", want_b[2], (H, k // H)), ("work", want_b[3], (a.nnz, H))):
        assert _same_bits(got[key][:-pad].reshape(shape), want), key


# ---- 7. refusals

def test_the_real_library_answers_the_refusal_table_and_a_refused_row_writes_nothing():
    """Every row of tests/gatv2_entry_table.py on real plans and real tensors.  A row that expects no launch must leave every writable
    operand as it was; the valid row must write its outputs; the other launching rows run kernels that the tests above run on checked
    operands and are not launched again here.  A refused row is refused before any launch, whatever its pointers."""
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
        for row, change, code, launches in table.rows_of(name):
            if launches and row != "valid":
                assert code == table.OK, (name, row)
                continue
            handle, args = table.arguments(name, change, plans, ops)
            assert fn(handle, *args, stream) == code, (name, row)
            torch.cuda.synchronize()
            if not launches:
                assert all(bool((t[x] == SENTINEL).all()) for x in written), f"{name}, row {row}: it wrote something"
            else:
                assert all(bool((t[x][:sizes[x]] != SENTINEL).all()) for x in written), f"{name}, row {row}: an output was not written"
                for x in written:
                    t[x].fill_(SENTINEL)


# ---- 8. a row-range shard

def test_a_shard_writes_its_own_rows_and_entries_only_and_has_no_backward():
    name, k, H = "long_rows", 32, 4
    a = graph(name)
    xt, xs, att = v2.operands(v2.scenarios_of(H, shift=3), a, k, seed=9)
    whole, whole_p = _forward(plan(name, k), a, xt, xs, att)
    xtd, xsd, attd = _dev(xt), _dev(xs), _dev(att)
    s = torch.cuda.current_stream().cuda_stream
    cuts = [0, 17, 18, 18, 101, 260, a.m]
    union, union_p = np.full((a.m, k), np.float32(SENTINEL)), np.full((a.nnz, H), np.float32(SENTINEL))
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        shard = flex_amd.Plan(a, k, rows=(r0, r1), attention=True)
        shard.self_check()
        e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
        out, pd = torch.full((a.m, k), SENTINEL, device="cuda"), torch.full((a.nnz, H), SENTINEL, device="cuda")
        shard.gatv2_attention_ptr(H, xtd.data_ptr() + 4 * k * r0, xsd.data_ptr(), attd.data_ptr(), SLOPE, out.data_ptr() + 4 * k * r0, pd.data_ptr(), s)
        out, pd = _host(out), _host(pd)
        assert np.all(out[:r0] == SENTINEL) and np.all(out[r1:] == SENTINEL), (r0, r1)
        assert np.all(pd[:e0] == SENTINEL) and np.all(pd[e1:] == SENTINEL), (r0, r1)
        if r1 > r0:
            v2.check(a, xt[r0:r1], xs, att, SLOPE, out[r0:r1], pd[e0:e1], rows=(r0, r1), what=f"rows [{r0}, {r1})")
        union[r0:r1], union_p[e0:e1] = out[r0:r1], pd[e0:e1]
    assert _same_bits(union, whole) and _same_bits(union_p, whole_p)
    shard = flex_amd.Plan(a, k, rows=(17, 101), attention=True)  # a shard cannot carry FLEX_PLAN_ATTENTION_BACKWARD: the backward refuses it
    outs = [torch.full(shape, SENTINEL, device="cuda") for shape in ((a.m, k), (a.n, k), (H, k // H), (a.nnz, H), (4096,))]
    gd, pd = _dev(_grad(a, k, 9)), _dev(whole_p)
    with pytest.raises(binding.FlexError, match="invalid"):
        shard.gatv2_attention_backward_ptr(H, xtd.data_ptr(), xsd.data_ptr(), attd.data_ptr(), pd.data_ptr(), gd.data_ptr(), SLOPE,
                                           *(t.data_ptr() for t in outs), s)
    assert all(bool((_host(t) == SENTINEL).all()) for t in outs)


# ---- 9. autograd

def _float64_layer(a, xt, xs, att, slope, gOut, shared=False):
    """(Out, gXt, gXs, gAtt) of the layer in float64 torch on the CPU; shared: xt is xs, and gXs holds the sum of both gradients."""
    row, col, _ = v2.coo(a)
    H, d = att.shape
    row_t, col_t = torch.from_numpy(row.astype(np.int64)), torch.from_numpy(col.astype(np.int64))
    xs_t, att_t = (torch.from_numpy(x).double().requires_grad_() for x in (xs, att))
    xt_t = xs_t if shared else torch.from_numpy(xt).double().requires_grad_()
    s = (torch.nn.functional.leaky_relu((xt_t[row_t] + xs_t[col_t]).view(-1, H, d), float(np.float32(slope))) * att_t).sum(-1)
    M = torch.full((a.m, H), -np.inf, dtype=torch.float64).scatter_reduce(0, row_t[:, None].expand(-1, H), s.detach(), "amax")
    t = torch.exp(s - M[row_t])
    pr = t / torch.zeros((a.m, H), dtype=torch.float64).index_add_(0, row_t, t)[row_t]
    out = torch.zeros((a.m, H, d), dtype=torch.float64).index_add_(0, row_t, pr[:, :, None] * xs_t.view(a.n, H, d)[col_t]).reshape(a.m, H * d)
    out.backward(torch.from_numpy(gOut).double())
    return tuple(x.detach().numpy() for x in (out, xt_t.grad, xs_t.grad, att_t.grad))


@pytest.mark.parametrize("k,H", [(64, 8), (32, 4)])
def test_the_operator_and_its_gradients_against_float64(k, H):
    a = _directed(300, seed=6, dup=True)
    xt, xs, att = v2.operands((["uniform4", "x_zero", "spread80", "att_signs"] * 2)[:H], a, k, seed=10)
    gOut = _grad(a, k, 10)
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    xtd, xsd, attd = (_dev(x).requires_grad_() for x in (xt, xs, att))
    out = op.gatv2_attention(xtd, xsd, attd)  # the default slope: 0.2
    # another call with other values in between must not disturb the first one's backward
    other = op.gatv2_attention(_dev(xt + 1).requires_grad_(), _dev(xs * 0.5), _dev(att * 2), negative_slope=0.5)
    out.backward(_dev(gOut))
    got = tuple(_host(t) for t in (out.detach(), xtd.grad, xsd.grad, attd.grad))
    want = _float64_layer(a, xt, xs, att, 0.2, gOut)
    tols = v2.propagated_bounds(a, xt, xs, att, 0.2, gOut)
    worst = 0.0
    for what, x, ref, tol in zip(("Out", "grad_xt", "grad_xs", "grad_att"), got, want, tols):
        err = np.abs(x.astype(np.float64) - ref)
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), f"{what} k={k} H={H}: worst err / tolerance {float((err / tol).max()):.3g}"
    print(f"k={k} H={H}: worst err / tolerance {worst:.3g}")
    assert other.shape == out.shape
    with torch.no_grad():  # no gradient wanted: nothing nnz-sized is written, the same Out
        assert _same_bits(_host(op.gatv2_attention(xtd, xsd, attd)), got[0])
    # only the gradients that are needed
    ts = [_dev(x).requires_grad_(j == 2) for j, x in enumerate((xt, xs, att))]
    op.gatv2_attention(*ts).backward(_dev(gOut))
    assert ts[0].grad is None and ts[1].grad is None and _same_bits(_host(ts[2].grad), got[3])
    if a.m == a.n:  # xt is xs: autograd sums the two gradients
        x = _dev(xs).requires_grad_()
        op.gatv2_attention(x, x, _dev(att)).backward(_dev(gOut))
        ref = _float64_layer(a, None, xs, att, 0.2, gOut, shared=True)[2]
        b = v2.propagated_bounds(a, xs, xs, att, 0.2, gOut)
        assert np.all(np.abs(_host(x.grad).astype(np.float64) - ref) <= 1.001 * (b[1] + b[2] + v2.U * np.abs(ref)))


def test_the_operator_needs_both_fused_paths_and_float32():
    a, k = _directed(120, seed=9), 32
    xt, xs, att = (_dev(x) for x in v2.operands(["uniform4"] * 4, a, k, seed=11))
    for kw in (dict(), dict(learn_values=True), dict(learn_values=True, fused_attention=True)):
        with pytest.raises(NotImplementedError, match="fused_backward=True"):
            flex_amd.SparseOperator(a, k, **kw).gatv2_attention(xt, xs, att)
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    assert _same_bits(_host(op.gatv2_attention(xt, xs, att, negative_slope=0.1)), _host(op.plan.gatv2_attention(xt, xs, att, 0.1)))
    for bad in ((xt.double(), xs, att), (xt, xs.double(), att), (xt, xs, att.double()), (xt.bfloat16(), xs.bfloat16(), att)):
        with pytest.raises(TypeError, match="float32"):
            op.gatv2_attention(*bad)


# ---- 10. the census

def shipped_gatv2_kernels(so):
    """The kernel handles (data symbols, not the launchers' code) of flex::gatv2 in a built library, as `nm -C` names them without the
    outer namespace and the parameters."""
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-C", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        _, kind, sym = line.split(" ", 2)
        if kind in "tTwW" or "__device_stub__" in sym:
            continue
        head = sym.split("(", 1)[0]
        if "flex::gatv2::" in head:
            names.add(head.split("flex::", 1)[1])
    return names


def test_every_shipped_gatv2_kernel_is_launched_by_a_case_of_the_float64_test():
    so = os.path.join(os.path.dirname(binding.__file__), "lib", "libflex_spmm.so")
    shipped = shipped_gatv2_kernels(so)
    launched = {"gatv2::gatt_reduce"}
    for _, k, _ in CASES:  # a case runs the forward and the backward with every gradient wanted: all four launches in the form of its k
        W, NS = FORM_OF_K[k]
        launched |= {f"gatv2::{kern}<{W}, {NS}>" for kern in ("rows", "rows_backward", "columns_backward")}
    assert {FORM_OF_K[k] for _, k, _ in CASES} == set(FORMS)
    assert len(shipped) == 3 * len(FORMS) + 1 and shipped == launched, (sorted(shipped - launched), sorted(launched - shipped))

"""The fused GAT attention on the GPU (flex_gat_attention, flex_gat_attention_backward): Out, P, gEl, gEr, gV and dx against the float64
reference and the bounds of tests/gat_attention_ref.py on every element, with a different scenario in every head of a call, over every
(k, H) of tests/attention_forms.py's GAT table and every row and column class; against the composition of existing calls it replaces; head isolation; the
output invariants (dP = NULL, subsets of the gradients, run to run, a captured graph, sentinels, padded leading dimensions); refusals;
a row-range shard; and SparseOperator.gat_attention with its gradients against a float64 torch evaluation.

Graphs: threshold_graph() (rows of 31 / 32 / 33 and 511 / 512 / 513 entries: the slot, wave and block classes and their boundaries),
its lift both_sides() (the same classes in the COLUMNS, which the backward's second launch walks), _directed(250, 260, seed=7) (empty
rows and columns) and long_rows_graph().  The wide pairs (k >= 256) run on the two threshold graphs alone."""
import numpy as np
import pytest

import flex_amd
import gat_attention_ref as gat
from attention_forms import GAT_PAIRS as PAIRS
from backward_ref import _directed
from flex_amd import binding
from softmax_ref import long_rows_graph

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GRAPHS = {
    "thresholds": gat.threshold_graph,
    "thresholds_lifted": lambda: gat.both_sides(gat.threshold_graph()),
    "directed_empty": lambda: _directed(250, 260, seed=7),
    "long_rows": long_rows_graph,
}
CASES = [(name, k, H) for k, H in PAIRS for name in (sorted(GRAPHS) if k < 256 else ["thresholds", "thresholds_lifted"])]
SENTINEL = -12345.5
SLOPE = gat.SLOPE
_graphs, _plans = {}, {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = GRAPHS[name]()
    return _graphs[name]


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


def _forward(p, a, el, er, V, with_p=True):
    """(Out, P [nnz, H]) on the host; both start at the sentinel."""
    pd = torch.full((a.nnz, el.shape[1]), SENTINEL, device="cuda") if with_p else None
    out = torch.full((a.m, V.shape[1]), SENTINEL, device="cuda")
    p.gat_attention(_dev(el), _dev(er), _dev(V), SLOPE, out=out, p=pd)
    return _host(out), (_host(pd) if with_p else None)


def _backward(p, a, el, er, V, pr, g, want=(True, True, True)):
    """(gEl, gEr, gV, dx [nnz, H]) on the host; an output that is not wanted is None, dx is what dWork holds afterwards."""
    work = torch.full((a.nnz, el.shape[1]), SENTINEL, device="cuda")
    outs = p.gat_attention_backward(_dev(el), _dev(er), _dev(V), _dev(pr), _dev(g), SLOPE, work=work, want=want)
    return tuple(None if t is None else _host(t) for t in outs) + (_host(work),)


# ---- 1. against float64

@pytest.mark.parametrize("name,k,H", CASES)
def test_every_output_against_float64_with_a_scenario_per_head(name, k, H):
    a, p = graph(name), plan(name, k)
    names = gat.scenarios_of(H, shift=PAIRS.index((k, H)) + sorted(GRAPHS).index(name))
    el, er, V = gat.operands(names, a, k, seed=1)
    g = _grad(a, k, 1)
    out, pr = _forward(p, a, el, er, V)
    wf = gat.check(a, el, er, V, SLOPE, out, pr, what=f"{name} k={k} H={H}")
    each = {}
    wb = gat.check_backward(a, el, er, V, pr, g, SLOPE, *_backward(p, a, el, er, V, pr, g), what=f"{name} k={k} H={H}", ratios=each)
    print(f"{name} k={k} H={H} {'/'.join(names[:6])}: worst err / bound forward {wf:.3g}, backward {wb:.3g} (" + " ".join(f"{key} {v:.3g}" for key, v in each.items()) + ")")


# ---- 2. against the composition of existing calls, head by head

@pytest.mark.parametrize("name,k,H", [("thresholds_lifted", 16, 4), ("long_rows", 64, 8), ("thresholds_lifted", 512, 2)])
def test_agreement_with_the_composition_it_replaces(name, k, H):
    a, p, d = graph(name), plan(name, k), k // H
    single = flex_amd.Plan(a, d, ldb=k, ldc=k, mutable_values=True)
    single_t = flex_amd.Plan(a, d, ldb=k, ldc=k, transpose=True, mutable_values=True)
    names = gat.scenarios_of(H, shift=1)
    el, er, V = gat.operands(names, a, k, seed=3)
    g = _grad(a, k, 3)
    out, pr = _forward(p, a, el, er, V)
    mine = (out, pr) + _backward(p, a, el, er, V, pr, g)
    row, col, _ = gat.coo(a)
    rowd, cold = _dev(row), _dev(col)
    eld, erd, Vd, gd = (_dev(x) for x in (el, er, V, g))
    s = torch.cuda.current_stream().cuda_stream
    o1, gv1 = torch.zeros((a.m, k), device="cuda"), torch.zeros((a.n, k), device="cuda")
    p1, dx1, gel1, ger1 = [], [], [], []
    for h in range(H):
        off = 4 * h * d
        x = eld[rowd, h] + erd[cold, h]
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
    theirs = (_host(o1), np.stack(p1, 1), np.stack(gel1, 1), np.stack(ger1, 1), _host(gv1), np.stack(dx1, 1))
    ref, refb = gat.reference(a, el, er, V, SLOPE), gat.backward_reference(a, el, er, V, pr, g, SLOPE)
    ref2, refb2 = gat.reference(a, el, er, V, SLOPE, c_r=32), gat.backward_reference(a, el, er, V, pr, g, SLOPE, a_r=4, b_r=32)
    bounds = [x + y for x, y in ((ref["out_bound"], ref2["out_bound"]), (ref["p_bound"], ref2["p_bound"]), (refb["gel_bound"], refb2["gel_bound"]),
                                 (refb["ger_bound"], refb2["ger_bound"]), (refb["gv_bound"], refb2["gv_bound"]), (refb["dx_bound"], refb2["dx_bound"]))]
    for key, x, y, b in zip(("out", "p", "gel", "ger", "gv", "dx"), mine, theirs, bounds):
        assert np.array_equal(np.isfinite(x), np.isfinite(y)), f"{key}: the non-finite elements differ in {int((np.isfinite(x) != np.isfinite(y)).sum())} places"
        fin = np.isfinite(x) & np.isfinite(b)
        ratio = np.abs(x[fin].astype(np.float64) - y[fin]) / b[fin]
        worst = float(ratio.max()) if ratio.size else 0.0
        print(f"{name} k={k} H={H} {key}: against the composition, worst err / (sum of the two bounds) {worst:.3g}; same bits: {_same_bits(x, y)}")
        assert worst <= 1.0, f"{name} k={k} H={H} {key}: {worst:.3g}"


# ---- 3. head isolation

@pytest.mark.parametrize("k,H", [(8, 2), (48, 3), (512, 2)])
def test_what_one_head_holds_reaches_no_other_head(k, H):
    name = "thresholds_lifted"
    a, p, d = graph(name), plan(name, k), k // H
    el, er, V = gat.operands(gat.scenarios_of(H, shift=2), a, k, seed=4)
    g = _grad(a, k, 4)

    def run(el, er, V, g):
        out, pr = _forward(p, a, el, er, V)
        return (out, pr) + _backward(p, a, el, er, V, pr, g)

    base = run(el, er, V, g)
    rng = np.random.default_rng(5)
    for j in sorted({0, H - 1}):
        c = gat.head_columns(k, H, j)
        el2, er2, V2, g2 = (x.copy() for x in (el, er, V, g))
        el2[:, j] = rng.uniform(-3, 3, a.m).astype(np.float32)
        er2[:, j] = rng.uniform(-3, 3, a.n).astype(np.float32)
        el2[rng.integers(0, a.m, 3), j] = [np.nan, np.inf, -np.inf]
        er2[rng.integers(0, a.n, 3), j] = [np.nan, np.inf, -np.inf]
        for x in (V2, g2):
            x[:, c] = rng.uniform(-3, 3, (x.shape[0], d)).astype(np.float32)
            x[rng.integers(0, x.shape[0], 9), c.start + rng.integers(0, d, 9)] = [np.nan, np.inf, -np.inf] * 3
        other = run(el2, er2, V2, g2)
        keep_cols = np.ones(k, bool)
        keep_cols[c] = False
        keep_heads = np.arange(H) != j
        for key, x, y in zip(("out", "p", "gel", "ger", "gv", "dx"), base, other):
            sel = keep_cols if key in ("out", "gv") else keep_heads
            assert _same_bits(x[:, sel], y[:, sel]), f"k={k} H={H}: changing head {j} changed {key} of another head"
        assert not _same_bits(base[0][:, c], other[0][:, c])


# ---- 4. output invariants

def test_without_p_the_same_out_and_every_gradient_has_the_same_bits_whichever_others_are_asked_for():
    name, k, H = "thresholds_lifted", 48, 3
    a, p = graph(name), plan(name, k)
    el, er, V = gat.operands(["masked30", "zero", "rows_masked"], a, k, seed=6)
    g = _grad(a, k, 6)
    out, pr = _forward(p, a, el, er, V)
    assert _same_bits(_forward(p, a, el, er, V, with_p=False)[0], out)
    full = _backward(p, a, el, er, V, pr, g)
    devs = [_dev(x) for x in (el, er, V, pr, g)]
    for mask in range(8):
        want = tuple(bool(mask >> i & 1) for i in range(3))
        sent = [torch.full(shape, SENTINEL, device="cuda") for shape in ((a.m, H), (a.n, H), (a.n, k))]
        work = torch.full((a.nnz, H), SENTINEL, device="cuda")
        p.gat_attention_backward_ptr(H, *(t.data_ptr() for t in devs), SLOPE,
                                     *(t.data_ptr() if w else None for t, w in zip(sent, want)), work.data_ptr(), torch.cuda.current_stream().cuda_stream)
        for i in range(3):
            got = _host(sent[i])
            assert _same_bits(got, full[i]) if want[i] else np.all(got == SENTINEL), (want, i)
        if want[0] or want[1]:
            assert _same_bits(_host(work), full[3]), want
        else:
            assert np.all(_host(work) == SENTINEL), want  # neither gEl nor gEr: the row launch is skipped and dWork is not written


def test_two_runs_and_a_captured_graph_give_the_same_bits():
    name, k, H = "long_rows", 128, 8
    a, p = graph(name), plan(name, k)
    el, er, V = gat.operands(gat.scenarios_of(H), a, k, seed=7)
    g = _grad(a, k, 7)
    out, pr = _forward(p, a, el, er, V)
    first = (out, pr) + _backward(p, a, el, er, V, pr, g)
    out2, pr2 = _forward(p, a, el, er, V)
    again = (out2, pr2) + _backward(p, a, el, er, V, pr2, g)
    for x, y in zip(first, again):
        assert _same_bits(x, y)
    eld, erd, Vd, gd = (_dev(x) for x in (el, er, V, g))
    o, pd, work = torch.empty((a.m, k), device="cuda"), torch.empty((a.nnz, H), device="cuda"), torch.empty((a.nnz, H), device="cuda")
    gel, ger, gv = torch.empty((a.m, H), device="cuda"), torch.empty((a.n, H), device="cuda"), torch.empty((a.n, k), device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=side):  # one stream: the three launches are a chain
        p.gat_attention(eld, erd, Vd, SLOPE, out=o, p=pd)
        p.gat_attention_backward(eld, erd, Vd, pd, gd, SLOPE, grad_el=gel, grad_er=ger, grad_v=gv, work=work)
    for t in (o, pd, work, gel, ger, gv):
        t.fill_(SENTINEL)
    graph_.replay()
    for x, t in zip(first, (o, pd, gel, ger, gv, work)):
        assert _same_bits(x, _host(t))


def test_padded_leading_dimensions_and_everything_outside_the_defined_elements_keep_their_fill():
    name, k, H, ldb, ldc = "directed_empty", 16, 4, 24, 20
    a, p = graph(name), plan(name, k, ldb=ldb, ldc=ldc)
    el, er, V = gat.operands(gat.scenarios_of(H, shift=4), a, k, seed=8)
    g = _grad(a, k, 8)
    want_out, want_p = _forward(plan(name, k), a, el, er, V)
    want_b = _backward(plan(name, k), a, el, er, V, want_p, g)
    Vp, gp = torch.full((a.n, ldb), SENTINEL, device="cuda"), torch.full((a.m, ldc), SENTINEL, device="cuda")
    Vp[:, :k], gp[:, :k] = _dev(V), _dev(g)
    pad = 8  # floats of sentinel after every array
    arrays = {key: torch.full((n + pad,), SENTINEL, device="cuda") for key, n in
              (("out", a.m * ldc), ("p", a.nnz * H), ("gel", a.m * H), ("ger", a.n * H), ("gv", a.n * ldb), ("work", a.nnz * H))}
    eld, erd = _dev(el), _dev(er)
    s = torch.cuda.current_stream().cuda_stream
    p.gat_attention_ptr(H, eld.data_ptr(), erd.data_ptr(), Vp.data_ptr(), SLOPE, arrays["out"].data_ptr(), arrays["p"].data_ptr(), s)
    p.gat_attention_backward_ptr(H, eld.data_ptr(), erd.data_ptr(), Vp.data_ptr(), arrays["p"].data_ptr(), gp.data_ptr(), SLOPE,
                                 arrays["gel"].data_ptr(), arrays["ger"].data_ptr(), arrays["gv"].data_ptr(), arrays["work"].data_ptr(), s)
    got = {key: _host(t) for key, t in arrays.items()}
    for key in got:
        assert np.all(got[key][-pad:] == SENTINEL), f"{key}: written past its end"
    out, gv = got["out"][:-pad].reshape(a.m, ldc), got["gv"][:-pad].reshape(a.n, ldb)
    assert np.all(out[:, k:] == SENTINEL) and np.all(gv[:, k:] == SENTINEL), "a padded tail was written"
    assert _same_bits(out[:, :k], want_out) and _same_bits(gv[:, :k], want_b[2])
    for key, want, shape in (("p", want_p, (a.nnz, H)), ("gel", want_b[0], (a.m, H)), ("ger", want_b[1], (a.n, H)), ("work", want_b[3], (a.nnz, H))):
        assert _same_bits(got[key][:-pad].reshape(shape), want), key


# ---- 5. refusals

def test_refused_calls():
    name, k = "directed_empty", 32
    a, p = graph(name), plan(name, k)
    s = torch.cuda.current_stream().cuda_stream

    def calls(pl, H, kk, Vd=None, shift=0, same_work=False, slope=SLOPE, ldb=None, off=None):
        """(forward, backward) through the pointer forms; nothing may be launched, so every output is checked to keep its fill.
        off: "out", "g" or "gv" -- that operand is passed 4 bytes past its (16-byte aligned) start."""
        by = lambda key: 4 if off == key else 0  # noqa: E731
        h = max(H, 1)
        eld, erd = torch.zeros((a.m, h), device="cuda"), torch.zeros((a.n, h), device="cuda")
        Vd = torch.zeros((a.n, ldb or kk), device="cuda") if Vd is None else Vd
        gd = torch.zeros((a.m, kk + 4), device="cuda")
        outs = [torch.full((n,), SENTINEL, device="cuda") for n in (a.m * (kk + 4) + 4, a.m * h, a.n * h, a.n * (ldb or kk) + 4)]
        edge = [torch.full((a.nnz * h,), SENTINEL, device="cuda") for _ in range(2)]
        fwd = lambda: pl.gat_attention_ptr(H, eld.data_ptr(), erd.data_ptr(), Vd.data_ptr() + shift, slope, outs[0].data_ptr() + by("out"), edge[0].data_ptr(), s)
        bwd = lambda: pl.gat_attention_backward_ptr(H, eld.data_ptr(), erd.data_ptr(), Vd.data_ptr() + shift, edge[0].data_ptr(), gd.data_ptr() + by("g"), slope,
                                                    outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr() + by("gv"), edge[0 if same_work else 1].data_ptr(), s)
        untouched = lambda: all(bool((_host(t) == SENTINEL).all()) for t in outs + edge)
        return fwd, bwd, untouched

    def refused(pl, H, kk, match, **kw):
        fwd, bwd, untouched = calls(pl, H, kk, **kw)
        for f in (fwd, bwd):
            with pytest.raises(binding.FlexError, match=match):
                f()
        assert untouched()

    refused(p, 0, k, "invalid")
    refused(p, -2, k, "invalid")
    refused(flex_amd.Plan(a, k), 4, k, "invalid")                                 # no FLEX_PLAN_ATTENTION
    for slope in (0.0, -0.2, 1.5, float("inf"), float("nan")):
        refused(p, 4, k, "invalid", slope=slope)
    refused(p, 3, k, "not supported")                                             # 3 does not divide 32
    refused(plan(name, 24), 2, 24, "not supported")                               # d = 12
    refused(plan(name, 12), 1, 12, "not supported")                               # d = 12 with one head
    refused(plan(name, 300), 1, 300, "not supported")                             # k = 300 with one head: no single-head form here
    refused(plan(name, 1024), 2, 1024, "not supported")                           # d = 512
    refused(plan(name, k, ldb=34, ldc=36), 4, k, "not supported", ldb=34)         # ldb % 4 != 0
    refused(plan(name, k, ldb=36, ldc=34), 4, k, "not supported", ldb=36)         # ldc % 4 != 0
    big = torch.zeros(a.n * k + 4, device="cuda")
    refused(p, 4, k, "not supported", Vd=big, shift=4)                            # V offset by 4 bytes
    for off in ("out", "g", "gv"):                                                # every other row operand offset by 4 bytes, in the call that takes it
        fwd, bwd, untouched = calls(p, 4, k, off=off)
        with pytest.raises(binding.FlexError, match="not supported"):
            (fwd if off == "out" else bwd)()
        assert untouched()
    refused(plan(name, 2048), 8, 2048, "not supported")                           # k > 1024 with a legal d = 256
    refused(plan(name, 1028), 257, 1028, "not supported")                         # k > 1024 with a legal d = 4
    fwd, bwd, untouched = calls(plan(name, k, attention_backward=False), 4, k)    # the forward's flag alone
    fwd()
    with pytest.raises(binding.FlexError, match="invalid"):
        bwd()
    fwd, bwd, untouched = calls(p, 4, k, same_work=True)                          # dWork == dP
    with pytest.raises(binding.FlexError, match="invalid"):
        bwd()
    assert untouched()
    z = torch.zeros(max(a.m, a.n) * k + a.nnz * 4, device="cuda")
    full = [z.data_ptr()] * 3
    for missing in range(4):  # El, Er, V, Out
        args = [None if i == missing else z.data_ptr() for i in range(3)]
        with pytest.raises(binding.FlexError, match="invalid"):
            p.gat_attention_ptr(4, *args, SLOPE, None if missing == 3 else z.data_ptr(), None, s)
    w = torch.zeros(a.nnz * 4, device="cuda")
    for missing in range(6):  # El, Er, V, P, GradOut, Work
        args = [None if i == missing else z.data_ptr() for i in range(5)]
        with pytest.raises(binding.FlexError, match="invalid"):
            p.gat_attention_backward_ptr(4, *args, SLOPE, *full, None if missing == 5 else w.data_ptr(), s)
    assert bool((z == 0).all()) and bool((w == 0).all())
    empty = binding.HostCsr(np.zeros(41, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=17)
    pe = flex_amd.Plan(empty, k, attention=True, attention_backward=True)
    pe.gat_attention_ptr(4, None, None, None, SLOPE, None)  # no entries: no launch, nothing read
    pe.gat_attention_backward_ptr(4, None, None, None, None, None, SLOPE, None, None, None, None)


# ---- 6. a row-range shard

def test_a_shard_writes_its_own_rows_and_entries_only_and_has_no_backward():
    name, k, H = "long_rows", 32, 4
    a = graph(name)
    el, er, V = gat.operands(gat.scenarios_of(H, shift=3), a, k, seed=9)
    whole, whole_p = _forward(plan(name, k), a, el, er, V)
    eld, erd, Vd = _dev(el), _dev(er), _dev(V)
    s = torch.cuda.current_stream().cuda_stream
    cuts = [0, 17, 18, 18, 101, 260, a.m]
    union, union_p = np.full((a.m, k), np.float32(SENTINEL)), np.full((a.nnz, H), np.float32(SENTINEL))
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        shard = flex_amd.Plan(a, k, rows=(r0, r1), attention=True)
        shard.self_check()
        e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
        out, pd = torch.full((a.m, k), SENTINEL, device="cuda"), torch.full((a.nnz, H), SENTINEL, device="cuda")
        shard.gat_attention_ptr(H, eld.data_ptr() + 4 * H * r0, erd.data_ptr(), Vd.data_ptr(), SLOPE, out.data_ptr() + 4 * k * r0, pd.data_ptr(), s)
        out, pd = _host(out), _host(pd)
        assert np.all(out[:r0] == SENTINEL) and np.all(out[r1:] == SENTINEL), (r0, r1)
        assert np.all(pd[:e0] == SENTINEL) and np.all(pd[e1:] == SENTINEL), (r0, r1)
        if r1 > r0:
            gat.check(a, el[r0:r1], er, V, SLOPE, out[r0:r1], pd[e0:e1], rows=(r0, r1), what=f"rows [{r0}, {r1})")
        union[r0:r1], union_p[e0:e1] = out[r0:r1], pd[e0:e1]
    assert _same_bits(union, whole) and _same_bits(union_p, whole_p)
    # as flex_attention_heads_backward: a shard cannot carry FLEX_PLAN_ATTENTION_BACKWARD, so the backward refuses it and writes nothing
    with pytest.raises(binding.FlexError, match="not supported"):
        flex_amd.Plan(a, k, rows=(17, 101), attention=True, attention_backward=True)
    shard = flex_amd.Plan(a, k, rows=(17, 101), attention=True)
    outs = [torch.full(shape, SENTINEL, device="cuda") for shape in ((a.m, H), (a.n, H), (a.n, k), (a.nnz, H))]
    gd, pd = _dev(_grad(a, k, 9)), _dev(whole_p)
    with pytest.raises(binding.FlexError, match="invalid"):
        shard.gat_attention_backward_ptr(H, eld.data_ptr(), erd.data_ptr(), Vd.data_ptr(), pd.data_ptr(), gd.data_ptr(), SLOPE, *(t.data_ptr() for t in outs), s)
    assert all(bool((_host(t) == SENTINEL).all()) for t in outs)


# ---- 7. autograd

def _float64_layer(a, el, er, V, slope, gOut):
    """(Out, gEl, gEr, gV) of the layer in float64 torch on the CPU."""
    row, col, _ = gat.coo(a)
    H, k = el.shape[1], V.shape[1]
    row_t, col_t = torch.from_numpy(row), torch.from_numpy(col)
    el_t, er_t, V_t = (torch.from_numpy(x).double().requires_grad_() for x in (el, er, V))
    s = torch.nn.functional.leaky_relu(el_t[row_t] + er_t[col_t], float(np.float32(slope)))
    M = torch.full((a.m, H), -np.inf, dtype=torch.float64).scatter_reduce(0, row_t[:, None].expand(-1, H), s.detach(), "amax")
    t = torch.exp(s - M[row_t])
    pr = t / torch.zeros((a.m, H), dtype=torch.float64).index_add_(0, row_t, t)[row_t]
    out = torch.zeros((a.m, H, k // H), dtype=torch.float64).index_add_(0, row_t, pr[:, :, None] * V_t.view(a.n, H, k // H)[col_t]).reshape(a.m, k)
    out.backward(torch.from_numpy(gOut).double())
    return tuple(x.detach().numpy() for x in (out, el_t.grad, er_t.grad, V_t.grad))


@pytest.mark.parametrize("k,H", [(64, 8), (32, 4)])
def test_the_operator_and_its_gradients_against_float64(k, H):
    a = _directed(300, seed=6, dup=True)
    el, er, V = gat.operands((["uniform4", "zero", "spread80"] * 3)[:H], a, k, seed=10)
    gOut = _grad(a, k, 10)
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    eld, erd, Vd = (_dev(x).requires_grad_() for x in (el, er, V))
    out = op.gat_attention(eld, erd, Vd)  # the default slope: 0.2
    # another call with other values in between must not disturb the first one's backward
    other = op.gat_attention(_dev(el + 1).requires_grad_(), _dev(er * 0.5), _dev(V * 2), negative_slope=0.5)
    out.backward(_dev(gOut))
    got = tuple(_host(t) for t in (out.detach(), eld.grad, erd.grad, Vd.grad))
    want = _float64_layer(a, el, er, V, 0.2, gOut)
    tols = gat.propagated_bounds(a, el, er, V, 0.2, gOut)
    worst = 0.0
    for what, x, ref, tol in zip(("Out", "grad_el", "grad_er", "grad_V"), got, want, tols):
        err = np.abs(x.astype(np.float64) - ref)
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), f"{what} k={k} H={H}: worst err / tolerance {float((err / tol).max()):.3g}"
    print(f"k={k} H={H}: worst err / tolerance {worst:.3g}")
    assert other.shape == out.shape
    with torch.no_grad():  # no gradient wanted: nothing nnz-sized is written, the same Out
        assert _same_bits(_host(op.gat_attention(eld, erd, Vd)), got[0])
    # only the gradients that are needed
    ts = [_dev(x).requires_grad_(j == 1) for j, x in enumerate((el, er, V))]
    op.gat_attention(*ts).backward(_dev(gOut))
    assert ts[0].grad is None and ts[2].grad is None and _same_bits(_host(ts[1].grad), got[2])


def test_the_operator_needs_both_fused_paths():
    a, k = _directed(120, seed=9), 32
    el, er, V = (_dev(x) for x in gat.operands(["uniform4"] * 4, a, k, seed=11))
    for kw in (dict(), dict(learn_values=True), dict(learn_values=True, fused_attention=True)):
        with pytest.raises(NotImplementedError, match="fused_backward=True"):
            flex_amd.SparseOperator(a, k, **kw).gat_attention(el, er, V)
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    assert _same_bits(_host(op.gat_attention(el, er, V, negative_slope=0.1)), _host(op.plan.gat_attention(el, er, V, 0.1)))

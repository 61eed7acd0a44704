"""The multi-head fused attention on the GPU (flex_attention_heads, flex_attention_heads_backward): Out, P, gQ, gK, gV and ds against the
stacked float64 reference and the per-head bounds of tests/multihead_attention_ref.py on every element, with a different score scenario
in every head of a call, over every (k, H) of tests/attention_forms.py's table and every row and column class; heads = 1 through the new entry points
against flex_attention / flex_attention_backward bit for bit; against H single-head calls on a strided plan; head isolation; the output
invariants (dP = NULL, subsets of the gradients, run to run, a captured graph); refusals; a row-range shard; and
SparseOperator.attention(..., heads=H) with its gradients against a float64 torch evaluation.

Graphs: threshold_graph() (rows of 31 / 32 / 33 and 511 / 512 / 513 entries: the slot, wave and block classes and their boundaries),
its lift both_sides() (the same classes in the COLUMNS, which the backward's second launch walks), _directed(250, 260, seed=7) (empty
rows and columns) and long_rows_graph().  The wide pairs (k >= 256) run on the two threshold graphs alone."""
import numpy as np
import pytest

import flex_amd
import multihead_attention_ref as mh
from attention_forms import HEADS_PAIRS as PAIRS
import test_gpu_attention as composition
from backward_ref import _directed
from flex_amd import binding
from fused_attention_backward_ref import both_sides
from fused_attention_ref import coo, threshold_graph
from softmax_ref import long_rows_graph

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GRAPHS = {
    "thresholds": threshold_graph,
    "thresholds_lifted": lambda: both_sides(threshold_graph()),
    "directed_empty": lambda: _directed(250, 260, seed=7),
    "long_rows": long_rows_graph,
}
CASES = [(name, k, H) for k, H in PAIRS for name in (sorted(GRAPHS) if k < 256 else ["thresholds", "thresholds_lifted"])]
SENTINEL = -12345.5
SCALE = 0.25
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


def _forward(p, a, Q, K, V, H, scale=SCALE, with_p=True):
    """(Out, P [nnz, H]) on the host; P starts at the sentinel."""
    pd = torch.full((a.nnz, H), SENTINEL, device="cuda") if with_p else None
    out = p.attention(_dev(Q), _dev(K), _dev(V), scale, p=pd, heads=H)
    return _host(out), (_host(pd) if with_p else None)


def _backward(p, a, Q, K, V, pr, g, H, scale=SCALE, want=(True, True, True)):
    """(gQ, gK, gV, ds [nnz, H]) on the host; an output that is not wanted is None, ds is what dWork holds afterwards."""
    work = torch.full((a.nnz, H), SENTINEL, device="cuda")
    outs = p.attention_backward(_dev(Q), _dev(K), _dev(V), _dev(pr), _dev(g), scale, work=work, want=want, heads=H)
    return tuple(None if t is None else _host(t) for t in outs) + (_host(work),)


# ---- 1. against float64

@pytest.mark.parametrize("name,k,H", CASES)
def test_every_output_against_float64_with_a_scenario_per_head(name, k, H):
    a, p = graph(name), plan(name, k)
    names = mh.scenarios_of(H, shift=PAIRS.index((k, H)) + sorted(GRAPHS).index(name))
    Q, K, V = mh.operands(names, a, k, seed=1)
    g = _grad(a, k, 1)
    out, pr = _forward(p, a, Q, K, V, H)
    wf = mh.check(a, Q, K, V, SCALE, H, out, pr, what=f"{name} k={k} H={H}")
    each = {}
    wb = mh.check_backward(a, Q, K, V, pr, g, SCALE, H, *_backward(p, a, Q, K, V, pr, g, H), what=f"{name} k={k} H={H}", ratios=each)
    print(f"{name} k={k} H={H} {'/'.join(names[:5])}: worst err / bound forward {wf:.3g}, backward {wb:.3g} (" + " ".join(f"{key} {v:.3g}" for key, v in each.items()) + ")")


# ---- 2. heads = 1 is the single-head call

@pytest.mark.parametrize("k", [30, 32, 300])
def test_one_head_through_the_new_entry_points_is_the_single_head_call_bit_for_bit(k):
    name = "thresholds_lifted"
    a, p = graph(name), plan(name, k)
    Q, K, V = mh.operands(["masked30"], a, k, seed=2)
    g = _grad(a, k, 2)
    Qd, Kd, Vd, gd = (_dev(x) for x in (Q, K, V, g))
    s = torch.cuda.current_stream().cuda_stream
    out1, p1 = torch.empty((a.m, k), device="cuda"), torch.full((a.nnz,), SENTINEL, device="cuda")
    p.attention(Qd, Kd, Vd, SCALE, out=out1, p=p1)
    outh, ph = torch.empty((a.m, k), device="cuda"), torch.full((a.nnz,), SENTINEL, device="cuda")
    p.attention_ptr(Qd.data_ptr(), Kd.data_ptr(), Vd.data_ptr(), SCALE, outh.data_ptr(), ph.data_ptr(), s, heads=1)
    assert _same_bits(_host(out1), _host(outh)) and _same_bits(_host(p1), _host(ph))
    work1 = torch.full((a.nnz,), SENTINEL, device="cuda")
    want = p.attention_backward(Qd, Kd, Vd, p1, gd, SCALE, work=work1)
    got = [torch.empty_like(t) for t in want]
    workh = torch.full((a.nnz,), SENTINEL, device="cuda")
    p.attention_backward_ptr(Qd.data_ptr(), Kd.data_ptr(), Vd.data_ptr(), p1.data_ptr(), gd.data_ptr(), SCALE,
                             *(t.data_ptr() for t in got), workh.data_ptr(), s, heads=1)
    for x, y in zip(list(want) + [work1], got + [workh]):
        assert _same_bits(_host(x), _host(y))
    # and through the tensor forms, where heads=1 takes flex_attention itself
    assert _same_bits(_host(p.attention(Qd, Kd, Vd, SCALE, heads=1)), _host(out1))


# ---- 3. against H single-head calls on a strided plan

@pytest.mark.parametrize("name,k,H", [("thresholds_lifted", 16, 4), ("thresholds_lifted", 48, 3), ("long_rows", 64, 4), ("directed_empty", 128, 8),
                                      ("thresholds_lifted", 512, 4)])
def test_agreement_with_a_loop_of_single_head_calls_on_a_strided_plan(name, k, H):
    a, p, d = graph(name), plan(name, k), k // H
    single = plan(name, d, ldb=k, ldc=k)
    names = mh.scenarios_of(H, shift=1)
    Q, K, V = mh.operands(names, a, k, seed=3)
    g = _grad(a, k, 3)
    out, pr = _forward(p, a, Q, K, V, H)
    mine = (out, pr) + _backward(p, a, Q, K, V, pr, g, H)
    Qd, Kd, Vd, gd = (_dev(x) for x in (Q, K, V, g))
    s = torch.cuda.current_stream().cuda_stream
    o1 = torch.empty((a.m, k), device="cuda")
    grads = [torch.empty((r, k), device="cuda") for r in (a.m, a.n, a.n)]
    p1, w1 = [], []
    for h in range(H):
        off = 4 * h * d
        ph, wh = torch.zeros(a.nnz, device="cuda"), torch.empty(a.nnz, device="cuda")
        single.attention_ptr(Qd.data_ptr() + off, Kd.data_ptr() + off, Vd.data_ptr() + off, SCALE, o1.data_ptr() + off, ph.data_ptr(), s)
        pin = _dev(pr[:, h])  # the backward of both sides starts from the same probabilities
        single.attention_backward_ptr(Qd.data_ptr() + off, Kd.data_ptr() + off, Vd.data_ptr() + off, pin.data_ptr(), gd.data_ptr() + off, SCALE,
                                      *(t.data_ptr() + off for t in grads), wh.data_ptr(), s)
        p1.append(_host(ph))
        w1.append(_host(wh))
    theirs = (_host(o1), np.stack(p1, 1), *(_host(t) for t in grads), np.stack(w1, 1))
    ref, refb = mh.reference(a, Q, K, V, SCALE, H), mh.backward_reference(a, Q, K, V, pr, g, SCALE, H)
    bounds = (ref["out_bound"], ref["p_bound"], refb["gq_bound"], refb["gk_bound"], refb["gv_bound"], refb["ds_bound"])
    for key, x, y, b in zip(("out", "p", "gq", "gk", "gv", "ds"), mine, theirs, bounds):
        assert np.array_equal(np.isfinite(x), np.isfinite(y)), f"{key}: the non-finite elements differ in {int((np.isfinite(x) != np.isfinite(y)).sum())} places"
        fin = np.isfinite(x) & np.isfinite(b)
        ratio = np.abs(x[fin].astype(np.float64) - y[fin]) / (2.0 * b[fin])
        worst = float(ratio.max()) if ratio.size else 0.0
        print(f"{name} k={k} H={H} {key}: against {H} single-head calls, worst err / (sum of the two bounds) {worst:.3g}; same bits: {_same_bits(x, y)}")
        assert worst <= 1.0, f"{name} k={k} H={H} {key}: {worst:.3g}"


# ---- 4. head isolation

@pytest.mark.parametrize("k,H", [(32, 4), (48, 3), (512, 4)])
def test_what_one_head_holds_reaches_no_other_head(k, H):
    name = "thresholds_lifted"
    a, p, d = graph(name), plan(name, k), k // H
    Q, K, V = mh.operands(mh.scenarios_of(H, shift=2), a, k, seed=4)
    g = _grad(a, k, 4)

    def run(Q, K, V, g):
        out, pr = _forward(p, a, Q, K, V, H)
        return (out, pr) + _backward(p, a, Q, K, V, pr, g, H)

    base = run(Q, K, V, g)
    rng = np.random.default_rng(5)
    for j in sorted({0, H // 2, H - 1}):
        c = mh.head_columns(k, H, j)
        Q2, K2, V2, g2 = (x.copy() for x in (Q, K, V, g))
        for x in (Q2, K2, V2, g2):
            x[:, c] = rng.uniform(-3, 3, (x.shape[0], d)).astype(np.float32)
            x[rng.integers(0, x.shape[0], 9), c.start + rng.integers(0, d, 9)] = [np.nan, np.inf, -np.inf] * 3
        other = run(Q2, K2, V2, g2)
        keep_cols = np.ones(k, bool)
        keep_cols[c] = False
        keep_heads = np.arange(H) != j
        for key, x, y in zip(("out", "p", "gq", "gk", "gv", "ds"), base, other):
            sel = keep_heads if key in ("p", "ds") else keep_cols
            assert _same_bits(x[:, sel], y[:, sel]), f"k={k} H={H}: changing head {j} changed {key} of another head"
        assert not _same_bits(base[0][:, c], other[0][:, c])


# ---- 5. output invariants

def test_without_p_the_same_out_and_every_gradient_has_the_same_bits_whichever_others_are_asked_for():
    name, k, H = "thresholds_lifted", 48, 3
    a, p = graph(name), plan(name, k)
    Q, K, V = mh.operands(["masked30", "uniform4", "rows_masked"], a, k, seed=6)
    g = _grad(a, k, 6)
    out, pr = _forward(p, a, Q, K, V, H)
    assert _same_bits(_forward(p, a, Q, K, V, H, with_p=False)[0], out)
    full = _backward(p, a, Q, K, V, pr, g, H)
    for mask in range(7):
        want = tuple(bool(mask >> i & 1) for i in range(3))
        got = _backward(p, a, Q, K, V, pr, g, H, want=want)
        for i in range(3):
            assert (got[i] is None) if not want[i] else _same_bits(got[i], full[i]), (want, i)
        if want[0] or want[1]:
            assert _same_bits(got[3], full[3]), want
        else:
            assert np.all(got[3] == SENTINEL), want  # neither gQ nor gK: the row launch is skipped and dWork is not written


def test_two_runs_and_a_captured_graph_give_the_same_bits():
    name, k, H = "long_rows", 128, 8
    a, p = graph(name), plan(name, k)
    Q, K, V = mh.operands(mh.scenarios_of(H), a, k, seed=7)
    g = _grad(a, k, 7)
    out, pr = _forward(p, a, Q, K, V, H)
    first = (out, pr) + _backward(p, a, Q, K, V, pr, g, H)
    out2, pr2 = _forward(p, a, Q, K, V, H)
    again = (out2, pr2) + _backward(p, a, Q, K, V, pr2, g, H)
    for x, y in zip(first, again):
        assert _same_bits(x, y)
    Qd, Kd, Vd, gd = (_dev(x) for x in (Q, K, V, g))
    o, pd, work = torch.empty((a.m, k), device="cuda"), torch.empty((a.nnz, H), device="cuda"), torch.empty((a.nnz, H), device="cuda")
    gq, gk, gv = torch.empty((a.m, k), device="cuda"), torch.empty((a.n, k), device="cuda"), torch.empty((a.n, k), device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=side):  # one stream: the three launches are a chain
        p.attention(Qd, Kd, Vd, SCALE, out=o, p=pd, heads=H)
        p.attention_backward(Qd, Kd, Vd, pd, gd, SCALE, grad_q=gq, grad_k=gk, grad_v=gv, work=work, heads=H)
    for t in (o, pd, work, gq, gk, gv):
        t.fill_(SENTINEL)
    graph_.replay()
    for x, t in zip(first, (o, pd, gq, gk, gv, work)):
        assert _same_bits(x, _host(t))


# ---- 6. refusals

def test_refused_calls():
    name, k = "directed_empty", 32
    a, p = graph(name), plan(name, k)
    Q, K, V = (_dev(x) for x in mh.operands(["uniform4"], a, k))
    g = _dev(_grad(a, k, 8))
    s = torch.cuda.current_stream().cuda_stream

    def calls(pl, H, kk, Qd=None, shift=0, same_work=False):
        """(forward, backward) through the pointer forms; nothing may be launched, so every output is checked to keep its fill."""
        Qd = torch.zeros((a.m, kk), device="cuda") if Qd is None else Qd
        Kd, Vd, gd = torch.zeros((a.n, kk), device="cuda"), torch.zeros((a.n, kk), device="cuda"), torch.zeros((a.m, kk), device="cuda")
        outs = [torch.full((r * kk + 4,), SENTINEL, device="cuda") for r in (a.m, a.m, a.n, a.n)]
        edge = [torch.full((a.nnz * max(H, 1),), SENTINEL, device="cuda") for _ in range(2)]
        fwd = lambda: pl.attention_ptr(Qd.data_ptr() + shift, Kd.data_ptr(), Vd.data_ptr(), SCALE, outs[0].data_ptr(), edge[0].data_ptr(), s, heads=H)
        bwd = lambda: pl.attention_backward_ptr(Qd.data_ptr() + shift, Kd.data_ptr(), Vd.data_ptr(), edge[0].data_ptr(), gd.data_ptr(), SCALE,
                                                *(t.data_ptr() for t in outs[1:]), edge[0 if same_work else 1].data_ptr(), s, heads=H)
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
    refused(p, 3, k, "not supported")                                             # 3 does not divide 32
    refused(plan(name, 24), 2, 24, "not supported")                               # d = 12
    refused(plan(name, 1024), 2, 1024, "not supported")                           # d = 512
    refused(plan(name, k, ldb=34, ldc=36), 4, 36, "not supported")                # ldb % 4 != 0
    big = torch.zeros(a.m * k + 4, device="cuda")
    refused(p, 4, k, "not supported", Qd=big, shift=4)                            # Q offset by 4 bytes
    refused(flex_amd.Plan(a, k), 4, k, "invalid")                                 # no FLEX_PLAN_ATTENTION
    fwd, bwd, untouched = calls(plan(name, k, attention_backward=False), 4, k)    # the forward's flag alone
    fwd()
    with pytest.raises(binding.FlexError, match="invalid"):
        bwd()
    fwd, bwd, untouched = calls(p, 4, k, same_work=True)                          # dWork == dP
    with pytest.raises(binding.FlexError, match="invalid"):
        bwd()
    assert untouched()
    pd = torch.zeros((a.nnz, 4), device="cuda")
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(binding.FlexError, match="invalid"):
            p.attention(Q, K, V, scale, heads=4)
        with pytest.raises(binding.FlexError, match="invalid"):
            p.attention_backward(Q, K, V, pd, g, scale, heads=4)
    with pytest.raises(binding.FlexError, match="invalid"):
        p.attention_ptr(None, K.data_ptr(), V.data_ptr(), SCALE, g.data_ptr(), None, s, heads=4)
    empty = binding.HostCsr(np.zeros(41, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=17)
    pe = flex_amd.Plan(empty, k, attention=True, attention_backward=True)
    pe.attention_ptr(None, None, None, 1.0, None, heads=4)  # no entries: no launch, nothing read
    pe.attention_backward_ptr(None, None, None, None, None, 1.0, None, None, None, None, heads=4)


# ---- 7. a row-range shard, forward

def test_a_shard_writes_its_own_rows_and_entries_only():
    name, k, H = "long_rows", 32, 4
    a = graph(name)
    Q, K, V = mh.operands(mh.scenarios_of(H, shift=3), a, k, seed=9)
    whole, whole_p = _forward(plan(name, k), a, Q, K, V, H)
    Qd, Kd, Vd = _dev(Q), _dev(K), _dev(V)
    s = torch.cuda.current_stream().cuda_stream
    cuts = [0, 17, 18, 18, 101, 260, a.m]
    union, union_p = np.full((a.m, k), np.float32(SENTINEL)), np.full((a.nnz, H), np.float32(SENTINEL))
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        shard = flex_amd.Plan(a, k, rows=(r0, r1), attention=True)
        shard.self_check()
        e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
        out, pd = torch.full((a.m, k), SENTINEL, device="cuda"), torch.full((a.nnz, H), SENTINEL, device="cuda")
        shard.attention_ptr(Qd.data_ptr() + 4 * k * r0, Kd.data_ptr(), Vd.data_ptr(), SCALE, out.data_ptr() + 4 * k * r0, pd.data_ptr(), s, heads=H)
        out, pd = _host(out), _host(pd)
        assert np.all(out[:r0] == SENTINEL) and np.all(out[r1:] == SENTINEL), (r0, r1)
        assert np.all(pd[:e0] == SENTINEL) and np.all(pd[e1:] == SENTINEL), (r0, r1)
        if r1 > r0:
            mh.check(a, Q[r0:r1], K, V, SCALE, H, out[r0:r1], pd[e0:e1], rows=(r0, r1), what=f"rows [{r0}, {r1})")
        union[r0:r1], union_p[e0:e1] = out[r0:r1], pd[e0:e1]
    assert _same_bits(union, whole) and _same_bits(union_p, whole_p)


# ---- 8. autograd

@pytest.mark.parametrize("k,H", [(32, 4), (128, 8)])
def test_the_operator_with_heads_and_its_gradients_against_float64(k, H):
    from test_gpu_fused_attention_backward import _fused_backward_tolerances
    a = _directed(300, seed=6, dup=True)
    d = k // H
    rng = np.random.default_rng([k, H, 23])
    Q, K, V = (rng.uniform(-1, 1, (r, k)).astype(np.float32) for r in (a.m, a.n, a.n))
    gOut = rng.uniform(-1, 1, (a.m, k)).astype(np.float32)
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    Qd, Kd, Vd = (_dev(x).requires_grad_() for x in (Q, K, V))
    out = op.attention(Qd, Kd, Vd, heads=H)  # the default scale: d ** -0.5
    out.backward(_dev(gOut))
    got = tuple(_host(t) for t in (out.detach(), Qd.grad, Kd.grad, Vd.grad))
    scale = d ** -0.5
    worst = 0.0
    for h in range(H):
        c = mh.head_columns(k, H, h)
        want = composition._attention_f64(a, Q[:, c], K[:, c], V[:, c], scale, gOut[:, c])
        tols = _fused_backward_tolerances(a, Q[:, c], K[:, c], V[:, c], scale, gOut[:, c], want[5])
        for what, x, ref, tol in zip(("Out", "grad_Q", "grad_K", "grad_V"), got, want[:4], tols):
            err = np.abs(x[:, c].astype(np.float64) - ref)
            worst = max(worst, float((err / tol).max()))
            assert np.all(err <= tol), f"{what} k={k} H={H} head {h}: worst err / tolerance {float((err / tol).max()):.3g}"
    print(f"k={k} H={H}: worst err / tolerance {worst:.3g}")
    with torch.no_grad():  # no gradient wanted: nothing nnz-sized is written, the same Out
        assert _same_bits(_host(op.attention(Qd, Kd, Vd, heads=H)), got[0])
    # only the gradients that are needed
    ts = [_dev(x).requires_grad_(j == 1) for j, x in enumerate((Q, K, V))]
    op.attention(*ts, heads=H).backward(_dev(gOut))
    assert ts[0].grad is None and ts[2].grad is None and _same_bits(_host(ts[1].grad), got[2])


def test_heads_need_both_fused_paths_and_one_head_takes_the_paths_it_took():
    a, k = _directed(120, seed=9), 32
    Q, K, V = (_dev(x) for x in mh.operands(["uniform4"], a, k, seed=10))
    for kw in (dict(), dict(fused_attention=True)):
        op = flex_amd.SparseOperator(a, k, learn_values=True, **kw)
        with pytest.raises(NotImplementedError, match="fused_backward=True"):
            op.attention(Q, K, V, heads=4)
        assert _same_bits(_host(op.attention(Q, K, V, heads=1)), _host(op.attention(Q, K, V)))
    with pytest.raises(NotImplementedError, match="learn_values"):
        flex_amd.SparseOperator(a, k).attention(Q, K, V, heads=4)
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    with pytest.raises(ValueError):
        op.attention(Q, K, V, heads=0)
    with pytest.raises(binding.FlexError, match="not supported"):
        op.attention(Q, K, V, heads=3)
    assert _same_bits(_host(op.attention(Q, K, V, heads=1)), _host(op.attention(Q, K, V)))  # default scale k ** -0.5 either way
    want = op.plan.attention(Q, K, V, 8 ** -0.5, heads=4)
    assert _same_bits(_host(op.attention(Q, K, V, heads=4)), _host(want))

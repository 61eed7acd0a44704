"""Sparse graph attention on the GPU: flex_edge_softmax and flex_edge_softmax_backward against the float64 reference of
tests/softmax_ref.py on every entry (bounds and exact classes as include/flex_spmm.h states them), on every kind of plan, in place,
run to run and inside a captured graph; and SparseOperator.attention with its gradients against a float64 torch evaluation."""
import os

import numpy as np
import pytest

import flex_amd
from attention_walk_graphs import walk_graph
from backward_ref import _directed
from conftest import GOLDEN
from f64ref import scenario
from flex_amd import binding
from softmax_ref import (SCALES, SCORE_SCENARIOS, U, boundary_graph, check_backward, check_forward, forward_ref, gamma, long_rows_graph,
                         scores)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GRAPHS = {
    "pubmed": lambda: flex_amd.csv_load(os.path.join(GOLDEN, "pubmed.csv")),
    "directed_dups": lambda: _directed(300, seed=6, dup=True),
    "directed_empty": lambda: _directed(250, 260, seed=7),
    "long_rows": long_rows_graph,
    "rows_256_257": boundary_graph,
    "wide_512": lambda: scenario("wide", k=32, m=512)[0],
    "wide_3000": lambda: scenario("wide", k=32, m=3000)[0],
    "walk_7_copies": lambda: walk_graph(7),
}
# flex_plan_softmax_info's group budget (group_entries): every graph above plans at the floor of 256 but the last, 7 copies of
# tests/attention_walk_graphs.py's graph (490 000 rows, 1 495 606 entries), where a group holds two items on average
GROUP_ENTRIES = {"walk_7_copies": 512}
_cache = {}


def graph_and_plan(name):
    if name not in _cache:
        a = GRAPHS[name]()
        _cache[name] = (a, flex_amd.Plan(a, 32, mutable_values=True))
    return _cache[name]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same_bits(x, y):
    return bool(np.array_equal(np.asarray(x, np.float32).view(np.uint32), np.asarray(y, np.float32).view(np.uint32)))


def _grad(nnz, seed):
    return np.random.default_rng([seed, 9]).uniform(-2, 2, nnz).astype(np.float32)


@pytest.mark.parametrize("graph", sorted(GRAPHS))
@pytest.mark.parametrize("name", SCORE_SCENARIOS)
def test_forward_and_backward_against_float64(graph, name):
    a, plan = graph_and_plan(graph)
    assert plan.softmax_info()["group_entries"] == GROUP_ENTRIES.get(graph, 256)
    s = scores(name, a.rowPtr, seed=1)
    g = _grad(a.nnz, 2)
    sd, gd = _dev(s), _dev(g)
    for scale in SCALES:
        what = f"{graph} {name} scale {scale:.4g}"
        p = _host(plan.edge_softmax(sd, scale))
        wf = check_forward(a.rowPtr, s, scale, p, what)
        gs = _host(plan.edge_softmax_backward(_dev(p), gd, scale))
        wb = check_backward(a.rowPtr, p, g, scale, gs, what)
        print(f"{what}: worst err / bound forward {wf:.3g} backward {wb:.3g}")


@pytest.mark.parametrize("graph", ["directed_dups", "long_rows", "rows_256_257", "pubmed"])
def test_the_transposed_plan_gives_the_same_bits(graph):
    a, plan = graph_and_plan(graph)
    t = flex_amd.Plan(a, 32, transpose=True, mutable_values=True)
    for name in ("spread80", "poisoned"):
        s, g = _dev(scores(name, a.rowPtr, seed=4)), _dev(_grad(a.nnz, 5))
        p, pt = plan.edge_softmax(s, 0.125), t.edge_softmax(s, 0.125)
        assert _same_bits(_host(p), _host(pt))
        assert _same_bits(_host(plan.edge_softmax_backward(p, g, 0.125)), _host(t.edge_softmax_backward(pt, g, 0.125)))


def test_a_mapped_plan_works_in_the_order_of_the_reordered_csr():
    a = scenario("wide", k=32, m=3000)[0]
    vo, ap = flex_amd.perm_csr(a, flex_amd.order_rcm(a))
    plan = flex_amd.Plan(ap, 32, vo_mp=vo, mutable_values=True)
    s, g = scores("masked30", ap.rowPtr, seed=6), _grad(ap.nnz, 7)
    p = _host(plan.edge_softmax(_dev(s), 1.0))
    check_forward(ap.rowPtr, s, 1.0, p, "mapped")
    check_backward(ap.rowPtr, p, g, 1.0, _host(plan.edge_softmax_backward(_dev(p), _dev(g), 1.0)), "mapped")


def test_shards_write_their_own_rows_only_and_their_union_is_the_unsharded_result():
    a, plan = graph_and_plan("long_rows")
    s, g = scores("rows_masked", a.rowPtr, seed=8), _grad(a.nnz, 9)
    sd, gd = _dev(s), _dev(g)
    whole_p = plan.edge_softmax(sd, 0.125)
    whole_gs = _host(plan.edge_softmax_backward(whole_p, gd, 0.125))
    whole_p = _host(whole_p)
    cuts = [0, 17, 18, 101, 260, a.m]
    sentinel = np.float32(-12345.5)
    union_p, union_gs = np.full(a.nnz, sentinel), np.full(a.nnz, sentinel)
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        shard = flex_amd.Plan(a, 32, rows=(r0, r1), mutable_values=True)
        e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
        out = torch.full((a.nnz,), float(sentinel), device="cuda")
        p = _host(shard.edge_softmax(sd, 0.125, out=out))
        assert np.all(p[:e0] == sentinel) and np.all(p[e1:] == sentinel), (r0, r1)
        out2 = torch.full((a.nnz,), float(sentinel), device="cuda")
        gs = _host(shard.edge_softmax_backward(_dev(whole_p), gd, 0.125, out=out2))
        assert np.all(gs[:e0] == sentinel) and np.all(gs[e1:] == sentinel), (r0, r1)
        union_p[e0:e1], union_gs[e0:e1] = p[e0:e1], gs[e0:e1]
        t = flex_amd.Plan(a, 32, rows=(r0, min(r1, a.n)), transpose=True, mutable_values=True)
        with pytest.raises(binding.FlexError, match="not supported"):
            t.edge_softmax(sd, 0.125)
        with pytest.raises(binding.FlexError, match="not supported"):
            t.edge_softmax_backward(sd, gd, 0.125)
    assert _same_bits(union_p, whole_p) and _same_bits(union_gs, whole_gs)


def test_refused_calls():
    a, plan = graph_and_plan("directed_dups")
    s = _dev(scores("uniform4", a.rowPtr))
    plain = flex_amd.Plan(a, 32)
    with pytest.raises(binding.FlexError, match="invalid"):
        plain.edge_softmax(s)
    with pytest.raises(binding.FlexError, match="invalid"):
        plain.edge_softmax_backward(s, s)
    with pytest.raises(binding.FlexError, match="invalid"):
        plain.softmax_info()
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(binding.FlexError, match="invalid"):
            plan.edge_softmax(s, scale)
        with pytest.raises(binding.FlexError, match="invalid"):
            plan.edge_softmax_backward(s, s, scale)


def test_rows_without_entries_and_an_empty_matrix():
    a = binding.HostCsr(np.zeros(41, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=17)
    plan = flex_amd.Plan(a, 32, mutable_values=True)
    plan.edge_softmax_ptr(0, 1.0, 0)  # nnz == 0: no launch, nothing read
    plan.edge_softmax_backward_ptr(0, 0, 1.0, 0)
    assert plan.softmax_info()["items"] == 0


@pytest.mark.parametrize("graph", ["long_rows", "rows_256_257", "directed_dups"])
def test_in_place_unaligned_and_repeated_runs_give_the_same_bits(graph):
    a, plan = graph_and_plan(graph)
    for name in ("spread80", "poisoned"):
        s, g = scores(name, a.rowPtr, seed=10), _grad(a.nnz, 11)
        sd, gd = _dev(s), _dev(g)
        p = plan.edge_softmax(sd, 0.125)
        gs = plan.edge_softmax_backward(p, gd, 0.125)
        want_p, want_gs = _host(p), _host(gs)
        assert _same_bits(_host(plan.edge_softmax(sd, 0.125)), want_p) and _same_bits(_host(plan.edge_softmax_backward(p, gd, 0.125)), want_gs)
        s2, g2 = sd.clone(), gd.clone()
        assert plan.edge_softmax(s2, 0.125, out=s2) is s2 and _same_bits(_host(s2), want_p)
        assert plan.edge_softmax_backward(p, g2, 0.125, out=g2) is g2 and _same_bits(_host(g2), want_gs)
        # arrays one float off the 16-byte mark: 4-byte accesses, the same lanes and order
        big_s, big_g, big_o = (torch.zeros(a.nnz + 1, device="cuda") for _ in range(3))
        big_s[1:], big_g[1:] = sd, gd
        s = torch.cuda.current_stream().cuda_stream
        plan.edge_softmax_ptr(big_s.data_ptr() + 4, 0.125, big_o.data_ptr() + 4, s)
        assert _same_bits(_host(big_o)[1:], want_p)
        plan.edge_softmax_backward_ptr(p.data_ptr(), big_g.data_ptr() + 4, 0.125, big_o.data_ptr() + 4, s)
        assert _same_bits(_host(big_o)[1:], want_gs)


def test_forward_and_backward_in_a_captured_graph_replayed_with_new_scores():
    a, plan = graph_and_plan("long_rows")
    s1, s2, g = scores("uniform4", a.rowPtr, seed=12), scores("rows_masked", a.rowPtr, seed=13), _grad(a.nnz, 14)
    sd, gd = _dev(s1), _dev(g)
    p, gs = torch.empty_like(sd), torch.empty_like(sd)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.edge_softmax(sd, 0.125, out=p)
        plan.edge_softmax_backward(p, gd, 0.125, out=gs)
    sd.copy_(_dev(s2))
    graph.replay()
    got_p, got_gs = _host(p).copy(), _host(gs).copy()
    want_p = plan.edge_softmax(_dev(s2), 0.125)
    want_gs = plan.edge_softmax_backward(want_p, gd, 0.125)
    assert _same_bits(got_p, _host(want_p)) and _same_bits(got_gs, _host(want_gs))
    check_forward(a.rowPtr, s2, 0.125, got_p, "replay")


# ---- autograd: Out = A(alpha) V, alpha = softmax over each row of scale <Q[row], K[col]> ------------------------------------------------

def _attention_f64(a, Q, K, V, scale, gOut):
    """Out and the gradients in Q, K, V by torch autograd in float64, rows padded to the longest one (a masked pad is -inf)."""
    rp, col = a.rowPtr.astype(np.int64), a.col.astype(np.int64)
    deg = np.diff(rp)
    width = int(deg.max())
    row = np.repeat(np.arange(a.m), deg)
    pos = np.arange(a.nnz) - np.repeat(rp[:-1], deg)
    Q, K, V = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (Q, K, V))
    s = (Q[row] * K[col]).sum(1)
    S = torch.full((a.m, width), -np.inf, dtype=torch.float64)
    S = S.index_put((torch.tensor(row), torch.tensor(pos)), s)
    alpha = torch.softmax(scale * S, dim=1)
    alpha = torch.where(torch.tensor(deg == 0)[:, None], torch.zeros_like(alpha), alpha)  # a row without entries attends to nothing
    al = alpha[torch.tensor(row), torch.tensor(pos)]
    out = torch.zeros((a.m, V.shape[1]), dtype=torch.float64).index_add(0, torch.tensor(row), al[:, None] * V[col])
    out.backward(torch.tensor(gOut, dtype=torch.float64))
    return out.detach().numpy(), Q.grad.numpy(), K.grad.numpy(), V.grad.numpy(), s.detach().numpy(), al.detach().numpy()


def _row_sum(x, seg, n):
    out = np.zeros((n,) + x.shape[1:])
    np.add.at(out, seg, x)
    return out


def _attention_tolerances(a, Q, K, V, scale, gOut, s, al):
    """First-order propagation of the header bounds through the five engine calls of one attention step, in float64, inflated by 1e-3
    for the products of two errors (every relative error below is < 1e-3).  P = 32: the padding allowance of flex_spmm's bound.
      scores   ds  = gamma(k) sum_j |Q K|                                   (flex_sddmm)
      alpha    da  = forward bound + alpha (exp(2 scale max_row ds) - 1)    (flex_edge_softmax; a softmax moves by at most that factor)
      Out      dO  = gamma(n_r + P) sum alpha |V| + sum da |V|              (flex_spmm)
      gV       the same on A^T with gOut
      galpha   dga = gamma(k) sum_j |gOut V|                                (flex_sddmm)
      gs       dgs = backward bound + scale [da (|ga| + sum alpha |ga|) + alpha (dga + sum (da |ga| + alpha dga))]
      gQ, gK   gamma(n + P) sum |gs| |K or Q| + sum dgs |K or Q|            (flex_spmm on the plan of A and of A^T)"""
    rp, col = a.rowPtr.astype(np.int64), a.col.astype(np.int64)
    deg = np.diff(rp)
    row = np.repeat(np.arange(a.m), deg)
    k = Q.shape[1]
    P = 32
    aQ, aK, aV, aG = (np.abs(np.asarray(x, np.float64)) for x in (Q, K, V, gOut))
    ds = gamma(k) * (aQ[row] * aK[col]).sum(1) + k * 2.0 ** -149
    _, fb = forward_ref(rp, s.astype(np.float32), scale)
    ds_row = np.zeros(a.m)
    np.maximum.at(ds_row, row, ds + np.abs(s) * U)  # + the rounding of the float64 score to the fp32 one the reference bound starts from
    da = fb + al * np.expm1(2 * scale * ds_row[row]) + al * gamma(8)
    n_r = deg[row]
    dO = _row_sum((gamma(n_r + P) * al + da)[:, None] * aV[col], row, a.m) + 2.0 ** -126
    cdeg = np.bincount(col, minlength=a.n)
    dgV = _row_sum((gamma(cdeg[col] + P) * al + da)[:, None] * aG[row], col, a.n) + 2.0 ** -126
    G64, V64 = np.asarray(gOut, np.float64), np.asarray(V, np.float64)
    ga = (G64[row] * V64[col]).sum(1)
    dga = gamma(k) * (aG[row] * aV[col]).sum(1) + k * 2.0 ** -149
    aga = np.abs(ga)
    dgs = (gamma(n_r + 4) * scale * al * (aga + _row_sum(al * aga, row, a.m)[row]) + n_r * 2.0 ** -149
           + scale * (da * (aga + _row_sum(al * aga, row, a.m)[row]) + al * (dga + _row_sum(da * aga + al * dga, row, a.m)[row])))
    gs = np.abs(scale * al * (ga - _row_sum(al * ga, row, a.m)[row]))
    dgQ = _row_sum((gamma(n_r + P) * gs + dgs)[:, None] * aK[col], row, a.m) + 2.0 ** -126
    dgK = _row_sum((gamma(cdeg[col] + P) * gs + dgs)[:, None] * aQ[row], col, a.n) + 2.0 ** -126
    return tuple(1.001 * t for t in (dO, dgQ, dgK, dgV))


@pytest.mark.parametrize("k", [8, 32, 100])
@pytest.mark.parametrize("graph", ["directed_dups", "directed_empty_long"])
def test_attention_and_its_gradients_against_float64(graph, k):
    a = _directed(300, seed=6, dup=True) if graph == "directed_dups" else _directed(260, 260, seed=7)
    rng = np.random.default_rng([k, 21])
    Q, K, V = (rng.uniform(-1, 1, (r, k)).astype(np.float32) for r in (a.m, a.n, a.n))
    gOut = rng.uniform(-1, 1, (a.m, k)).astype(np.float32)
    op = flex_amd.SparseOperator(a, k, learn_values=True)
    Qd, Kd, Vd = (_dev(x).requires_grad_() for x in (Q, K, V))
    out = op.attention(Qd, Kd, Vd)
    # another product with other values between the forward and the backward: every Function sets its values before it uses a plan
    other = op(_dev(V), values=_dev(rng.uniform(-1, 1, a.nnz).astype(np.float32)))
    out.backward(_dev(gOut))
    del other
    scale = k ** -0.5
    want = _attention_f64(a, Q, K, V, scale, gOut)
    tols = _attention_tolerances(a, Q, K, V, scale, gOut, want[4], want[5])
    for what, got, ref, tol in zip(("Out", "grad_Q", "grad_K", "grad_V"), (out.detach(), Qd.grad, Kd.grad, Vd.grad), want[:4], tols):
        err = np.abs(_host(got).astype(np.float64) - ref)
        assert np.all(err <= tol), f"{what} k={k}: worst err / tolerance {float((err / tol).max()):.3g}"
        print(f"{graph} k={k} {what}: worst err / tolerance {float((err / tol).max()):.3g}")


def test_the_attention_pieces_need_learn_values():
    a = _directed(60, seed=9)
    op = flex_amd.SparseOperator(a, 8)
    x = torch.zeros((a.m, 8), device="cuda")
    for call in (lambda: op.sddmm(x, x), lambda: op.edge_softmax(torch.zeros(a.nnz, device="cuda")), lambda: op.attention(x, x, x)):
        with pytest.raises(NotImplementedError, match="learn_values"):
            call()

"""The fused attention backward on the GPU (flex_attention_backward, FLEX_PLAN_ATTENTION_BACKWARD): gQ, gK, gV and ds against the float64
reference and the bounds of tests/fused_attention_backward_ref.py on every element, on every row and column class, slot width and score
scenario, in the 16-byte form and in the generic form of every (W, NS) (the k tables are tests/attention_forms.py's, whose cases
tests/test_attention_routes.py holds to the kernels they launch), with p taken from flex_attention on the same operands; against the chain of eight engine calls on the same p; non-finite
operands; strided and unaligned operands; subsets of the outputs; run to run and inside a captured graph; and
SparseOperator(fused_attention=True, fused_backward=True) with its gradients against a float64 torch evaluation.

Worst err / bound seen on an MI355X (printed per case and per output): gQ 0.171, gK 0.155, ds 0.148, and gV 0.998 -- on
columns of one entry, where gV = fl(p g) is a single rounding held to gamma(1) |p g|: the bound is tight there by construction."""
import os

import numpy as np
import pytest

import flex_amd
import test_gpu_attention as composition
from attention_forms import (COLUMN_KERNEL_ALONE, GENERIC_ALIGNED_KS, GENERIC_ODD_KS, ROW_KERNEL_ALONE, SINGLE_KS as KS, SINGLE_OTHER_KS,
                             SINGLE_STRIDED_KS)
from backward_ref import _directed
from conftest import GOLDEN
from flex_amd import binding
from fused_attention_backward_ref import both_sides, check, reference
from fused_attention_ref import QKV_SCENARIOS, coo, operands, threshold_graph
from fused_attention_ref import reference as forward_reference
from softmax_ref import SCALES, boundary_graph, gamma, long_rows_graph

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GRAPHS = {
    "pubmed": lambda: flex_amd.csv_load(os.path.join(GOLDEN, "pubmed.csv")),
    "directed_dups": lambda: _directed(300, seed=6, dup=True),
    "directed_empty": lambda: _directed(250, 260, seed=7),
    "long_rows_lifted": lambda: both_sides(long_rows_graph()),
    "rows_256_257_lifted": lambda: both_sides(boundary_graph()),
    "thresholds_lifted": lambda: both_sides(threshold_graph()),
}
UNLIFTED = {"thresholds": threshold_graph}  # the generic forms' second graph: no long column
SENTINEL = -12345.5
_graphs, _plans = {}, {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = (GRAPHS.get(name) or UNLIFTED[name])()
    return _graphs[name]


def plan(name, k, **kw):
    key = (name, k, tuple(sorted(kw.items())))
    if key not in _plans:
        _plans[key] = flex_amd.Plan(graph(name), k, attention=True, attention_backward=True, **kw)
        _plans[key].self_check()
    return _plans[key]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same_bits(x, y):
    return bool(np.array_equal(np.asarray(x, np.float32).view(np.uint32), np.asarray(y, np.float32).view(np.uint32)))


def _each(r):
    return " ".join(f"{key} {v:.3g}" for key, v in r.items())


def _grad(a, k, seed):
    return np.random.default_rng([seed, k, 77]).uniform(-1, 1, (a.m, k)).astype(np.float32)


def _forward_p(p, a, Q, K, V, scale):
    pd = torch.zeros(a.nnz, device="cuda")
    p.attention(_dev(Q), _dev(K), _dev(V), scale, p=pd)
    return _host(pd)


def _run(p, a, Q, K, V, pr, g, scale, want=(True, True, True)):
    """(gQ, gK, gV, ds) on the host; an output that is not wanted is None, ds is what dWork holds afterwards."""
    work = torch.full((a.nnz,), SENTINEL, device="cuda")
    outs = p.attention_backward(_dev(Q), _dev(K), _dev(V), _dev(pr), _dev(g), scale, work=work, want=want)
    return tuple(None if t is None else _host(t) for t in outs) + (_host(work),)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_every_gradient_against_float64(name, k):
    a, p = graph(name), plan(name, k)
    Q, K, V = operands("uniform4", a, k, seed=1)
    g = _grad(a, k, 1)
    for scale in SCALES:
        pr = _forward_p(p, a, Q, K, V, scale)
        each = {}
        worst = check(a, Q, K, V, pr, g, scale, *_run(p, a, Q, K, V, pr, g, scale), what=f"{name} k={k} scale {scale:.4g}", ratios=each)
        print(f"{name} k={k} scale {scale:.4g}: worst err / bound {worst:.3g} ({_each(each)})")


@pytest.mark.parametrize("k", [32, 100])
@pytest.mark.parametrize("scenario", QKV_SCENARIOS)
def test_score_scenarios(scenario, k):
    name = "thresholds_lifted"
    a, p = graph(name), plan(name, k)
    Q, K, V = operands(scenario, a, k, seed=2)
    g = _grad(a, k, 2)
    for scale in (1.0, 0.125):
        pr = _forward_p(p, a, Q, K, V, scale)
        each = {}
        worst = check(a, Q, K, V, pr, g, scale, *_run(p, a, Q, K, V, pr, g, scale), what=f"{scenario} k={k} scale {scale}", ratios=each)
        print(f"{name} {scenario} k={k} scale {scale}: worst err / bound {worst:.3g} ({_each(each)})")


@pytest.mark.parametrize("k", SINGLE_OTHER_KS)
def test_the_other_slot_widths_and_slabs(k):
    """k = 30: the generic instantiation; 64: slots of 16 lanes; 300 and 600: two and four slabs of 256 columns."""
    name = "thresholds_lifted"
    a, p = graph(name), plan(name, k)
    g = _grad(a, k, 3)
    for scenario in ("uniform4", "poisoned"):
        Q, K, V = operands(scenario, a, k, seed=3)
        pr = _forward_p(p, a, Q, K, V, 0.125)
        each = {}
        worst = check(a, Q, K, V, pr, g, 0.125, *_run(p, a, Q, K, V, pr, g, 0.125), what=f"k={k} {scenario}", ratios=each)
        print(f"{name} {scenario} k={k}: worst err / bound {worst:.3g} ({_each(each)})")


def _chain(pf, pt, Q, K, V, pr, g, scale):
    """The eight engine calls of _FusedAttention.backward without fused_backward, on the same p: (gQ, gK, gV, gs)."""
    Qd, Kd, Vd, pd, gd = (_dev(x) for x in (Q, K, V, pr, g))
    pt.set_values(pd)
    gV = pt(gd)
    gs = pf.edge_softmax_backward(pd, pf.sddmm(gd, Vd), scale)
    pf.set_values(gs)
    gQ = pf(Kd)
    pt.set_values(gs)
    gK = pt(Qd)
    return _host(gQ), _host(gK), _host(gV), _host(gs)


@pytest.mark.parametrize("scenario", ["uniform4", "poisoned", "masked30", "rows_masked"])
@pytest.mark.parametrize("name", ["directed_dups", "long_rows_lifted", "pubmed"])
def test_agreement_with_the_chain_of_eight_calls(name, scenario):
    k, scale = 32, 0.125
    a = graph(name)
    pf, pt = plan(name, k, mutable_values=True), flex_amd.Plan(a, k, transpose=True, mutable_values=True)
    Q, K, V = operands(scenario, a, k, seed=4)
    g = _grad(a, k, 4)
    pr = _forward_p(pf, a, Q, K, V, scale)
    mine = _run(pf, a, Q, K, V, pr, g, scale)
    theirs = _chain(pf, pt, Q, K, V, pr, g, scale)
    ref, ref8 = reference(a, Q, K, V, pr, g, scale), reference(a, Q, K, V, pr, g, scale, a_r=4, b_r=32)
    for key, x, y in zip(("gq", "gk", "gv", "ds"), mine, theirs):
        assert np.array_equal(np.isfinite(x), np.isfinite(y)), f"{name} {scenario} {key}: the non-finite elements differ in {int((np.isfinite(x) != np.isfinite(y)).sum())} places"
        fin = np.isfinite(x) & np.isfinite(ref[key])
        ratio = np.abs(x[fin].astype(np.float64) - y[fin]) / (ref[key + "_bound"][fin] + ref8[key + "_bound"][fin])
        worst = float(ratio.max()) if ratio.size else 0.0
        print(f"{name} {scenario} {key}: against the chain, worst err / (bound + the chain's bound) {worst:.3g}")
        assert worst <= 1.0, f"{name} {scenario} {key}: {worst:.3g}"


def test_a_nan_and_an_inf_reach_exactly_the_rows_of_the_adjacent_columns():
    name, k, scale = "long_rows_lifted", 32, 0.125
    a, p = graph(name), plan(name, k)
    Q, K, V = operands("uniform4", a, k, seed=5)
    g = _grad(a, k, 5)
    pr = _forward_p(p, a, Q, K, V, scale)  # a clean forward; the poison enters the backward only
    row, col, rp = coo(a)
    deg = np.diff(rp)
    r_nan, r_inf = (int(r) for r in np.flatnonzero((deg >= 2) & (deg <= 8))[[1, 5]])
    g[r_nan, 5], Q[r_inf, 7] = np.nan, np.inf
    gq, gk, gv, ds = _run(p, a, Q, K, V, pr, g, scale)
    check(a, Q, K, V, pr, g, scale, gq, gk, gv, ds, what="non-finite g and Q")
    c_nan, c_inf = col[row == r_nan], col[row == r_inf]
    hit_v = np.zeros((a.n, k), bool)
    hit_v[c_nan, 5] = True  # p_e g[r]: the one column of g
    hit_k = np.zeros((a.n, k), bool)
    hit_k[c_nan, :] = True  # ds of the whole row is NaN, times a finite Q row
    hit_k[c_inf, 7] = True  # ds_e x inf
    hit_q = np.zeros((a.m, k), bool)
    hit_q[r_nan, :] = True
    assert np.array_equal(~np.isfinite(gv), hit_v) and np.array_equal(~np.isfinite(gk), hit_k) and np.array_equal(~np.isfinite(gq), hit_q)
    assert np.array_equal(~np.isfinite(ds), row == r_nan)


@pytest.mark.parametrize("k", SINGLE_STRIDED_KS)
def test_strided_and_unaligned_operands(k):
    name, scale = "thresholds_lifted", 0.125
    a = graph(name)
    Q, K, V = operands("uniform4", a, k, seed=6)
    g = _grad(a, k, 6)
    pr = _forward_p(plan(name, k), a, Q, K, V, scale)
    want = _run(plan(name, k), a, Q, K, V, pr, g, scale)
    check(a, Q, K, V, pr, g, scale, *want, what=f"dense k={k}")
    s = torch.cuda.current_stream().cuda_stream
    for ldb, ldc, off in ((k + 4, k + 8, 0), (k + 3, k + 1, 0), (k, k, 1)):
        p = plan(name, k, ldb=ldb, ldc=ldc)
        shapes = ((a.m, ldc), (a.n, ldb), (a.n, ldb), (a.m, ldc))  # Q, K, V, g
        ins = [torch.full((rows * ld + 1,), float("nan"), device="cuda") for rows, ld in shapes]
        for t, x, (_, ld) in zip(ins, (Q, K, V, g), shapes):
            t[off:off + x.shape[0] * ld].view(x.shape[0], ld)[:, :k] = _dev(x)
        oshapes = ((a.m, ldc), (a.n, ldb), (a.n, ldb))  # gQ, gK, gV
        outs = [torch.full((rows * ld + 1,), SENTINEL, device="cuda") for rows, ld in oshapes]
        pd, work = torch.full((a.nnz + 1,), 0.5, device="cuda"), torch.full((a.nnz + 1,), SENTINEL, device="cuda")
        pd[off:off + a.nnz] = _dev(pr)
        p.attention_backward_ptr(*(t.data_ptr() + 4 * off for t in ins[:3]), pd.data_ptr() + 4 * off, ins[3].data_ptr() + 4 * off, scale,
                                 *(t.data_ptr() + 4 * off for t in outs), work.data_ptr() + 4 * off, s)
        for t, (rows, ld), w in zip(outs, oshapes, want[:3]):
            flat = _host(t)
            got = flat[off:off + rows * ld].reshape(rows, ld)
            assert _same_bits(got[:, :k], w) and np.all(got[:, k:] == SENTINEL), (ldb, ldc, off)
            assert flat[0 if off else -1] == SENTINEL, (ldb, ldc, off)  # the element outside the operand
        wk = _host(work)
        assert _same_bits(wk[off:off + a.nnz], want[3]) and wk[0 if off else -1] == SENTINEL


# ---- the generic form of every (W, NS): tests/attention_forms.py, GENERIC_ODD_KS and GENERIC_ALIGNED_KS

def _run_embedded(name, k, Q, K, V, pr, g, scale, ldb, ldc, off, want=(True, True, True)):
    """(gQ [m, ldc], gK [n, ldb], gV [n, ldb] with their cells past k, ds) of a run whose row operands lie `off` floats into NaN-filled
    buffers of one float more, ldb / ldc floats from row to row: whatever is read past k, or outside an operand, poisons the result,
    and an output that is not wanted is NULL and stays NaN."""
    a, p = graph(name), plan(name, k, ldb=ldb, ldc=ldc)
    shapes = ((a.m, ldc), (a.n, ldb), (a.n, ldb), (a.m, ldc))  # Q, K, V, g
    ins = [torch.full((rows * ld + 1,), float("nan"), device="cuda") for rows, ld in shapes]
    for t, x, (_, ld) in zip(ins, (Q, K, V, g), shapes):
        t[off:off + x.shape[0] * ld].view(x.shape[0], ld)[:, :k] = _dev(x)
    oshapes = ((a.m, ldc), (a.n, ldb), (a.n, ldb))  # gQ, gK, gV
    outs = [torch.full((rows * ld + 1,), float("nan"), device="cuda") for rows, ld in oshapes]
    pd, work = torch.full((a.nnz + 1,), 0.5, device="cuda"), torch.full((a.nnz + 1,), SENTINEL, device="cuda")
    pd[off:off + a.nnz] = _dev(pr)
    p.attention_backward_ptr(*(t.data_ptr() + 4 * off for t in ins[:3]), pd.data_ptr() + 4 * off, ins[3].data_ptr() + 4 * off, scale,
                             *(t.data_ptr() + 4 * off if w else None for t, w in zip(outs, want)), work.data_ptr() + 4 * off,
                             torch.cuda.current_stream().cuda_stream)
    got = []
    for t, (rows, ld), w in zip(outs, oshapes, want):
        flat = _host(t)
        assert np.isnan(flat[0 if off else -1]) and (w or np.all(np.isnan(flat))), (k, ldb, ldc, off, want)  # the float outside the operand
        got.append(flat[off:off + rows * ld].reshape(rows, ld))
    wk = _host(work)
    assert wk[0 if off else -1] == SENTINEL
    return tuple(got) + (wk[off:off + a.nnz],)


def _check_embedded(a, k, Q, K, V, pr, g, scale, got, what):
    each = {}
    worst = check(a, Q, K, V, pr, g, scale, *(x[:, :k] for x in got[:3]), got[3], what=what, ratios=each)
    assert all(np.all(np.isnan(x[:, k:])) for x in got[:3]), what  # the cells past k
    print(f"{what} (generic): worst err / bound {worst:.3g} ({_each(each)})")


def _each_kernel_alone(name, k, Q, K, V, pr, g, scale, ldb, ldc, off, full):
    """gQ alone is the row launch alone, gV alone the column launch alone: the bits of the full run, which is checked against float64."""
    rows_only = _run_embedded(name, k, Q, K, V, pr, g, scale, ldb, ldc, off, want=ROW_KERNEL_ALONE)
    assert _same_bits(rows_only[0][:, :k], full[0][:, :k]) and _same_bits(rows_only[3], full[3]), (k, "gQ alone")
    cols_only = _run_embedded(name, k, Q, K, V, pr, g, scale, ldb, ldc, off, want=COLUMN_KERNEL_ALONE)
    assert _same_bits(cols_only[2][:, :k], full[2][:, :k]) and np.all(cols_only[3] == SENTINEL), (k, "gV alone")


@pytest.mark.parametrize("k", GENERIC_ODD_KS)
@pytest.mark.parametrize("name", ["thresholds", "thresholds_lifted"])
def test_the_generic_form_of_every_width_at_a_k_that_is_no_multiple_of_4(name, k):
    """One k per (W, NS) with scalar tails: 6, 50, 101 and 250 on slots of 4, 16, 32 and 64 lanes, 301 on two slabs, 601 on three slabs
    of the four-slab form (one idle), 1023 on four slabs one column short.  Dense rows, and rows in padded ones whose cells past k must
    stay NaN; then each of the two kernels alone."""
    a, scale = graph(name), 0.125
    g = _grad(a, k, 12)
    for scenario in ("uniform4", "poisoned") + (("rows_masked",) if name == "thresholds_lifted" else ()):
        Q, K, V = operands(scenario, a, k, seed=12)
        pr = _forward_p(plan(name, k), a, Q, K, V, scale)
        for ldb, ldc in ((k, k), (k + 3, k + 1)):
            got = _run_embedded(name, k, Q, K, V, pr, g, scale, ldb, ldc, 0)
            _check_embedded(a, k, Q, K, V, pr, g, scale, got, f"{name} {scenario} k={k} ldb {ldb} ldc {ldc}")
        if scenario == "uniform4":
            _each_kernel_alone(name, k, Q, K, V, pr, g, scale, k + 3, k + 1, 0, got)


@pytest.mark.parametrize("k", GENERIC_ALIGNED_KS)
@pytest.mark.parametrize("name", ["thresholds", "thresholds_lifted"])
def test_the_generic_form_of_every_width_through_misaligned_and_oddly_strided_operands(name, k):
    """An aligned k reaches the generic form when every row operand is one float off 16 bytes, or the leading dimensions are odd: against
    float64, and bit for bit what the 16-byte form gives on the same numbers, as test_strided_and_unaligned_operands has it at k = 32."""
    a, scale = graph(name), 0.125
    g = _grad(a, k, 13)
    for scenario in ("uniform4", "poisoned") + (("rows_masked",) if name == "thresholds_lifted" else ()):
        Q, K, V = operands(scenario, a, k, seed=13)
        pr = _forward_p(plan(name, k), a, Q, K, V, scale)
        want = _run(plan(name, k), a, Q, K, V, pr, g, scale)
        for ldb, ldc, off in ((k + 3, k + 1, 0), (k, k, 1)):
            got = _run_embedded(name, k, Q, K, V, pr, g, scale, ldb, ldc, off)
            _check_embedded(a, k, Q, K, V, pr, g, scale, got, f"{name} {scenario} k={k} ldb {ldb} ldc {ldc} off {off}")
            for x, w in zip(got[:3], want[:3]):
                assert _same_bits(x[:, :k], w), (scenario, k, ldb, ldc, off)
            assert _same_bits(got[3], want[3]), (scenario, k, ldb, ldc, off)
        if scenario == "uniform4":
            _each_kernel_alone(name, k, Q, K, V, pr, g, scale, k, k, 1, got)


def test_every_output_has_the_same_bits_whichever_others_are_asked_for():
    name, k, scale = "thresholds_lifted", 32, 0.125
    a, p = graph(name), plan(name, k)
    Q, K, V = operands("masked30", a, k, seed=7)
    g = _grad(a, k, 7)
    pr = _forward_p(p, a, Q, K, V, scale)
    full = _run(p, a, Q, K, V, pr, g, scale)
    for mask in range(7):
        want = tuple(bool(mask >> i & 1) for i in range(3))
        got = _run(p, a, Q, K, V, pr, g, scale, want=want)
        for i in range(3):
            assert (got[i] is None) if not want[i] else _same_bits(got[i], full[i]), (want, i)
        if want[0] or want[1]:
            assert _same_bits(got[3], full[3]), want
        else:
            assert np.all(got[3] == SENTINEL), want  # neither gQ nor gK: the row launch is skipped and dWork is not written


def test_repeated_runs_and_a_run_after_another_plan_give_the_same_bits():
    name, k = "long_rows_lifted", 100
    a, p = graph(name), plan(name, k)
    Q, K, V = operands("spread80", a, k, seed=8)
    g = _grad(a, k, 8)
    pr = _forward_p(p, a, Q, K, V, 1.0)
    first = _run(p, a, Q, K, V, pr, g, 1.0)
    again = _run(p, a, Q, K, V, pr, g, 1.0)
    b = graph("pubmed")
    Qb, Kb, Vb = operands("uniform4", b, 32, seed=9)
    _run(plan("pubmed", 32), b, Qb, Kb, Vb, _forward_p(plan("pubmed", 32), b, Qb, Kb, Vb, 0.125), _grad(b, 32, 9), 0.125)
    after = _run(p, a, Q, K, V, pr, g, 1.0)
    for x, y, z in zip(first, again, after):
        assert _same_bits(x, y) and _same_bits(x, z)


def test_forward_and_backward_in_one_captured_graph_replayed_with_new_operands():
    name, k, scale = "long_rows_lifted", 32, 0.125
    a, p = graph(name), plan(name, k)
    first = operands("uniform4", a, k, seed=10) + (_grad(a, k, 10),)
    second = operands("rows_masked", a, k, seed=11) + (_grad(a, k, 11),)
    Qd, Kd, Vd, gd = (_dev(x) for x in first)
    out, pd, work = torch.empty((a.m, k), device="cuda"), torch.empty(a.nnz, device="cuda"), torch.empty(a.nnz, device="cuda")
    gq, gk, gv = torch.empty((a.m, k), device="cuda"), torch.empty((a.n, k), device="cuda"), torch.empty((a.n, k), device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=side):
        p.attention(Qd, Kd, Vd, scale, out=out, p=pd)
        p.attention_backward(Qd, Kd, Vd, pd, gd, scale, grad_q=gq, grad_k=gk, grad_v=gv, work=work)
    for t, x in zip((Qd, Kd, Vd, gd), second):
        t.copy_(_dev(x))
    graph_.replay()
    got = tuple(_host(t).copy() for t in (gq, gk, gv, work))
    pr = _forward_p(p, a, *second[:3], scale)
    want = _run(p, a, *second[:3], pr, second[3], scale)
    for x, y in zip(got, want):
        assert _same_bits(x, y)
    check(a, *second[:3], pr, second[3], scale, *got, what="replay")


def test_refused_calls():
    k = 32
    a, p = graph("directed_dups"), plan("directed_dups", k)
    Q, K, V = (_dev(x) for x in operands("uniform4", a, k))
    g, pd = _dev(_grad(a, k, 12)), torch.full((a.nnz,), 0.25, device="cuda")
    for other in (flex_amd.Plan(a, k), flex_amd.Plan(a, k, attention=True), flex_amd.Plan(a, k, attention=True, mutable_values=True)):
        with pytest.raises(binding.FlexError, match="invalid"):
            other.attention_backward(Q, K, V, pd, g, 0.125)
        with pytest.raises(binding.FlexError, match="invalid"):
            other.attention_backward_info()
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(binding.FlexError, match="invalid"):
            p.attention_backward(Q, K, V, pd, g, scale)
    outs = [torch.empty((r, k), device="cuda") for r in (a.m, a.n, a.n)]
    work = torch.empty(a.nnz, device="cuda")
    ptrs = [Q.data_ptr(), K.data_ptr(), V.data_ptr(), pd.data_ptr(), g.data_ptr()]
    optrs = [t.data_ptr() for t in outs]
    for missing in range(6):  # NULL Q, K, V, P, GradOut or Work
        args = [None if i == missing else x for i, x in enumerate(ptrs + [work.data_ptr()])]
        with pytest.raises(binding.FlexError, match="invalid"):
            p.attention_backward_ptr(*args[:5], 0.125, *optrs, args[5])
    with pytest.raises(binding.FlexError, match="invalid"):  # dWork must not be dP
        p.attention_backward_ptr(*ptrs, 0.125, *optrs, pd.data_ptr())
    with pytest.raises(binding.FlexError, match="not supported"):
        flex_amd.Plan(a, 1028, attention=True, attention_backward=True).attention_backward_ptr(*ptrs, 0.125, *optrs, work.data_ptr())
    p.attention_backward_ptr(*ptrs, 0.125, None, None, None, work.data_ptr())  # nothing asked for: no launch
    empty = binding.HostCsr(np.zeros(41, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=17)
    pe = flex_amd.Plan(empty, k, attention=True, attention_backward=True)
    pe.self_check()
    pe.attention_backward_ptr(None, None, None, None, None, 1.0, None, None, None, None)  # no entries: no launch, nothing read


# ---- autograd: tests/test_gpu_fused_attention.py::test_fused_attention_and_its_gradients_against_float64 restated for the fused backward

def _fused_backward_tolerances(a, Q, K, V, scale, gOut, al):
    """test_gpu_fused_attention._fused_tolerances with this backward's bounds in place of the chain's: its sums have depth n (no padding
    allowance: b = 0 for P = 32) and its ds costs a = 3 roundings for flex_edge_softmax_backward's 4; alpha's own error da enters as there."""
    ref = forward_reference(a, Q, K, V, scale)
    row, col, rp = coo(a)
    k = Q.shape[1]
    aQ, aK, aV, aG = (np.abs(np.asarray(x, np.float64)) for x in (Q, K, V, gOut))
    da, n_r = ref["p_bound"], np.diff(rp)[row]
    rs = composition._row_sum
    cdeg = np.bincount(col, minlength=a.n)
    dgV = rs((gamma(cdeg[col] + 0) * al + da)[:, None] * aG[row], col, a.n) + 2.0 ** -126
    ga = (np.asarray(gOut, np.float64)[row] * np.asarray(V, np.float64)[col]).sum(1)
    dga = gamma(k) * (aG[row] * aV[col]).sum(1) + k * 2.0 ** -149
    aga = np.abs(ga)
    dgs = (gamma(n_r + 3) * scale * al * (aga + rs(al * aga, row, a.m)[row]) + max(1.0, scale) * n_r * 2.0 ** -149
           + scale * (da * (aga + rs(al * aga, row, a.m)[row]) + al * (dga + rs(da * aga + al * dga, row, a.m)[row])))
    gs = np.abs(scale * al * (ga - rs(al * ga, row, a.m)[row]))
    dgQ = rs((gamma(n_r + 0) * gs + dgs)[:, None] * aK[col], row, a.m) + 2.0 ** -126
    dgK = rs((gamma(cdeg[col] + 0) * gs + dgs)[:, None] * aQ[row], col, a.n) + 2.0 ** -126
    return tuple(1.001 * t for t in (ref["out_bound"], dgQ, dgK, dgV))


@pytest.mark.parametrize("name,k", [("directed_dups", 8), ("directed_dups", 32), ("directed_dups", 100), ("long_rows_lifted", 32)])
def test_fused_attention_with_the_fused_backward_against_float64_and_against_the_chain(name, k):
    from test_gpu_fused_attention import _fused_tolerances
    a = graph(name)
    rng = np.random.default_rng([k, 22])
    Q, K, V = (rng.uniform(-1, 1, (r, k)).astype(np.float32) for r in (a.m, a.n, a.n))
    gOut = rng.uniform(-1, 1, (a.m, k)).astype(np.float32)
    results = {}
    for fused_backward in (True, False):
        op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=fused_backward)
        Qd, Kd, Vd = (_dev(x).requires_grad_() for x in (Q, K, V))
        out = op.attention(Qd, Kd, Vd)
        other = op(_dev(V), values=_dev(rng.uniform(-1, 1, a.nnz).astype(np.float32)))  # other values between the forward and the backward
        out.backward(_dev(gOut))
        del other
        results[fused_backward] = tuple(_host(t) for t in (out.detach(), Qd.grad, Kd.grad, Vd.grad))
    scale = k ** -0.5
    want = composition._attention_f64(a, Q, K, V, scale, gOut)
    tols = _fused_backward_tolerances(a, Q, K, V, scale, gOut, want[5])
    tols8 = _fused_tolerances(a, Q, K, V, scale, gOut, want[5])
    for what, got, got8, ref, tol, tol8 in zip(("Out", "grad_Q", "grad_K", "grad_V"), results[True], results[False], want[:4], tols, tols8):
        err = np.abs(got.astype(np.float64) - ref)
        print(f"{name} k={k} {what}: worst err / tolerance {float((err / tol).max()):.3g}")
        assert np.all(err <= tol), f"{what} k={k}: worst err / tolerance {float((err / tol).max()):.3g}"
        assert np.all(np.abs(got.astype(np.float64) - got8) <= tol + tol8), f"{what} k={k}: against fused_backward=False"
    assert _same_bits(results[True][0], results[False][0])  # the forward is the same call


def test_only_the_gradients_that_are_needed_are_computed_and_the_guard():
    a, k = graph("directed_dups"), 32
    with pytest.raises(NotImplementedError, match="fused_attention"):
        flex_amd.SparseOperator(a, k, learn_values=True, fused_backward=True)
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True)
    assert not op.fused_backward
    with pytest.raises(binding.FlexError, match="invalid"):
        op.plan.attention_backward_info()
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    Q, K, V = operands("uniform4", a, k, seed=13)
    g = _dev(_grad(a, k, 13))
    Qd, Kd, Vd = (_dev(x).requires_grad_() for x in (Q, K, V))
    op.attention(Qd, Kd, Vd).backward(g)
    full = tuple(_host(t.grad) for t in (Qd, Kd, Vd))
    for i in range(3):
        ts = [_dev(x).requires_grad_(j == i) for j, x in enumerate((Q, K, V))]
        op.attention(*ts).backward(g)
        assert all((t.grad is None) == (j != i) for j, t in enumerate(ts)) and _same_bits(_host(ts[i].grad), full[i])

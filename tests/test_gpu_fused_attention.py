"""The fused attention forward on the GPU (flex_attention, FLEX_PLAN_ATTENTION): Out and P against the float64 reference and the bounds
of tests/fused_attention_ref.py on every element, on every row class, slot width and score scenario, in the 16-byte form and in the
generic form of every (W, NS) (the k tables are tests/attention_forms.py's, whose cases tests/test_attention_routes.py holds to the
kernels they launch); against the four-call composition on the same plan; on strided, unaligned and shard plans; run to run and inside a captured graph; and SparseOperator(fused_attention=True)
with its gradients against a float64 torch evaluation."""
import os

import numpy as np
import pytest

import flex_amd
import test_gpu_attention as composition
from attention_forms import GENERIC_ALIGNED_KS, GENERIC_ODD_KS, SINGLE_KS as KS, SINGLE_OTHER_KS, SINGLE_STRIDED_KS
from backward_ref import _directed
from conftest import GOLDEN
from flex_amd import binding
from fused_attention_backward_ref import both_sides
from fused_attention_ref import QKV_SCENARIOS, check, coo, operands, reference, threshold_graph
from softmax_ref import SCALES, boundary_graph, gamma, long_rows_graph

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GRAPHS = {
    "pubmed": lambda: flex_amd.csv_load(os.path.join(GOLDEN, "pubmed.csv")),
    "directed_dups": lambda: _directed(300, seed=6, dup=True),
    "directed_empty": lambda: _directed(250, 260, seed=7),
    "long_rows": long_rows_graph,
    "rows_256_257": boundary_graph,
    "thresholds": threshold_graph,
}
LIFTED = {"thresholds_lifted": lambda: both_sides(threshold_graph())}  # the generic forms' second graph: the classes in the columns too
_graphs, _plans = {}, {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = (GRAPHS.get(name) or LIFTED[name])()
    return _graphs[name]


def plan(name, k, **kw):
    key = (name, k, tuple(sorted(kw.items())))
    if key not in _plans:
        _plans[key] = flex_amd.Plan(graph(name), k, attention=True, **kw)
        _plans[key].self_check()
    return _plans[key]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same_bits(x, y):
    return bool(np.array_equal(np.asarray(x, np.float32).view(np.uint32), np.asarray(y, np.float32).view(np.uint32)))


def _run(p, a, Q, K, V, scale, with_p=True):
    pd = torch.full((a.nnz,), -7.0, device="cuda") if with_p else None
    out = p.attention(_dev(Q), _dev(K), _dev(V), scale, p=pd)
    return _host(out), (_host(pd) if with_p else None)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_out_and_p_against_float64(name, k):
    a, p = graph(name), plan(name, k)
    Q, K, V = operands("uniform4", a, k, seed=1)
    for scale in SCALES:
        out, pr = _run(p, a, Q, K, V, scale)
        worst = check(a, Q, K, V, scale, out, pr, what=f"{name} k={k} scale {scale:.4g}")
        print(f"{name} k={k} scale {scale:.4g}: worst err / bound {worst:.3g}")


@pytest.mark.parametrize("k", [32, 100])
@pytest.mark.parametrize("scenario", QKV_SCENARIOS)
@pytest.mark.parametrize("name", ["directed_dups", "long_rows", "thresholds"])
def test_score_scenarios(name, scenario, k):
    a, p = graph(name), plan(name, k)
    Q, K, V = operands(scenario, a, k, seed=2)
    for scale in (1.0, 0.125):
        out, pr = _run(p, a, Q, K, V, scale)
        worst = check(a, Q, K, V, scale, out, pr, what=f"{name} {scenario} k={k} scale {scale}")
        print(f"{name} {scenario} k={k} scale {scale}: worst err / bound {worst:.3g}")


@pytest.mark.parametrize("k", SINGLE_OTHER_KS)
def test_the_other_slot_widths_and_slabs(k):
    """k = 30: the generic instantiation; 64: slots of 16 lanes; 300 and 600: two and four slabs of 256 columns."""
    a, p = graph("thresholds"), plan("thresholds", k)
    for scenario in ("uniform4", "poisoned"):
        Q, K, V = operands(scenario, a, k, seed=3)
        out, pr = _run(p, a, Q, K, V, 0.125)
        print(f"thresholds {scenario} k={k}: worst err / bound {check(a, Q, K, V, 0.125, out, pr, what=f'k={k} {scenario}'):.3g}")


@pytest.mark.parametrize("name", ["directed_dups", "long_rows", "pubmed"])
def test_agreement_with_the_four_call_composition(name):
    k, scale = 32, 0.125
    a, p = graph(name), plan(name, k, mutable_values=True)
    for scenario in ("uniform4", "masked30"):
        Q, K, V = operands(scenario, a, k, seed=4)
        Qd, Kd, Vd = _dev(Q), _dev(K), _dev(V)
        out, pr = _run(p, a, Q, K, V, scale)
        alpha = p.edge_softmax(p.sddmm(Qd, Kd), scale)
        p.set_values(alpha)
        out4, alpha = _host(p(Vd)), _host(alpha)
        ref = reference(a, Q, K, V, scale)
        row, col, rp = coo(a)
        n_r = np.diff(rp)[row]
        aV = np.abs(V.astype(np.float64))[col]
        # the composition's own bounds: its alpha is inside dalpha (which grants more than flex_edge_softmax needs), its SpMM pads to n_r + 32
        b4 = np.zeros_like(ref["out"])
        np.add.at(b4, row, (gamma(n_r + 32) * ref["p"] + ref["p_bound"])[:, None] * aV)
        assert np.all(np.abs(pr.astype(np.float64) - alpha) <= 2 * ref["p_bound"]), f"{name} {scenario}: P"
        err = np.abs(out.astype(np.float64) - out4)
        assert np.all(err <= ref["out_bound"] + b4 + 2.0 ** -126), f"{name} {scenario}: Out, worst {float((err / (ref['out_bound'] + b4)).max()):.3g}"
        # Out against sum P V in float64 on the returned fp32 P: Out's bound plus P's own error carried through |V|
        pv, bp = np.zeros_like(ref["out"]), np.zeros_like(ref["out"])
        np.add.at(pv, row, pr.astype(np.float64)[:, None] * V.astype(np.float64)[col])
        np.add.at(bp, row, ref["p_bound"][:, None] * aV)
        err = np.abs(out.astype(np.float64) - pv)
        assert np.all(err <= ref["out_bound"] + bp), f"{name} {scenario}: Out against sum P V"
        print(f"{name} {scenario}: Out against the composition, worst err / bound {float((np.abs(out.astype(np.float64) - out4) / (ref['out_bound'] + b4)).max()):.3g}")


def test_without_p_the_same_out_and_nonfinite_v_rows_reach_their_neighbours_only():
    k = 32
    a, p = graph("long_rows"), plan("long_rows", k)
    Q, K, V = operands("masked30", a, k, seed=5)
    out, _ = _run(p, a, Q, K, V, 0.125)
    assert _same_bits(out, _run(p, a, Q, K, V, 0.125, with_p=False)[0])
    row, col, _ = coo(a)
    c_nan, c_inf = int(col[3]), int(col[len(col) // 2])
    assert c_nan != c_inf
    V[c_nan, 5], V[c_inf, 7] = np.nan, np.inf
    out, pr = _run(p, a, Q, K, V, 0.125)
    check(a, Q, K, V, 0.125, out, pr, what="non-finite V")
    hit = np.zeros((a.m, k), bool)
    hit[row[col == c_nan], 5] = True
    hit[row[col == c_inf], 7] = True
    assert hit.any() and np.array_equal(~np.isfinite(out), hit)


@pytest.mark.parametrize("k", SINGLE_STRIDED_KS)
def test_strided_and_unaligned_operands(k):
    a = graph("thresholds")
    Q, K, V = operands("uniform4", a, k, seed=6)
    want, want_p = _run(plan("thresholds", k), a, Q, K, V, 0.125)
    check(a, Q, K, V, 0.125, want, want_p, what=f"dense k={k}")
    s = torch.cuda.current_stream().cuda_stream
    for ldb, ldc, off in ((k + 4, k + 8, 0), (k + 3, k + 1, 0), (k, k, 1)):
        p = plan("thresholds", k, ldb=ldb, ldc=ldc)
        big = [torch.full((rows * ld + 1,), float("nan"), device="cuda") for rows, ld in ((a.m, ldc), (a.n, ldb), (a.n, ldb), (a.m, ldc))]
        for t, x, ld in zip(big, (Q, K, V), (ldc, ldb, ldb)):
            t[off:off + x.shape[0] * ld].view(x.shape[0], ld)[:, :k] = _dev(x)
        pd = torch.full((a.nnz + 1,), -7.0, device="cuda")
        p.attention_ptr(*(t.data_ptr() + 4 * off for t in big[:3]), 0.125, big[3].data_ptr() + 4 * off, pd.data_ptr() + 4 * off, s)
        got = _host(big[3])[off:off + a.m * ldc].reshape(a.m, ldc)
        assert _same_bits(got[:, :k], want) and np.all(np.isnan(got[:, k:])), (ldb, ldc, off)
        assert _same_bits(_host(pd)[off:off + a.nnz], want_p)


# ---- the generic form of every (W, NS): tests/attention_forms.py, GENERIC_ODD_KS and GENERIC_ALIGNED_KS

def _run_embedded(name, k, Q, K, V, scale, ldb, ldc, off):
    """(Out [m, ldc] with the cells past k, P) of a run whose row operands lie `off` floats into NaN-filled buffers of one float more,
    ldb / ldc floats from row to row: whatever is read past k, or outside an operand, poisons the result."""
    a, p = graph(name), plan(name, k, ldb=ldb, ldc=ldc)
    big = [torch.full((rows * ld + 1,), float("nan"), device="cuda") for rows, ld in ((a.m, ldc), (a.n, ldb), (a.n, ldb), (a.m, ldc))]
    for t, x, ld in zip(big, (Q, K, V), (ldc, ldb, ldb)):
        t[off:off + x.shape[0] * ld].view(x.shape[0], ld)[:, :k] = _dev(x)
    pd = torch.full((a.nnz + 1,), -7.0, device="cuda")
    p.attention_ptr(*(t.data_ptr() + 4 * off for t in big[:3]), 0.125, big[3].data_ptr() + 4 * off, pd.data_ptr() + 4 * off,
                    torch.cuda.current_stream().cuda_stream)
    flat, pr = _host(big[3]), _host(pd)
    assert np.isnan(flat[0 if off else -1]) and pr[0 if off else -1] == -7.0, (k, ldb, ldc, off)  # the float outside the operand
    return flat[off:off + a.m * ldc].reshape(a.m, ldc), pr[off:off + a.nnz]


@pytest.mark.parametrize("k", GENERIC_ODD_KS)
@pytest.mark.parametrize("name", ["thresholds", "thresholds_lifted"])
def test_the_generic_form_of_every_width_at_a_k_that_is_no_multiple_of_4(name, k):
    """One k per (W, NS) with scalar tails: 6, 50, 101 and 250 on slots of 4, 16, 32 and 64 lanes, 301 on two slabs, 601 on three slabs
    of the four-slab form (one idle), 1023 on four slabs one column short.  Dense rows, and rows in padded ones whose cells past k must
    stay NaN."""
    a = graph(name)
    for scenario in ("uniform4", "poisoned") + (("rows_masked",) if name == "thresholds_lifted" else ()):
        Q, K, V = operands(scenario, a, k, seed=12)
        for ldb, ldc in ((k, k), (k + 3, k + 1)):
            out, pr = _run_embedded(name, k, Q, K, V, 0.125, ldb, ldc, 0)
            worst = check(a, Q, K, V, 0.125, out[:, :k], pr, what=f"{name} {scenario} k={k} ldb {ldb} ldc {ldc}")
            assert np.all(np.isnan(out[:, k:])), (scenario, k, ldb, ldc)
            print(f"{name} {scenario} k={k} ldb {ldb} ldc {ldc} (generic): worst err / bound {worst:.3g}")


@pytest.mark.parametrize("k", GENERIC_ALIGNED_KS)
@pytest.mark.parametrize("name", ["thresholds", "thresholds_lifted"])
def test_the_generic_form_of_every_width_through_misaligned_and_oddly_strided_operands(name, k):
    """An aligned k reaches the generic form when every row operand is one float off 16 bytes, or the leading dimensions are odd: against
    float64, and bit for bit what the 16-byte form gives on the same numbers, as test_strided_and_unaligned_operands has it at k = 32."""
    a = graph(name)
    for scenario in ("uniform4", "poisoned") + (("rows_masked",) if name == "thresholds_lifted" else ()):
        Q, K, V = operands(scenario, a, k, seed=13)
        want, want_p = _run(plan(name, k), a, Q, K, V, 0.125)
        for ldb, ldc, off in ((k + 3, k + 1, 0), (k, k, 1)):
            out, pr = _run_embedded(name, k, Q, K, V, 0.125, ldb, ldc, off)
            worst = check(a, Q, K, V, 0.125, out[:, :k], pr, what=f"{name} {scenario} k={k} ldb {ldb} ldc {ldc} off {off}")
            assert np.all(np.isnan(out[:, k:])), (scenario, k, ldb, ldc, off)
            print(f"{name} {scenario} k={k} ldb {ldb} ldc {ldc} off {off} (generic): worst err / bound {worst:.3g}")
            assert _same_bits(out[:, :k], want) and _same_bits(pr, want_p), (scenario, k, ldb, ldc, off)


def test_shards_write_their_own_rows_and_entries_only_and_their_union_is_the_unsharded_result():
    k = 32
    a = graph("long_rows")
    Q, K, V = operands("rows_masked", a, k, seed=7)
    whole, whole_p = _run(plan("long_rows", k), a, Q, K, V, 0.125)
    Qd, Kd, Vd = _dev(Q), _dev(K), _dev(V)
    cuts = [0, 17, 18, 18, 101, 260, a.m]
    sentinel = np.float32(-12345.5)
    union, union_p = np.full((a.m, k), sentinel), np.full(a.nnz, sentinel)
    s = torch.cuda.current_stream().cuda_stream
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        shard = flex_amd.Plan(a, k, rows=(r0, r1), attention=True)
        shard.self_check()
        e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
        out = torch.full((a.m, k), float(sentinel), device="cuda")
        pd = torch.full((a.nnz,), float(sentinel), device="cuda")
        shard.attention_ptr(Qd.data_ptr() + 4 * k * r0, Kd.data_ptr(), Vd.data_ptr(), 0.125, out.data_ptr() + 4 * k * r0, pd.data_ptr(), s)
        out, pd = _host(out), _host(pd)
        assert np.all(out[:r0] == sentinel) and np.all(out[r1:] == sentinel), (r0, r1)
        assert np.all(pd[:e0] == sentinel) and np.all(pd[e1:] == sentinel), (r0, r1)
        union[r0:r1], union_p[e0:e1] = out[r0:r1], pd[e0:e1]
    assert _same_bits(union, whole) and _same_bits(union_p, whole_p)


def test_repeated_runs_and_a_run_after_another_plan_give_the_same_bits():
    k = 100
    a, p = graph("long_rows"), plan("long_rows", k)
    Q, K, V = operands("spread80", a, k, seed=8)
    out, pr = _run(p, a, Q, K, V, 1.0)
    again, again_p = _run(p, a, Q, K, V, 1.0)
    assert _same_bits(out, again) and _same_bits(pr, again_p)
    b = graph("pubmed")
    _run(plan("pubmed", 32), b, *operands("uniform4", b, 32, seed=9), 0.125)
    after, after_p = _run(p, a, Q, K, V, 1.0)
    assert _same_bits(out, after) and _same_bits(pr, after_p)


def test_a_forward_in_a_captured_graph_replayed_with_new_operands():
    k = 32
    a, p = graph("long_rows"), plan("long_rows", k)
    first, second = operands("uniform4", a, k, seed=10), operands("rows_masked", a, k, seed=11)
    Qd, Kd, Vd = (_dev(x) for x in first)
    out, pd = torch.empty((a.m, k), device="cuda"), torch.empty(a.nnz, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        p.attention(Qd, Kd, Vd, 0.125, out=out, p=pd)
    for t, x in zip((Qd, Kd, Vd), second):
        t.copy_(_dev(x))
    g.replay()
    got, got_p = _host(out).copy(), _host(pd).copy()
    want, want_p = _run(p, a, *second, 0.125)
    assert _same_bits(got, want) and _same_bits(got_p, want_p)
    check(a, *second, 0.125, got, got_p, what="replay")


def test_refused_calls():
    k = 32
    a, p = graph("directed_dups"), plan("directed_dups", k)
    Q, K, V = (_dev(x) for x in operands("uniform4", a, k))
    for other in (flex_amd.Plan(a, k), flex_amd.Plan(a, k, mutable_values=True)):
        with pytest.raises(binding.FlexError, match="invalid"):
            other.attention(Q, K, V, 0.125)
        with pytest.raises(binding.FlexError, match="invalid"):
            other.attention_info()
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(binding.FlexError, match="invalid"):
            p.attention(Q, K, V, scale)
    out = torch.empty((a.m, k), device="cuda")
    ptrs = [Q.data_ptr(), K.data_ptr(), V.data_ptr(), out.data_ptr()]
    for missing in range(4):
        args = [None if i == missing else x for i, x in enumerate(ptrs)]
        with pytest.raises(binding.FlexError, match="invalid"):
            p.attention_ptr(args[0], args[1], args[2], 0.125, args[3])
    with pytest.raises(binding.FlexError, match="not supported"):
        flex_amd.Plan(a, 1028, attention=True).attention_ptr(*ptrs[:3], 0.125, ptrs[3])
    empty = binding.HostCsr(np.zeros(41, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=17)
    flex_amd.Plan(empty, k, attention=True).attention_ptr(None, None, None, 1.0, None)  # no entries: no launch, nothing read


# ---- autograd: tests/test_gpu_attention.py::test_attention_and_its_gradients_against_float64 restated for the fused forward

def _fused_tolerances(a, Q, K, V, scale, gOut, al):
    """composition._attention_tolerances with the fused kernel's dalpha (fused_attention_ref.reference: it contains the scores' share)
    in place of the composition's, and the fused Out bound; the backward calls are the composition's own."""
    ref = reference(a, Q, K, V, scale)
    row, col, rp = coo(a)
    k, P = Q.shape[1], 32
    aQ, aK, aV, aG = (np.abs(np.asarray(x, np.float64)) for x in (Q, K, V, gOut))
    da, n_r = ref["p_bound"], np.diff(rp)[row]
    rs = composition._row_sum
    cdeg = np.bincount(col, minlength=a.n)
    dgV = rs((gamma(cdeg[col] + P) * al + da)[:, None] * aG[row], col, a.n) + 2.0 ** -126
    ga = (np.asarray(gOut, np.float64)[row] * np.asarray(V, np.float64)[col]).sum(1)
    dga = gamma(k) * (aG[row] * aV[col]).sum(1) + k * 2.0 ** -149
    aga = np.abs(ga)
    dgs = (gamma(n_r + 4) * scale * al * (aga + rs(al * aga, row, a.m)[row]) + n_r * 2.0 ** -149
           + scale * (da * (aga + rs(al * aga, row, a.m)[row]) + al * (dga + rs(da * aga + al * dga, row, a.m)[row])))
    gs = np.abs(scale * al * (ga - rs(al * ga, row, a.m)[row]))
    dgQ = rs((gamma(n_r + P) * gs + dgs)[:, None] * aK[col], row, a.m) + 2.0 ** -126
    dgK = rs((gamma(cdeg[col] + P) * gs + dgs)[:, None] * aQ[row], col, a.n) + 2.0 ** -126
    return tuple(1.001 * t for t in (ref["out_bound"], dgQ, dgK, dgV))


@pytest.mark.parametrize("k", [8, 32, 100])
@pytest.mark.parametrize("name", ["directed_dups", "directed_empty_long"])
def test_fused_attention_and_its_gradients_against_float64(name, k):
    a = _directed(300, seed=6, dup=True) if name == "directed_dups" else _directed(260, 260, seed=7)
    rng = np.random.default_rng([k, 21])
    Q, K, V = (rng.uniform(-1, 1, (r, k)).astype(np.float32) for r in (a.m, a.n, a.n))
    gOut = rng.uniform(-1, 1, (a.m, k)).astype(np.float32)
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True)
    Qd, Kd, Vd = (_dev(x).requires_grad_() for x in (Q, K, V))
    out = op.attention(Qd, Kd, Vd)
    other = op(_dev(V), values=_dev(rng.uniform(-1, 1, a.nnz).astype(np.float32)))  # other values between the forward and the backward
    out.backward(_dev(gOut))
    del other
    scale = k ** -0.5
    want = composition._attention_f64(a, Q, K, V, scale, gOut)
    tols = _fused_tolerances(a, Q, K, V, scale, gOut, want[5])
    for what, got, ref, tol in zip(("Out", "grad_Q", "grad_K", "grad_V"), (out.detach(), Qd.grad, Kd.grad, Vd.grad), want[:4], tols):
        err = np.abs(_host(got).astype(np.float64) - ref)
        print(f"{name} k={k} {what}: worst err / tolerance {float((err / tol).max()):.3g}")
        assert np.all(err <= tol), f"{what} k={k}: worst err / tolerance {float((err / tol).max()):.3g}"
    with torch.no_grad():  # no gradient wanted: nothing nnz-sized is written, the same Out
        assert _same_bits(_host(op.attention(Qd, Kd, Vd)), _host(out.detach()))


def test_fused_attention_needs_learn_values_and_the_default_is_the_composition():
    a = _directed(60, seed=9)
    with pytest.raises(NotImplementedError, match="learn_values"):
        flex_amd.SparseOperator(a, 8, fused_attention=True)
    op = flex_amd.SparseOperator(a, 8, learn_values=True)
    assert not op.fused_attention
    with pytest.raises(binding.FlexError, match="invalid"):
        op.plan.attention_info()

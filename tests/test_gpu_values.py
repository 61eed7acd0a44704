"""Learnable edge values on the GPU (FLEX_PLAN_MUTABLE_VALUES): the value refresh is exact -- a plan refreshed to new values computes
bit for bit what a plan made from them computes, on every flat route, transposed too -- and flex_sddmm is within its float64 bound with
exact classes on every kind of plan, deterministic, and the gradient that SparseOperator(learn_values=True) hands to torch."""
import numpy as np
import pytest

import flex_amd
from backward_ref import _directed, transpose
from f64ref import _VALUES, ROUTES, scenario
from flex_amd import binding
from sddmm_ref import _gb, assert_sddmm_within_bound, sddmm64

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FLAT_ROUTES = sorted(r for r in ROUTES if not r.startswith(("mfma", "blocks")))
# (first values, refreshed values): every pair changes which branch of the padding rule a task's padding takes
VALUE_PAIRS = [("wide", "subnormal_A_large_B"), ("zeros", "nonfinite_A"), ("nonfinite_A", "tiny_vs_inf_B"),
               ("tiny_vs_inf_B", "zeros"), ("huge", "products_underflow"), ("inf_A_vs_inf_B", "wide")]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _same_bits(x, y):
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    return bool(np.all((x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))))


def _with_values(a, vals):
    return binding.HostCsr(a.rowPtr, a.col, np.asarray(vals, np.float32), n=a.n)


def _values_of(name, a, k, seed):
    """Values of scenario `name` drawn for a's pattern (and that scenario's B)."""
    rng = np.random.default_rng([seed, 77, k])
    vals, B = _VALUES[name](rng, a.rowPtr.astype(np.int64), a.col.astype(np.int64), a.n, k)
    return np.asarray(vals, np.float32), np.ascontiguousarray(B, np.float32)


def _plans(route, a, transposed, **kw):
    spec = ROUTES[route]
    k, tn = spec["k"], dict(spec["tuning"], **kw.pop("extra_tuning", {}))
    kw = dict(kw, tuning=tn, transpose=transposed)
    if spec.get("mapped"):
        vo, ap = flex_amd.perm_csr(a, flex_amd.order_rcm(a))
        return [flex_amd.Plan(ap, k, vo_mp=vo, **kw)], ap
    if spec.get("shards"):
        b = flex_amd.shard_rows(transpose(a) if transposed else a, k, spec["shards"])
        return [flex_amd.Plan(a, k, rows=(int(b[i]), int(b[i + 1])), **kw) for i in range(spec["shards"])], a
    ldb, ldc = spec.get("ld", (None, None))
    return [flex_amd.Plan(a, k, order=spec.get("order", 0), ldb=ldb, ldc=ldc, **kw)], a


def _spmm(spec, plans, B):
    """C of plans on B, launched the way the route needs (shards, stamped, unaligned, strided)."""
    k = spec["k"]
    s = torch.cuda.current_stream().cuda_stream
    Bd = _dev(B)
    m_out = sum(p.info()["m"] for p in plans) if spec.get("shards") else plans[0].info()["m"]
    if spec.get("shards"):
        C = torch.cat([p(Bd) for p in plans])
    elif spec.get("stamped"):
        C = torch.full((m_out, k), -7.0, device="cuda")
        plans[0].measure_imbalance(Bd.data_ptr(), C.data_ptr(), s)
    elif spec.get("unaligned"):
        bb = torch.zeros(B.size + 1, device="cuda")
        bb[1:] = Bd.ravel()
        cc = torch.full((m_out * k + 1,), -7.0, device="cuda")
        plans[0].spmm(bb[1:].data_ptr(), cc[1:].data_ptr(), s)
        C = cc[1:].reshape(m_out, k)
    elif "ld" in spec:
        ldb, ldc = spec["ld"]
        Bs = torch.full((B.shape[0], ldb), float("nan"), device="cuda")
        Bs[:, :k] = Bd
        Cs = torch.full((m_out, ldc), -7.0, device="cuda")
        plans[0].spmm(Bs.data_ptr(), Cs.data_ptr(), s)
        C = Cs[:, :k]
    else:
        C = plans[0](Bd)
    torch.cuda.synchronize()
    return np.ascontiguousarray(C.cpu().numpy())


# ---- the refresh ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", FLAT_ROUTES)
@pytest.mark.parametrize("transposed", [False, True])
def test_refresh_gives_the_plan_of_the_new_values_bit_for_bit(route, transposed):
    spec = ROUTES[route]
    k = spec["k"]
    for i, (first, second) in enumerate(VALUE_PAIRS):
        a, _ = scenario(first, k=k, m=spec.get("m", 512), seed=i)
        v2, B = _values_of(second, a, k, i)
        a2 = _with_values(a, v2)
        if transposed:
            B = np.ascontiguousarray(np.random.default_rng(i).uniform(-1, 1, (a.m, k)).astype(np.float32))
        fresh_plans, a2_planned = _plans(route, a2, transposed, mutable_values=True)
        plans, _ = _plans(route, a, transposed, mutable_values=True)
        for p in plans:
            p.set_values(_dev(a2_planned.vals))  # in the CSR order of what the plan was made from (the reordered CSR of a mapped plan)
        for p in plans:
            p.self_check()
        got = _spmm(spec, plans, B)
        fresh = _spmm(spec, fresh_plans, B)
        plain = _spmm(spec, _plans(route, a2, transposed, extra_tuning={"mfma": 2, "blocks": 2})[0], B)
        assert _same_bits(got, fresh), (route, first, second)
        assert _same_bits(got, plain), (route, first, second)


def test_refresh_back_and_forth_and_autotuned_plans():
    a, B = scenario("wide", k=128, m=3000)
    v2, _ = _values_of("nonfinite_A", a, 128, 3)
    p = flex_amd.Plan(a, 128, order=flex_amd.FLEX_PLAN_AUTOTUNE | flex_amd.FLEX_ORDER_CLUSTER, mutable_values=True)
    C0 = _spmm({"k": 128}, [p], B)
    p.set_values(_dev(v2))
    p.set_values(_dev(a.vals))
    p.self_check()
    assert _same_bits(_spmm({"k": 128}, [p], B), C0)


def test_set_values_and_sddmm_need_the_flag():
    a = _directed(100, seed=1)
    p = flex_amd.Plan(a, 32)
    with pytest.raises(binding.FlexError, match="invalid"):
        p.set_values(_dev(a.vals))
    with pytest.raises(binding.FlexError, match="invalid"):
        p.sddmm(torch.zeros((a.m, 32), device="cuda"), torch.zeros((a.n, 32), device="cuda"))


def test_refresh_in_a_captured_graph():
    a, B = scenario("wide", k=64, m=800)
    v2, _ = _values_of("zeros", a, 64, 5)
    p = flex_amd.Plan(a, 64, mutable_values=True)
    Bd, vd = _dev(B), _dev(v2)
    C = torch.empty((a.m, 64), device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        p.set_values(vd)
        p(Bd, out=C)
    g.replay()
    torch.cuda.synchronize()
    want = _spmm({"k": 64}, [flex_amd.Plan(_with_values(a, v2), 64)], B)
    assert _same_bits(C.cpu().numpy(), want)


# ---- the SDDMM --------------------------------------------------------------------------------------------------------------------

def _coo(a):
    rows = np.repeat(np.arange(a.m, dtype=np.int64), np.diff(a.rowPtr.astype(np.int64)))
    return rows, a.col.astype(np.int64)


def _run_sddmm(p, G, B, nnz, ld=None, unaligned=False, sentinel=None):
    """flex_sddmm of plan p on host G, B; ld = (ldb, ldc) lays them out strided (NaN in the tails), unaligned one float off."""
    s = torch.cuda.current_stream().cuda_stream
    k = G.shape[1]
    out = torch.full((nnz + 1,), -7.0 if sentinel is None else sentinel, device="cuda")
    if ld:
        ldb, ldc = ld
        Gs = torch.full((G.shape[0], ldc), float("nan"), device="cuda")
        Bs = torch.full((B.shape[0], ldb), float("nan"), device="cuda")
        Gs[:, :k], Bs[:, :k] = _dev(G), _dev(B)
        p.sddmm_ptr(Gs.data_ptr(), Bs.data_ptr(), out.data_ptr(), s)
    elif unaligned:
        gg = torch.zeros(G.size + 1, device="cuda")
        bb = torch.zeros(B.size + 1, device="cuda")
        gg[1:], bb[1:] = _dev(G).ravel(), _dev(B).ravel()
        p.sddmm_ptr(gg[1:].data_ptr(), bb[1:].data_ptr(), out[1:].data_ptr(), s)
        torch.cuda.synchronize()
        return out[1:].cpu().numpy()
    else:
        Gd, Bd = _dev(G), _dev(B)
        p.sddmm_ptr(Gd.data_ptr(), Bd.data_ptr(), out.data_ptr(), s)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert o[nnz] == (-7.0 if sentinel is None else sentinel)  # nothing past the last entry
    return o[:nnz]


@pytest.mark.parametrize("k", [7, 12, 16, 32, 64, 128, 256])
@pytest.mark.parametrize("kind", ["uniform", "wide", "underflow", "subnormal", "nonfinite"])
def test_sddmm_within_the_float64_bound(k, kind):
    a, _ = scenario("wide", k=k, m=600, seed=k)
    p = flex_amd.Plan(a, k, mutable_values=True)
    G, B = _gb(kind, a.m, a.n, k, 1)
    rows, cols = _coo(a)
    ref, T = sddmm64(rows, cols, G, B)
    got = _run_sddmm(p, G, B, a.nnz)
    assert_sddmm_within_bound(got, ref, T, k, f"k={k} {kind}")
    assert _same_bits(got, _run_sddmm(p, G, B, a.nnz)), "a second run gave other bits"


@pytest.mark.parametrize("case", ["strided", "unaligned", "unaligned_odd_k"])
def test_sddmm_strided_and_unaligned_operands(case):
    k = {"strided": 20, "unaligned": 32, "unaligned_odd_k": 13}[case]
    a, _ = scenario("zeros", k=k, m=500)
    G, B = _gb("nonfinite", a.m, a.n, k, 2)
    rows, cols = _coo(a)
    ref, T = sddmm64(rows, cols, G, B)
    if case == "strided":
        p = flex_amd.Plan(a, k, ldb=28, ldc=24, mutable_values=True)
        got = _run_sddmm(p, G, B, a.nnz, ld=(28, 24))
    else:
        p = flex_amd.Plan(a, k, mutable_values=True)
        got = _run_sddmm(p, G, B, a.nnz, unaligned=True)
    assert_sddmm_within_bound(got, ref, T, k, case)


@pytest.mark.parametrize("k", [16, 128])
def test_sddmm_edge_shapes(k):
    """Empty rows, a row of 2 600 nonzeros (and one of 9 000 in a graph too small to split it), duplicate (r, c) entries."""
    rng = np.random.default_rng(k)
    m, n = 500, 9500
    deg = rng.poisson(4, m)
    deg[rng.random(m) < 0.2] = 0
    deg[3], deg[250] = 2600, 9000
    cols = [rng.integers(0, n, d) for d in deg]
    cols[7] = np.array([5, 5, 5, 9, 5], np.int64)[: deg[7]] if deg[7] else cols[7]
    rp = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.uint32)
    col = np.concatenate(cols).astype(np.uint32)
    a = binding.HostCsr(rp, col, rng.uniform(-1, 1, rp[-1]).astype(np.float32), n=n)
    G, B = _gb("uniform", m, n, k, 3)
    rows, c64 = _coo(a)
    ref, T = sddmm64(rows, c64, G, B)
    for tn in (None, {"long_row": 24, "piece_records": 16}):
        p = flex_amd.Plan(a, k, tuning=tn, mutable_values=True)
        assert_sddmm_within_bound(_run_sddmm(p, G, B, a.nnz), ref, T, k, f"edge k={k} {tn}")


def test_sddmm_of_transposed_mapped_and_shard_plans():
    k = 32
    a = _directed(700, 650, seed=4, dup=True)
    rows, cols = _coo(a)
    # A^T: G is n x k (C's shape), B is m x k; entry e of A pairs G[col(e)] with B[row(e)]
    G, B = _gb("nonfinite", a.n, a.m, k, 4)
    ref, T = sddmm64(cols, rows, G, B)
    pt = flex_amd.Plan(a, k, transpose=True, mutable_values=True)
    assert_sddmm_within_bound(_run_sddmm(pt, G, B, a.nnz), ref, T, k, "transposed")
    # shards of A: slice-local G rows; the entries of other shards keep the sentinel
    G, B = _gb("wide", a.m, a.n, k, 5)
    ref, T = sddmm64(rows, cols, G, B)
    bounds = flex_amd.shard_rows(a, k, 3)
    out = torch.full((a.nnz,), 1234.5, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for i in range(3):
        r0, r1 = int(bounds[i]), int(bounds[i + 1])
        p = flex_amd.Plan(a, k, rows=(r0, r1), mutable_values=True)
        mine = (rows >= r0) & (rows < r1)
        before = out.cpu().numpy()
        Gd, Bd = _dev(G[r0:r1]), _dev(B)
        p.sddmm_ptr(Gd.data_ptr(), Bd.data_ptr(), out.data_ptr(), s)
        torch.cuda.synchronize()
        after = out.cpu().numpy()
        assert np.array_equal(after[~mine], before[~mine]), f"shard {i} wrote entries it does not hold"
        assert_sddmm_within_bound(after[mine], ref[mine], T[mine], k, f"shard {i}")
    # shards of A^T (columns of A): entries of A whose column lies in the shard
    G, B = _gb("uniform", a.n, a.m, k, 6)
    ref, T = sddmm64(cols, rows, G, B)
    bt = flex_amd.shard_rows(transpose(a), k, 2)
    out = torch.full((a.nnz,), 1234.5, device="cuda")
    for i in range(2):
        c0, c1 = int(bt[i]), int(bt[i + 1])
        p = flex_amd.Plan(a, k, rows=(c0, c1), transpose=True, mutable_values=True)
        Gd, Bd = _dev(G[c0:c1]), _dev(B)
        p.sddmm_ptr(Gd.data_ptr(), Bd.data_ptr(), out.data_ptr(), s)
    torch.cuda.synchronize()
    assert_sddmm_within_bound(out.cpu().numpy(), ref, T, k, "transposed shards")
    # a mapped plan of a reordered square CSR: row r' writes C row vo[r'], column c' reads B row vo[c']
    sq, _ = scenario("wide", k=k, m=600)
    vo, ap = flex_amd.perm_csr(sq, flex_amd.order_rcm(sq))
    rr, cc = _coo(ap)
    G, B = _gb("nonfinite", ap.m, ap.n, k, 7)
    ref, T = sddmm64(vo[rr].astype(np.int64), vo[cc].astype(np.int64), G, B)
    for t in (False, True):
        p = flex_amd.Plan(ap, k, vo_mp=vo, transpose=t, mutable_values=True)
        if t:  # the plan of A'^T under the same map: entry e pairs G[vo[c'(e)]] with B[vo[r'(e)]]
            ref_t, T_t = sddmm64(vo[cc].astype(np.int64), vo[rr].astype(np.int64), G, B)
            assert_sddmm_within_bound(_run_sddmm(p, G, B, ap.nnz), ref_t, T_t, k, "mapped transposed")
        else:
            assert_sddmm_within_bound(_run_sddmm(p, G, B, ap.nnz), ref, T, k, "mapped")


def test_sddmm_is_the_adjoint_of_the_plans_own_spmm():
    """<G, A(v) B> is linear in v with gradient sddmm(G, B): a float64 check of the definition on a route with split rows and bundles."""
    k = 64
    a, _ = scenario("wide", k=k, m=900, seed=9)
    a = _with_values(a, np.random.default_rng(9).uniform(-1, 1, a.nnz).astype(np.float32))
    G, B = _gb("uniform", a.m, a.n, k, 9)
    p = flex_amd.Plan(a, k, tuning={"long_row": 24, "piece_records": 16, "bundle": 1}, mutable_values=True)
    g = _run_sddmm(p, G, B, a.nnz).astype(np.float64)
    rows, cols = _coo(a)
    lin = np.dot(g, a.vals.astype(np.float64))  # <grad, v> = <G, A(v) B>
    C = _spmm({"k": k}, [p], B).astype(np.float64)
    assert abs(lin - np.sum(G.astype(np.float64) * C)) <= 1e-4 * np.sum(np.abs(G.astype(np.float64)) * np.abs(C)) + 1e-6


# ---- autograd ------------------------------------------------------------------------------------------------------------------

def _grads64(a, v, B, R):
    """float64 (grad_v, grad_B) of sum(R * A(v) B): grad_v[e] = <R[row e], B[col e]>, grad_B = A(v)^T R."""
    rows, cols = _coo(a)
    gv, Tv = sddmm64(rows, cols, R, B)
    av = _with_values(a, v)
    at = transpose(av)
    from f64ref import f64_bound, spmm_f64
    return (gv, Tv), (spmm_f64(at, R), f64_bound(at, R))


def _check_grads(a, v, B, R, gv, gB, k):
    (gv64, Tv), (gB64, bB) = _grads64(a, v, B, R)
    assert_sddmm_within_bound(gv, gv64, Tv, k, "grad_v")
    assert np.all(np.abs(gB.astype(np.float64) - gB64) <= bB), "grad_B beyond the float64 bound"


@pytest.mark.parametrize("shape", ["square", "rectangular"])
def test_sparse_operator_gradients_in_values_and_b(shape):
    k = 32
    a = _directed(400, 400 if shape == "square" else 310, seed=12, dup=True)
    rng = np.random.default_rng(12)
    v = rng.uniform(-1, 1, a.nnz).astype(np.float32)
    B = rng.uniform(-1, 1, (a.n, k)).astype(np.float32)
    R = rng.uniform(-1, 1, (a.m, k)).astype(np.float32)
    op = flex_amd.SparseOperator(a, k, learn_values=True)
    vd, Bd = _dev(v).requires_grad_(True), _dev(B).requires_grad_(True)
    C = op(Bd, values=vd)
    C.backward(_dev(R))
    torch.cuda.synchronize()
    _check_grads(a, v, B, R, vd.grad.cpu().numpy(), Bd.grad.cpu().numpy(), k)
    from f64ref import assert_within_f64_bound
    assert_within_f64_bound(_with_values(a, v), B, C.detach().cpu().numpy(), "forward")
    # op(B) alone: a's own values
    C0 = op(_dev(B)).detach().cpu().numpy()
    assert_within_f64_bound(a, B, C0, "forward with a's values")


def test_two_forwards_then_two_backwards_each_get_their_own_values():
    k = 16
    a = _directed(300, seed=13)
    rng = np.random.default_rng(13)
    op = flex_amd.SparseOperator(a, k, learn_values=True)
    runs = []
    for i in range(2):
        v = rng.uniform(-1, 1, a.nnz).astype(np.float32) * (1 + 3 * i)
        B = rng.uniform(-1, 1, (a.n, k)).astype(np.float32)
        R = rng.uniform(-1, 1, (a.m, k)).astype(np.float32)
        vd, Bd = _dev(v).requires_grad_(True), _dev(B).requires_grad_(True)
        runs.append((v, B, R, vd, Bd, op(Bd, values=vd)))
    for v, B, R, vd, Bd, C in reversed(runs):
        C.backward(_dev(R))
    torch.cuda.synchronize()
    for v, B, R, vd, Bd, C in runs:
        _check_grads(a, v, B, R, vd.grad.cpu().numpy(), Bd.grad.cpu().numpy(), k)


def test_a_training_loop_of_set_values_forward_backward_on_one_stream():
    k = 64
    a = _directed(500, seed=14)
    rng = np.random.default_rng(14)
    op = flex_amd.SparseOperator(a, k, learn_values=True, order=flex_amd.FLEX_ORDER_NATURAL)
    v = torch.nn.Parameter(_dev(rng.uniform(-1, 1, a.nnz).astype(np.float32)))
    X = torch.nn.Parameter(_dev(rng.uniform(-1, 1, (a.n, k)).astype(np.float32)))
    R = rng.uniform(-1, 1, (a.m, k)).astype(np.float32)
    opt = torch.optim.SGD([v, X], lr=0.05)
    for step in range(4):
        v_now, X_now = v.detach().cpu().numpy().copy(), X.detach().cpu().numpy().copy()
        opt.zero_grad()
        (op(X, values=v) * _dev(R)).sum().backward()
        torch.cuda.synchronize()
        _check_grads(a, v_now, X_now, R, v.grad.cpu().numpy(), X.grad.cpu().numpy(), k)
        opt.step()

"""The backward pass on the GPU: transposed SpMM plans (FLEX_PLAN_TRANSPOSE) through every route against the float64 bound and bit for
bit against the plan of the explicit A^T; flex_axw_backward against the float64 references of tests/backward_ref.py with exact classes;
the autograd layer against torch float64 CPU autograd."""
import numpy as np
import pytest

import flex_amd
import oracle
from backward_ref import _directed, backward_case, check_dw, check_dx, dw_chain, route_plans, transpose
from f64ref import AXW_SCENARIOS, ROUTES, SCENARIOS, assert_within_f64_bound, f64_bound, scenario, spmm64

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _axw():
    from flex_amd import axw
    return axw


def _n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _same_bits(x, y):
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    return bool(np.all((x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))))


# ---- transposed SpMM ---------------------------------------------------------------------------------------------------------------

def _run(spec, plans, m_out, B):
    """C [m_out x k] of plans on B, launched the way the route needs (shards, stamped, unaligned, strided)."""
    k = spec["k"]
    stream = torch.cuda.current_stream().cuda_stream
    for p in plans:
        p.self_check()
    Bd = torch.from_numpy(B).cuda()
    if spec.get("shards"):
        C = torch.cat([p(Bd) for p in plans])
    elif spec.get("stamped"):
        C = torch.full((m_out, k), -7.0, device="cuda")
        plans[0].measure_imbalance(Bd.data_ptr(), C.data_ptr(), stream)
    elif spec.get("unaligned"):
        bb = torch.zeros(B.size + 1, device="cuda")
        bb[1:] = Bd.ravel()
        cc = torch.full((m_out * k + 1,), -7.0, device="cuda")
        plans[0].spmm(bb[1:].data_ptr(), cc[1:].data_ptr(), stream)
        C = cc[1:].reshape(m_out, k)
    elif "ld" in spec:
        ldb, ldc = spec["ld"]
        Bs = torch.full((B.shape[0], ldb), float("nan"), device="cuda")
        Bs[:, :k] = Bd
        Cs = torch.full((m_out, ldc), -7.0, device="cuda")
        plans[0].spmm(Bs.data_ptr(), Cs.data_ptr(), stream)
        torch.cuda.synchronize()
        assert bool((Cs[:, k:] == -7.0).all())
        C = Cs[:, :k]
    else:
        C = plans[0](Bd)
    torch.cuda.synchronize()
    return np.ascontiguousarray(C.cpu().numpy())


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", SCENARIOS)
def test_transposed_route_within_the_float64_bound(route, name):
    """A scenario's A (non-symmetric: random columns) planned with the flag: C = A^T B within the bound of A^T, and the same bits as
    the plan of the explicit A^T."""
    spec = ROUTES[route]
    a, B = scenario(name, k=spec["k"], m=spec.get("m", 512), pattern=spec.get("pattern", "random"))
    at = transpose(a)
    C = _run(spec, route_plans(route, a, True), a.n, B)
    assert_within_f64_bound(at, B, C, f"{route}^T/{name}")
    assert _same_bits(C, _run(spec, route_plans(route, a, False), a.n, B)), (route, name)


_RECT_ROUTES = ["flat_g8", "flat_g32", "split_rows2", "two_d", "strided", "generic_unaligned", "shards", "mfma"]


@pytest.mark.parametrize("route,shape", [(r, s) for r in _RECT_ROUTES for s in ((400, 400), (300, 500), (500, 300))]
                         + [("order_rcm", (400, 400)), ("order_cluster", (400, 400)), ("mapped", (400, 400))])  # reorderings: square A
def test_transposed_rectangular_and_directed(route, shape):
    spec = ROUTES[route]
    a = _directed(shape[0], shape[1], seed=11, dup=True)
    rng = np.random.default_rng(5)
    B = rng.uniform(-1, 1, (a.m, spec["k"])).astype(np.float32)
    C = _run(spec, route_plans(route, a, True), a.n, B)
    assert_within_f64_bound(transpose(a), B, C, f"{route}^T")
    assert _same_bits(C, _run(spec, route_plans(route, a, False), a.n, B))
    if a.m == a.n:  # the mutant that plans A instead of A^T fails the bound
        with pytest.raises(AssertionError):
            assert_within_f64_bound(a, B, C, "mutant")


# ---- flex_axw_backward ---------------------------------------------------------------------------------------------------------------

def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _dout(h, D):
    """dOut [n x ld] with D in its first c columns and NaN in the padding (never read)."""
    d = torch.full((h.n, h.ld), float("nan"), device="cuda")
    d[:, : h.c] = _dev(D)
    return d


def _backward(a, X, W, D, blas=False, unaligned_x=False, order=flex_amd.FLEX_ORDER_CLUSTER, need_x=True, need_w=True):
    axw = _axw()
    h = axw.Axw(a, X.shape[1], W.shape[1], order=order | (axw.FLEX_AXW_USE_BLAS if blas else 0), backward=True)
    Xd = _dev(X)
    if unaligned_x:
        buf = torch.zeros(X.size + 1, device="cuda")
        buf[1:] = Xd.ravel()
        Xd = buf[1:].view(X.shape)
        assert Xd.data_ptr() % 16 == 4
    gx, gw = h.backward(_dout(h, D), Xd, _dev(W), need_x=need_x, need_w=need_w)
    torch.cuda.synchronize()
    return (None if gx is None else gx.cpu().numpy()), (None if gw is None else gw.cpu().numpy())


def _check_backward(a, X, W, D, gx, gw, blas=False):
    at = transpose(a)
    msg = check_dx(at, D, W, gx)
    assert msg is None, msg
    msg = check_dw(at, X, D, gw, a.n if blas else dw_chain(a.n, _n_cus()))
    assert msg is None, msg


@pytest.mark.parametrize("blas", [False, True])
@pytest.mark.parametrize("name", AXW_SCENARIOS)
def test_backward_scenarios_within_the_bound(name, blas):
    a, X, W, D = backward_case(name, 600, 128, 100)
    gx, gw = _backward(a, X, W, D, blas=blas)
    _check_backward(a, X, W, D, gx, gw, blas)


def _edge_cases():
    out = [(n, dim, c) for n in (32, 33, 517) for dim in (4, 32, 100, 128, 256) for c in (1, 100, 128, 256)]
    return out + [(89250, 128, 100), (89250, 128, 128)]  # the flickr shape


@pytest.mark.parametrize("n,dim,c", _edge_cases())
def test_backward_edge_shapes(n, dim, c):
    a, X, W, D = backward_case("uniform", n, dim, c)
    gx, gw = _backward(a, X, W, D)
    _check_backward(a, X, W, D, gx, gw)


def test_the_mutant_that_uses_a_instead_of_its_transpose_fails():
    a, X, W, D = backward_case("uniform", 517, 32, 100)
    gx, gw = _backward(a, X, W, D)
    _check_backward(a, X, W, D, gx, gw)
    assert check_dx(a, D, W, gx) is not None  # judged as if A were A^T
    assert check_dw(a, X, D, gw, dw_chain(a.n, _n_cus())) is not None


@pytest.mark.parametrize("blas", [False, True])
def test_an_unaligned_x_gives_the_right_answer(blas):
    a, X, W, D = backward_case("wide", 700, 128, 100)
    gx, gw = _backward(a, X, W, D, blas=blas, unaligned_x=True)
    _check_backward(a, X, W, D, gx, gw, blas)
    assert _same_bits(gw, _backward(a, X, W, D, blas=blas)[1])


def test_null_outputs_skip_their_product():
    a, X, W, D = backward_case("uniform", 600, 128, 100)
    gx, gw = _backward(a, X, W, D)
    gx1, gw1 = _backward(a, X, W, D, need_w=False)
    assert gw1 is None and _same_bits(gx1, gx)
    gx2, gw2 = _backward(a, X, W, D, need_x=False)
    assert gx2 is None and _same_bits(gw2, gw)
    axw = _axw()
    h = axw.Axw(a, 128, 100, backward=True)
    gw3 = torch.empty((128, 100), device="cuda")
    Xd, d = _dev(X), _dout(h, D)  # held: a temporary's memory could be handed to the next allocation before the call
    rc = axw.lib().flex_axw_backward(h._h, Xd.data_ptr(), None, d.data_ptr(), None, gw3.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)  # W is not needed
    torch.cuda.synchronize()
    assert rc == 0 and _same_bits(gw3.cpu().numpy(), gw)


def test_a_handle_without_the_flag_is_refused():
    a, X, W, D = backward_case("uniform", 64, 32, 32)
    axw = _axw()
    h = axw.Axw(a, 32, 32)
    Xd, Wd, d = _dev(X), _dev(W), _dout(h, D)
    with pytest.raises(flex_amd.FlexError, match="backward=True"):
        h.backward(d, Xd, Wd)
    with pytest.raises(flex_amd.FlexError, match="backward=True"):
        h.layer(Xd, Wd)
    gx, gw = torch.empty((64, 32), device="cuda"), torch.empty((32, 32), device="cuda")
    assert axw.lib().flex_axw_backward(h._h, Xd.data_ptr(), Wd.data_ptr(), d.data_ptr(), gx.data_ptr(), gw.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream) == -1  # the C ABI: FLEX_ERR_INVALID


@pytest.mark.parametrize("dim,c", [(128, 100), (32, 1), (256, 256), (64, 128)])
def test_the_mfma_dx_is_its_fmaf_chain_bit_for_bit(dim, c):
    """dGradX = G W^T on the forward's GEMM kernel: oracle_axw_gemm_chain(G, W^T zero-padded to cp rows), G from the transposed plan."""
    a, X, W, D = backward_case("wide", 517, dim, c)
    gx, _ = _backward(a, X, W, D)
    cp = _axw().lib().flex_axw_ld(c)
    G = torch.zeros((a.n, cp), device="cuda")
    p = flex_amd.Plan(a, c, order=flex_amd.FLEX_ORDER_CLUSTER, ldb=cp, ldc=cp, transpose=True)
    Dp = _dev(np.pad(D, ((0, 0), (0, cp - c))))
    p.spmm(Dp.data_ptr(), G.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    Wt = np.zeros((cp, dim), np.float32)
    Wt[:c] = W.T
    want = oracle.axw_gemm_chain(G.cpu().numpy(), Wt, nthreads=16)[:, :dim]
    assert _same_bits(gx, want)


def test_two_calls_give_the_same_bits():
    a, X, W, D = backward_case("wide", 2000, 128, 100)
    axw = _axw()
    h = axw.Axw(a, 128, 100, backward=True)
    d, Xd, Wd = _dout(h, D), _dev(X), _dev(W)
    r1 = [t.cpu().numpy() for t in h.backward(d, Xd, Wd)]
    r2 = [t.cpu().numpy() for t in h.backward(d, Xd, Wd)]
    assert _same_bits(r1[0], r2[0]) and _same_bits(r1[1], r2[1])


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", ["wide", "nonfinite_A", "nonfinite_X"])
def test_the_forward_is_unchanged_by_the_backward_flag(name, order):
    a, X, W, _ = backward_case(name, 600, 128, 100)
    axw = _axw()
    outs = []
    for bwd in (False, True):
        h = axw.Axw(a, 128, 100, backward=bwd)
        outs.append(h.run(_dev(X), _dev(W), order).cpu().numpy())
    assert _same_bits(outs[0], outs[1])


def test_a_captured_graph_of_forward_and_backward_matches_eager():
    a, X, W, D = backward_case("uniform", 3000, 128, 100)
    axw = _axw()
    h = axw.Axw(a, 128, 100, backward=True)
    Xd, Wd = _dev(X), _dev(W)
    d = _dout(h, D)
    out = torch.empty((h.n, h.ld), device="cuda")
    gx = torch.empty((h.n, 128), device="cuda")
    gw = torch.empty((128, 100), device="cuda")
    L = axw.lib()

    def step(stream):
        assert L.flex_axw_run(h._h, 0, Xd.data_ptr(), Wd.data_ptr(), out.data_ptr(), stream, None, None) == 0
        assert L.flex_axw_backward(h._h, Xd.data_ptr(), Wd.data_ptr(), d.data_ptr(), gx.data_ptr(), gw.data_ptr(), stream) == 0

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        step(s.cuda_stream)
    torch.cuda.synchronize()
    eager = [t.cpu().numpy() for t in (out, gx, gw)]
    for t in (out, gx, gw):
        t.fill_(-7.0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        step(s.cuda_stream)
    g.replay()
    torch.cuda.synchronize()
    for e, t in zip(eager, (out, gx, gw)):
        assert _same_bits(e, t.cpu().numpy())


# ---- autograd -------------------------------------------------------------------------------------------------------------------

def _torch_sparse64(a):
    rows = np.repeat(np.arange(a.m), np.diff(a.rowPtr.astype(np.int64)))
    idx = torch.from_numpy(np.stack([rows, a.col.astype(np.int64)]))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(a.vals.astype(np.float64)), (a.m, a.n))


@pytest.mark.parametrize("shape", [(400, 400), (300, 500), (500, 300)])
def test_sparse_operator_gradient_matches_torch_float64(shape):
    from flex_amd.autograd import SparseOperator
    a = _directed(shape[0], shape[1], seed=21)
    k = 32
    rng = np.random.default_rng(1)
    B = rng.uniform(-1, 1, (a.n, k)).astype(np.float32)
    R = rng.uniform(-1, 1, (a.m, k)).astype(np.float32)
    op = SparseOperator(a, k)
    Bd = _dev(B).requires_grad_(True)
    C = op(Bd)
    C.backward(_dev(R))
    torch.cuda.synchronize()
    B64 = torch.from_numpy(B.astype(np.float64)).requires_grad_(True)
    C64 = torch.sparse.mm(_torch_sparse64(a), B64)
    C64.backward(torch.from_numpy(R.astype(np.float64)))
    got, want = Bd.grad.cpu().numpy().astype(np.float64), B64.grad.numpy()
    assert np.all(np.abs(got - want) <= f64_bound(transpose(a), R))
    assert np.all(np.abs(C.detach().cpu().numpy() - C64.detach().numpy()) <= f64_bound(a, B))
    with pytest.raises(NotImplementedError):
        op(Bd, values=torch.ones(a.nnz, requires_grad=True))


def test_axw_layer_gradients_match_torch_float64():
    a, X, W, D = backward_case("uniform", 700, 64, 100)
    axw = _axw()
    h = axw.Axw(a, 64, 100, backward=True)
    Xd, Wd = _dev(X).requires_grad_(True), _dev(W).requires_grad_(True)
    out = h.layer(Xd, Wd)
    assert tuple(out.shape) == (a.n, 100)
    out.backward(_dev(D))
    torch.cuda.synchronize()
    X64 = torch.from_numpy(X.astype(np.float64)).requires_grad_(True)
    W64 = torch.from_numpy(W.astype(np.float64)).requires_grad_(True)
    out64 = torch.sparse.mm(_torch_sparse64(a), X64 @ W64)
    out64.backward(torch.from_numpy(D.astype(np.float64)))
    at = transpose(a)
    assert check_dx(at, D, W, Xd.grad.cpu().numpy()) is None
    assert check_dw(at, X, D, Wd.grad.cpu().numpy(), dw_chain(a.n, _n_cus())) is None
    # the float64 references of backward_ref are torch's float64 autograd, to float64 rounding (relative to the largest term sum)
    g64, s64 = spmm64(at, D), spmm64(at, D, absolute=True)
    tol_x = 1e-12 * (s64 @ np.abs(W.astype(np.float64)).T)
    tol_w = 1e-12 * (np.abs(X.astype(np.float64)).T @ s64)
    assert np.all(np.abs(X64.grad.numpy() - g64 @ W.astype(np.float64).T) <= tol_x)
    assert np.all(np.abs(W64.grad.numpy() - X.astype(np.float64).T @ g64) <= tol_w)

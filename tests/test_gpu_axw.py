"""libflex_axw.so on the GPU: the MFMA GEMM bit for bit against its fmaf-chain emulator (oracle_axw_gemm_chain), flex_axw_run end to
end against the composed float64 bound of its association order (tests/f64ref.py) with exact classes and +0 padding, and
flex_gather_rows bit for bit."""
import numpy as np
import pytest

import flex_amd
import oracle
from f64ref import AX_W, AXW_SCENARIOS, A_XW, axw_reference, axw_scenario, check_axw, check_gemm_bound

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HIP_ERROR_INVALID_VALUE = 1
SENTINEL = np.float32(-3.4028235e38)  # -FLT_MAX: no result of these inputs comes near it (every stage sum < 2^120)


def _axw():
    from flex_amd import axw
    return axw


def _n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _same_bits(x, y):
    """Bitwise equality, except that any NaN matches any NaN (+0 and -0 differ)."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    return (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))


def _first_diff(got, want):
    bad = ~_same_bits(got, want)
    r, j = np.argwhere(bad)[0]
    return f"{int(bad.sum())} entries differ; first at ({r}, {j}): got {got[r, j]!r} ({got[r, j].view(np.uint32):#010x}), " \
           f"want {want[r, j]!r} ({want[r, j].view(np.uint32):#010x})"


# ---- the MFMA GEMM, bit for bit --------------------------------------------------------------------------------------------------

GEMM_N = [32, 33, 47, 63, 64, 65, 97, 1000, 140001]  # 140 001 > 8 waves x 256 CUs x 32 rows x 2: waves take several panels
GEMM_DIM = [4, 8, 12, 20, 60, 64, 68, 124, 128, 132, 196, 252, 256]
GEMM_CP = [32, 64, 96, 128, 160, 224, 256]


def _gemm_cases():
    """(n, dim, cp, c, scenario): a seeded subset of N x DIM x CP that meets every value of each axis, the 3-tile (96-column) pass at
    both of its widths, and every scenario in L and W."""
    rng = np.random.default_rng(2024)
    cases = [(140001, 4, 32), (1000, 256, 256), (64, 128, 96), (97, 20, 224)]  # the big n at a small dim x cp; NT = 3 twice
    dims = [d for d in GEMM_DIM if d not in (4, 256, 128, 20)]
    ns = [n for n in GEMM_N if n not in (140001, 1000, 64, 97)]
    cps = list(rng.permutation([cp for cp in GEMM_CP if cp not in (32, 256, 96, 224)]))
    for i, d in enumerate(rng.permutation(dims)):
        cases.append((ns[i % len(ns)] if i < len(ns) else int(rng.choice(GEMM_N[:8])), int(d), int(cps[i % len(cps)] if i < len(cps) else rng.choice(GEMM_CP))))
    out = []
    for i, (n, d, cp) in enumerate(cases):
        c = cp - int(rng.integers(0, 32)) if i % 3 else cp  # padding columns in two cases of three
        out.append((n, d, cp, max(1, c), AXW_SCENARIOS[i % len(AXW_SCENARIOS)]))
    return out


GEMM_CASES = _gemm_cases()


def test_the_gemm_cases_cover_every_axis():
    assert {n for n, *_ in GEMM_CASES} == set(GEMM_N)
    assert {d for _, d, *_ in GEMM_CASES} == set(GEMM_DIM)
    assert {cp for _, _, cp, *_ in GEMM_CASES} == set(GEMM_CP)
    assert {s for *_, s in GEMM_CASES} == set(AXW_SCENARIOS)
    assert sum(n * d * cp for n, d, cp, *_ in GEMM_CASES) < 2e9  # emulated fmas


def run_gemm(L, Wp, c, n_cus=None):
    """Out of the MFMA kernel, every entry of n x cp first set to SENTINEL."""
    n, dim = L.shape
    cp = Wp.shape[1]
    Ld, Wd = torch.from_numpy(L).cuda(), torch.from_numpy(Wp).cuda()
    Od = torch.full((n, cp), float(SENTINEL), device="cuda")
    rc = _axw()._gemm_launch(Ld.data_ptr(), Wd.data_ptr(), Od.data_ptr(), n, dim, c, cp, n_cus or _n_cus(),
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return Od.cpu().numpy()


@pytest.mark.parametrize("n,dim,cp,c,name", GEMM_CASES)
def test_the_gemm_kernel_is_its_fmaf_chain_bit_for_bit(n, dim, cp, c, name):
    _, L, W = axw_scenario(name, n, dim, c, seed=1)
    Wp = np.zeros((dim, cp), np.float32)
    Wp[:, :c] = W
    out = run_gemm(L, Wp, c)
    assert not (out == SENTINEL).any(), "entries left unwritten"
    assert not np.ascontiguousarray(out[:, c:]).view(np.uint32).any(), "padding columns are not +0.0"
    want = oracle.axw_gemm_chain(L, Wp, nthreads=16)[:, :c]
    got = out[:, :c]
    assert _same_bits(got, want).all(), f"{name} n={n} dim={dim} cp={cp} c={c}: " + _first_diff(got, want)
    assert check_gemm_bound(L, W, got) is None


def test_a_short_grid_deals_panels_the_same_way():
    """Fewer CUs than the card has: every wave walks many panels and the second wave of a SIMD gets work; the result is unchanged."""
    _, L, W = axw_scenario("wide", 5000, 68, 96, seed=2)
    full = run_gemm(L, W, 96)
    for n_cus in (1, 3):
        assert _same_bits(run_gemm(L, W, 96, n_cus), full).all()


def test_the_launcher_refuses_what_it_cannot_take():
    """Every call would stay inside these buffers even if launched: the pointers sit 64 rows into allocations far larger than needed."""
    big = torch.ones(400 * 272, device="cuda")
    off = 64 * 272
    Lp, Wp, Op = (big.data_ptr() + 4 * off for _ in range(3))
    s = torch.cuda.current_stream().cuda_stream
    go = _axw()._gemm_launch
    for args in [(31, 8, 32, 32), (0, 8, 32, 32), (40, 6, 32, 32), (40, 260, 32, 32), (40, 0, 32, 32), (40, 8, 48, 48),
                 (40, 8, 32, 0), (40, 8, 32, 33)]:
        assert go(Lp, Wp, Op, *args, _n_cus(), s) == HIP_ERROR_INVALID_VALUE, args
    assert go(Lp + 4, Wp, Op, 40, 8, 32, 32, _n_cus(), s) == HIP_ERROR_INVALID_VALUE  # L 4 bytes off 16-byte alignment
    assert go(Lp, Wp + 8, Op, 40, 8, 32, 32, _n_cus(), s) == HIP_ERROR_INVALID_VALUE  # Wp 8 bytes off
    assert go(Lp, Wp, Op, 40, 8, 32, 32, 0, s) == HIP_ERROR_INVALID_VALUE
    assert go(0, Wp, Op, 40, 8, 32, 32, _n_cus(), s) == HIP_ERROR_INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((big == 1).all())  # nothing was launched


# ---- flex_axw_run end to end -----------------------------------------------------------------------------------------------------

ORDERS = {"natural": flex_amd.FLEX_ORDER_NATURAL, "cluster": flex_amd.FLEX_ORDER_CLUSTER, "rcm": flex_amd.FLEX_ORDER_RCM}
# (n, dim, c, row order, scenario): every n, dim and c of the issue's lists, every row order, every scenario
RUN_CASES = [
    (5, 1, 1, "natural", "uniform"),
    (31, 7, 31, "cluster", "wide"),
    (32, 4, 32, "rcm", "zeros"),
    (33, 64, 33, "natural", "nonfinite_A"),
    (40, 128, 65, "cluster", "nonfinite_X"),
    (40, 4, 100, "rcm", "large_X_subnormal_W"),
    (3000, 132, 96, "rcm", "subnormal_X_large_W"),
    (3000, 256, 100, "natural", "nonfinite_W"),
    (3000, 260, 130, "rcm", "cancel"),
    (3000, 128, 96, "natural", "huge"),
    (60000, 64, 130, "cluster", "products_underflow"),
]


def uses_blas(n, dim, blas_flag, x_aligned=True, order=A_XW):
    """The library's rule (axw.cpp): rocBLAS when asked, for shapes the MFMA kernel does not take, and for an X that is not 16-byte
    aligned in order A_XW (the only order whose GEMM reads X)."""
    return bool(blas_flag) or dim % 4 != 0 or dim > 256 or n < 32 or (order == A_XW and not x_aligned)


def test_the_run_cases_cover_every_axis_and_both_gemm_paths():
    assert {n for n, *_ in RUN_CASES} == {5, 31, 32, 33, 40, 3000, 60000}
    assert {d for _, d, *_ in RUN_CASES} == {1, 4, 7, 64, 128, 132, 256, 260}
    assert {c for _, _, c, *_ in RUN_CASES} == {1, 31, 32, 33, 65, 96, 100, 130}
    assert {o for *_, o, _ in RUN_CASES} == set(ORDERS)
    assert {s for *_, s in RUN_CASES} == set(AXW_SCENARIOS)
    paths = {uses_blas(n, d, flag) for n, d, *_ in RUN_CASES for flag in (0, 1)}
    assert paths == {True, False}
    assert {uses_blas(n, d, 0) for n, d, *_ in RUN_CASES} == {True, False}  # both without the flag too


@pytest.mark.parametrize("n,dim,c,row_order,name", RUN_CASES)
def test_axw_run_within_the_composed_bound(n, dim, c, row_order, name):
    """Both orders and AUTO, with the MFMA kernel where it applies and with FLEX_AXW_USE_BLAS: every entry within the bound of its
    association order or of exactly its class, the padding +0.0 bit for bit, and AUTO bit-identical to the order it names."""
    axw = _axw()
    a, X, W = axw_scenario(name, n, dim, c, seed=9)
    refs = {order: axw_reference(a, X, W, order, route=name) for order in (A_XW, AX_W)}
    Xd, Wd = torch.from_numpy(X).cuda(), torch.from_numpy(W).cuda()
    for flag in (0, axw.FLEX_AXW_USE_BLAS):
        h = axw.Axw(a, dim, c, order=ORDERS[row_order] | flag)
        outs = {}
        for order in (A_XW, AX_W):
            out = h.run(Xd, Wd, order)
            torch.cuda.synchronize()
            outs[order] = out.cpu().numpy()
            route = f"{name} n={n} dim={dim} c={c} {row_order} order={order} blas={uses_blas(n, dim, flag)}"
            msg = check_axw(a, X, W, outs[order], order, route=route, ref=refs[order])
            assert msg is None, msg
        auto = h.run(Xd, Wd).cpu().numpy()
        named = A_XW if h.ld <= dim else AX_W
        assert _same_bits(auto, outs[named]).all(), _first_diff(auto, outs[named])
        h.destroy()


def test_an_x_off_16_byte_alignment_gives_the_right_answer():
    """X 4 bytes off alignment: order A_XW takes rocBLAS for the GEMM (the kernel loads 16 bytes at a time), AX_W gives it to the SpMM's
    generic kernels."""
    axw = _axw()
    n, dim, c = 3000, 64, 33
    assert uses_blas(n, dim, 0) is False and uses_blas(n, dim, 0, x_aligned=False) is True
    a, X, W = axw_scenario("wide", n, dim, c, seed=10)
    buf = torch.zeros(n * dim + 1, device="cuda")
    Xv = buf[1:].view(n, dim)
    Xv.copy_(torch.from_numpy(X).cuda())
    assert Xv.data_ptr() % 16 == 4
    h = axw.Axw(a, dim, c)
    for order in (A_XW, AX_W):
        out = h.run(Xv, torch.from_numpy(W).cuda(), order)
        torch.cuda.synchronize()
        msg = check_axw(a, X, W, out.cpu().numpy(), order, route=f"unaligned X order={order}")
        assert msg is None, msg
    h.destroy()


def _one_inf_case(where):
    """n = 64 (the MFMA kernel), dim = 8, c = 5 (27 padding columns), uniform values and ONE +inf: in X or in A."""
    a, X, W = axw_scenario("uniform", 64, 8, 5, seed=12)
    if where == "X":
        X[10, 3] = np.inf
    else:
        vals = a.vals.copy()
        vals[int(a.rowPtr[20])] = np.inf
        a = flex_amd.HostCsr(a.rowPtr, a.col, vals, n=a.n)
    return a, X, W


@pytest.mark.parametrize("where,order,blas", [("X", A_XW, 0), ("X", AX_W, 0), ("X", A_XW, 1), ("X", AX_W, 1), ("A", A_XW, 0),
                                              ("A", A_XW, 1), ("A", AX_W, 0)])
def test_padding_is_plus_zero_with_one_inf_in_x_or_a(where, order, blas):
    """Wp's zero columns times an inf are NaN: the GEMM (kernel and rocBLAS) and, in order A_XW with an inf in A, the SpMM over X W's
    zero padding put NaN in columns c .. cp-1 unless the library keeps them +0."""
    axw = _axw()
    a, X, W = _one_inf_case(where)
    h = axw.Axw(a, 8, 5, order=flex_amd.FLEX_ORDER_NATURAL | (axw.FLEX_AXW_USE_BLAS if blas else 0))
    out = h.run(torch.from_numpy(X).cuda(), torch.from_numpy(W).cuda(), order).cpu().numpy()
    h.destroy()
    pad = np.ascontiguousarray(out[:, 5:])
    bad = pad.view(np.uint32) != 0
    assert not bad.any(), f"{int(bad.sum())} padding entries are not +0.0, e.g. {pad[bad][:4]}"
    msg = check_axw(a, X, W, out, order)
    assert msg is None, msg


# ---- flex_gather_rows, bit for bit -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 3, 4, 5, 64, 100, 257])
def test_gather_rows_is_a_bitwise_copy(k):
    """dst[r] = src[idx[r]] for n = 20 000 rows (past the 2048-workgroup cap: the grid-stride loop runs), reversed and repeated
    indices, NaN payloads (quiet and signalling) and -0 kept; 16-byte aligned pointers and pointers 4 bytes off."""
    rng = np.random.default_rng(k)
    n_src, n = 7000, 20000
    bits = rng.integers(0, 1 << 32, size=(n_src, k), dtype=np.uint64).astype(np.uint32)  # every pattern: NaN payloads, subnormals
    bits[rng.random((n_src, k)) < 0.05] = 0x80000000  # -0
    bits[rng.random((n_src, k)) < 0.05] = 0x7F800001  # a signalling NaN
    idx = np.concatenate([np.arange(n_src)[::-1], rng.integers(0, n_src, size=n - 2 * n_src), np.full(n_src, 17)]).astype(np.int32)
    want = bits[idx]
    idx_d = torch.from_numpy(idx).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for off in (0, 1):  # floats of offset from a 256-byte aligned allocation
        src = torch.zeros(n_src * k + off, dtype=torch.int32, device="cuda")
        dst = torch.full((n * k + off,), 0x7FBADBAD, dtype=torch.int32, device="cuda")
        src[off:] = torch.from_numpy(bits.view(np.int32).ravel()).cuda()
        flex_amd.gather_rows(dst[off:].data_ptr(), src[off:].data_ptr(), idx_d.data_ptr(), n, k, stream)
        torch.cuda.synchronize()
        got = dst.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[off:].reshape(n, k), want), (k, off)
        assert (got[:off] == 0x7FBADBAD).all()

"""The bf16 A*X*W layer on the GPU (include/flex_axw.h: FLEX_AXW_BF16): its bf16 MFMA GEMM alone and flex_axw_run_bf16 in both orders
against float64 and the bounds of tests/axw_bf16_ref.py, inf / NaN classes and +0 padding, and what the calls refuse."""
import numpy as np
import pytest

import axw_bf16_ref as ref
import f64ref
from attention_bf16_ref import to_bf16
from flex_amd import FlexError, HostCsr, axw

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HIP_ERROR_INVALID_VALUE, FLEX_ERR_INVALID, FLEX_ERR_UNSUPPORTED = 1, -1, -4


_dev = lambda x: torch.from_numpy(to_bf16(x).view(np.int16)).cuda().view(torch.bfloat16)  # noqa: E731
_bits = lambda t: t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)  # noqa: E731


def run_gemm(L, W, cp, n_cus=None):
    """bf16 bits [n x cp] of the kernel on L and W padded to cp columns; Out starts as -7.0 everywhere."""
    (n, dim), c = L.shape, W.shape[1]
    Ld, Wd = _dev(L), _dev(np.pad(W, ((0, 0), (0, cp - c))))
    Od = torch.full((n, cp), -7.0, dtype=torch.bfloat16, device="cuda")
    rc = axw._gemm_bf16_launch(Ld.data_ptr(), Wd.data_ptr(), Od.data_ptr(), n, dim, c, cp,
                               n_cus or torch.cuda.get_device_properties(0).multi_processor_count, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return _bits(Od)


# n: one panel, an overlapping last panel (33, 95), 20 panels on one and two workgroups (the persistent loop, the second wave of a SIMD);
# dim: one k-step, an odd number, 9 (a unit of 8 and a unit of 1), the largest W; (c, cp): every tile count, padding inside a tile
@pytest.mark.parametrize("cancel", [False, True], ids=["plain", "cancel"])
@pytest.mark.parametrize("n,dim,c,cp,n_cus", [(32, 16, 1, 64, None), (33, 48, 64, 64, None), (95, 256, 100, 128, None), (613, 48, 200, 256, 1),
                                              (613, 256, 256, 256, 2), (33, 144, 130, 192, None), (613, 16, 64, 64, 2)])
def test_the_bf16_gemm_is_within_its_float64_bound(n, dim, c, cp, n_cus, cancel):
    L, W = ref.operands(np.random.default_rng([5, n, dim, c, cancel]), n, dim, c, cancel)
    r64, g = f64ref.gemm_f64(L, W), ref.gemm_bound(L, W)
    msg, worst = ref.check(r64, g, run_gemm(L, W, cp, n_cus), f"gemm n={n} dim={dim} c={c} cp={cp}")
    print(f"worst err/bound {worst:.4g} (gamma({ref.M} dim))")
    assert msg is None, msg


def _layer(n, dim, c, seed, long_row=False, positive=False):
    """(A, X, W): the f64ref pattern, or short rows and one of 5 000 entries (cut into pieces: its fix-up runs between the two stages)"""
    rng = np.random.default_rng([seed, n, dim, c])
    if long_row:
        deg = rng.integers(1, 9, size=n)
        deg[7] = 5000
        rp = np.concatenate([[0], np.cumsum(deg)])
        col = rng.integers(0, n, size=rp[-1])
    else:
        rp, col = f64ref._axw_pattern(rng, n)
    vals = ref.rounded(f64ref._logu(rng, -4, 4, int(rp[-1])))
    X, W = ref.operands(rng, n, dim, c)
    return HostCsr(rp.astype(np.uint32), col.astype(np.uint32), vals, n=n), *((np.abs(X), np.abs(W)) if positive else (X, W))


def run_layer(a, X, W, order):
    h = axw.Axw(a, X.shape[1], W.shape[1], bf16=True)
    out, auto = h.run(_dev(X), _dev(W), order), h.run(_dev(X), _dev(W))
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (a.n, h.ld) and h.ld % 64 == 0
    rule = f64ref.A_XW if h.ld <= h.dim else f64ref.AX_W
    assert (order != rule) or np.array_equal(_bits(out), _bits(auto)), "AUTO is the order with fewer SpMM columns, bit for bit"
    h.destroy()
    return _bits(out)


@pytest.mark.parametrize("order", [f64ref.A_XW, f64ref.AX_W])
@pytest.mark.parametrize("n,dim,c,long_row", [(512, 16, 7, False), (512, 128, 100, False), (512, 256, 64, False), (5120, 128, 100, True)])
def test_the_bf16_layer_is_within_its_composed_bound(n, dim, c, long_row, order):
    a, X, W = _layer(n, dim, c, 11, long_row)
    msg, worst = ref.check(*ref.layer_reference(a, X, W, order), run_layer(a, X, W, order), f"layer order={order} dim={dim} c={c}")
    print(f"worst err/bound {worst:.4g}")
    assert msg is None, msg


@pytest.mark.parametrize("where", ["gemm", "X_A_XW", "X_AX_W", "A_A_XW"])
def test_inf_and_nan_keep_the_reference_classes_and_the_padding_stays_zero(where):
    n = 97
    a, X, W = _layer(n, 48, 40, 13, positive=True)
    if where == "A_A_XW":
        a.vals[a.rowPtr[n // 3] + 1] = np.inf
    else:
        X[3, 5], X[n - 2, 0] = np.inf, np.nan
    if where == "gemm":
        r64, b, out = f64ref.gemm_f64(X, W), ref.gemm_bound(X, W), run_gemm(X, W, 64)
    else:
        order = f64ref.AX_W if where == "X_AX_W" else f64ref.A_XW
        r64, b, out = *ref.layer_reference(a, X, W, order), run_layer(a, X, W, order)
    msg, _ = ref.check(r64, b, out, where)
    assert msg is None, msg


@pytest.mark.parametrize("what", ["launcher", "create", "run", "dtype"])
def test_what_the_bf16_calls_refuse(what):
    a, _, _ = _layer(64, 16, 8, 17)
    x32, w32 = torch.zeros((64, 16), device="cuda"), torch.zeros((16, 8), device="cuda")
    if what == "launcher":
        p, ok = torch.zeros(1 << 16, dtype=torch.bfloat16, device="cuda").data_ptr(), dict(n=64, dim=32, c=64, cp=64, n_cus=4)
        for kw in (dict(n=31), dict(dim=24), dict(dim=272), dict(dim=0), dict(cp=96), dict(cp=320), dict(c=0), dict(c=65), dict(n_cus=0)):
            assert axw._gemm_bf16_launch(p, p, p, **{**ok, **kw}) == HIP_ERROR_INVALID_VALUE, kw
        for ptrs in ((p + 8, p, p), (p, p + 2, p), (p, p, p + 8), (0, p, p)):
            assert axw._gemm_bf16_launch(*ptrs, **ok) == HIP_ERROR_INVALID_VALUE, ptrs
    elif what == "create":
        for kw in (dict(dim=16, c=8, backward=True), dict(dim=24, c=8), dict(dim=16, c=300)):
            with pytest.raises(FlexError, match=rf"\({FLEX_ERR_UNSUPPORTED}\)"):
                axw.Axw(a, bf16=True, **kw)
    elif what == "run":
        for bf16, call in ((True, axw.lib().flex_axw_run), (False, axw.lib().flex_axw_run_bf16)):
            h = axw.Axw(a, 16, 8, bf16=bf16)
            out = torch.zeros((64, 64), device="cuda")
            assert call(h._h, 0, x32.data_ptr(), w32.data_ptr(), out.data_ptr(), None, None, None) == FLEX_ERR_INVALID
            h.destroy()
    else:
        h = axw.Axw(a, 16, 8, bf16=True)
        with pytest.raises(TypeError):
            h.run(x32, w32)
        with pytest.raises(FlexError):
            h.backward(None, None, None)
        h.destroy()

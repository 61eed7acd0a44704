"""The bf16 A*X*W layer at 256 < dim <= 4096 on the GPU (axw_bf16_wide_kernels.hip): the wide GEMM, dX and dW launchers alone and the
layer through Axw, against float64 and the bounds of tests/axw_bf16_ref.py and tests/axw_bf16_backward_ref.py, which hold unchanged."""
import numpy as np
import pytest

import axw_bf16_backward_ref as bref
import axw_bf16_ref as ref
import f64ref
from flex_amd import FlexError, axw
from test_gpu_axw_bf16 import _bits, _dev, _layer

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HIP_ERROR_INVALID_VALUE, FLEX_ERR_UNSUPPORTED = 1, -4

_cus = lambda n_cus=None: n_cus or torch.cuda.get_device_properties(0).multi_processor_count  # noqa: E731
_stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
_filled = lambda *shape: torch.full(shape, -7.0, dtype=torch.bfloat16, device="cuda")  # noqa: E731


def run_gemm(L, W, cp, n_cus=None):
    (n, dim), c = L.shape, W.shape[1]
    Ld, Wd, Wf, Od = _dev(L), _dev(W), _filled(dim * cp), _filled(n, cp)
    rc = axw._gemm_bf16_wide_launch(Ld.data_ptr(), Wd.data_ptr(), Wf.data_ptr(), Od.data_ptr(), n, dim, c, cp, _cus(n_cus), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return _bits(Od)


# A slab of W is 128 values of k.  dim: 272 = two slabs and one k-step (the first width past the narrow kernel), 384 and 512 = whole slabs,
# an odd and an even count (both LDS buffers end a round), 400 = three slabs and a k-step, 4096; n: one panel, an overlapping last panel,
# 613 rows on one and two workgroups (several rounds, the second wave of a SIMD, both panels of a wave at cp = 64, a round whose last
# waves have no panel); (c, cp): every tile count, padding inside a tile, c = 1
@pytest.mark.parametrize("cancel", [False, True], ids=["plain", "cancel"])
@pytest.mark.parametrize("n,dim,c,cp,n_cus", [(32, 272, 1, 64, None), (33, 384, 64, 64, None), (95, 400, 100, 128, None), (613, 272, 200, 256, 1),
                                              (613, 512, 256, 256, 2), (33, 4096, 130, 192, None), (613, 400, 64, 64, 2), (613, 384, 128, 128, 1)])
def test_the_wide_gemm_is_within_its_float64_bound(n, dim, c, cp, n_cus, cancel):
    L, W = ref.operands(np.random.default_rng([5, n, dim, c, cancel]), n, dim, c, cancel)
    msg, worst = ref.check(f64ref.gemm_f64(L, W), ref.gemm_bound(L, W), run_gemm(L, W, cp, n_cus), f"gemm n={n} dim={dim} c={c} cp={cp}")
    print(f"worst err/bound {worst:.4g} (gamma({ref.M} dim))")
    assert msg is None, msg


# one pass and a 32-column last pass, two full passes, a last pass narrower than 256, 16 passes
@pytest.mark.parametrize("n,cp,dim", [(33, 64, 288), (95, 128, 512), (613, 256, 544), (613, 64, 4096)])
def test_the_wide_dx_product_is_within_its_float64_bound(n, cp, dim):
    G, Wt = ref.operands(np.random.default_rng([9, n, cp, dim]), n, cp, dim)
    out, Gd, Wd = _filled(n, dim), _dev(G), _dev(Wt)
    rc = axw._dx_bf16_wide_launch(Gd.data_ptr(), Wd.data_ptr(), out.data_ptr(), n, cp, dim, _cus(), _stream())
    assert rc == 0, rc
    msg, worst = ref.check(f64ref.gemm_f64(G, Wt), ref.gemm_bound(G, Wt), _bits(out), f"dX n={n} cp={cp} dim={dim}")
    print(f"worst err/bound {worst:.4g}")
    assert msg is None, msg


# slices by the rule of flex_axw_dw_bf16_wide_slices on a card of at least 20 CUs: S0 = min(ceil(n / 256), ceil(2 CUs / blocks), n // (2 c))
@pytest.mark.parametrize("cancel", [False, True], ids=["plain", "cancel"])
@pytest.mark.parametrize("n,dim,c,cp,n_cus,want", [(33, 288, 1, 64, None, 1), (47, 512, 100, 128, 1, 1), (613, 544, 200, 256, 2, 1),
                                                   (613, 544, 64, 64, 8, 3), (5120, 1024, 64, 64, None, 20)])
def test_the_wide_dw_kernel_is_within_its_float64_bound(n, dim, c, cp, n_cus, want, cancel):
    Xt, G = ref.operands(np.random.default_rng([7, n, dim, c, cancel]), dim, n + n % 2, c, cancel)
    X, G = np.ascontiguousarray(Xt.T[:n]), G[:n]
    slices = axw._dw_bf16_wide_slices(n, dim, c, _cus(n_cus))
    assert slices == want and (n < 2 * c or slices * dim * c * 4 <= n * dim * 2)
    Xd, Gd = _dev(X), _dev(np.pad(G, ((0, 0), (0, cp - c)), constant_values=5.0))  # G's padding columns are computed and dropped
    out, part = _filled(dim * c + 64), torch.empty(slices * dim * c, device="cuda")
    rc = axw._dw_bf16_wide_launch(Xd.data_ptr(), Gd.data_ptr(), out.data_ptr(), part.data_ptr(), n, dim, c, cp, _cus(n_cus), _stream())
    assert rc == 0 and (out[dim * c:] == -7.0).all(), (rc, "written past dim x c")
    msg, worst = ref.check(*bref.dw_reference(X, G, slices), _bits(out[: dim * c].view(dim, c)), f"dW n={n} dim={dim} c={c} slices={slices}")
    print(f"worst err/bound {worst:.4g} (gamma({ref.M} L))")
    assert msg is None, msg


def _case(n, dim, c, seed, long_row=False, positive=False, inf_in_a=False):
    a, X, W = _layer(n, dim, c, seed, long_row, positive)
    if inf_in_a:
        a.vals[a.rowPtr[n // 3] + 1] = np.inf
    dOut = ref.rounded(f64ref._logu(np.random.default_rng([seed, n, c]), -4, 4, (n, c)))
    return a, X, W, (np.abs(dOut) if positive else dOut), axw.Axw(a, dim, c, bf16=True, backward=True)


def _check_forward(a, X, W, h, what):
    outs = {order: _bits(h.run(_dev(X), _dev(W), order)) for order in (f64ref.A_XW, f64ref.AX_W)}
    for order, out in outs.items():
        msg, worst = ref.check(*ref.layer_reference(a, X, W, order), out, f"forward order={order} {what}")
        print(f"order {order} worst err/bound {worst:.4g}")
        assert msg is None, msg
    assert np.array_equal(_bits(h.run(_dev(X), _dev(W))), outs[f64ref.A_XW]), "AUTO is A (X W) at dim > cp, bit for bit"


def _check_backward(a, X, W, dOut, h, gx, gw, what, R=(None, None)):
    slices = axw._dw_bf16_wide_slices(a.n, h.dim, h.c, _cus())
    for name, (r, b), got, r2 in zip(("dX", "dW"), bref.backward_reference(a, X, W, dOut, h.ld, slices), (gx, gw), R):
        msg, worst = ref.check(r if r2 is None else r2, b, _bits(got), f"{name} {what}")
        print(f"{name} worst err/bound {worst:.4g}")
        assert got.dtype == torch.bfloat16 and msg is None, msg


@pytest.mark.parametrize("n,dim,c,long_row", [(512, 320, 64, False), (512, 1024, 100, False), (5120, 512, 100, True)])
def test_the_wide_layer_is_within_its_composed_bounds(n, dim, c, long_row):
    a, X, W, dOut, h = _case(n, dim, c, 11, long_row)
    _check_forward(a, X, W, h, f"n={n} dim={dim} c={c}")
    pad = lambda v: _dev(np.pad(dOut, ((0, 0), (0, h.ld - c)), constant_values=v))  # noqa: E731
    Xd, Wd, d0 = _dev(X), _dev(W), pad(0.0)
    gx, gw = h.backward(d0, Xd, Wd)
    _check_backward(a, X, W, dOut, h, gx, gw, f"n={n} dim={dim} c={c}")
    same = lambda p, q: np.array_equal(_bits(p), _bits(q))  # noqa: E731
    for v, why in ((0.0, "a second call gives other bits"), (3.0, "finite padding columns of dOut change the result")):
        gx2, gw2 = h.backward(pad(v), Xd, Wd)
        assert same(gx, gx2) and same(gw, gw2), why
    for skip in (0, 1):  # a NULL dGradX (0) or dGradW (1) skips that product, its input may be NULL, and the other comes out the same
        outs = [torch.full_like(gx, -7.0), torch.full_like(gw, -7.0)]
        args = [None if skip else Xd.data_ptr(), Wd.data_ptr() if skip else None, d0.data_ptr(),
                *(None if i == skip else o.data_ptr() for i, o in enumerate(outs))]
        assert axw.lib().flex_axw_backward_bf16(h._h, *args, _stream()) == 0
        assert (outs[skip] == -7.0).all() and same(outs[1 - skip], (gx, gw)[1 - skip]), skip
    h.destroy()


def test_autograd_through_the_wide_layer():
    a, X, W, dOut, h = _case(n := 512, 320, 24, 17)
    Xd, Wd = _dev(X).requires_grad_(), _dev(W).requires_grad_()
    h.layer(Xd, Wd).backward(_dev(dOut))
    A64 = torch.zeros((n, n), dtype=torch.float64)
    A64.index_put_((torch.from_numpy(np.repeat(np.arange(n), np.diff(a.rowPtr.astype(np.int64)))), torch.from_numpy(a.col.astype(np.int64))),
                   torch.from_numpy(a.vals.astype(np.float64)), accumulate=True)
    X64, W64 = torch.from_numpy(X.astype(np.float64)).requires_grad_(), torch.from_numpy(W.astype(np.float64)).requires_grad_()
    (A64 @ X64 @ W64).backward(torch.from_numpy(dOut.astype(np.float64)))
    _check_backward(a, X, W, dOut, h, Xd.grad, Wd.grad, "autograd", (X64.grad.numpy(), W64.grad.numpy()))
    h.destroy()


@pytest.mark.parametrize("where", ["X", "dOut", "A"])
def test_inf_and_nan_keep_the_reference_classes_and_the_padding_stays_zero(where):
    n, dim, c = 97, 272, 40
    a, X, W = _layer(n, dim, c, 13, positive=True)
    dOut = np.abs(ref.rounded(f64ref._logu(np.random.default_rng([13, n, c]), -4, 4, (n, c))))
    if where == "A":
        a.vals[a.rowPtr[n // 3] + 1] = np.inf
    else:
        t = X if where == "X" else dOut
        t[3, 5], t[n - 2, 0] = np.inf, np.nan
    hf = axw.Axw(a, dim, c, bf16=True)  # 272 % 32 != 0: forward only
    for order in {"X": (f64ref.A_XW, f64ref.AX_W), "A": (f64ref.A_XW,), "dOut": ()}[where]:
        msg, _ = ref.check(*ref.layer_reference(a, X, W, order), _bits(hf.run(_dev(X), _dev(W), order)), f"{where} order={order}")
        assert msg is None, msg
    hf.destroy()
    if where != "X":  # the backward needs dim % 32 == 0: the same operands, 16 more columns of X and rows of W
        X2, W2 = np.pad(X, ((0, 0), (0, 16)), constant_values=1.0), np.pad(W, ((0, 16), (0, 0)), constant_values=1.0)
        hb = axw.Axw(a, dim + 16, c, bf16=True, backward=True)
        gx, gw = hb.backward(_dev(np.pad(dOut, ((0, 0), (0, hb.ld - c)))), _dev(X2), _dev(W2))
        _check_backward(a, X2, W2, dOut, hb, gx, gw, where)
        hb.destroy()


@pytest.mark.parametrize("what", ["launchers", "create"])
def test_what_the_wide_path_refuses(what):
    a, _, _ = _layer(64, 16, 8, 19)
    if what == "create":
        for kw in (dict(dim=4112, c=8), dict(dim=272, c=8, backward=True)):
            with pytest.raises(FlexError, match=rf"\({FLEX_ERR_UNSUPPORTED}\)"):
                axw.Axw(a, bf16=True, **kw)
        axw.Axw(a, 272, 8, bf16=True).destroy()
        return
    buf, fbuf = torch.zeros(1 << 19, dtype=torch.bfloat16, device="cuda"), torch.zeros(1 << 16, device="cuda")
    p, fp, ok = buf.data_ptr(), fbuf.data_ptr(), dict(n=64, dim=288, c=64, cp=64, n_cus=4)
    for kw in (dict(dim=256), dict(dim=264), dict(dim=4112), dict(n=31), dict(cp=96), dict(cp=320), dict(c=0), dict(c=65), dict(n_cus=0)):
        args = {**ok, **kw}
        assert axw._gemm_bf16_wide_launch(p, p, p, p, **args) == HIP_ERROR_INVALID_VALUE, kw
        if kw != dict(cp=96):  # the dW kernel takes any multiple of 32, as its narrow twin does
            assert axw._dw_bf16_wide_launch(p, p, p, fp, **args) == HIP_ERROR_INVALID_VALUE, kw
        if "c" not in kw:
            assert axw._dx_bf16_wide_launch(p, p, p, **{k: v for k, v in args.items() if k != "c"}) == HIP_ERROR_INVALID_VALUE, kw
    assert axw._dx_bf16_wide_launch(p, p, p, 64, 64, 272, 4) == HIP_ERROR_INVALID_VALUE and axw._dw_bf16_wide_slices(64, 288, 0, 4) == 0
    for ptrs in ((p + 8, p, p, p), (p, p, p + 8, p), (p, p, p, p + 8), (0, p, p, p), (p, 0, p, p)):
        assert axw._gemm_bf16_wide_launch(*ptrs, **ok) == HIP_ERROR_INVALID_VALUE, ptrs
    for ptrs in ((0, p, p, fp), (p, p, p, 0), (p + 8, p, p, fp), (p, p + 8, p, fp)):
        assert axw._dw_bf16_wide_launch(*ptrs, **ok) == HIP_ERROR_INVALID_VALUE, ptrs
    for ptrs in ((0, p, p), (p + 8, p, p), (p, p + 8, p), (p, p, p + 8)):
        assert axw._dx_bf16_wide_launch(*ptrs, 64, 64, 288, 4) == HIP_ERROR_INVALID_VALUE, ptrs

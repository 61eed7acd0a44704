"""flex_axw_backward_bf16 on the GPU (include/flex_axw.h) against float64 and the bounds of tests/axw_bf16_backward_ref.py."""
import numpy as np
import pytest

import axw_bf16_backward_ref as bref
import axw_bf16_ref as ref
import f64ref
from flex_amd import FlexError, axw
from test_gpu_axw_bf16 import _bits, _dev, _layer

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HIP_ERROR_INVALID_VALUE, FLEX_ERR_INVALID, FLEX_ERR_UNSUPPORTED = 1, -1, -4


_cus = lambda n_cus=None: n_cus or torch.cuda.get_device_properties(0).multi_processor_count  # noqa: E731
_stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731


@pytest.mark.parametrize("cancel", [False, True], ids=["plain", "cancel"])
@pytest.mark.parametrize("n,dim,c,cp,n_cus", [(32, 32, 1, 64, None), (33, 32, 64, 64, None), (47, 96, 100, 128, 1), (613, 256, 256, 256, 1),
                                              (613, 256, 200, 256, 2), (5120, 160, 7, 64, None)])
def test_the_bf16_dw_kernel_is_within_its_float64_bound(n, dim, c, cp, n_cus, cancel):
    # cancel: rows of X in pairs (x, -x (1 + 2^-7)) against constant columns of G; an odd n leaves its last row unpaired
    Xt, G = ref.operands(np.random.default_rng([7, n, dim, c, cancel]), dim, n + n % 2, c, cancel)
    X, G = np.ascontiguousarray(Xt.T[:n]), G[:n]
    slices = axw.lib().flex_axw_dw_bf16_slices(n, _cus(n_cus))
    assert slices == {32: 1, 33: 1, 47: 1, 613: n_cus, 5120: 20}[n]
    Xd, Gd = _dev(X), _dev(np.pad(G, ((0, 0), (0, cp - c)), constant_values=5.0))  # G's padding columns are computed and dropped
    out = torch.full((dim * c + 64,), -7.0, dtype=torch.bfloat16, device="cuda")
    part = torch.empty(slices * dim * c, device="cuda")
    rc = axw._dw_bf16_launch(Xd.data_ptr(), Gd.data_ptr(), out.data_ptr(), part.data_ptr(), n, dim, c, cp, _cus(n_cus), _stream())
    assert rc == 0 and (out[dim * c:] == -7.0).all(), (rc, "written past dim x c")
    msg, worst = ref.check(*bref.dw_reference(X, G, slices), _bits(out[: dim * c].view(dim, c)), f"dW n={n} dim={dim} c={c} slices={slices}")
    print(f"worst err/bound {worst:.4g} (gamma({ref.M} L))")
    assert msg is None, msg


@pytest.mark.parametrize("n,cp,dim", [(33, 64, 32), (95, 128, 96), (613, 256, 224), (613, 64, 256)])
def test_the_bf16_dx_product_is_within_its_float64_bound(n, cp, dim):
    G, Wt = ref.operands(np.random.default_rng([9, n, cp, dim]), n, cp, dim)
    out = torch.full((n, dim), -7.0, dtype=torch.bfloat16, device="cuda")
    Gd, Wd = _dev(G), _dev(Wt)
    rc = axw._dx_bf16_launch(Gd.data_ptr(), Wd.data_ptr(), out.data_ptr(), n, cp, dim, _cus(), _stream())
    assert rc == 0, rc
    msg, worst = ref.check(f64ref.gemm_f64(G, Wt), ref.gemm_bound(G, Wt), _bits(out), f"dX n={n} cp={cp} dim={dim}")
    print(f"worst err/bound {worst:.4g}")
    assert msg is None, msg


def _case(n, dim, c, seed, long_row=False, positive=False, inf_in_a=False):
    a, X, W = _layer(n, dim, c, seed, long_row, positive)
    if inf_in_a:
        a.vals[a.rowPtr[n // 3] + 1] = np.inf
    dOut = ref.rounded(f64ref._logu(np.random.default_rng([seed, n, c]), -4, 4, (n, c)))
    return a, X, W, (np.abs(dOut) if positive else dOut), axw.Axw(a, dim, c, bf16=True, backward=True)


def _check_both(a, X, W, dOut, h, gx, gw, what, R=(None, None)):
    slices = axw.lib().flex_axw_dw_bf16_slices(a.n, _cus())
    for name, (r, b), got, r2 in zip(("dX", "dW"), bref.backward_reference(a, X, W, dOut, h.ld, slices), (gx, gw), R):
        msg, worst = ref.check(r if r2 is None else r2, b, _bits(got), f"{name} {what}")
        print(f"{name} worst err/bound {worst:.4g}")
        assert got.dtype == torch.bfloat16 and msg is None, msg


@pytest.mark.parametrize("n,dim,c,long_row", [(512, 32, 7, False), (512, 128, 100, False), (512, 256, 64, False), (5120, 128, 100, True)])
def test_the_bf16_backward_is_within_its_composed_bound(n, dim, c, long_row):
    a, X, W, dOut, h = _case(n, dim, c, 11, long_row)
    pad = lambda v: _dev(np.pad(dOut, ((0, 0), (0, h.ld - c)), constant_values=v))  # noqa: E731
    Xd, Wd, d0 = _dev(X), _dev(W), pad(0.0)
    gx, gw = h.backward(d0, Xd, Wd)
    _check_both(a, X, W, dOut, h, gx, gw, f"n={n} dim={dim} c={c}")
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


@pytest.mark.parametrize("where", ["X", "dOut", "A"])
def test_inf_and_nan_keep_the_reference_classes(where):
    a, X, W, dOut, h = _case(n := 97, 64, c := 40, 13, positive=True, inf_in_a=where == "A")
    if where != "A":
        t = X if where == "X" else dOut
        t[3, 5], t[n - 2, 0] = np.inf, np.nan
    gx, gw = h.backward(_dev(np.pad(dOut, ((0, 0), (0, h.ld - c)))), _dev(X), _dev(W))
    _check_both(a, X, W, dOut, h, gx, gw, where)
    h.destroy()


def test_autograd_through_the_bf16_layer():
    a, X, W, dOut, h = _case(n := 512, 64, 24, 17)
    Xd, Wd = _dev(X).requires_grad_(), _dev(W).requires_grad_()
    h.layer(Xd, Wd).backward(_dev(dOut))
    A64 = torch.zeros((n, n), dtype=torch.float64)
    A64.index_put_((torch.from_numpy(np.repeat(np.arange(n), np.diff(a.rowPtr.astype(np.int64)))), torch.from_numpy(a.col.astype(np.int64))),
                   torch.from_numpy(a.vals.astype(np.float64)), accumulate=True)
    X64, W64 = torch.from_numpy(X.astype(np.float64)).requires_grad_(), torch.from_numpy(W.astype(np.float64)).requires_grad_()
    (A64 @ X64 @ W64).backward(torch.from_numpy(dOut.astype(np.float64)))
    _check_both(a, X, W, dOut, h, Xd.grad, Wd.grad, "autograd", (X64.grad.numpy(), W64.grad.numpy()))
    h.destroy()


@pytest.mark.parametrize("what", ["calls", "launchers"])
def test_what_the_bf16_backward_refuses(what):
    a, _, _ = _layer(64, 32, 8, 19)
    L = axw.lib()
    if what == "calls":
        with pytest.raises(FlexError, match=rf"\({FLEX_ERR_UNSUPPORTED}\)"):
            axw.Axw(a, 48, 8, bf16=True, backward=True)  # dim % 32 != 0
        h16, h32 = axw.Axw(a, 32, 8, bf16=True, backward=True), axw.Axw(a, 32, 8, backward=True)
        x, w, g, gx, gw = (torch.zeros(s, dtype=torch.bfloat16, device="cuda") for s in ((64, 32), (32, 8), (64, 64), (64, 32), (32, 8)))
        p = [t.data_ptr() for t in (x, w, g, gx, gw)]
        assert L.flex_axw_backward(h16._h, *p, None) == FLEX_ERR_INVALID and L.flex_axw_backward_bf16(h32._h, *p, None) == FLEX_ERR_INVALID
        assert L.flex_axw_backward_bf16(h16._h, p[0], p[1], p[2] + 2, p[3], p[4], None) == FLEX_ERR_UNSUPPORTED
        assert L.flex_axw_backward_bf16(h16._h, *p, None) == 0
        with pytest.raises(TypeError):
            h16.backward(g.float(), x.float(), w.float())
        h16.destroy(), h32.destroy()
    else:
        buf, fbuf = torch.zeros(1 << 17, dtype=torch.bfloat16, device="cuda"), torch.zeros(1 << 16, device="cuda")
        p, fp, ok = buf.data_ptr(), fbuf.data_ptr(), dict(n=64, dim=32, c=64, cp=64, n_cus=4)
        for kw in (dict(n=31), dict(dim=0), dict(dim=272), dict(cp=320), dict(c=0), dict(c=65), dict(n_cus=0)):
            assert axw._dw_bf16_launch(p, p, p, fp, **{**ok, **kw}) == HIP_ERROR_INVALID_VALUE, kw
            if "c" not in kw:
                assert axw._dx_bf16_launch(p, p, p, **{k: v for k, v in {**ok, **kw}.items() if k != "c"}) == HIP_ERROR_INVALID_VALUE, kw
        for ptrs in ((0, p, p, fp), (p, p, p, 0), (p + 8, p, p, fp)):
            assert axw._dw_bf16_launch(*ptrs, **ok) == HIP_ERROR_INVALID_VALUE, ptrs
        assert axw._dx_bf16_launch(0, p, p, 64, 64, 32, 4) == HIP_ERROR_INVALID_VALUE

"""flex_axw_backward_root_bf16 on the GPU (include/flex_axw.h): the one-pass dW / dR / db kernel and the dual-source dX kernel alone, and the
whole call through Axw.backward_root and Axw.root_layer, every element against float64 and the bounds of tests/axw_bf16_root_backward_ref.py."""
import numpy as np
import pytest

import axw_bf16_backward_ref as bref
import axw_bf16_ref as ref
import axw_bf16_root_backward_ref as rbref
import axw_bf16_root_ref as rref
import f64ref
from flex_amd import FlexError, axw
from test_gpu_axw_bf16 import _bits, _dev, _layer
from test_gpu_axw_bf16_wide import _cus, _filled, _stream

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HIP_ERROR_INVALID_VALUE, FLEX_ERR_INVALID, FLEX_ERR_UNSUPPORTED = 1, -1, -4
_same = lambda p, q: np.array_equal(_bits(p), _bits(q))  # noqa: E731


# The table of the issue, and one case more: under the slice rule (at most n / (4 c) slices) its row (613, 256, 200, n_cus = 2) is ONE
# slice, so (2048, 256, 200, n_cus = 8) runs two windows and two row blocks on two slices.
@pytest.mark.parametrize("cancel", [False, True], ids=["plain", "cancel"])
@pytest.mark.parametrize("n,dim,c,cp,n_cus,want_slices", [(32, 32, 1, 64, None, 1), (33, 32, 64, 64, None, 1), (47, 96, 100, 128, 1, 1),
                                                          (613, 256, 200, 256, 2, 1), (613, 288, 192, 192, 1, 1), (5120, 160, 7, 64, None, 20),
                                                          (2048, 256, 200, 256, 8, 2)])
def test_the_dual_dw_kernel_is_within_its_float64_bounds(n, dim, c, cp, n_cus, want_slices, cancel):
    # cancel: rows of X in pairs (x, -x (1 + 2^-7)) against constant columns of G and of dOut; an odd n leaves its last row unpaired
    rng = np.random.default_rng([29, n, dim, c, cancel])
    Xt, G = ref.operands(rng, dim, n + n % 2, c, cancel)
    D = ref.operands(rng, 8, n + n % 2, c, cancel)[1][:n]
    X, G = np.ascontiguousarray(Xt.T[:n]), G[:n]
    slices = axw._dw_bf16_root_slices(n, dim, c, _cus(n_cus))
    assert slices == want_slices
    Xd, Gd, Dd = _dev(X), *(_dev(np.pad(t, ((0, 0), (0, cp - c)), constant_values=5.0)) for t in (G, D))  # padding: computed and dropped
    dW, dR, db = _filled(dim * c + 64), _filled(dim * c + 64), torch.full((c + 16,), -7.0, device="cuda")
    part = torch.empty(slices * (2 * dim * c + c), device="cuda")
    rc = axw._dw_bf16_root_launch(Xd.data_ptr(), Gd.data_ptr(), Dd.data_ptr(), dW.data_ptr(), dR.data_ptr(), db.data_ptr(), part.data_ptr(), n, dim,
                                  c, cp, _cus(n_cus), _stream())
    assert rc == 0 and (dW[dim * c:] == -7.0).all() and (dR[dim * c:] == -7.0).all() and (db[c:] == -7.0).all(), (rc, "written past an output")
    checks = [ref.check(*bref.dw_reference(X, t, slices), _bits(o[: dim * c].view(dim, c)), f"{name} n={n} dim={dim} c={c} slices={slices}")
              for name, t, o in (("dW", G, dW), ("dR", D, dR))] + [rbref.check_db(*rbref.db_reference(D, slices), db[:c].cpu().numpy(), f"n={n} c={c}")]
    print("worst err/bound dW %.4g dR %.4g db %.4g" % tuple(w for _, w in checks))
    assert all(msg is None for msg, _ in checks), [msg for msg, _ in checks if msg]


# (n, cp, c, dim): NT = 1; an odd NT with 2-byte pack loads; NT = 7; one full pass and a one-tile remainder; sixteen passes (plain only).
# cancel: dOut = G and R = -W (1 + 2^-7): the two products cancel across the seam.  G's and dOut's columns c .. hold 3.0.
@pytest.mark.parametrize("n,cp,c,dim,cancel", [(n, cp, c, dim, k) for n, cp, c, dim in ((33, 64, 64, 32), (95, 128, 100, 96), (613, 256, 256, 224),
                                                                                        (613, 64, 40, 288), (300, 256, 256, 4096))
                                               for k in (False, True) if not (k and dim == 4096)])
def test_the_dual_dx_kernel_is_within_its_float64_bound(n, cp, c, dim, cancel):
    G, Wt, D, Rt, _, _ = rref.operands(np.random.default_rng([31, n, cp, c, dim, cancel]), n, c, c, dim, dim, False, False, cancel)
    Gp, Dp = (np.pad(t, ((0, 0), (0, cp - c)), constant_values=3.0) for t in (G, D))
    Wtp, Rtp = (np.pad(t, ((0, cp - c), (0, 0))) for t in (Wt, Rt))
    t = [_dev(x) for x in (Gp, np.ascontiguousarray(Wt.T), Dp, np.ascontiguousarray(Rt.T))]
    Wf, out = _filled(2 * dim * cp), _filled(n * dim + 64)
    rc = axw._dx_bf16_root_launch(*(x.data_ptr() for x in t), Wf.data_ptr(), out.data_ptr(), n, c, cp, dim, _cus(), _stream())
    assert rc == 0 and (out[n * dim:] == -7.0).all(), (rc, "written past n x dim")
    msg, worst = ref.check(*rref.dense_reference(Gp, Wtp, Dp, Rtp), _bits(out[: n * dim].view(n, dim)), f"dX n={n} cp={cp} c={c} dim={dim}")
    print(f"worst err/bound {worst:.4g} (gamma(2 cp + 2))")
    assert msg is None, msg


def _case(n, dim, c, seed, long_row=False, positive=False, inf_in_a=False):
    a, X, W = _layer(n, dim, c, seed, long_row, positive)
    if inf_in_a:
        a.vals[a.rowPtr[n // 3] + 1] = np.inf
    rng = np.random.default_rng([seed, n, c])
    dOut, R = ref.rounded(f64ref._logu(rng, -4, 4, (n, c))), ref.rounded(f64ref._logu(rng, -4, 4, (dim, c)))
    h = axw.Axw(a, dim, c, bf16=True, backward=True, root=True)
    return a, X, W, *((np.abs(R), np.abs(dOut)) if positive else (R, dOut)), h


def _check_all(a, X, W, R, dOut, h, got, what, refs=(None,) * 4):
    slices = axw._dw_bf16_root_slices(a.n, h.dim, h.c, _cus())
    for name, (r, b), g, r2 in zip(("dX", "dW", "dR", "db"), rbref.backward_reference(a, X, W, R, dOut, h.ld, slices), got, refs):
        r = r if r2 is None else r2
        msg, worst = rbref.check_db(r, b, g.cpu().numpy(), what) if name == "db" else ref.check(r, b, _bits(g), f"{name} {what}")
        print(f"{name} worst err/bound {worst:.4g}")
        assert g.dtype == (torch.float32 if name == "db" else torch.bfloat16) and msg is None, msg


@pytest.mark.parametrize("n,dim,c,long_row", [(512, 32, 7, False), (512, 128, 100, False), (512, 608, 128, False), (5120, 128, 100, True)])
def test_the_root_backward_is_within_its_composed_bounds(n, dim, c, long_row):
    a, X, W, R, dOut, h = _case(n, dim, c, 11, long_row)
    pad = lambda v: _dev(np.pad(dOut, ((0, 0), (0, h.ld - c)), constant_values=v))  # noqa: E731
    Xd, Wd, Rd, d0 = _dev(X), _dev(W), _dev(R), pad(0.0)
    got = h.backward_root(d0, Xd, Wd, Rd)
    _check_all(a, X, W, R, dOut, h, got, f"n={n} dim={dim} c={c}")
    for v, why in ((0.0, "a second call gives other bits"), (3.0, "finite padding columns of dOut change the result")):
        assert all(_same(p, q) for p, q in zip(got, h.backward_root(pad(v), Xd, Wd, Rd))), why
    assert _same(h.backward_root(d0, Xd, Wd, torch.zeros_like(Rd), need_w=False, need_b=False)[0], h.backward(d0, Xd, Wd, need_w=False)[0]), "R = 0"
    for skip in ((0,), (1, 2), (3,)):  # a NULL output is left alone, its inputs may be NULL, and the others come out the same
        outs = [torch.full_like(g, -7.0) for g in got]
        ins = [None if skip == (1, 2) else Xd, *((None, None) if skip == (0,) else (Wd, Rd)), d0]
        rc = axw.lib().flex_axw_backward_root_bf16(h._h, *(None if t is None else t.data_ptr() for t in ins),
                                                   *(None if i in skip else o.data_ptr() for i, o in enumerate(outs)), _stream())
        assert rc == 0 and all((o == -7.0).all() if i in skip else _same(o, g) for i, (o, g) in enumerate(zip(outs, got))), skip
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        replayed = h.backward_root(d0, Xd, Wd, Rd)
    for _ in range(2):
        for t in replayed:
            t.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(_same(p, q) for p, q in zip(got, replayed)), "a replayed graph gives other bits"
    h.destroy()


@pytest.mark.parametrize("where", ["X", "dOut", "A"])
def test_inf_and_nan_keep_the_reference_classes(where):
    a, X, W, R, dOut, h = _case(n := 97, 64, c := 40, 13, positive=True, inf_in_a=where == "A")
    if where != "A":
        t = X if where == "X" else dOut
        t[3, 5], t[n - 2, 0] = np.inf, np.nan
    got = h.backward_root(_dev(np.pad(dOut, ((0, 0), (0, h.ld - c)))), _dev(X), _dev(W), _dev(R))
    _check_all(a, X, W, R, dOut, h, got, where)
    h.destroy()


def test_autograd_through_the_root_layer():
    a, X, W, R, dOut, h = _case(n := 512, 64, c := 24, 17)
    bias = f64ref._logu(np.random.default_rng(37), -4, 4, c)
    leaves = [_dev(X).requires_grad_(), _dev(W).requires_grad_(), _dev(R).requires_grad_(), torch.from_numpy(bias).cuda().requires_grad_()]
    h.root_layer(*leaves).backward(_dev(dOut))
    A64 = torch.zeros((n, n), dtype=torch.float64)
    A64.index_put_((torch.from_numpy(np.repeat(np.arange(n), np.diff(a.rowPtr.astype(np.int64)))), torch.from_numpy(a.col.astype(np.int64))),
                   torch.from_numpy(a.vals.astype(np.float64)), accumulate=True)
    X64, W64, R64, b64 = (torch.from_numpy(t.astype(np.float64)).requires_grad_() for t in (X, W, R, bias))
    (A64 @ X64 @ W64 + X64 @ R64 + b64).backward(torch.from_numpy(dOut.astype(np.float64)))
    _check_all(a, X, W, R, dOut, h, [t.grad for t in leaves], "autograd", [t.grad.numpy() for t in (X64, W64, R64, b64)])
    h.destroy()


@pytest.mark.parametrize("what", ["calls", "launchers"])
def test_what_the_root_backward_refuses(what):
    a, _, _ = _layer(64, 32, 8, 19)
    L = axw.lib()
    if what == "calls":
        x, w, g, gx, gw, gr = (torch.zeros(s, dtype=torch.bfloat16, device="cuda") for s in ((64, 32), (32, 8), (64, 64), (64, 32), (32, 8), (32, 8)))
        gb = torch.zeros(8, device="cuda")
        p = [t.data_ptr() for t in (x, w, w, g, gx, gw, gr, gb)]
        for missing in ("bf16", "backward", "root"):
            flags = {k: k != missing for k in ("bf16", "backward", "root") if not (missing == "bf16" and k == "root")}  # root needs bf16
            h = axw.Axw(a, 32, 8, **flags)
            assert L.flex_axw_backward_root_bf16(h._h, *p, None) == FLEX_ERR_INVALID, missing
            with pytest.raises(FlexError):
                h.backward_root(g, x, w, w)
            h.destroy()
        h = axw.Axw(a, 32, 8, bf16=True, backward=True, root=True)
        assert L.flex_axw_backward_root_bf16(h._h, *p[:5], p[5], None, p[7], None) == FLEX_ERR_INVALID  # dW without dR
        assert L.flex_axw_backward_root_bf16(h._h, *p[:5], None, p[6], p[7], None) == FLEX_ERR_INVALID
        assert L.flex_axw_backward_root_bf16(h._h, *p[:3], p[3] + 2, *p[4:], None) == FLEX_ERR_UNSUPPORTED  # a misaligned dOut
        assert L.flex_axw_backward_root_bf16(h._h, *p, None) == 0
        with pytest.raises(TypeError):
            h.backward_root(g.float(), x.float(), w.float(), w.float())
        h.destroy()
    else:
        buf, fbuf = torch.zeros(1 << 17, dtype=torch.bfloat16, device="cuda"), torch.zeros(1 << 16, device="cuda")
        p, fp, ok = buf.data_ptr(), fbuf.data_ptr(), dict(n=64, dim=32, c=64, cp=64, n_cus=4)
        dx = lambda ptrs, kw: axw._dx_bf16_root_launch(*ptrs, kw["n"], kw["c"], kw["cp"], kw["dim"], kw["n_cus"])  # noqa: E731
        dw = lambda ptrs, kw: axw._dw_bf16_root_launch(*ptrs, kw["n"], kw["dim"], kw["c"], kw["cp"], kw["n_cus"])  # noqa: E731
        for kw in (dict(n=31), dict(cp=320), dict(c=0), dict(c=65), dict(n_cus=0)):
            assert dx((p,) * 6, {**ok, **kw}) == dw((p,) * 6 + (fp,), {**ok, **kw}) == HIP_ERROR_INVALID_VALUE, kw
        assert dx((p,) * 6, {**ok, "dim": 48}) == HIP_ERROR_INVALID_VALUE and dw((p,) * 6 + (fp,), {**ok, "dim": 36}) == HIP_ERROR_INVALID_VALUE
        for bad in (0, p + 8):  # NULL and misaligned pointers
            assert all(dx(tuple(bad if i == k else p for i in range(6)), ok) == HIP_ERROR_INVALID_VALUE for k in (0, 2, 4, 5)), bad
            assert all(dw(tuple(bad if i == k else p for i in range(6)) + (fp,), ok) == HIP_ERROR_INVALID_VALUE for k in (0, 1, 2)), bad
        assert dx((p, 0, p, p, p, p), ok) == dw((p,) * 6 + (0,), ok) == HIP_ERROR_INVALID_VALUE
    torch.cuda.synchronize()

"""The bf16 layer with a root-weight term on the GPU (flex_axw_run_root_bf16, axw_bf16_root_kernels.hip): the dual-source kernel alone and
the layer through Axw.run_root, every element against float64 and the bounds of tests/axw_bf16_root_ref.py."""
import numpy as np
import pytest

import axw_bf16_root_ref as ref
import f64ref
from flex_amd import FlexError, axw
from test_gpu_axw_bf16 import _bits, _dev, _layer
from test_gpu_axw_bf16_wide import _cus, _filled, _stream

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HIP_ERROR_INVALID_VALUE, FLEX_ERR_INVALID, FLEX_ERR_UNSUPPORTED = 1, -1, -4
_ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
_f32 = lambda b: None if b is None else torch.from_numpy(b).cuda()  # noqa: E731


def run_kernel(L1, W1, L2, W2, Cin, bias, cp, n_cus=None):
    """bf16 bits [n x cp] of the launcher; Out and Wf start as -7.0 everywhere."""
    (n, d1), c, d2 = L1.shape, W1.shape[1], 0 if L2 is None else L2.shape[1]
    t = [None if x is None else _dev(x) for x in (L1, W1, L2, W2, Cin)]
    bd, Wf, Od = _f32(bias), _filled((d1 + d2) * cp), _filled(n, cp)
    rc = axw._gemm_bf16_root_launch(*map(_ptr, t[:2]), d1, *map(_ptr, t[2:4]), d2, _ptr(t[4]), _ptr(bd), Wf.data_ptr(), Od.data_ptr(), n, c, cp,
                                    _cus(n_cus), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return _bits(Od)


# (n, d1, d2, c, Cin, bias, n_cus, kind).  A slab is 8 k-steps of 16: one and two k-steps on a single panel; the seam in the middle of the
# first slab with an overlapping last panel and padding columns; the seam on a slab boundary and both panels of a wave (cp = 64); the seam
# in the middle of a later slab at NT = 6 with several rounds a workgroup (the W stream carries over); the longest chain; the single-source
# form of order A_XW; Cin and bias rotated over the dual-source shapes.  cancel: the two products cancel across the seam.  classes: a +inf
# in row 7 of L2 and a NaN in bias[9] -- that row and that column take the reference's classes and nothing else does.
@pytest.mark.parametrize("n,d1,d2,c,cin,bias,n_cus,kind", [
    (32, 16, 0, 1, False, False, None, ""), (32, 16, 16, 1, True, True, None, ""), (32, 16, 16, 1, False, False, None, ""),
    (33, 48, 48, 100, True, False, None, ""), (33, 48, 48, 100, False, True, None, ""), (47, 128, 128, 64, False, True, None, ""),
    (47, 128, 128, 64, True, False, None, ""), (613, 272, 272, 192, True, True, 2, ""), (613, 272, 272, 192, False, False, 2, ""),
    (300, 4096, 4096, 256, False, False, None, ""), (300, 4096, 4096, 256, True, True, None, ""), (33, 48, 0, 100, True, True, None, ""),
    (613, 608, 0, 128, True, True, None, ""), (33, 48, 48, 100, False, False, None, "cancel"), (613, 272, 272, 192, False, False, 2, "cancel"),
    (33, 48, 48, 100, True, True, None, "classes")])
def test_the_root_kernel_is_within_its_float64_bound(n, d1, d2, c, cin, bias, n_cus, kind):
    cp = (c + 63) // 64 * 64
    L1, W1, L2, W2, Cin, b = ref.operands(np.random.default_rng([3, n, d1, d2, c, len(kind)]), n, d1, d2, c, cp, cin, bias, kind == "cancel")
    if kind == "classes":
        L2[7, 40], b[9] = np.inf, np.nan
    r64, g = ref.dense_reference(L1, W1, L2, W2, None if Cin is None else Cin[:, :c], b)  # Cin's padding (3.0) must not reach Out
    assert kind != "classes" or (np.isfinite(r64) == ((np.arange(n) != 7)[:, None] & (np.arange(c) != 9))).all()
    msg, worst = ref.check(r64, g, run_kernel(L1, W1, L2, W2, Cin, b, cp, n_cus), f"n={n} d1={d1} d2={d2} c={c} Cin={cin} bias={bias} {kind}")
    print(f"worst err/bound {worst:.4g} (gamma(d1 + d2 + 2))")
    assert msg is None, msg


@pytest.fixture(scope="module")
def case():
    """case(dim, c, with_bias) = (A, X, W, R, bias, the handle, {order: bits of run_root}) on the other bf16 layer tests' graph, made once"""
    made = {}

    def get(dim, c, with_bias):
        if (dim, c, with_bias) not in made:
            a, X, W = _layer(512, dim, c, 11)
            rng = np.random.default_rng([23, dim, c])
            R, b = ref.rounded(f64ref._logu(rng, -4, 4, (dim, c))), (f64ref._logu(rng, -4, 4, c) if with_bias else None)
            h = axw.Axw(a, dim, c, bf16=True, root=True)
            out = {o: _bits(h.run_root(_dev(X), _dev(W), _dev(R), _f32(b), o)) for o in (f64ref.A_XW, f64ref.AX_W)}
            made[dim, c, with_bias] = a, X, W, R, b, h, out
        return made[dim, c, with_bias]
    yield get
    for v in made.values():
        v[5].destroy()


@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("order", [f64ref.A_XW, f64ref.AX_W, axw.FLEX_AXW_AUTO], ids=["A_XW", "AX_W", "AUTO"])
@pytest.mark.parametrize("dim,c", [(64, 100), (608, 128)])
def test_the_root_layer_is_within_its_composed_bound(case, dim, c, order, with_bias):
    a, X, W, R, b, h, out = case(dim, c, with_bias)
    if order == axw.FLEX_AXW_AUTO:  # cp <= dim gives A (X W)
        got = h.run_root(_dev(X), _dev(W), _dev(R), _f32(b))
        assert got.dtype == torch.bfloat16 and tuple(got.shape) == (512, h.ld)
        assert np.array_equal(_bits(got), out[f64ref.A_XW if h.ld <= dim else f64ref.AX_W]), "AUTO gives the bits of the order its rule names"
        return
    msg, worst = ref.check(*ref.layer_reference(a, X, W, R, b, order), out[order], f"order={order} dim={dim} c={c} bias={with_bias}")  # padding too
    print(f"worst err/bound {worst:.4g}")
    assert msg is None, msg


@pytest.mark.parametrize("dim,c", [(64, 100), (608, 128)])
def test_a_zero_root_weight_gives_the_gcn_layer(case, dim, c):
    a, X, W, _, _, h, _ = case(dim, c, False)
    Xd, Wd, Z = _dev(X), _dev(W), torch.zeros((dim, c), dtype=torch.bfloat16, device="cuda")
    # (A X) W: the same chain, and zero products change no accumulator
    assert np.array_equal(_bits(h.run_root(Xd, Wd, Z, None, f64ref.AX_W)), _bits(h.run(Xd, Wd, f64ref.AX_W)))
    got, want = h.run_root(Xd, Wd, Z, None, f64ref.A_XW).float().cpu().numpy(), h.run(Xd, Wd, f64ref.A_XW).float().cpu().numpy()
    assert np.array_equal(got, want, equal_nan=True)  # A (X W): S + 0 is S, but for the sign of a zero


@pytest.mark.parametrize("order,dim,c", [(f64ref.AX_W, 64, 100), (f64ref.A_XW, 608, 128)])
def test_a_second_call_and_a_replayed_graph_give_the_same_bits(case, order, dim, c):
    a, X, W, R, b, h, out = case(dim, c, True)
    args = (_dev(X), _dev(W), _dev(R), _f32(b), order)
    assert np.array_equal(_bits(h.run_root(*args)), out[order])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = h.run_root(*args)
    for _ in range(3):
        got.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(got), out[order])


@pytest.mark.parametrize("what", ["no_flag", "flag_without_bf16", "overlap", "bias_dtype"])
def test_what_the_root_calls_refuse(what):
    a, X, W = _layer(64, 16, 8, 19)
    Xd, Wd, out = _dev(X), _dev(W), _filled(64, 64)
    p, o = Xd.data_ptr(), out.data_ptr()
    if what == "flag_without_bf16":
        with pytest.raises(FlexError, match=rf"\({FLEX_ERR_UNSUPPORTED}\)"):
            axw.Axw(a, 16, 8, root=True)
    elif what == "overlap":  # Cin = Out, and a Cin that starts in Out's last row
        for cin in (o, o + 64 * 63 * 2):
            rc = axw._gemm_bf16_root_launch(p, Wd.data_ptr(), 16, None, None, 0, cin, None, _filled(16 * 64).data_ptr(), o, 64, 8, 64, 4, _stream())
            assert rc == HIP_ERROR_INVALID_VALUE
    else:
        h = axw.Axw(a, 16, 8, bf16=True, root=what == "bias_dtype")
        for bias in (None,) if what == "no_flag" else (torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros(8, device="cuda").bfloat16()):
            with pytest.raises(FlexError if what == "no_flag" else TypeError):
                h.run_root(Xd, Wd, Wd, bias)
        if what == "no_flag":
            assert axw.lib().flex_axw_run_root_bf16(h._h, 0, p, Wd.data_ptr(), Wd.data_ptr(), None, o, None, None, None) == FLEX_ERR_INVALID
        h.destroy()
    torch.cuda.synchronize()
    assert (out == -7.0).all(), "a refused call wrote its output"

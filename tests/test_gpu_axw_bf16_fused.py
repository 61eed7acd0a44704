"""Order FLEX_AXW_AX_W_FUSED of the bf16 layer on the GPU (axw_bf16_fused_kernels.hip: the gather of A X and the product with W, R in one
launch): the plain and the root forms against the float64 references and bounds of order AX_W (tests/axw_bf16_ref.py,
axw_bf16_root_ref.py, axw_bf16_act_ref.py -- they hold for any order of the row sum), inf / NaN classes, +0 padding, and the contract."""
import numpy as np
import pytest

import axw_bf16_act_ref as aref
import axw_bf16_ref as ref
import axw_bf16_root_ref as rref
import f64ref
from flex_amd import FlexError, axw
from test_gpu_axw_bf16 import _bits, _dev, _layer
from test_gpu_axw_bf16_root import _f32, _ptr
from test_gpu_axw_bf16_wide import _filled, _stream

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HIP_ERROR_INVALID_VALUE, FLEX_ERR_INVALID, FLEX_ERR_UNSUPPORTED = 1, -1, -4
FUSED, SEED = axw.FLEX_AXW_AX_W_FUSED, 0x5EED0000AD04


def _launch(h, X, W, R=None, b=None, relu=False, p=0.0, seed=0, groups=1):
    out = _filled(h.n, h.ld)
    rc = axw._fused_bf16_launch(h, X.data_ptr(), W.data_ptr(), _ptr(R), _ptr(b), out.data_ptr(), relu, p, seed, groups, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return out


# a tail panel with repeated rows and an odd k-step count; one k-step, NT = 2, a tile that is all padding but 7 columns; padding inside
# a tile; the largest W (one T tile); the workgroup gather of a 5000-entry row among 160 panels.  Each through run() and through the
# launcher on 1 and 3 workgroups: the persistent loop, the cut search, a long row sharing a workgroup with other rows.
@pytest.mark.parametrize("n,dim,c,long_row", [(97, 48, 40, False), (512, 16, 7, False), (512, 128, 100, False), (512, 256, 256, False),
                                              (5120, 128, 100, True)])
def test_the_fused_layer_is_within_the_bound_of_order_ax_w(n, dim, c, long_row):
    a, X, W = _layer(n, dim, c, 11, long_row)
    r64, bound = ref.layer_reference(a, X, W, f64ref.AX_W)
    h, Xd, Wd = axw.Axw(a, dim, c, bf16=True, fused=True), _dev(X), _dev(W)
    for what, out in (("run", h.run(Xd, Wd, FUSED)), ("1 workgroup", _launch(h, Xd, Wd)), ("3 workgroups", _launch(h, Xd, Wd, groups=3))):
        msg, worst = ref.check(r64, bound, _bits(out), f"fused {what} n={n} dim={dim} c={c}")
        print(f"{what}: worst err/bound {worst:.4g}")
        assert msg is None and tuple(out.shape) == (n, h.ld), msg
    h.destroy()


@pytest.mark.parametrize("act", [None, 0.0, 0.5], ids=["none", "relu", "relu_dropout"])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("dim,c", [(64, 100), (128, 256)])
def test_the_fused_root_forms_are_within_the_bound_of_order_ax_w(dim, c, bias, act):
    a, X, W = _layer(n := 512, dim, c, 11)
    rng = np.random.default_rng([53, dim, c])
    R = ref.rounded(f64ref._logu(rng, -4, 4, (dim, c)))
    b = f64ref._logu(rng, -4, 4, c).astype(np.float32) if bias else None
    r64, E = rref.layer_reference(a, X, W, R, b, f64ref.AX_W)
    h, t = axw.Axw(a, dim, c, bf16=True, root=True, fused=True), (_dev(X), _dev(W), _dev(R), _f32(b))
    if act is None:
        out = h.run_root(*t, FUSED)
        msg, worst = ref.check(r64, E, _bits(out), f"root dim={dim} c={c}")
    else:
        out = h.run_root_act(*t, act, SEED, FUSED)
        msg, worst, nonzero, dropped = aref.check_act(r64, E, act, SEED, _bits(out), f"act p={act} dim={dim} c={c}")
        print(f"nonzero {nonzero:.3f}, dropped {dropped:.3f}")
        assert act == 0 or (nonzero >= 0.2 and dropped >= 0.4), (nonzero, dropped)
        assert (act > 0) == (not np.array_equal(_bits(h.run_root_act(*t, act, SEED + 1, FUSED)), _bits(out))), "a second seed, other bits"
        assert np.array_equal(_bits(_launch(h, *t, True, act, SEED, 3)), _bits(out)), "the grid size changes no bit"
    print(f"worst err/bound {worst:.4g}")
    assert msg is None, msg
    h.destroy()


@pytest.mark.parametrize("where", ["X", "A"])
def test_inf_and_nan_keep_the_reference_classes_and_the_padding_stays_zero(where):
    a, X, W = _layer(n := 97, 48, 40, 13, positive=True)
    if where == "A":
        a.vals[a.rowPtr[n // 3] + 1] = np.inf
    else:
        X[3, 5], X[n - 2, 0] = np.inf, np.nan
    h = axw.Axw(a, 48, 40, bf16=True, fused=True)
    msg, _ = ref.check(*ref.layer_reference(a, X, W, f64ref.AX_W), _bits(h.run(_dev(X), _dev(W), FUSED)), where)
    assert msg is None, msg
    h.destroy()


@pytest.mark.parametrize("what", ["same_bits", "root_layer", "no_flag", "create", "root_too_large", "launcher"])
def test_the_contract_of_the_fused_order(what):
    if what == "same_bits":
        a, X, W = _layer(5120, 128, 100, 11, long_row=True)
        h = axw.Axw(a, 128, 100, bf16=True, fused=True)
        assert np.array_equal(_bits(h.run(_dev(X), _dev(W), FUSED)), _bits(h.run(_dev(X), _dev(W), FUSED)))
        return h.destroy()
    a, X, W = _layer(n := 512, 64, 100, 11)
    Xd, Wd = _dev(X), _dev(W)
    if what == "root_layer":
        h = axw.Axw(a, 64, 100, bf16=True, root=True, backward=True, fused=True)
        assert np.array_equal(_bits(h.root_layer(Xd, Wd, Wd, order=FUSED)), _bits(h.run_root(Xd, Wd, Wd, order=FUSED)[:, :100]))
    elif what == "no_flag":
        h, out = axw.Axw(a, 64, 100, bf16=True, root=True), _filled(n, 128)
        assert not h.has_fused
        assert axw.lib().flex_axw_run_bf16(h._h, FUSED, Xd.data_ptr(), Wd.data_ptr(), out.data_ptr(), None, None, None) == FLEX_ERR_INVALID
        assert axw.lib().flex_axw_run_root_bf16(h._h, FUSED, Xd.data_ptr(), Wd.data_ptr(), Wd.data_ptr(), None, out.data_ptr(), None, None,
                                                None) == FLEX_ERR_INVALID
        assert axw._fused_bf16_launch(h, Xd.data_ptr(), Wd.data_ptr(), None, None, out.data_ptr(), False, 0.0, 0, 1) == HIP_ERROR_INVALID_VALUE
    elif what == "create":
        for kw in (dict(dim=512, bf16=True), dict(dim=64, bf16=False)):
            with pytest.raises(FlexError, match=rf"\({FLEX_ERR_UNSUPPORTED}\)"):
                axw.Axw(a, c=100, fused=True, **kw)
        return
    elif what == "root_too_large":
        h, out = axw.Axw(a, 256, 256, bf16=True, root=True, fused=True), _filled(n, 256)
        x, w = _filled(n, 256).data_ptr(), _filled(256, 256).data_ptr()
        assert axw.lib().flex_axw_run_root_bf16(h._h, FUSED, x, w, w, None, out.data_ptr(), None, None, None) == FLEX_ERR_UNSUPPORTED
        assert axw._fused_bf16_launch(h, x, w, w, None, out.data_ptr(), False, 0.0, 0, 1) == HIP_ERROR_INVALID_VALUE
    else:
        h, out = axw.Axw(a, 64, 100, bf16=True, fused=True), _filled(n, 128)
        for x, groups in ((Xd.data_ptr(), 0), (Xd.data_ptr() + 8, 1)):
            assert axw._fused_bf16_launch(h, x, Wd.data_ptr(), None, None, out.data_ptr(), False, 0.0, 0, groups) == HIP_ERROR_INVALID_VALUE
    torch.cuda.synchronize()
    assert what == "root_layer" or (out == -7.0).all(), "a refused call wrote"
    h.destroy()

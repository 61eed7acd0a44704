"""ReLU and dropout fused into the bf16 root layer on the GPU (flex_axw_run_root_act_bf16, flex_axw_backward_root_act_bf16,
axw_bf16_act_kernels.hip).  Forward: dropped entries (binding.dropout_mask over idx = row * c + col) and padding are +0 bits; kept entries
lie within bound_bf16(cs relu(ref), cs (1 + 2^-23) E + 2^-24 cs relu(|ref| + E)) of cs relu(ref), (ref, E) the root reference's
(tests/axw_bf16_act_ref.py: ReLU is 1-Lipschitz, one fp32 rounding of the product, the bf16 rounding applied to cs relu(ref)); at p = 0 the
bits are max(root kernel, +0).  Backward: dZ bit for bit against numpy, the call bit for bit against backward_root(dZ)."""
import numpy as np
import pytest

import axw_bf16_act_ref as aref
import axw_bf16_root_ref as rref
import f64ref
from flex_amd import FlexError, axw
from test_gpu_axw_bf16 import _bits, _dev, _layer
from test_gpu_axw_bf16_root import _f32, _ptr, run_kernel
from test_gpu_axw_bf16_root_backward import _case, _check_all, _same
from test_gpu_axw_bf16_wide import _cus, _filled, _stream

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HIP_ERROR_INVALID_VALUE, FLEX_ERR_INVALID = 1, -1
# About half of z is positive, so "a quarter nonzero" at p = 0.5 hangs on the seed: under this one the float64 references alone of all the
# cases below (kernel and layer) have at least 0.2515 of their entries positive and kept and at least 0.49 dropped (checked on the CPU).
SEED = 0x5EED0000AD04


# (n, d1, d2, c, cp, n_cus): one partial slab at NT = 2 / P = 2 with an overlapping last panel; a slab and a tail per source with padding
# inside a tile (NT = 4); NT = 8 with several rounds a workgroup; NT = 6 without padding.  Cin (padding 3.0) and bias present.
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("n,d1,d2,c,cp,n_cus", [(33, 16, 0, 1, 64, None), (47, 288, 288, 100, 128, 1), (613, 160, 160, 200, 256, 2),
                                                (95, 64, 64, 192, 192, 1)])
def test_the_act_kernel_is_within_its_float64_bound(n, d1, d2, c, cp, n_cus, p):
    L1, W1, L2, W2, Cin, b = rref.operands(np.random.default_rng([41, n, d1, d2, c]), n, d1, d2, c, cp, True, True)
    t = [None if x is None else _dev(x) for x in (L1, W1, L2, W2, Cin)]
    bd, Wf, Od = _f32(b), _filled((d1 + d2) * cp), _filled(n, cp)
    rc = axw._gemm_bf16_root_act_launch(*map(_ptr, t[:2]), d1, *map(_ptr, t[2:4]), d2, _ptr(t[4]), _ptr(bd), Wf.data_ptr(), Od.data_ptr(), n, c, cp,
                                        _cus(n_cus), p, SEED, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    msg, worst, nonzero, dropped = aref.check_act(*rref.dense_reference(L1, W1, L2, W2, Cin[:, :c], b), p, SEED, _bits(Od), f"n={n} c={c} p={p}")
    print(f"worst err/bound {worst:.4g}, nonzero {nonzero:.3f}, dropped {dropped:.3f}")
    assert msg is None, msg
    if p > 0:
        assert nonzero >= 0.25 and dropped >= 0.25, (nonzero, dropped)
    else:  # rounding is monotone and keeps the sign: the root kernel's bits, +0 where the sign bit is set, NaN left as it is
        root = run_kernel(L1, W1, L2, W2, Cin, b, cp, n_cus)
        assert np.array_equal(_bits(Od), np.where((root >> 15 == 1) & ((root & 0x7FFF) <= 0x7F80), 0, root))


@pytest.mark.parametrize("n,c,cp", [(33, 7, 64), (613, 200, 256)])
def test_the_grad_kernel_gives_the_bits_of_numpy(n, c, cp):
    rng = np.random.default_rng([43, n, c])
    out, dout = aref.to_bf16(f64ref._logu(rng, -4, 4, (n, cp))), rref.rounded(f64ref._logu(rng, -4, 4, (n, cp)))
    out[::2, 1::3] |= 0x8000  # negative entries
    out[3, :5] = 0x0000, 0x8000, 0x7FC0, 0x7F80, 0x0001  # +0, -0, NaN, +inf, the smallest positive subnormal
    dout[:, c:] = 3.0
    Od, Dd, Zd = torch.from_numpy(out.view(np.int16)).cuda().view(torch.bfloat16), _dev(dout), _filled(n, cp)
    for p in (0.0, 0.3):
        assert axw._act_grad_bf16_launch(Od.data_ptr(), Dd.data_ptr(), Zd.data_ptr(), n, c, cp, float(aref.cs_of(p)), _stream()) == 0
        assert np.array_equal(_bits(Zd), aref.dz_bits(out, dout, c, p)), p


@pytest.mark.parametrize("dim,c", [(64, 40), (320, 100)])
def test_the_act_layer_forward_backward_and_autograd(dim, c):
    a, X, W, R, dOut, h = _case(n := 512, dim, c, 11)
    b = f64ref._logu(np.random.default_rng([47, c]), -4, 4, c).astype(np.float32)
    Xd, Wd, Rd, bd, p = _dev(X), _dev(W), _dev(R), _f32(b), 0.5
    for order in (f64ref.A_XW, f64ref.AX_W):
        out = h.run_root_act(Xd, Wd, Rd, bd, p, SEED, order)
        msg, worst, nonzero, dropped = aref.check_act(*rref.layer_reference(a, X, W, R, b, order), p, SEED, _bits(out), f"order={order} dim={dim}")
        print(f"order {order} worst err/bound {worst:.4g}, nonzero {nonzero:.3f}, dropped {dropped:.3f}")
        assert msg is None and nonzero >= 0.25 and dropped >= 0.25, (msg, nonzero, dropped)
        assert np.array_equal(_bits(h.run_root_act(Xd, Wd, Rd, bd, p, SEED, order)), _bits(out)), "one seed, other bits"
        assert not np.array_equal(_bits(h.run_root_act(Xd, Wd, Rd, bd, p, SEED + 1, order)), _bits(out)), "two seeds, the same bits"
    # the backward on the stored Out (order (A X) W's): bit for bit backward_root of numpy's dZ, dOut's padding ignored
    d3 = _dev(np.pad(dOut, ((0, 0), (0, h.ld - c)), constant_values=3.0))
    dz = aref.dz_bits(_bits(out), np.pad(dOut, ((0, 0), (0, h.ld - c))), c, p)
    want = h.backward_root(torch.from_numpy(dz.view(np.int16)).cuda().view(torch.bfloat16), Xd, Wd, Rd)
    assert all(_same(g, w) for g, w in zip(h.backward_root_act(d3, out, Xd, Wd, Rd, p), want))
    # autograd: the gradients within the root backward's bounds on dZ (exact in float64: cs = 2) built from the GPU's own Out
    leaves = [t.clone().requires_grad_() for t in (Xd, Wd, Rd, bd)]
    got = h.root_layer(*leaves, relu=True, dropout=p, seed=SEED)
    got.backward(_dev(dOut))
    assert np.array_equal(_bits(got), _bits(h.run_root_act(Xd, Wd, Rd, bd, p, SEED)[:, :c]))
    dZ = np.where(got.detach().float().cpu().numpy() > 0, dOut * np.float32(2), np.float32(0))
    _check_all(a, X, W, R, dZ, h, [t.grad for t in leaves], f"autograd dim={dim}")
    assert np.array_equal(_bits(h.root_layer(Xd, Wd, Rd, bd)), _bits(h.run_root(Xd, Wd, Rd, bd)[:, :c])), "the defaults are today's path"
    h.destroy()


@pytest.mark.parametrize("what", ["drop_p", "work", "launcher", "python"])
def test_what_the_act_calls_refuse(what):
    a, X, W = _layer(64, 32, 8, 19)
    Xd, Wd, out, g = _dev(X), _dev(W), _filled(64, 64), _filled(64, 64)
    h = axw.Axw(a, 32, 8, bf16=True, root=True, backward=True)
    L, x, w, o = axw.lib(), Xd.data_ptr(), Wd.data_ptr(), out.data_ptr()
    if what == "drop_p":
        for p in (1.0, -0.1, float("nan")):
            assert L.flex_axw_run_root_act_bf16(h._h, 0, x, w, w, None, o, p, 1, None, None, None) == FLEX_ERR_INVALID, p
            assert L.flex_axw_backward_root_act_bf16(h._h, x, w, w, g.data_ptr(), g.data_ptr() + 16, o, None, None, None, None, p, None) == FLEX_ERR_INVALID
    elif what == "work":  # dWork == dOut, dWork == Out
        for fwd, d in ((g.data_ptr(), o), (o, g.data_ptr())):
            assert L.flex_axw_backward_root_act_bf16(h._h, x, w, w, fwd, d, o, _filled(64, 32).data_ptr(), None, None, None, 0.5, None) == FLEX_ERR_INVALID
    elif what == "launcher":
        wf = _filled(32 * 320).data_ptr()
        assert axw._gemm_bf16_root_act_launch(x, w, 32, None, None, 0, None, None, wf, o, 64, 8, 320, 4, 0.5, 1, _stream()) == HIP_ERROR_INVALID_VALUE
        assert axw._gemm_bf16_root_act_launch(x, w, 32, None, None, 0, None, None, wf, o, 64, 8, 64, 4, 1.0, 1, _stream()) == HIP_ERROR_INVALID_VALUE
        assert axw._act_grad_bf16_launch(o, g.data_ptr(), o, 64, 8, 64, 2.0, _stream()) == HIP_ERROR_INVALID_VALUE
    else:
        with pytest.raises(TypeError):
            h.run_root_act(Xd.float(), Wd, Wd)
        with pytest.raises(ValueError):
            h.root_layer(Xd, Wd, Wd, dropout=0.5)
        plain = axw.Axw(a, 32, 8, bf16=True)
        with pytest.raises(FlexError):
            plain.run_root_act(Xd, Wd, Wd)
        plain.destroy()
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (g == -7.0).all(), "a refused call wrote"
    h.destroy()

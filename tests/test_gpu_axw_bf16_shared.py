"""What the bf16 A*X*W launchers share (axw_bf16_device.h, axw_bf16_dw_device.h), pinned on the GPU bit for bit:
  * the wide forward is the root forward without a second source, an addend and a bias: the same Out bits and the same Wf bytes;
  * tests/golden/axw_bf16_bits.json holds a sha256 of what every bf16 launcher writes at the smallest shapes that reach every branch.  The
    kernels use no atomics and a fixed summation order, so the digests hold from run to run and from card to card (n_cus is an argument).
    They were recorded before the launchers were made to share their code, by running this module as a script
    (python tests/test_gpu_axw_bf16_shared.py); a later change that deliberately alters a summation order records them again."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
from flex_amd import axw  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GOLDEN = os.path.join(ROOT, "tests", "golden", "axw_bf16_bits.json")

# (n, dim, c, n_cus): an overlapping last panel, a partial last slab and masked padding; P = 2; NT = 6 on two workgroups (a workgroup runs
# several rounds: the next round's first slab is staged during a round's last); NT = 8 and the longest contraction
WIDE = [(33, 272, 100, 4), (47, 512, 64, 4), (613, 608, 192, 2), (613, 4096, 256, 2)]
_cp = lambda c: (c + 63) // 64 * 64  # noqa: E731
_stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
_filled = lambda *shape: torch.full(shape, -7.0, dtype=torch.bfloat16, device="cuda")  # noqa: E731
_raw = lambda t: (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().tobytes()  # noqa: E731
_ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731


def _normals(rng, *shape):
    """bf16 normals on the device: a random sign, an exponent from 2^-4 to 2^3 and a random mantissa, built as bits"""
    bits = (rng.integers(0, 2, shape) << 15) | (rng.integers(123, 131, shape) << 7) | rng.integers(0, 128, shape)
    return torch.from_numpy(bits.astype(np.uint16).view(np.int16)).cuda().view(torch.bfloat16)


def _ok(rc, *outs):
    torch.cuda.synchronize()
    assert rc == 0, rc
    return outs


def gemm_wide(L, W, n_cus):
    (n, dim), c = L.shape, W.shape[1]
    Wf, out = _filled(dim * _cp(c)), _filled(n, _cp(c))
    return _ok(axw._gemm_bf16_wide_launch(_ptr(L), _ptr(W), _ptr(Wf), _ptr(out), n, dim, c, _cp(c), n_cus, _stream()), out, Wf)


def gemm_root(L1, W1, L2, W2, Cin, bias, n_cus):
    (n, d1), c, d2 = L1.shape, W1.shape[1], 0 if L2 is None else L2.shape[1]
    Wf, out = _filled((d1 + d2) * _cp(c)), _filled(n, _cp(c))
    return _ok(axw._gemm_bf16_root_launch(_ptr(L1), _ptr(W1), d1, _ptr(L2), _ptr(W2), d2, _ptr(Cin), _ptr(bias), _ptr(Wf), _ptr(out), n, c, _cp(c),
                                          n_cus, _stream()), out, Wf)


def gemm_narrow(rng, n, dim, c, n_cus):
    L, Wp, out = _normals(rng, n, dim), _normals(rng, dim, _cp(c)), _filled(n, _cp(c))
    Wp[:, c:] = 0
    return _ok(axw._gemm_bf16_launch(_ptr(L), _ptr(Wp), _ptr(out), n, dim, c, _cp(c), n_cus, _stream()), out)


def dx(rng, launch, n, cp, dim, n_cus):
    G, Wt, out = _normals(rng, n, cp), _normals(rng, cp, dim), _filled(n, dim)
    return _ok(launch(_ptr(G), _ptr(Wt), _ptr(out), n, cp, dim, n_cus, _stream()), out)


def dw(rng, launch, slices, n, dim, c, n_cus):
    X, G, out, part = _normals(rng, n, dim), _normals(rng, n, _cp(c)), _filled(dim, c), torch.empty(slices * dim * c, device="cuda")
    return _ok(launch(_ptr(X), _ptr(G), _ptr(out), _ptr(part), n, dim, c, _cp(c), n_cus, _stream()), out)


def dx_root(rng, n, c, dim, n_cus):
    cp = _cp(c)
    G, W, D, R = _normals(rng, n, cp), _normals(rng, dim, c), _normals(rng, n, cp), _normals(rng, dim, c)
    Wf, out = _filled(2 * dim * cp), _filled(n, dim)
    return _ok(axw._dx_bf16_root_launch(_ptr(G), _ptr(W), _ptr(D), _ptr(R), _ptr(Wf), _ptr(out), n, c, cp, dim, n_cus, _stream()), out, Wf)


def dw_root(rng, n, dim, c, n_cus, with_x):
    cp = _cp(c)
    X, G, D = _normals(rng, n, dim), _normals(rng, n, cp), _normals(rng, n, cp)
    dW, dR, db = _filled(dim, c), _filled(dim, c), torch.full((c,), -7.0, device="cuda")
    part = torch.empty(axw._dw_bf16_root_slices(n, dim, c, n_cus) * (2 * dim * c + c), device="cuda")
    args = (_ptr(X), _ptr(G), _ptr(D), _ptr(dW), _ptr(dR)) if with_x else (None, _ptr(G), _ptr(D), None, None)
    return _ok(axw._dw_bf16_root_launch(*args, _ptr(db), _ptr(part), n, dim, c, cp, n_cus, _stream()), dW, dR, db)


def cases():
    """name -> a call that returns the tensors a launcher wrote.  Every case seeds a generator of its own."""
    out = {}

    def add(name, f, *args):
        seed = [41, len(out), *(int(a) for a in args)]
        out[f"{name}{args}"] = lambda: f(np.random.default_rng(seed), *args)

    for n, dim, c, n_cus in [(33, 48, 100, 4), (613, 256, 256, 2)]:
        add("gemm_narrow", gemm_narrow, n, dim, c, n_cus)
    for n, cp, dim in [(33, 128, 96), (613, 256, 256)]:  # an odd tile count, the widest
        add("dx_narrow", lambda r, *a: dx(r, axw._dx_bf16_launch, *a), n, cp, dim, 4)
    for n, dim, c, n_cus in [(33, 48, 100, 4), (613, 256, 256, 2), (613, 256, 256, 256)]:  # one slice and several
        add("dw_narrow", lambda r, *a: dw(r, axw._dw_bf16_launch, axw.lib().flex_axw_dw_bf16_slices(a[0], a[3]), *a), n, dim, c, n_cus)
    for n, dim, c, n_cus in WIDE:
        add("gemm_wide", lambda r, n, dim, c, k: gemm_wide(_normals(r, n, dim), _normals(r, dim, c), k), n, dim, c, n_cus)
    for n, cp, dim in [(33, 64, 288), (613, 256, 544)]:  # a tail pass of one tile; two full passes and a tail
        add("dx_wide", lambda r, *a: dx(r, axw._dx_bf16_wide_launch, *a), n, cp, dim, 4)
    for n, dim, c, n_cus in [(613, 544, 200, 2), (613, 544, 64, 256)]:  # one slice and several
        add("dw_wide", lambda r, *a: dw(r, axw._dw_bf16_wide_launch, axw._dw_bf16_wide_slices(*a), *a), n, dim, c, n_cus)
    for (n, d1, c, n_cus), d2 in zip(WIDE, (48, 512, 608, 4096)):  # Cin, a bias and a second source; the seam inside a slab and on its edge
        add("gemm_root", lambda r, n, d1, d2, c, k: gemm_root(_normals(r, n, d1), _normals(r, d1, c), _normals(r, n, d2), _normals(r, d2, c),
                                                              _normals(r, n, _cp(c)), _normals(r, c).float(), k), n, d1, d2, c, n_cus)
    for n, c, dim in [(95, 100, 96), (33, 40, 288), (613, 256, 544)]:  # 2-byte pack loads and NT = 3; 16-byte pack loads and a tail of one tile
        add("dx_root", dx_root, n, c, dim, 4)
    for n, dim, c, n_cus in [(613, 256, 64, 2), (613, 256, 64, 256), (613, 288, 192, 2), (2048, 288, 192, 256)]:  # NT = 2 and 4 (two windows)
        add("dw_root", dw_root, n, dim, c, n_cus, True)
    add("dw_root", dw_root, 613, 256, 64, 256, False)  # db alone
    return out


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(_raw(t))
    return h.hexdigest()


@pytest.mark.parametrize("n,dim,c,n_cus", WIDE)
def test_the_wide_gemm_is_the_root_gemm_without_its_extras(n, dim, c, n_cus):
    rng = np.random.default_rng([43, n, dim, c])
    L, W = _normals(rng, n, dim), _normals(rng, dim, c)
    (out_w, wf_w), (out_r, wf_r) = gemm_wide(L, W, n_cus), gemm_root(L, W, None, None, None, None, n_cus)
    assert _raw(wf_w) == _raw(wf_r), "the two launchers pack W into other bytes"
    assert _raw(out_w) == _raw(out_r), "the two launchers write other bits"


@pytest.mark.parametrize("name", list(cases()))
def test_every_bf16_launcher_writes_the_recorded_bits(name):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert digest(cases()[name]()) == want[name], f"{name}: other bits than recorded"


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump({name: digest(run()) for name, run in cases().items()}, f, indent=1)
        f.write("\n")
    print(f"recorded {len(cases())} digests in {GOLDEN}")

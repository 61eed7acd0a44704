"""ctypes binding of include/flex_axw.h (libflex_axw.so): the GCN layer product Out = A * X * W around
the engine's SpMM (≙ run1 / run2 of the reference's cusp.cu).  No fallback: raises if the library is missing."""
from __future__ import annotations

import ctypes as C
import os

from . import binding

FLEX_AXW_AUTO, FLEX_AXW_A_XW, FLEX_AXW_AX_W = 0, 1, 2
FLEX_AXW_USE_BLAS = 0x10000  # flex_axw_create flag: rocBLAS for the dense half
FLEX_AXW_BACKWARD = 0x20000  # flex_axw_create flag: plan A^T too, for flex_axw_backward
_lib = None


def lib():
    global _lib
    if _lib is None:
        binding.lib()  # torch's HIP runtime first, then the engine, then this library on top of it
        path = os.path.join(os.path.dirname(binding.lib_path()), "libflex_axw.so")
        if not os.path.exists(path):
            raise binding.FlexError(f"{path} is missing: build it with `make -C flex_amd/csrc all`")
        L = C.CDLL(path)
        vp = C.c_void_p
        L.flex_axw_create.argtypes = [C.POINTER(vp), C.POINTER(binding._Csr), C.c_int, C.c_int, C.c_int, C.c_uint]
        L.flex_axw_run.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.flex_axw_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.flex_axw_destroy.argtypes = [vp]
        L.flex_axw_ld.argtypes = [C.c_int]
        L.flex_axw_gemm_launch.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
        L.flex_axw_gemm_launch.restype = C.c_int
        _lib = L
    return _lib


def _gemm_launch(L_ptr: int, Wp_ptr: int, Out_ptr: int, n: int, dim: int, c: int, cp: int, n_cus: int, stream: int = 0) -> int:
    """The MFMA GEMM of the dense half on its own (flex_axw_gemm_launch, exported by libflex_axw.so but not part of
    flex_axw.h): Out[n x cp] = L[n x dim] @ Wp[dim x cp], columns >= c written as +0.  Returns the hipError_t; for tests."""
    return lib().flex_axw_gemm_launch(L_ptr, Wp_ptr, Out_ptr, n, dim, c, cp, n_cus, stream)


class Axw:
    """flex_axw handle: plans A for both SpMM widths once; run() computes A @ X @ W in either order."""

    def __init__(self, a: binding.HostCsr, dim: int, c: int, device: int = 0, order: int = binding.FLEX_ORDER_CLUSTER,
                 backward: bool = False):
        """backward: also plan A^T (FLEX_AXW_BACKWARD), for backward() and layer()."""
        self._h = C.c_void_p()
        v = a.view()
        flags = order | (FLEX_AXW_BACKWARD if backward else 0)
        binding._check(lib().flex_axw_create(C.byref(self._h), C.byref(v), dim, c, device, flags), "flex_axw_create")
        self.n, self.dim, self.c, self.ld = a.n, dim, c, lib().flex_axw_ld(c)
        self.has_backward = backward

    def run(self, X, W, order: int = FLEX_AXW_AUTO, timed: bool = False):
        """X [n, dim], W [dim, c]: contiguous float32 cuda tensors.  Returns Out [n, ld] (columns >= c are zero)
        and, if timed, (gemm_ms, spmm_ms)."""
        import torch
        assert X.is_cuda and W.is_cuda and X.dtype == W.dtype == torch.float32 and X.is_contiguous() and W.is_contiguous()
        assert tuple(X.shape) == (self.n, self.dim) and tuple(W.shape) == (self.dim, self.c)
        out = torch.empty((self.n, self.ld), dtype=torch.float32, device=X.device)
        g, s = C.c_float(), C.c_float()
        binding._check(lib().flex_axw_run(self._h, order, X.data_ptr(), W.data_ptr(), out.data_ptr(),
                                          torch.cuda.current_stream(X.device).cuda_stream,
                                          C.byref(g) if timed else None, C.byref(s) if timed else None), "flex_axw_run")
        return (out, (g.value, s.value)) if timed else out

    def backward(self, dOut, X, W, need_x: bool = True, need_w: bool = True):
        """flex_axw_backward: dOut [n, ld] (its padding columns are never read) -> (dX [n, dim] or None, dW [dim, c] or None),
        dX = A^T dOut W^T and dW = X^T (A^T dOut).  X and W are the forward's inputs (only the ones a requested gradient needs)."""
        import torch
        if not self.has_backward:
            raise binding.FlexError("Axw.backward: the handle was made without backward=True (FLEX_AXW_BACKWARD)")
        assert dOut.is_cuda and dOut.dtype == torch.float32 and dOut.is_contiguous() and tuple(dOut.shape) == (self.n, self.ld)
        for t, need, shape in ((X, need_w, (self.n, self.dim)), (W, need_x, (self.dim, self.c))):
            if need:
                assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
        gx = torch.empty((self.n, self.dim), dtype=torch.float32, device=dOut.device) if need_x else None
        gw = torch.empty((self.dim, self.c), dtype=torch.float32, device=dOut.device) if need_w else None
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        binding._check(lib().flex_axw_backward(self._h, ptr(X) if need_w else None, ptr(W) if need_x else None, dOut.data_ptr(),
                                               ptr(gx), ptr(gw), torch.cuda.current_stream(dOut.device).cuda_stream),
                       "flex_axw_backward")
        return gx, gw

    def layer(self, X, W, order: int = FLEX_AXW_AUTO):
        """Differentiable A X W: Out [n, c] (a view of the padded product); its gradient flows to X and W through backward()."""
        if not self.has_backward:
            raise binding.FlexError("Axw.layer: the handle was made without backward=True (FLEX_AXW_BACKWARD)")
        from .autograd import functions
        return functions()[1].apply(X, W, self, order)

    def destroy(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().flex_axw_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

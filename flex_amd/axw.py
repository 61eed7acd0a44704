"""ctypes binding of include/flex_axw.h (libflex_axw.so): the GCN layer product Out = A * X * W around
the engine's SpMM (≙ run1 / run2 of the reference's cusp.cu).  No fallback: raises if the library is missing."""
from __future__ import annotations

import ctypes as C
import os

from . import binding

FLEX_AXW_AUTO, FLEX_AXW_A_XW, FLEX_AXW_AX_W = 0, 1, 2
FLEX_AXW_AX_W_FUSED = 3  # order of run / run_root / run_root_act on a handle made with fused=True: (A X) W in one launch, no intermediate
FLEX_AXW_USE_BLAS = 0x10000  # flex_axw_create flag: rocBLAS for the dense half
FLEX_AXW_BACKWARD = 0x20000  # flex_axw_create flag: plan A^T too, for flex_axw_backward
FLEX_AXW_BF16 = 0x200000  # flex_axw_create flag: the bf16 layer (flex_axw_run_bf16; with FLEX_AXW_BACKWARD flex_axw_backward_bf16)
FLEX_AXW_ROOT = 0x400000  # flex_axw_create flag, with FLEX_AXW_BF16: the buffers of flex_axw_run_root_bf16 (A X W + X R + b)
FLEX_AXW_FUSED = 0x800000  # flex_axw_create flag, with FLEX_AXW_BF16: A's CSR and the row panels on the device, for order FLEX_AXW_AX_W_FUSED
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
        L.flex_axw_run_bf16.argtypes = L.flex_axw_run.argtypes
        L.flex_axw_ld_bf16.argtypes = [C.c_int]
        L.flex_axw_gemm_bf16_launch.argtypes = L.flex_axw_gemm_launch.argtypes
        L.flex_axw_gemm_bf16_launch.restype = C.c_int
        L.flex_axw_backward_bf16.argtypes = L.flex_axw_backward.argtypes
        L.flex_axw_dw_bf16_launch.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
        L.flex_axw_dw_bf16_launch.restype = C.c_int
        L.flex_axw_dw_bf16_slices.argtypes = [C.c_int, C.c_int]
        L.flex_axw_dx_bf16_launch.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
        L.flex_axw_dx_bf16_launch.restype = C.c_int
        L.flex_axw_gemm_bf16_wide_launch.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
        L.flex_axw_gemm_bf16_wide_launch.restype = C.c_int
        L.flex_axw_dx_bf16_wide_launch.argtypes = L.flex_axw_dx_bf16_launch.argtypes
        L.flex_axw_dx_bf16_wide_launch.restype = C.c_int
        L.flex_axw_dw_bf16_wide_launch.argtypes = L.flex_axw_dw_bf16_launch.argtypes
        L.flex_axw_dw_bf16_wide_launch.restype = C.c_int
        L.flex_axw_dw_bf16_wide_slices.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        L.flex_axw_run_root_bf16.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.flex_axw_gemm_bf16_root_launch.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
        L.flex_axw_gemm_bf16_root_launch.restype = C.c_int
        L.flex_axw_backward_root_bf16.argtypes = [vp] * 10
        L.flex_axw_dx_bf16_root_launch.argtypes = [vp] * 6 + [C.c_int] * 5 + [vp]
        L.flex_axw_dx_bf16_root_launch.restype = C.c_int
        L.flex_axw_dw_bf16_root_launch.argtypes = [vp] * 7 + [C.c_int] * 5 + [vp]
        L.flex_axw_dw_bf16_root_launch.restype = C.c_int
        L.flex_axw_dw_bf16_root_slices.argtypes = [C.c_int] * 4
        L.flex_axw_run_root_act_bf16.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_float, C.c_uint64, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.flex_axw_backward_root_act_bf16.argtypes = [vp] * 11 + [C.c_float, vp]
        L.flex_axw_gemm_bf16_root_act_launch.argtypes = L.flex_axw_gemm_bf16_root_launch.argtypes[:-1] + [C.c_float, C.c_uint64, vp]
        L.flex_axw_gemm_bf16_root_act_launch.restype = C.c_int
        L.flex_axw_act_grad_bf16_launch.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, vp]
        L.flex_axw_act_grad_bf16_launch.restype = C.c_int
        L.flex_axw_fused_bf16_launch.argtypes = [vp] * 6 + [C.c_int, C.c_float, C.c_uint64, C.c_int, vp]
        L.flex_axw_fused_bf16_launch.restype = C.c_int
        _lib = L
    return _lib


def _gemm_launch(L_ptr: int, Wp_ptr: int, Out_ptr: int, n: int, dim: int, c: int, cp: int, n_cus: int, stream: int = 0) -> int:
    """The MFMA GEMM of the dense half on its own (flex_axw_gemm_launch, exported by libflex_axw.so but not part of
    flex_axw.h): Out[n x cp] = L[n x dim] @ Wp[dim x cp], columns >= c written as +0.  Returns the hipError_t; for tests."""
    return lib().flex_axw_gemm_launch(L_ptr, Wp_ptr, Out_ptr, n, dim, c, cp, n_cus, stream)


def _gemm_bf16_launch(L_ptr: int, Wp_ptr: int, Out_ptr: int, n: int, dim: int, c: int, cp: int, n_cus: int, stream: int = 0) -> int:
    """The bf16 MFMA GEMM of the bf16 layer on its own (flex_axw_gemm_bf16_launch, exported like flex_axw_gemm_launch): bf16
    Out[n x cp] = L[n x dim] @ Wp[dim x cp] with fp32 sums, columns >= c written as +0 bits.  Returns the hipError_t; for tests."""
    return lib().flex_axw_gemm_bf16_launch(L_ptr, Wp_ptr, Out_ptr, n, dim, c, cp, n_cus, stream)


def _dw_bf16_launch(X_ptr: int, G_ptr: int, dW_ptr: int, part_ptr: int, n: int, dim: int, c: int, cp: int, n_cus: int, stream: int = 0) -> int:
    """The bf16 dW kernel of flex_axw_backward_bf16 on its own (flex_axw_dw_bf16_launch): bf16 dW[dim x c] = X[n x dim]^T @ G[n x cp] through
    the fp32 partials `part` (flex_axw_dw_bf16_slices(n, n_cus) x dim x c floats).  Returns the hipError_t; for tests."""
    return lib().flex_axw_dw_bf16_launch(X_ptr, G_ptr, dW_ptr, part_ptr, n, dim, c, cp, n_cus, stream)


def _dx_bf16_launch(G_ptr: int, Wt_ptr: int, dX_ptr: int, n: int, cp: int, dim: int, n_cus: int, stream: int = 0) -> int:
    """The dX product of flex_axw_backward_bf16 on its own (flex_axw_dx_bf16_launch): bf16 dX[n x dim] = G[n x cp] @ Wt[cp x dim], dim any
    multiple of 32.  Returns the hipError_t; for tests."""
    return lib().flex_axw_dx_bf16_launch(G_ptr, Wt_ptr, dX_ptr, n, cp, dim, n_cus, stream)


def _gemm_bf16_wide_launch(L_ptr: int, W_ptr: int, Wf_ptr: int, Out_ptr: int, n: int, dim: int, c: int, cp: int, n_cus: int, stream: int = 0) -> int:
    """The bf16 GEMM of the bf16 layer at 256 < dim <= 4096 on its own (flex_axw_gemm_bf16_wide_launch): bf16 Out[n x cp] = L[n x dim] @
    W[dim x c] -- W unpadded -- through the scratch Wf (dim x cp elements: W as MFMA fragments), columns >= c written as +0 bits.  Returns
    the hipError_t; for tests."""
    return lib().flex_axw_gemm_bf16_wide_launch(L_ptr, W_ptr, Wf_ptr, Out_ptr, n, dim, c, cp, n_cus, stream)


def _dx_bf16_wide_launch(G_ptr: int, Wt_ptr: int, dX_ptr: int, n: int, cp: int, dim: int, n_cus: int, stream: int = 0) -> int:
    """_dx_bf16_launch at 256 < dim <= 4096 (flex_axw_dx_bf16_wide_launch): dX in passes of 256 columns.  Returns the hipError_t; for tests."""
    return lib().flex_axw_dx_bf16_wide_launch(G_ptr, Wt_ptr, dX_ptr, n, cp, dim, n_cus, stream)


def _dw_bf16_wide_launch(X_ptr: int, G_ptr: int, dW_ptr: int, part_ptr: int, n: int, dim: int, c: int, cp: int, n_cus: int, stream: int = 0) -> int:
    """_dw_bf16_launch at 256 < dim <= 4096, dim % 32 == 0 (flex_axw_dw_bf16_wide_launch); `part` holds _dw_bf16_wide_slices(n, dim, c, n_cus)
    x dim x c floats.  Returns the hipError_t; for tests."""
    return lib().flex_axw_dw_bf16_wide_launch(X_ptr, G_ptr, dW_ptr, part_ptr, n, dim, c, cp, n_cus, stream)


def _dw_bf16_wide_slices(n: int, dim: int, c: int, n_cus: int) -> int:
    """n-slices of the wide dW kernel (flex_axw_dw_bf16_wide_slices): at most n / (2 c), so that the fp32 partials stay below the bytes of X."""
    return lib().flex_axw_dw_bf16_wide_slices(n, dim, c, n_cus)


def _gemm_bf16_root_launch(L1_ptr: int, W1_ptr: int, d1: int, L2_ptr, W2_ptr, d2: int, Cin_ptr, bias_ptr, Wf_ptr: int, Out_ptr: int, n: int,
                           c: int, cp: int, n_cus: int, stream: int = 0) -> int:
    """The dense stage of flex_axw_run_root_bf16 on its own (flex_axw_gemm_bf16_root_launch): bf16 Out[n x cp] = L1[n x d1] @ W1[d1 x c] +
    L2[n x d2] @ W2[d2 x c] + Cin[n x cp] + bias[c] (fp32) in one fp32 chain, through the scratch Wf ((d1 + d2) x cp elements); L2 / W2 with
    d2 = 0, Cin and bias may each be None.  Columns >= c are written as +0 bits.  Returns the hipError_t; for tests."""
    return lib().flex_axw_gemm_bf16_root_launch(L1_ptr, W1_ptr, d1, L2_ptr, W2_ptr, d2, Cin_ptr, bias_ptr, Wf_ptr, Out_ptr, n, c, cp, n_cus, stream)


def _dx_bf16_root_launch(G_ptr: int, W_ptr: int, dOut_ptr: int, R_ptr: int, Wf_ptr: int, dX_ptr: int, n: int, c: int, cp: int, dim: int,
                         n_cus: int, stream: int = 0) -> int:
    """The dX product of flex_axw_backward_root_bf16 on its own (flex_axw_dx_bf16_root_launch): bf16 dX[n x dim] = G[n x cp] @ W[dim x c].T +
    dOut[n x cp] @ R[dim x c].T in one fp32 chain, dim any multiple of 32 up to 4096, through the scratch Wf (2 dim x cp elements).  Returns the
    hipError_t; for tests."""
    return lib().flex_axw_dx_bf16_root_launch(G_ptr, W_ptr, dOut_ptr, R_ptr, Wf_ptr, dX_ptr, n, c, cp, dim, n_cus, stream)


def _dw_bf16_root_launch(X_ptr, G_ptr: int, dOut_ptr: int, dW_ptr, dR_ptr, db_ptr, part_ptr: int, n: int, dim: int, c: int, cp: int, n_cus: int,
                         stream: int = 0) -> int:
    """The one-pass kernel of flex_axw_backward_root_bf16 on its own (flex_axw_dw_bf16_root_launch): bf16 dW = X.T @ G and dR = X.T @ dOut
    [dim x c] and fp32 db = dOut.sum(0) [c] through the fp32 partials `part` (_dw_bf16_root_slices(n, dim, c, n_cus) x (2 dim c + c) floats);
    an output that is None is not written.  Returns the hipError_t; for tests."""
    return lib().flex_axw_dw_bf16_root_launch(X_ptr, G_ptr, dOut_ptr, dW_ptr, dR_ptr, db_ptr, part_ptr, n, dim, c, cp, n_cus, stream)


def _dw_bf16_root_slices(n: int, dim: int, c: int, n_cus: int) -> int:
    """n-slices of the one-pass dW / dR / db kernel (flex_axw_dw_bf16_root_slices): at most n / (4 c)."""
    return lib().flex_axw_dw_bf16_root_slices(n, dim, c, n_cus)


def _gemm_bf16_root_act_launch(L1_ptr: int, W1_ptr: int, d1: int, L2_ptr, W2_ptr, d2: int, Cin_ptr, bias_ptr, Wf_ptr: int, Out_ptr: int, n: int,
                               c: int, cp: int, n_cus: int, drop_p: float, seed: int, stream: int = 0) -> int:
    """The dense stage of flex_axw_run_root_act_bf16 on its own (flex_axw_gemm_bf16_root_act_launch): _gemm_bf16_root_launch with ReLU and
    dropout (probability drop_p, mask binding.dropout_mask(seed, drop_p, 0, n * c) as [n, c]) before the one rounding.  Returns the
    hipError_t; for tests."""
    return lib().flex_axw_gemm_bf16_root_act_launch(L1_ptr, W1_ptr, d1, L2_ptr, W2_ptr, d2, Cin_ptr, bias_ptr, Wf_ptr, Out_ptr, n, c, cp, n_cus,
                                                    drop_p, seed, stream)


def _act_grad_bf16_launch(Out_ptr: int, dOut_ptr: int, dZ_ptr: int, n: int, c: int, cp: int, cs: float, stream: int = 0) -> int:
    """The first pass of flex_axw_backward_root_act_bf16 on its own (flex_axw_act_grad_bf16_launch): bf16 dZ[n x cp] = dOut * cs where
    Out > 0, +0 elsewhere and in columns >= c.  Returns the hipError_t; for tests."""
    return lib().flex_axw_act_grad_bf16_launch(Out_ptr, dOut_ptr, dZ_ptr, n, c, cp, cs, stream)


def _fused_bf16_launch(h: "Axw", X_ptr: int, W_ptr: int, R_ptr, bias_ptr, Out_ptr: int, relu: bool, drop_p: float, seed: int, n_workgroups: int,
                       stream: int = 0) -> int:
    """The one launch of order FLEX_AXW_AX_W_FUSED on its own (flex_axw_fused_bf16_launch), with the grid size as an argument: any
    n_workgroups > 0 gives the same bits.  R_ptr None: the plain layer (bias None, relu False, drop_p 0); else the root forms.  Returns the
    hipError_t; for tests."""
    return lib().flex_axw_fused_bf16_launch(h._h, X_ptr, W_ptr, R_ptr, bias_ptr, Out_ptr, int(relu), drop_p, seed, n_workgroups, stream)


class Axw:
    """flex_axw handle: plans A for both SpMM widths once; run() computes A @ X @ W in either order."""

    def __init__(self, a: binding.HostCsr, dim: int, c: int, device: int = 0, order: int = binding.FLEX_ORDER_CLUSTER,
                 backward: bool = False, bf16: bool = False, root: bool = False, fused: bool = False):
        """backward: also plan A^T (FLEX_AXW_BACKWARD), for backward() and layer().  bf16: the bf16 layer (FLEX_AXW_BF16): run() and backward() take
        and return torch.bfloat16 (dim % 16 == 0, dim <= 4096, c <= 256, n >= 32; with backward=True dim % 32 == 0).  dim > 256 runs the
        wide kernels (axw_bf16_wide_kernels.hip); a width that is no multiple of 16 (602, 1433) is served exactly by zero columns of X and
        zero rows of W.  root (with bf16=True only): the buffers of run_root() (FLEX_AXW_ROOT).  fused (with bf16=True only, dim <= 256): the
        handle also keeps A's CSR and its 32-row panels on the device (FLEX_AXW_FUSED), and run(), run_root(), run_root_act(), layer() and
        root_layer() take order=FLEX_AXW_AX_W_FUSED: order (A X) W as ONE kernel launch with no n x dim intermediate
        (axw_bf16_fused_kernels.hip), within the same bounds as FLEX_AXW_AX_W but not its bits; AUTO never picks it."""
        self._h = C.c_void_p()
        v = a.view()
        flags = order | (FLEX_AXW_BACKWARD if backward else 0) | (FLEX_AXW_BF16 if bf16 else 0) | (FLEX_AXW_ROOT if root else 0) | (
            FLEX_AXW_FUSED if fused else 0)
        binding._check(lib().flex_axw_create(C.byref(self._h), C.byref(v), dim, c, device, flags), "flex_axw_create")
        self.n, self.dim, self.c, self.ld = a.n, dim, c, (lib().flex_axw_ld_bf16(c) if bf16 else lib().flex_axw_ld(c))
        self.has_backward = backward
        self.bf16 = bf16
        self.has_root = root
        self.has_fused = fused

    def run(self, X, W, order: int = FLEX_AXW_AUTO, timed: bool = False):
        """X [n, dim], W [dim, c]: contiguous cuda tensors, float32 -- torch.bfloat16 on a bf16 handle (any other dtype: TypeError).
        Returns Out [n, ld] of that dtype (columns >= c are zero) and, if timed, (gemm_ms, spmm_ms).  order=FLEX_AXW_AX_W_FUSED (a fused=True
        handle): one launch, reported as spmm_ms with gemm_ms 0."""
        import torch
        want = torch.bfloat16 if self.bf16 else torch.float32
        if X.dtype != want or W.dtype != want:
            raise TypeError(f"Axw.run: this handle takes {want} X and W; got {X.dtype} and {W.dtype}")
        assert X.is_cuda and W.is_cuda and X.is_contiguous() and W.is_contiguous()
        assert tuple(X.shape) == (self.n, self.dim) and tuple(W.shape) == (self.dim, self.c)
        out = torch.empty((self.n, self.ld), dtype=want, device=X.device)
        g, s = C.c_float(), C.c_float()
        call, what = (lib().flex_axw_run_bf16, "flex_axw_run_bf16") if self.bf16 else (lib().flex_axw_run, "flex_axw_run")
        binding._check(call(self._h, order, X.data_ptr(), W.data_ptr(), out.data_ptr(), torch.cuda.current_stream(X.device).cuda_stream,
                            C.byref(g) if timed else None, C.byref(s) if timed else None), what)
        return (out, (g.value, s.value)) if timed else out

    def run_root(self, X, W, R, bias=None, order: int = FLEX_AXW_AUTO, timed: bool = False):
        """flex_axw_run_root_bf16: A @ X @ W + X @ R + bias with one rounding after the last sum.  X [n, dim], W and R [dim, c]: contiguous
        cuda torch.bfloat16; bias: float32 [c] or None (anything else: TypeError).  Returns Out [n, ld] in bfloat16 (columns >= c are zero)
        and, if timed, (gemm_ms, spmm_ms).  order=FLEX_AXW_AX_W_FUSED (a fused=True handle): the whole layer in one launch; FlexError
        (FLEX_ERR_UNSUPPORTED) where [W; R] does not fit in LDS (dim = 256, c > 128).  No autograd: root_layer() is the differentiable form."""
        import torch
        if not self.has_root:
            raise binding.FlexError("Axw.run_root: the handle was made without root=True (FLEX_AXW_ROOT)")
        if any(t.dtype != torch.bfloat16 for t in (X, W, R)):
            raise TypeError(f"Axw.run_root takes torch.bfloat16 X, W and R; got {X.dtype}, {W.dtype} and {R.dtype}")
        if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (self.c,)):
            raise TypeError(f"Axw.run_root takes a float32 bias of shape [{self.c}]; got {bias.dtype} {tuple(bias.shape)}")
        assert all(t.is_cuda and t.is_contiguous() for t in (X, W, R)) and (bias is None or (bias.is_cuda and bias.is_contiguous()))
        assert tuple(X.shape) == (self.n, self.dim) and tuple(W.shape) == tuple(R.shape) == (self.dim, self.c)
        out = torch.empty((self.n, self.ld), dtype=torch.bfloat16, device=X.device)
        g, s = C.c_float(), C.c_float()
        binding._check(lib().flex_axw_run_root_bf16(self._h, order, X.data_ptr(), W.data_ptr(), R.data_ptr(), None if bias is None else bias.data_ptr(),
                                                    out.data_ptr(), torch.cuda.current_stream(X.device).cuda_stream,
                                                    C.byref(g) if timed else None, C.byref(s) if timed else None), "flex_axw_run_root_bf16")
        return (out, (g.value, s.value)) if timed else out

    def run_root_act(self, X, W, R, bias=None, p: float = 0.0, seed: int = 0, order: int = FLEX_AXW_AUTO, timed: bool = False):
        """flex_axw_run_root_act_bf16: run_root() with ReLU and dropout (probability p, the kept entries scaled by 1 / (1 - p), the mask
        binding.dropout_mask(seed, p, 0, n * c) as [n, c]) applied in the last kernel before its one rounding.  Operands, errors and the
        return value as run_root().  No autograd: root_layer(relu=True) is the differentiable form."""
        import torch
        if not self.has_root:
            raise binding.FlexError("Axw.run_root_act: the handle was made without root=True (FLEX_AXW_ROOT)")
        if any(t.dtype != torch.bfloat16 for t in (X, W, R)):
            raise TypeError(f"Axw.run_root_act takes torch.bfloat16 X, W and R; got {X.dtype}, {W.dtype} and {R.dtype}")
        if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (self.c,)):
            raise TypeError(f"Axw.run_root_act takes a float32 bias of shape [{self.c}]; got {bias.dtype} {tuple(bias.shape)}")
        assert all(t.is_cuda and t.is_contiguous() for t in (X, W, R)) and (bias is None or (bias.is_cuda and bias.is_contiguous()))
        assert tuple(X.shape) == (self.n, self.dim) and tuple(W.shape) == tuple(R.shape) == (self.dim, self.c)
        out = torch.empty((self.n, self.ld), dtype=torch.bfloat16, device=X.device)
        g, s = C.c_float(), C.c_float()
        binding._check(lib().flex_axw_run_root_act_bf16(self._h, order, X.data_ptr(), W.data_ptr(), R.data_ptr(),
                                                        None if bias is None else bias.data_ptr(), out.data_ptr(), p, seed,
                                                        torch.cuda.current_stream(X.device).cuda_stream, C.byref(g) if timed else None,
                                                        C.byref(s) if timed else None), "flex_axw_run_root_act_bf16")
        return (out, (g.value, s.value)) if timed else out

    def backward(self, dOut, X, W, need_x: bool = True, need_w: bool = True):
        """flex_axw_backward: dOut [n, ld] -> (dX [n, dim] or None, dW [dim, c] or None), dX = A^T dOut W^T and dW = X^T (A^T dOut).  X and
        W are the forward's inputs (only the ones a requested gradient needs).  float32, dOut's padding columns never read; on a bf16
        handle flex_axw_backward_bf16: torch.bfloat16 in and out (any other dtype: TypeError), dOut's padding columns read and finite."""
        import torch
        if not self.has_backward:
            raise binding.FlexError("Axw.backward: the handle was made without backward=True (FLEX_AXW_BACKWARD)")
        want = torch.bfloat16 if self.bf16 else torch.float32
        given = [t for t, need in ((dOut, True), (X, need_w), (W, need_x)) if need]
        if any(t.dtype != want for t in given):
            raise TypeError(f"Axw.backward: this handle takes {want} dOut, X and W; got {[str(t.dtype) for t in given]}")
        assert dOut.is_cuda and dOut.is_contiguous() and tuple(dOut.shape) == (self.n, self.ld)
        for t, need, shape in ((X, need_w, (self.n, self.dim)), (W, need_x, (self.dim, self.c))):
            if need:
                assert t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape
        gx = torch.empty((self.n, self.dim), dtype=want, device=dOut.device) if need_x else None
        gw = torch.empty((self.dim, self.c), dtype=want, device=dOut.device) if need_w else None
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        call, what = (lib().flex_axw_backward_bf16, "flex_axw_backward_bf16") if self.bf16 else (lib().flex_axw_backward, "flex_axw_backward")
        binding._check(call(self._h, ptr(X) if need_w else None, ptr(W) if need_x else None, dOut.data_ptr(), ptr(gx), ptr(gw),
                            torch.cuda.current_stream(dOut.device).cuda_stream), what)
        return gx, gw

    def layer(self, X, W, order: int = FLEX_AXW_AUTO):
        """Differentiable A X W: Out [n, c] (a view of the padded product); its gradient flows to X and W through backward().  On a bf16
        handle X, W, Out and the gradients are torch.bfloat16."""
        if not self.has_backward:
            raise binding.FlexError("Axw.layer: the handle was made without backward=True (FLEX_AXW_BACKWARD)")
        from .autograd import functions
        return functions()[1].apply(X, W, self, order)

    def backward_root(self, dOut, X, W, R, need_x: bool = True, need_w: bool = True, need_b: bool = True, _act=None):
        """flex_axw_backward_root_bf16: dOut [n, ld] -> (dX [n, dim], dW [dim, c], dR [dim, c], db [c] float32), each None unless asked for:
        dX = A^T dOut W^T + dOut R^T in one chain, dW = X^T (A^T dOut), dR = X^T dOut, db = dOut.sum(0).  dW and dR come together (need_w).
        X, W and R are the forward's inputs (only the ones a requested gradient needs); torch.bfloat16 (any other dtype: TypeError);
        dOut's padding columns are read and must be finite.  _act = (Out, p): backward_root_act()."""
        import torch
        if not (self.has_backward and self.has_root):
            raise binding.FlexError("Axw.backward_root: the handle was made without backward=True and root=True")
        given = [t for t, need in ((dOut, True), (X, need_w), (W, need_x), (R, need_x)) if need] + ([] if _act is None else [_act[0]])
        if any(t.dtype != torch.bfloat16 for t in given):
            raise TypeError(f"Axw.backward_root takes torch.bfloat16 dOut, X, W and R; got {[str(t.dtype) for t in given]}")
        assert dOut.is_cuda and dOut.is_contiguous() and tuple(dOut.shape) == (self.n, self.ld)
        for t, need, shape in ((X, need_w, (self.n, self.dim)), (W, need_x, (self.dim, self.c)), (R, need_x, (self.dim, self.c))):
            if need:
                assert t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape
        new = lambda need, shape, dtype=torch.bfloat16: torch.empty(shape, dtype=dtype, device=dOut.device) if need else None  # noqa: E731
        gx, gw, gr = new(need_x, (self.n, self.dim)), new(need_w, (self.dim, self.c)), new(need_w, (self.dim, self.c))
        gb = new(need_b, (self.c,), torch.float32)
        ptr = lambda t, need=True: t.data_ptr() if need and t is not None else None  # noqa: E731
        stream = torch.cuda.current_stream(dOut.device).cuda_stream
        if _act is None:
            binding._check(lib().flex_axw_backward_root_bf16(self._h, ptr(X, need_w), ptr(W, need_x), ptr(R, need_x), dOut.data_ptr(), ptr(gx),
                                                             ptr(gw), ptr(gr), ptr(gb), stream), "flex_axw_backward_root_bf16")
        else:
            out, p = _act
            assert out.is_cuda and out.is_contiguous() and tuple(out.shape) == (self.n, self.ld)
            work = torch.empty_like(dOut)
            binding._check(lib().flex_axw_backward_root_act_bf16(self._h, ptr(X, need_w), ptr(W, need_x), ptr(R, need_x), out.data_ptr(),
                                                                 dOut.data_ptr(), work.data_ptr(), ptr(gx), ptr(gw), ptr(gr), ptr(gb), p, stream),
                           "flex_axw_backward_root_act_bf16")
        return gx, gw, gr, gb

    def backward_root_act(self, dOut, Out, X, W, R, p: float = 0.0, need_x: bool = True, need_w: bool = True, need_b: bool = True):
        """flex_axw_backward_root_act_bf16: backward_root() of dZ = dOut / (1 - p) where Out > 0, +0 elsewhere; Out [n, ld] is what
        run_root_act() returned under the same p (no mask, no seed).  dOut's padding columns are ignored."""
        return self.backward_root(dOut, X, W, R, need_x, need_w, need_b, _act=(Out, p))

    def root_layer(self, X, W, R, bias=None, order: int = FLEX_AXW_AUTO, relu: bool = False, dropout: float = 0.0, seed=None,
                   training: bool = True):
        """Differentiable A X W + X R + bias: Out [n, c] (a view of run_root()'s padded product); its gradient flows to X, W, R and bias
        through backward_root().  X, W, R, Out and their gradients are torch.bfloat16, bias and its gradient float32.
        relu=True: the hidden layer dropout(relu(.)) in the same kernels (run_root_act / backward_root_act): dropout is the drop probability
        (0 when training is False), seed the mask's (None: one is drawn from torch's generator); the backward keeps Out, not a mask.
        dropout > 0 without relu=True is a ValueError: the backward reads the mask off Out > 0, which needs the ReLU."""
        if not (self.has_backward and self.has_root):
            raise binding.FlexError("Axw.root_layer: the handle was made without backward=True and root=True")
        from .autograd import axw_root_act_functions, axw_root_functions
        if not relu:
            if dropout > 0:
                raise ValueError("Axw.root_layer: dropout > 0 needs relu=True")
            return axw_root_functions()[0].apply(X, W, R, bias, self, order)
        p = float(dropout) if training else 0.0
        if p > 0 and seed is None:
            import torch
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        return axw_root_act_functions()[0].apply(X, W, R, bias, self, order, p, int(seed or 0) & 0xFFFFFFFFFFFFFFFF)

    def destroy(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().flex_axw_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

"""torch autograd over the engine: the gradient of C = A B with respect to B is A^T grad_C (a plan made with FLEX_PLAN_TRANSPOSE),
and the GCN layer Out = A X W (flex_amd.axw.Axw.layer) differentiates through flex_axw_backward.  Gradients for A's values (SDDMM) are
not computed: asking for them raises.  torch is imported lazily, as in binding.py."""
from __future__ import annotations

from . import binding


def _function():
    import torch

    class _SpMM(torch.autograd.Function):
        @staticmethod
        def forward(ctx, B, op):
            ctx.op = op
            return op.forward_plan(B.contiguous())

        @staticmethod
        def backward(ctx, grad_C):
            return ctx.op.transposed_plan(grad_C.contiguous()), None

    class _AxwLayer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, X, W, h, order):
            X, W = X.contiguous(), W.contiguous()
            ctx.h = h
            ctx.save_for_backward(X, W)
            return h.run(X, W, order)[:, : h.c]

        @staticmethod
        def backward(ctx, grad_out):
            X, W = ctx.saved_tensors
            h = ctx.h
            dOut = torch.zeros((h.n, h.ld), dtype=torch.float32, device=grad_out.device)
            dOut[:, : h.c] = grad_out
            gx, gw = h.backward(dOut, X, W, need_x=ctx.needs_input_grad[0], need_w=ctx.needs_input_grad[1])
            return gx, gw, None, None

    return _SpMM, _AxwLayer


_cache = None


def functions():
    """(_SpMM, _AxwLayer): the autograd Functions, built at first use (torch is imported then)."""
    global _cache
    if _cache is None:
        _cache = _function()
    return _cache


class SparseOperator:
    """C = A B for a fixed sparse A, differentiable in B: grad_B = A^T grad_C.  Keeps the plan of A (k columns) and the plan of A^T.
    `a` is an m x n HostCsr; op(B) takes B [n, k] and returns C [m, k], float32 cuda tensors."""

    def __init__(self, a: binding.HostCsr, k: int, device: int = 0, order: int = binding.FLEX_ORDER_NATURAL, tuning: dict | None = None):
        self.m, self.n, self.k = a.m, a.n, k
        self.plan = binding.Plan(a, k, device=device, order=order, tuning=tuning)
        self.plan_t = binding.Plan(a, k, device=device, order=order, tuning=tuning, transpose=True)

    def forward_plan(self, B):
        return self.plan(B)

    def transposed_plan(self, G):
        return self.plan_t(G)

    def __call__(self, B, values=None):
        """values: must be None -- A's values are constants of the plan; a gradient for them (SDDMM) is not computed."""
        if values is not None:
            raise NotImplementedError("gradients for A's values (SDDMM) are not computed by SparseOperator")
        return functions()[0].apply(B, self)


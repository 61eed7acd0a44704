"""torch autograd over the engine: the gradient of C = A B with respect to B is A^T grad_C (a plan made with FLEX_PLAN_TRANSPOSE; on
bfloat16 operands with SparseOperator(..., bf16=True): FLEX_PLAN_BF16 plans and flex_spmm_bf16, both ways),
and the GCN layer Out = A X W (flex_amd.axw.Axw.layer) differentiates through flex_axw_backward.  With learn_values=True, SparseOperator
is differentiable in A's values as well: grad_v = SDDMM(grad_C, B) over A's pattern (flex_sddmm), and the values of every forward are
set into the plans (flex_plan_set_values) without planning again.  The same two plans run a graph-attention layer end to end:
scores by flex_sddmm as a forward op, their softmax over each row of A (flex_edge_softmax), and the SpMM with the result as A's values
(SparseOperator.attention).  fused_attention=True runs that forward as one launch (flex_attention), and fused_backward=True its backward as
two (flex_attention_backward) instead of the chain of eight calls; with both, attention(..., heads=H) runs H heads in the same three
launches (flex_attention_heads, flex_attention_heads_backward), on torch.bfloat16 Q, K and V as well (flex_attention_bf16,
flex_attention_bf16_backward: bf16 rows, float32 accumulation), and gat_attention(el, er, V) runs GAT's additive score
LeakyReLU(el[row] + er[col]) per head in the same three launches (flex_gat_attention, flex_gat_attention_backward).
attention(..., bias=b) adds a learned term per entry and head to the scaled score before the softmax, in float32 or bfloat16 rows, still
in three launches (flex_attention_bias, flex_attention_bf16_bias and their backward calls).  attention(..., dropout=p) drops the
probabilities after the softmax, with or without a bias, in the same three launches (flex_attention_dropout, flex_attention_bf16_dropout
and their backward calls): the mask is a hash of (seed, entry, head), so autograd keeps the seed and no mask.  gat_attention on a
torch.bfloat16 V, with or without dropout, runs the same three launches on bf16 V rows (flex_gat_attention_bf16,
flex_gat_attention_bf16_dropout and their backward calls: float32 scores and sums, Out and grad V in bfloat16).
gatv2_attention(xt, xs, att) runs GATv2's score att[h] . LeakyReLU(xt[row] + xs[col]), which needs the full rows, in one forward launch
and up to three backward launches (flex_gatv2_attention, flex_gatv2_attention_backward), float32 only; with dropout= it drops the
probabilities after the softmax in the same launches (flex_dropout_gatv2_attention and its backward call), keeping the seed and no
mask.  torch is imported lazily, as in binding.py."""
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

    class _SpMMValues(torch.autograd.Function):
        """C = A(v) B.  Backward: grad_B = A(v)^T grad_C on the transposed plan, set to THIS forward's v first (another forward may have
        set other values since); grad_v = SDDMM(grad_C, B) on the forward plan (it reads the pattern only)."""

        @staticmethod
        def forward(ctx, B, v, op):
            B, v = B.contiguous(), v.detach().contiguous()
            op.plan.set_values(v)
            ctx.op = op
            ctx.save_for_backward(B, v)
            return op.plan(B)

        @staticmethod
        def backward(ctx, grad_C):
            B, v = ctx.saved_tensors
            op = ctx.op
            grad_C = grad_C.contiguous()
            gB = gv = None
            if ctx.needs_input_grad[0]:
                op.plan_t.set_values(v)
                gB = op.plan_t(grad_C)
            if ctx.needs_input_grad[1]:
                gv = op.plan.sddmm(grad_C, B)
            return gB, gv, None

    class _Sddmm(torch.autograd.Function):
        """s[e] = <Q[row(e)], K[col(e)]> over A's pattern.  Backward, with g = grad_s as A's values: grad_Q = A(g) K on the forward plan,
        grad_K = A(g)^T Q on the transposed plan, each set to g immediately before it runs (the plans are shared with the other Functions)."""

        @staticmethod
        def forward(ctx, Q, K, op):
            Q, K = Q.contiguous(), K.contiguous()
            ctx.op = op
            ctx.save_for_backward(Q, K)
            return op.plan.sddmm(Q, K)

        @staticmethod
        def backward(ctx, grad_s):
            Q, K = ctx.saved_tensors
            op = ctx.op
            g = grad_s.contiguous()
            gQ = gK = None
            if ctx.needs_input_grad[0]:
                op.plan.set_values(g)
                gQ = op.plan(K)
            if ctx.needs_input_grad[1]:
                op.plan_t.set_values(g)
                gK = op.plan_t(Q)
            return gQ, gK, None

    class _EdgeSoftmax(torch.autograd.Function):
        """p = softmax of scale * s over each row of A; keeps p.  Backward: grad_s = scale p (grad_p - sum over the row of p grad_p)."""

        @staticmethod
        def forward(ctx, s, op, scale):
            p = op.plan.edge_softmax(s.contiguous(), scale)
            ctx.op, ctx.scale = op, scale
            ctx.save_for_backward(p)
            return p

        @staticmethod
        def backward(ctx, grad_p):
            (p,) = ctx.saved_tensors
            return ctx.op.plan.edge_softmax_backward(p, grad_p.contiguous(), ctx.scale), None, None

    class _FusedAttention(torch.autograd.Function):
        """Out = A(alpha) V, alpha = softmax over each row of A of scale <Q[row], K[col]>, by flex_attention in one launch; alpha is
        written and kept only when a gradient is needed.  Backward: the chain of _SpMMValues, _EdgeSoftmax and _Sddmm from the kept
        alpha, every plan set immediately before it is used -- or, on an operator made with fused_backward=True, the one call
        flex_attention_backward for the gradients that are needed (it sets no plan's values)."""

        @staticmethod
        def forward(ctx, Q, K, V, op, scale):
            Q, K, V = Q.contiguous(), K.contiguous(), V.contiguous()
            p = torch.zeros(op.nnz, dtype=torch.float32, device=Q.device) if any(ctx.needs_input_grad[:3]) else None
            out = op.plan.attention(Q, K, V, scale, p=p)
            ctx.op, ctx.scale = op, scale
            ctx.save_for_backward(Q, K, V, p)
            return out

        @staticmethod
        def backward(ctx, grad_out):
            Q, K, V, p = ctx.saved_tensors
            op = ctx.op
            g = grad_out.contiguous()
            if op.fused_backward:
                return (*op.plan.attention_backward(Q, K, V, p, g, ctx.scale, want=tuple(ctx.needs_input_grad[:3])), None, None)
            gQ = gK = gV = None
            if ctx.needs_input_grad[2]:
                op.plan_t.set_values(p)
                gV = op.plan_t(g)
            if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
                gs = op.plan.edge_softmax_backward(p, op.plan.sddmm(g, V), ctx.scale)
                if ctx.needs_input_grad[0]:
                    op.plan.set_values(gs)
                    gQ = op.plan(K)
                if ctx.needs_input_grad[1]:
                    op.plan_t.set_values(gs)
                    gK = op.plan_t(Q)
            return gQ, gK, gV, None, None

    class _FusedAttentionHeads(torch.autograd.Function):
        """_FusedAttention over `heads` heads of k / heads columns each, every head with its own softmax: flex_attention_heads in one
        launch, alpha [nnz, heads] kept only when a gradient is needed; backward: the one call flex_attention_heads_backward (two launches)
        for the gradients that are needed.  Only on an operator made with fused_attention=True and fused_backward=True."""

        @staticmethod
        def forward(ctx, Q, K, V, op, scale, heads):
            Q, K, V = Q.contiguous(), K.contiguous(), V.contiguous()
            p = torch.zeros((op.nnz, heads), dtype=torch.float32, device=Q.device) if any(ctx.needs_input_grad[:3]) else None
            out = op.plan.attention(Q, K, V, scale, p=p, heads=heads)
            ctx.op, ctx.scale, ctx.heads = op, scale, heads
            ctx.save_for_backward(Q, K, V, p)
            return out

        @staticmethod
        def backward(ctx, grad_out):
            Q, K, V, p = ctx.saved_tensors
            grads = ctx.op.plan.attention_backward(Q, K, V, p, grad_out.contiguous(), ctx.scale, want=tuple(ctx.needs_input_grad[:3]), heads=ctx.heads)
            return (*grads, None, None, None)

    class _FusedGatAttention(torch.autograd.Function):
        """Out = A(alpha) V per head, alpha = softmax over each row of A of leaky_relu(el[row, h] + er[col, h], slope): flex_gat_attention
        in one launch, alpha [nnz, heads] kept only when a gradient is needed; backward: the one call flex_gat_attention_backward (two
        launches) for the gradients that are needed, in el, er and V.  It sets no plan's values.  Only on an operator made with
        fused_attention=True and fused_backward=True."""

        @staticmethod
        def forward(ctx, el, er, V, op, slope):
            el, er, V = el.contiguous(), er.contiguous(), V.contiguous()
            p = torch.zeros((op.nnz, el.shape[1]), dtype=torch.float32, device=V.device) if any(ctx.needs_input_grad[:3]) else None
            out = op.plan.gat_attention(el, er, V, slope, p=p)
            ctx.op, ctx.slope = op, slope
            ctx.save_for_backward(el, er, V, p)
            return out

        @staticmethod
        def backward(ctx, grad_out):
            el, er, V, p = ctx.saved_tensors
            grads = ctx.op.plan.gat_attention_backward(el, er, V, p, grad_out.contiguous(), ctx.slope, want=tuple(ctx.needs_input_grad[:3]))
            return (*grads, None, None)

    class _FusedAttentionBf16(torch.autograd.Function):
        """_FusedAttentionHeads on torch.bfloat16 Q, K, V (heads = 1 included): flex_attention_bf16 in one launch, scores, softmax and sums
        in float32, alpha [nnz, heads] kept in float32 only when a gradient is needed; backward: the one call flex_attention_bf16_backward
        (two launches) for the gradients that are needed, which come back in bfloat16.  Only on an operator made with fused_attention=True
        and fused_backward=True."""

        @staticmethod
        def forward(ctx, Q, K, V, op, scale, heads):
            Q, K, V = Q.contiguous(), K.contiguous(), V.contiguous()
            p = torch.zeros((op.nnz, heads), dtype=torch.float32, device=Q.device) if any(ctx.needs_input_grad[:3]) else None
            out = op.plan.attention_bf16(Q, K, V, scale, heads=heads, p=p)
            ctx.op, ctx.scale, ctx.heads = op, scale, heads
            ctx.save_for_backward(Q, K, V, p)
            return out

        @staticmethod
        def backward(ctx, grad_out):
            Q, K, V, p = ctx.saved_tensors
            grads = ctx.op.plan.attention_bf16_backward(Q, K, V, p, grad_out.contiguous(), ctx.scale, heads=ctx.heads, want=tuple(ctx.needs_input_grad[:3]))
            return (*grads, None, None, None)

    class _FusedAttentionBias(torch.autograd.Function):
        """_FusedAttentionHeads / _FusedAttentionBf16 with bias [nnz, heads] (float32) added to the scaled score of every entry and head
        before the softmax, differentiable in Q, K, V and the bias: flex_attention_bias or flex_attention_bf16_bias (by the dtype of Q)
        in one launch, alpha [nnz, heads] kept only when a gradient is needed; backward: the one call of two launches for the gradients
        that are needed, which never reads the bias.  Only on an operator made with fused_attention=True and fused_backward=True."""

        @staticmethod
        def forward(ctx, Q, K, V, bias, op, scale, heads):
            Q, K, V, bias = Q.contiguous(), K.contiguous(), V.contiguous(), bias.detach().contiguous()
            p = torch.zeros((op.nnz, heads), dtype=torch.float32, device=Q.device) if any(ctx.needs_input_grad[:4]) else None
            run = op.plan.attention_bf16_bias if Q.dtype == torch.bfloat16 else op.plan.attention_bias
            out = run(Q, K, V, bias, scale, heads=heads, p=p)
            ctx.op, ctx.scale, ctx.heads, ctx.bias_shape = op, scale, heads, bias.shape
            ctx.save_for_backward(Q, K, V, p)
            return out

        @staticmethod
        def backward(ctx, grad_out):
            Q, K, V, p = ctx.saved_tensors
            run = ctx.op.plan.attention_bf16_bias_backward if Q.dtype == torch.bfloat16 else ctx.op.plan.attention_bias_backward
            gQ, gK, gV, gB = run(Q, K, V, p, grad_out.contiguous(), ctx.scale, heads=ctx.heads, want=tuple(ctx.needs_input_grad[:4]))
            return gQ, gK, gV, None if gB is None else gB.reshape(ctx.bias_shape), None, None, None

    return (_SpMM, _AxwLayer, _SpMMValues, _Sddmm, _EdgeSoftmax, _FusedAttention, _FusedAttentionHeads, _FusedGatAttention, _FusedAttentionBf16,
            _FusedAttentionBias)


_cache = None


def functions():
    """(_SpMM, _AxwLayer, _SpMMValues, _Sddmm, _EdgeSoftmax, _FusedAttention, _FusedAttentionHeads, _FusedGatAttention, _FusedAttentionBf16, _FusedAttentionBias): the autograd Functions, built at first use (torch is imported then)."""
    global _cache
    if _cache is None:
        _cache = _function()
    return _cache


def _dropout_function():
    import torch

    class _FusedAttentionDropout(torch.autograd.Function):
        """_FusedAttentionHeads / _FusedAttentionBf16 / _FusedAttentionBias with the probabilities dropped after the softmax (probability
        drop_p, the kept ones scaled by 1 / (1 - drop_p)): flex_attention_dropout or flex_attention_bf16_dropout (by the dtype of Q) in
        one launch, the UNDROPPED alpha [nnz, heads] kept only when a gradient is needed; backward: the one call of two launches under
        the same drop_p and seed, which recomputes the mask from the seed -- no mask is stored.  bias may be None.  Only on an operator
        made with fused_attention=True and fused_backward=True."""

        @staticmethod
        def forward(ctx, Q, K, V, bias, op, scale, heads, drop_p, seed):
            Q, K, V = Q.contiguous(), K.contiguous(), V.contiguous()
            b = None if bias is None else bias.detach().contiguous()
            p = torch.zeros((op.nnz, heads), dtype=torch.float32, device=Q.device) if any(ctx.needs_input_grad[:4]) else None
            run = op.plan.attention_bf16_dropout if Q.dtype == torch.bfloat16 else op.plan.attention_dropout
            out = run(Q, K, V, scale, drop_p, seed, heads=heads, bias=b, probs=p)
            ctx.op, ctx.scale, ctx.heads, ctx.drop_p, ctx.seed = op, scale, heads, drop_p, seed
            ctx.bias_shape = None if bias is None else bias.shape
            ctx.save_for_backward(Q, K, V, p)
            return out

        @staticmethod
        def backward(ctx, grad_out):
            Q, K, V, p = ctx.saved_tensors
            run = ctx.op.plan.attention_bf16_dropout_backward if Q.dtype == torch.bfloat16 else ctx.op.plan.attention_dropout_backward
            want = tuple(ctx.needs_input_grad[:3]) + (ctx.bias_shape is not None and ctx.needs_input_grad[3],)
            gQ, gK, gV, gB = run(Q, K, V, p, grad_out.contiguous(), ctx.scale, ctx.drop_p, ctx.seed, heads=ctx.heads, want=want)
            return gQ, gK, gV, None if gB is None else gB.reshape(ctx.bias_shape), None, None, None, None, None

    return (_FusedAttentionDropout,)


_dropout_cache = None


def dropout_functions():
    """(_FusedAttentionDropout,): the autograd Functions of the attention dropout, built at first use; functions() keeps its ten."""
    global _dropout_cache
    if _dropout_cache is None:
        _dropout_cache = _dropout_function()
    return _dropout_cache


def _gat_dropout_function():
    import torch

    class _FusedGatAttentionDropout(torch.autograd.Function):
        """_FusedGatAttention with the probabilities dropped after the softmax (probability drop_p, the kept ones scaled by
        1 / (1 - drop_p)): flex_gat_attention_dropout in one launch, the UNDROPPED alpha [nnz, heads] kept only when a gradient is
        needed; backward: the one call flex_gat_attention_dropout_backward (two launches) under the same drop_p and seed, which
        recomputes the mask from the seed -- no mask is stored.  Only on an operator made with fused_attention=True and
        fused_backward=True."""

        @staticmethod
        def forward(ctx, el, er, V, op, slope, drop_p, seed):
            el, er, V = el.contiguous(), er.contiguous(), V.contiguous()
            p = torch.zeros((op.nnz, el.shape[1]), dtype=torch.float32, device=V.device) if any(ctx.needs_input_grad[:3]) else None
            out = op.plan.gat_attention_dropout(el, er, V, slope, drop_p, seed, probs=p)
            ctx.op, ctx.slope, ctx.drop_p, ctx.seed = op, slope, drop_p, seed
            ctx.save_for_backward(el, er, V, p)
            return out

        @staticmethod
        def backward(ctx, grad_out):
            el, er, V, p = ctx.saved_tensors
            grads = ctx.op.plan.gat_attention_dropout_backward(el, er, V, p, grad_out.contiguous(), ctx.slope, ctx.drop_p, ctx.seed,
                                                               want=tuple(ctx.needs_input_grad[:3]))
            return (*grads, None, None, None, None)

    return (_FusedGatAttentionDropout,)


_gat_dropout_cache = None


def gat_dropout_functions():
    """(_FusedGatAttentionDropout,): the autograd Function of the GAT attention dropout, built at first use; functions() keeps its ten and
    dropout_functions() its one."""
    global _gat_dropout_cache
    if _gat_dropout_cache is None:
        _gat_dropout_cache = _gat_dropout_function()
    return _gat_dropout_cache


def _gat_edge_function():
    import torch

    class _FusedGatEdgeAttention(torch.autograd.Function):
        """_FusedGatAttention / _FusedGatAttentionDropout with a per-edge term ee [nnz, heads] inside the LeakyReLU:
        flex_edge_gat_attention in one launch (drop_p = 0: no mask), the UNDROPPED alpha kept only when a gradient is needed;
        backward: the one call flex_edge_gat_attention_backward (two launches) under the same drop_p and seed.  Keeps (el, er, ee, V, P)
        and the seed, never a mask; the gradient in ee is the call's work array, so nothing nnz-sized is allocated beside it.  Only on
        an operator made with fused_attention=True and fused_backward=True."""

        @staticmethod
        def forward(ctx, el, er, ee, V, op, slope, drop_p, seed):
            el, er, ee, V = el.contiguous(), er.contiguous(), ee.contiguous(), V.contiguous()
            p = torch.zeros((op.nnz, el.shape[1]), dtype=torch.float32, device=V.device) if any(ctx.needs_input_grad[:4]) else None
            out = op.plan.gat_edge_attention(el, er, ee, V, slope, drop_p, seed, probs=p)
            ctx.op, ctx.slope, ctx.drop_p, ctx.seed = op, slope, drop_p, seed
            ctx.save_for_backward(el, er, ee, V, p)
            return out

        @staticmethod
        def backward(ctx, grad_out):
            el, er, ee, V, p = ctx.saved_tensors
            grads = ctx.op.plan.gat_edge_attention_backward(el, er, ee, V, p, grad_out.contiguous(), ctx.slope, ctx.drop_p, ctx.seed,
                                                            want=tuple(ctx.needs_input_grad[:4]))
            return (*grads, None, None, None, None)

    return (_FusedGatEdgeAttention,)


_gat_edge_cache = None


def gat_edge_functions():
    """(_FusedGatEdgeAttention,): the autograd Function of the GAT attention with a per-edge score term, built at first use, as
    gat_dropout_functions(); functions(), gat_dropout_functions() and gat_bf16_functions() keep their counts."""
    global _gat_edge_cache
    if _gat_edge_cache is None:
        _gat_edge_cache = _gat_edge_function()
    return _gat_edge_cache


def _gatv2_function():
    import torch

    class _FusedGatv2Attention(torch.autograd.Function):
        """Out = A(alpha) xs per head, alpha = softmax over each row of A of <att[h], leaky_relu(xt[row] + xs[col], slope)> over the head's
        columns: flex_gatv2_attention in one launch, alpha [nnz, heads] kept only when a gradient is needed; backward: the one call
        flex_gatv2_attention_backward (up to three launches) for the gradients that are needed, in xt, xs and att.  xt may be xs: torch
        sums the two gradients.  It sets no plan's values.  Only on an operator made with fused_attention=True and fused_backward=True."""

        @staticmethod
        def forward(ctx, xt, xs, att, op, slope):
            xt, xs, att = xt.contiguous(), xs.contiguous(), att.contiguous()
            p = torch.zeros((op.nnz, att.shape[0]), dtype=torch.float32, device=xs.device) if any(ctx.needs_input_grad[:3]) else None
            out = op.plan.gatv2_attention(xt, xs, att, slope, p=p)
            ctx.op, ctx.slope = op, slope
            ctx.save_for_backward(xt, xs, att, p)
            return out

        @staticmethod
        def backward(ctx, grad_out):
            xt, xs, att, p = ctx.saved_tensors
            grads = ctx.op.plan.gatv2_attention_backward(xt, xs, att, p, grad_out.contiguous(), ctx.slope, want=tuple(ctx.needs_input_grad[:3]))
            return (*grads, None, None)

    return (_FusedGatv2Attention,)


_gatv2_cache = None


def gatv2_functions():
    """(_FusedGatv2Attention,): the autograd Function of the GATv2 attention, built at first use, as gat_dropout_functions()."""
    global _gatv2_cache
    if _gatv2_cache is None:
        _gatv2_cache = _gatv2_function()
    return _gatv2_cache


def _gatv2_dropout_function():
    import torch

    class _FusedGatv2AttentionDropout(torch.autograd.Function):
        """_FusedGatv2Attention with the probabilities dropped after the softmax (probability drop_p, the kept ones scaled by
        1 / (1 - drop_p)): flex_dropout_gatv2_attention in one launch, the UNDROPPED alpha [nnz, heads] kept only when a gradient is
        needed; backward: the one call flex_dropout_gatv2_attention_backward (up to three launches) under the same drop_p and seed, which
        recomputes the mask from the seed -- no mask is stored.  Only on an operator made with fused_attention=True and
        fused_backward=True."""

        @staticmethod
        def forward(ctx, xt, xs, att, op, slope, drop_p, seed):
            xt, xs, att = xt.contiguous(), xs.contiguous(), att.contiguous()
            p = torch.zeros((op.nnz, att.shape[0]), dtype=torch.float32, device=xs.device) if any(ctx.needs_input_grad[:3]) else None
            out = op.plan.gatv2_attention_dropout(xt, xs, att, slope, drop_p, seed, probs=p)
            ctx.op, ctx.slope, ctx.drop_p, ctx.seed = op, slope, drop_p, seed
            ctx.save_for_backward(xt, xs, att, p)
            return out

        @staticmethod
        def backward(ctx, grad_out):
            xt, xs, att, p = ctx.saved_tensors
            grads = ctx.op.plan.gatv2_attention_dropout_backward(xt, xs, att, p, grad_out.contiguous(), ctx.slope, ctx.drop_p, ctx.seed,
                                                                 want=tuple(ctx.needs_input_grad[:3]))
            return (*grads, None, None, None, None)

    return (_FusedGatv2AttentionDropout,)


_gatv2_dropout_cache = None


def gatv2_dropout_functions():
    """(_FusedGatv2AttentionDropout,): the autograd Function of the GATv2 attention dropout, built at first use; gatv2_functions() keeps
    its one."""
    global _gatv2_dropout_cache
    if _gatv2_dropout_cache is None:
        _gatv2_dropout_cache = _gatv2_dropout_function()
    return _gatv2_dropout_cache


def _gat_bf16_function():
    import torch

    class _FusedGatAttentionBf16(torch.autograd.Function):
        """_FusedGatAttention on torch.bfloat16 V (el and er float32): flex_gat_attention_bf16 in one launch, scores, softmax and sums in
        float32, alpha [nnz, heads] kept in float32 only when a gradient is needed; backward: the one call
        flex_gat_attention_bf16_backward (two launches) for the gradients that are needed -- grad V in bfloat16, grad el and grad er in
        float32.  Only on an operator made with fused_attention=True and fused_backward=True."""

        @staticmethod
        def forward(ctx, el, er, V, op, slope):
            el, er, V = el.contiguous(), er.contiguous(), V.contiguous()
            p = torch.zeros((op.nnz, el.shape[1]), dtype=torch.float32, device=V.device) if any(ctx.needs_input_grad[:3]) else None
            out = op.plan.gat_attention_bf16(el, er, V, slope, p=p)
            ctx.op, ctx.slope = op, slope
            ctx.save_for_backward(el, er, V, p)
            return out

        @staticmethod
        def backward(ctx, grad_out):
            el, er, V, p = ctx.saved_tensors
            grads = ctx.op.plan.gat_attention_bf16_backward(el, er, V, p, grad_out.contiguous(), ctx.slope, want=tuple(ctx.needs_input_grad[:3]))
            return (*grads, None, None)

    class _FusedGatAttentionBf16Dropout(torch.autograd.Function):
        """_FusedGatAttentionBf16 with the probabilities dropped after the softmax: flex_gat_attention_bf16_dropout and its backward under
        the same drop_p and seed, which recomputes the mask from the seed -- no mask is stored."""

        @staticmethod
        def forward(ctx, el, er, V, op, slope, drop_p, seed):
            el, er, V = el.contiguous(), er.contiguous(), V.contiguous()
            p = torch.zeros((op.nnz, el.shape[1]), dtype=torch.float32, device=V.device) if any(ctx.needs_input_grad[:3]) else None
            out = op.plan.gat_attention_bf16_dropout(el, er, V, slope, drop_p, seed, probs=p)
            ctx.op, ctx.slope, ctx.drop_p, ctx.seed = op, slope, drop_p, seed
            ctx.save_for_backward(el, er, V, p)
            return out

        @staticmethod
        def backward(ctx, grad_out):
            el, er, V, p = ctx.saved_tensors
            grads = ctx.op.plan.gat_attention_bf16_dropout_backward(el, er, V, p, grad_out.contiguous(), ctx.slope, ctx.drop_p, ctx.seed,
                                                                    want=tuple(ctx.needs_input_grad[:3]))
            return (*grads, None, None, None, None)

    return (_FusedGatAttentionBf16, _FusedGatAttentionBf16Dropout)


_gat_bf16_cache = None


def gat_bf16_functions():
    """(_FusedGatAttentionBf16, _FusedGatAttentionBf16Dropout): the autograd Functions of the GAT attention on bfloat16 V, built at first
    use; functions() keeps its ten, dropout_functions() and gat_dropout_functions() their one each."""
    global _gat_bf16_cache
    if _gat_bf16_cache is None:
        _gat_bf16_cache = _gat_bf16_function()
    return _gat_bf16_cache


class SparseOperator:
    """C = A B for a fixed sparse pattern A, differentiable in B: grad_B = A^T grad_C.  Keeps the plan of A (k columns) and the plan of A^T.
    `a` is an m x n HostCsr; op(B) takes B [n, k] and returns C [m, k], float32 cuda tensors.
    learn_values=True: both plans are made with FLEX_PLAN_MUTABLE_VALUES and op(B, values=v) -- v a float32 cuda tensor of a.nnz values
    in a's CSR order -- computes A(v) B, differentiable in B and in v (grad_v = SDDMM(grad_C, B) over A's pattern).  op(B) alone then
    uses a's own values.  With learn_values the operator also offers the pieces of graph attention over A's pattern, each differentiable:
    op.sddmm(Q, K) (scores per entry, Q [m, k], K [n, k]), op.edge_softmax(s, scale) (softmax over each row of A) and
    op.attention(Q, K, V, scale) = op(V, values=op.edge_softmax(op.sddmm(Q, K), scale)).
    fused_attention=True (with learn_values=True): the forward plan is also made with FLEX_PLAN_ATTENTION and op.attention runs its
    forward as one launch (flex_attention); the backward is the same chain of calls.
    fused_backward=True (with fused_attention=True): the forward plan is also made with FLEX_PLAN_ATTENTION_BACKWARD and the backward of
    op.attention is one call of two launches (flex_attention_backward) that sets no plan's values.  Off by default.
    With both fused flags the operator also offers op.gat_attention(el, er, V, negative_slope): GAT's additive attention, H = el.shape[1]
    heads in one forward launch and two backward launches (flex_gat_attention), differentiable in el [m, H], er [n, H] and V [n, k];
    dropout= drops its probabilities after the softmax in the same launches (flex_gat_attention_dropout); a torch.bfloat16 V takes the
    bf16 kernels (flex_gat_attention_bf16, flex_gat_attention_bf16_dropout), Out and grad V in bfloat16.
    bf16=True: both plans are made with FLEX_PLAN_BF16 (k a multiple of 8): op(B) takes and returns torch.bfloat16 (float32 raises
    TypeError, as bfloat16 does on an fp32 operator), sums in float32, and backpropagates A^T grad_C in bfloat16 through flex_spmm_bf16 on
    the transposed plan.  The plain product only: NotImplementedError with learn_values, the fused flags or values=."""

    def __init__(self, a: binding.HostCsr, k: int, device: int = 0, order: int = binding.FLEX_ORDER_NATURAL, tuning: dict | None = None,
                 learn_values: bool = False, fused_attention: bool = False, fused_backward: bool = False, bf16: bool = False):
        if bf16 and (learn_values or fused_attention or fused_backward):
            raise NotImplementedError("SparseOperator(..., bf16=True) is the plain product only: learnable values and the attention calls read "
                                      "fp32 plans (op.attention takes bfloat16 Q, K, V on an fp32 operator with both fused flags)")
        if fused_attention and not learn_values:
            raise NotImplementedError("fused_attention needs SparseOperator(..., learn_values=True): its backward sets the plans' values")
        if fused_backward and not fused_attention:
            raise NotImplementedError("fused_backward needs SparseOperator(..., fused_attention=True): it starts from the probabilities flex_attention keeps")
        self.m, self.n, self.k, self.nnz = a.m, a.n, k, a.nnz
        self.learn_values = learn_values
        self.fused_attention = fused_attention
        self.fused_backward = fused_backward
        self.bf16 = bf16
        self.plan = binding.Plan(a, k, device=device, order=order, tuning=tuning, mutable_values=learn_values, attention=fused_attention,
                                 attention_backward=fused_backward, bf16=bf16)
        self.plan_t = binding.Plan(a, k, device=device, order=order, tuning=tuning, transpose=True, mutable_values=learn_values, bf16=bf16)
        self._v0 = None
        if learn_values:
            import torch
            self._v0 = torch.from_numpy(a.vals.copy()).to(f"cuda:{device}")

    def forward_plan(self, B):
        return self.plan(B)

    def transposed_plan(self, G):
        return self.plan_t(G)

    def __call__(self, B, values=None):
        """values: A's values for this product (learn_values=True only; without it they are constants of the plan and passing them
        raises).  Differentiable in B and in values."""
        if not self.learn_values:
            if values is not None:
                raise NotImplementedError("gradients for A's values (SDDMM) need SparseOperator(..., learn_values=True)")
            return functions()[0].apply(B, self)
        if values is None:
            values = self._v0
        assert values.numel() == self.nnz, (values.numel(), self.nnz)
        return functions()[2].apply(B, values, self)


    def _needs_learn_values(self, what):
        if not self.learn_values:
            raise NotImplementedError(f"{what} needs SparseOperator(..., learn_values=True)")

    def sddmm(self, Q, K):
        """s [nnz] in a's CSR order: s[e] = <Q[row(e)], K[col(e)]>.  Differentiable in Q [m, k] and K [n, k]."""
        self._needs_learn_values("sddmm")
        return functions()[3].apply(Q, K, self)

    def edge_softmax(self, s, scale: float = 1.0):
        """The softmax of scale * s over each row of A (-inf = a masked edge).  Differentiable in s."""
        self._needs_learn_values("edge_softmax")
        assert s.numel() == self.nnz, (s.numel(), self.nnz)
        return functions()[4].apply(s, self, float(scale))

    def attention(self, Q, K, V, scale: float | None = None, heads: int = 1, bias=None, dropout: float = 0.0, seed: int | None = None,
                  training: bool = True):
        """Out [m, k] = A(alpha) V with alpha = softmax over each row of A of scale * <Q[row], K[col]>; scale defaults to
        (k / heads) ** -0.5.  Differentiable in Q [m, k], K [n, k] and V [n, k].  heads > 1: head h is columns [h k / heads, (h + 1) k / heads)
        of Q, K, V and Out and has its own scores and softmax, all heads in one forward launch and two backward launches
        (flex_attention_heads); needs fused_attention=True and fused_backward=True.  Q, K and V all torch.bfloat16, for any heads: the same
        three launches on bf16 rows with float32 scores, softmax and sums (flex_attention_bf16); Out and the gradients are bfloat16; needs
        both fused flags as well, and k / heads a power of two in 4 .. 256.  Mixed dtypes raise TypeError.
        bias (float32 [nnz, heads] in a's CSR order; [nnz] with heads == 1): alpha = softmax of scale * <Q[row], K[col]> + bias[e, h], the
        edge term of a graph transformer, -inf masking an entry for a head; differentiable in the bias as well, in the same three launches
        (flex_attention_bias, flex_attention_bf16_bias) for Q, K, V all float32 or all bfloat16; needs both fused flags and, for any
        heads, k / heads a power of two in 4 .. 256.  bias=None takes every path above exactly as without the argument.
        dropout (0 <= dropout < 1) with training=True: the probabilities are dropped after the softmax with that probability and the
        kept ones scaled by 1 / (1 - dropout), with or without a bias, in the same three launches (flex_attention_dropout,
        flex_attention_bf16_dropout): the mask is a hash of (seed, entry, head) that the backward recomputes, so nothing nnz-sized is added.
        seed=None draws 63 bits from torch's default generator (torch.manual_seed reproduces a run); the seed is kept for the backward.
        Needs both fused flags and k / heads a power of two in 4 .. 256.  dropout=0.0 or training=False takes every path above exactly as
        without the arguments."""
        import torch
        self._needs_learn_values("attention")
        if heads < 1:
            raise ValueError(f"heads must be at least 1, not {heads}")
        if scale is None:
            scale = (self.k / heads) ** -0.5
        dtypes = {t.dtype for t in (Q, K, V)}
        if not 0.0 <= dropout < 1.0:  # a NaN fails this too
            raise ValueError(f"dropout must be a probability in [0, 1), not {dropout}")
        if dropout > 0 and training:
            if not (self.fused_attention and self.fused_backward):
                raise NotImplementedError("attention(..., dropout=...) needs SparseOperator(..., fused_attention=True, fused_backward=True): "
                                          "only the fused forward and backward drop attention probabilities")
            if dtypes not in ({torch.float32}, {torch.bfloat16}):
                raise TypeError(f"attention takes Q, K and V of one dtype, all float32 or all bfloat16, not {[str(t.dtype) for t in (Q, K, V)]}")
            if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) not in ((self.nnz, heads),) + (((self.nnz,),) if heads == 1 else ())):
                raise TypeError(f"attention takes a float32 bias of shape [nnz, heads] = [{self.nnz}, {heads}], not {bias.dtype} {tuple(bias.shape)}")
            if seed is None:
                seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
            return dropout_functions()[0].apply(Q, K, V, bias, self, float(scale), int(heads), float(dropout), int(seed) & 0xFFFFFFFFFFFFFFFF)
        if bias is not None:
            if not (self.fused_attention and self.fused_backward):
                raise NotImplementedError("attention(..., bias=...) needs SparseOperator(..., fused_attention=True, fused_backward=True): "
                                          "only the fused forward and backward take a per-edge bias")
            if dtypes not in ({torch.float32}, {torch.bfloat16}):
                raise TypeError(f"attention takes Q, K and V of one dtype, all float32 or all bfloat16, not {[str(t.dtype) for t in (Q, K, V)]}")
            if bias.dtype != torch.float32 or tuple(bias.shape) not in ((self.nnz, heads),) + (((self.nnz,),) if heads == 1 else ()):
                raise TypeError(f"attention takes a float32 bias of shape [nnz, heads] = [{self.nnz}, {heads}], not {bias.dtype} {tuple(bias.shape)}")
            return functions()[9].apply(Q, K, V, bias, self, float(scale), int(heads))
        if torch.bfloat16 in dtypes:
            if len(dtypes) > 1:
                raise TypeError(f"attention takes Q, K and V of one dtype, all float32 or all bfloat16, not {[str(t.dtype) for t in (Q, K, V)]}")
            if not (self.fused_attention and self.fused_backward):
                raise NotImplementedError("attention(...) on bfloat16 needs SparseOperator(..., fused_attention=True, fused_backward=True): "
                                          "only the fused forward and backward read bf16 rows")
            return functions()[8].apply(Q, K, V, self, float(scale), int(heads))
        if heads > 1:
            if not (self.fused_attention and self.fused_backward):
                raise NotImplementedError("attention(..., heads > 1) needs SparseOperator(..., fused_attention=True, fused_backward=True): "
                                          "only the fused forward and backward run several heads in one launch")
            return functions()[6].apply(Q, K, V, self, float(scale), int(heads))
        if self.fused_attention:
            return functions()[5].apply(Q, K, V, self, float(scale))
        return self(V, values=self.edge_softmax(self.sddmm(Q, K), scale))

    def gat_attention(self, el, er, V, negative_slope: float = 0.2, dropout: float = 0.0, seed: int | None = None, training: bool = True,
                      edge=None):
        """Out [m, k] = A(alpha) V per head with alpha = softmax over each row of A of leaky_relu(el[row, h] + er[col, h], negative_slope):
        the attention of a GAT layer, el = <h W, a_l> and er = <h W, a_r> being one scalar per node and head.  H = el.shape[1] heads; head h
        is columns [h k / H, (h + 1) k / H) of V and Out.  Differentiable in el [m, H], er [n, H] and V [n, k]; all heads in one forward
        launch and two backward launches (flex_gat_attention); needs fused_attention=True and fused_backward=True.
        dropout (0 <= dropout < 1) with training=True: the probabilities are dropped after the softmax with that probability and the
        kept ones scaled by 1 / (1 - dropout), in the same three launches (flex_gat_attention_dropout): the mask is a hash of (seed,
        entry, head) that the backward recomputes, so nothing nnz-sized is added.  seed=None draws 63 bits from torch's default
        generator (torch.manual_seed reproduces a run); the seed is kept for the backward.  dropout=0.0 or training=False takes the path
        above exactly as without the arguments.
        A torch.bfloat16 V takes the bf16 kernels (flex_gat_attention_bf16, flex_gat_attention_bf16_dropout): V rows are gathered as
        bfloat16, every sum is float32, Out and grad V come back in bfloat16, rounded once.  el and er are then float32 or bfloat16;
        bfloat16 ones are widened before the call (the scores stay float32) and their gradients come back in bfloat16.  Any other mix
        of dtypes is a TypeError.
        edge (a float32 [nnz, H] tensor in a's CSR order, differentiable): a per-edge, per-head term inside the LeakyReLU, the score
        leaky_relu((el[row, h] + er[col, h]) + edge[e, h]) of a GAT layer with edge features (edge = <lin_edge(edge_attr), att_edge>),
        in the same launches (flex_edge_gat_attention); -inf masks one entry for one head.  dropout, seed and training work as without
        it.  float32 V only: anything else, and any other dtype or shape of edge, is a TypeError.  edge=None takes the paths above."""
        if not 0.0 <= dropout < 1.0:  # a NaN fails this too
            raise ValueError(f"dropout must be a probability in [0, 1), not {dropout}")
        if not (self.fused_attention and self.fused_backward):
            raise NotImplementedError("gat_attention needs SparseOperator(..., learn_values=True, fused_attention=True, fused_backward=True): "
                                      "only the fused forward and backward compute the additive score")
        import torch
        if edge is not None:
            if not (el.dtype == er.dtype == V.dtype == torch.float32):
                raise TypeError(f"gat_attention with edge takes float32 el, er and V, not {el.dtype}, {er.dtype} and {V.dtype}")
            if not isinstance(edge, torch.Tensor) or edge.dtype != torch.float32 or tuple(edge.shape) != (self.nnz, el.shape[1]):
                raise TypeError(f"gat_attention takes a float32 edge of shape [nnz, heads] = [{self.nnz}, {el.shape[1]}], not "
                                f"{getattr(edge, 'dtype', type(edge))} {tuple(getattr(edge, 'shape', ()))}")
            drop = float(dropout) if training else 0.0
            if drop > 0 and seed is None:
                seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
            return gat_edge_functions()[0].apply(el, er, edge, V, self, float(negative_slope), drop, int(seed or 0) & 0xFFFFFFFFFFFFFFFF)
        bf16 = V.dtype == torch.bfloat16
        if bf16:
            if any(t.dtype not in (torch.float32, torch.bfloat16) for t in (el, er)):
                raise TypeError(f"gat_attention on bfloat16 V takes el and er in float32 or bfloat16, not {el.dtype} and {er.dtype}")
            el, er = el.float(), er.float()  # outside the Function: torch carries a bfloat16 leaf's gradient back to bfloat16
        elif not (el.dtype == er.dtype == V.dtype == torch.float32):
            raise TypeError(f"gat_attention takes float32 el, er and V, or bfloat16 V with float32 or bfloat16 el and er, not {el.dtype}, {er.dtype} and {V.dtype}")
        if dropout > 0 and training:
            if seed is None:
                seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
            fn = gat_bf16_functions()[1] if bf16 else gat_dropout_functions()[0]
            return fn.apply(el, er, V, self, float(negative_slope), float(dropout), int(seed) & 0xFFFFFFFFFFFFFFFF)
        return (gat_bf16_functions()[0] if bf16 else functions()[7]).apply(el, er, V, self, float(negative_slope))

    def gatv2_attention(self, xt, xs, att, negative_slope: float = 0.2, dropout: float = 0.0, seed: int | None = None, training: bool = True):
        """Out [m, k] = A(alpha) xs per head with alpha = softmax over each row of A of <att[h], leaky_relu(xt[row] + xs[col],
        negative_slope)> over the head's columns: the attention of a GATv2 layer (PyG's and DGL's GATv2Conv), xt = h W_t and xs = h W_s
        being the transformed features and the source row score operand and value alike.  H = att.shape[0] heads; head h is columns
        [h k / H, (h + 1) k / H) of xt, xs and Out.  Differentiable in xt [m, k], xs [n, k] and att [H, k / H]; all heads in one forward
        launch and up to three backward launches (flex_gatv2_attention); needs fused_attention=True and fused_backward=True.  xt may be
        xs (share_weights): autograd sums the two gradients.  float32 only: any other dtype is a TypeError.
        dropout (0 <= dropout < 1) with training=True: the probabilities are dropped after the softmax with that probability and the
        kept ones scaled by 1 / (1 - dropout), in the same launches (flex_dropout_gatv2_attention); a dropped entry stays in the
        softmax.  The mask is a hash of (seed, entry, head) that the backward recomputes, so nothing nnz-sized is added.  seed=None
        draws 63 bits from torch's default generator (torch.manual_seed reproduces a run); the seed is kept for the backward.
        dropout=0.0 or training=False takes the path above exactly as without the arguments."""
        if not 0.0 <= dropout < 1.0:  # a NaN fails this too
            raise ValueError(f"dropout must be a probability in [0, 1), not {dropout}")
        if not (self.fused_attention and self.fused_backward):
            raise NotImplementedError("gatv2_attention needs SparseOperator(..., learn_values=True, fused_attention=True, fused_backward=True): "
                                      "only the fused forward and backward compute the score from the full rows")
        import torch
        if not (xt.dtype == xs.dtype == att.dtype == torch.float32):
            raise TypeError(f"gatv2_attention takes float32 xt, xs and att, not {xt.dtype}, {xs.dtype} and {att.dtype}")
        if dropout > 0 and training:
            if seed is None:
                seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
            return gatv2_dropout_functions()[0].apply(xt, xs, att, self, float(negative_slope), float(dropout), int(seed) & 0xFFFFFFFFFFFFFFFF)
        return gatv2_functions()[0].apply(xt, xs, att, self, float(negative_slope))

#!/usr/bin/env python3
"""Sparse graph attention, measured: the error of the exponential the edge softmax may use, and the time of flex_edge_softmax,
flex_edge_softmax_backward and a whole attention step.  Writes profiles/attention_probe.txt (or the file given with --out): the whole run
starts the file, a run of one part (--fused, --backward, --heads, --gat, --bf16, --bias, --dropout, --gat-dropout, --gat-bf16, --gatv2,
--gatv2-dropout, --gat-edge)
appends to it.

1. tools/exp_error.hip (built here with hipcc into flex_amd/lib if it is not there): the largest error in ulp of expf, __expf and
   exp2f on the prescaled argument over every fp32 argument in [-104, 0] against float64 exp.
2. Per graph (natural order, HIP events on torch's stream, warm-up, best of 3): forward and backward, their bytes per second at
   8 / 12 bytes per entry as a share of flex_hbm_probe's copy rate in the same run, flex_plan_set_values on the same plan, and the
   torch composition of the same op (scatter_reduce amax + index_add + two gathers over an int64 row index).
3. One attention step (forward + backward of SparseOperator.attention, k = 32 and 128) against the same step with the softmax done by
   that torch composition.
4. The fused forward (flex_attention, FLEX_PLAN_ATTENTION) with and without dP against the four-call forward (flex_sddmm,
   flex_edge_softmax, flex_plan_set_values, flex_spmm) on the same operator, k = 32 and 128: one process, the two alternating round by
   round, best of 3 rounds after warm-up and the spread over the rounds; the image's bytes per nonzero and the step's extra memory.
   --fused: only this part (and the copy rate).
5. The fused backward (flex_attention_backward, FLEX_PLAN_ATTENTION_BACKWARD), same graphs, k and protocol: the backward alone -- the
   chain of eight engine calls on the same operator against the one call, from the same kept alpha -- and the whole step (forward +
   backward through autograd) of fused_attention=True against fused_attention=True, fused_backward=True; the second part of the image
   in bytes per nonzero.  --backward: only this part (and the copy rate).
6. Several heads (flex_attention_heads, flex_attention_heads_backward), (k, H) = (64, 4), (128, 4), (128, 8), same graphs and protocol:
   the one-launch forward (with dP), the two-launch backward and the autograd step of attention(..., heads=H) against the loop a user
   had before -- H single-head calls on offset pointers of a strided plan (k = d, ldb = ldc = H d); for the step, H single-head
   attention calls of an operator of width d on column slices and a concatenation.  --heads: only this part (and the copy rate).
7. GAT's additive attention (flex_gat_attention, flex_gat_attention_backward), (k, H) = (64, 8), (128, 4), (256, 8), same graphs and
   protocol: the one-launch forward (with dP), the two-launch backward and the autograd step of gat_attention against what a user had
   before -- per head, torch index arithmetic for the scores on a row / col copy of the pattern, edge_softmax and the SpMM with
   values=alpha of an operator of width d on a column slice, torch autograd carrying the gradients of el and er.  --gat: only this
   part (and the copy rate).
8. bf16 row operands (flex_attention_bf16, flex_attention_bf16_backward), (k, H) = (64, 8), (128, 4), (256, 8), same graphs and protocol:
   the forward (with dP), the backward and the autograd step of attention(..., heads=H) on bfloat16 tensors against the same three on
   float32 tensors (flex_attention_heads, flex_attention_heads_backward) on the same operator, in the same process.  --bf16: only this
   part (and the copy rate).
9. A per-edge bias (flex_attention_bias, flex_attention_bf16_bias and their backward calls), (k, H) = (64, 8), (128, 4), (256, 8), same
   graphs and protocol: the forward (with dP), the backward (with gBias) and the autograd step of attention(..., heads=H, bias=b) in fp32
   and in bf16 against the unbiased flex_attention_heads / flex_attention_bf16 and their backward calls on the same operator in the same
   process -- what the bias costs: nnz x H floats read forward, nnz x H written backward -- and, at k = 64 with one head, against what a
   user needed before: flex_sddmm, a torch add, flex_edge_softmax and the SpMM with values=alpha, with their autograd.  --bias: only
   this part (and the copy rate).
10. Attention dropout (flex_attention_dropout, flex_attention_bf16_dropout and their backward calls), (k, H) = (64, 8), (128, 4), (256, 8),
   p = 0.1 and 0.6, same graphs and protocol: the forward (with dP) and the backward in fp32 and in bf16 against the undropped
   flex_attention_heads / flex_attention_bf16 and their backward calls on the same plan in the same process -- what the mask costs (four
   32-bit multiplies per entry and head in each of the three launches) and what the V and g rows that are not gathered behind dropped
   entries save.  --dropout: only this part (and the copy rate).
11. Attention dropout in GAT (flex_gat_attention_dropout and its backward call), (k, H) = (64, 8), (128, 4), (256, 8), p = 0.1 and 0.6,
   same graphs and protocol: the forward (with dP) and the backward against the undropped flex_gat_attention and
   flex_gat_attention_backward on the same plan in the same process.  --gat-dropout: only this part (and the copy rate).
12. GAT on bf16 V rows (flex_gat_attention_bf16, flex_gat_attention_bf16_dropout and their backward calls), (k, H) = (64, 8), (128, 4),
   (256, 8), without dropout and with p = 0.6, same graphs and protocol: the forward (with dP), the two-launch backward and the autograd
   step of gat_attention on bfloat16 V against the same three on float32 V (flex_gat_attention, flex_gat_attention_dropout) on the same
   operator, in the same process.  --gat-bf16: only this part (and the copy rate).
13. GATv2 (flex_gatv2_attention, flex_gatv2_attention_backward), (k, H) = (64, 8), (128, 4), (256, 8), same graphs and protocol: the
   one-launch forward (with dP), the backward (all three gradients: three launches) and the autograd step of gatv2_attention against
   what a user had before -- the [nnz, k] tensor Xt[row] + Xs[col] and the scores in torch, then per head edge_softmax and the SpMM
   with values=alpha of an operator of width d on a column slice, torch autograd carrying the gradients.  --gatv2: only this part
   (and the copy rate).
14. Attention dropout in GATv2 (flex_dropout_gatv2_attention and its backward call), (k, H) = (64, 8), (128, 4), (256, 8), p = 0.1 and
   0.6, same graphs and protocol: the forward (with dP) and the backward (all three gradients) against the undropped
   flex_gatv2_attention and flex_gatv2_attention_backward on the same plan in the same process -- what the mask costs where every Xs
   row is gathered all the same.  --gatv2-dropout: only this part (and the copy rate).
15. A per-edge term in GAT's score (flex_edge_gat_attention and its backward call: edge features), (k, H) = (64, 8), (128, 4), (256, 8),
   same graphs and protocol: the forward (with dP), the backward (all four gradients, gEe being the work array) and the autograd step
   of gat_attention(..., edge=e) against (a) what a user had before -- per head, torch index arithmetic for the scores with ee,
   edge_softmax and the SpMM with values=alpha of an operator of width d on a column slice, torch autograd carrying the gradients of
   el, er and ee -- and (b) the edge-less flex_gat_attention and flex_gat_attention_backward on the same operator: the difference from
   (b) is what the ee stream costs (nnz x H floats read in the forward and again in the row backward).  --gat-edge: only this part (and
   the copy rate).
Usage: probe_attention.py [--out FILE] [--fused | --backward | --heads | --gat | --bf16 | --bias | --dropout | --gat-dropout | --gat-bf16 | --gatv2 | --gatv2-dropout | --gat-edge] [graph ...]   (default: pubmed.csv flickr reddit soc-sign-epinions)"""
import ctypes as C
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flex_amd  # noqa: E402
from tools.probe_values import best_us, load  # noqa: E402

LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def exp_error():
    so = os.path.join(ROOT, "flex_amd", "lib", "libexp_error.so")
    src = os.path.join(ROOT, "tools", "exp_error.hip")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++20", "-fPIC", "-shared", "-o", so, src])
    worst = (C.c_double * 3)()
    rc = C.CDLL(so).exp_error_ulp(worst)
    assert rc == 0, rc
    say("largest error in ulp over every fp32 argument in [-104, 0] (1 120 927 745 values) against float64 exp: "
        f"expf {worst[0]:.3f}  __expf {worst[1]:.3f}  exp2f(x * log2 e) {worst[2]:.3f}")


def torch_softmax(s, rows, m, scale):
    """The composition a user needs without the engine: row maximum, exponentials, row sums, two gathers."""
    mx = torch.full((m,), float("-inf"), device=s.device).scatter_reduce(0, rows, s, "amax")
    t = torch.exp(scale * (s - mx[rows]))
    return t / torch.zeros(m, device=s.device).index_add(0, rows, t)[rows]


def torch_softmax_backward(p, g, rows, m, scale):
    return scale * p * (g - torch.zeros(m, device=p.device).index_add(0, rows, p * g)[rows])


def probe(name, a, copy_gbps):
    p = flex_amd.Plan(a, 32, mutable_values=True)
    i = p.softmax_info()
    gen = torch.Generator(device="cuda").manual_seed(1)
    s = torch.rand(a.nnz, device="cuda", generator=gen) * 8 - 4
    g = torch.rand(a.nnz, device="cuda", generator=gen) * 2 - 1
    out, gs = torch.empty_like(s), torch.empty_like(s)
    st = torch.cuda.current_stream().cuda_stream
    n = max(5, min(200, int(1e9 / max(1, a.nnz))))
    t_f = best_us(lambda: p.edge_softmax_ptr(s.data_ptr(), 0.125, out.data_ptr(), st), n)
    t_b = best_us(lambda: p.edge_softmax_backward_ptr(out.data_ptr(), g.data_ptr(), 0.125, gs.data_ptr(), st), n)
    t_set = best_us(lambda: p.set_values(out), n)
    rows = torch.repeat_interleave(torch.arange(a.m, device="cuda"), torch.from_numpy(a.rowPtr.astype("int64")).diff().cuda())
    t_tf = best_us(lambda: torch_softmax(s, rows, a.m, 0.125), max(3, n // 4))
    t_tb = best_us(lambda: torch_softmax_backward(out, g, rows, a.m, 0.125), max(3, n // 4))
    diff = (torch_softmax(s, rows, a.m, 0.125) - out).abs().max().item()
    rec = p.info()["n_records"]
    share = lambda b, t: f"{b / t / 1e3:.0f} GB/s, {100 * b / t / 1e3 / copy_gbps:.0f} % of copy"  # noqa: E731
    say(f"{name} m={a.m} nnz={a.nnz} (rows packed {i['rows_packed']} wave {i['rows_wave']} block {i['rows_block']}, {i['items']} items, {i['groups']} groups of <= {i['group_entries']}, "
        f"{i['device_bytes'] / max(1, a.nnz):.2f} B/nnz): forward {t_f:.1f} us ({share(8 * a.nnz, t_f)})  backward {t_b:.1f} us ({share(12 * a.nnz, t_b)})"
        f"  set_values {t_set:.1f} us ({share(rec * 16 + a.nnz * 4, t_set)})  torch forward {t_tf:.1f} us ({t_tf / t_f:.1f}x) backward {t_tb:.1f} us ({t_tb / t_b:.1f}x)"
        f"  max |torch - engine| {diff:.2g}")
    del p
    for k in (32, 128):
        op = flex_amd.SparseOperator(a, k, learn_values=True)
        Q, K, V = (torch.rand((r, k), device="cuda", generator=gen).requires_grad_() for r in (a.m, a.n, a.n))
        gO = torch.rand((a.m, k), device="cuda", generator=gen)
        scale = k ** -0.5

        def step(softmax):
            for x in (Q, K, V):
                x.grad = None
            op(V, values=softmax(op.sddmm(Q, K))).backward(gO)

        nn = max(3, min(50, int(2e8 / max(1, a.nnz * k))))
        t_eng = best_us(lambda: step(lambda sc: op.edge_softmax(sc, scale)), nn)
        t_tor = best_us(lambda: step(lambda sc: torch_softmax(sc, rows, a.m, scale)), nn)
        say(f"{name} k={k}: attention step (forward + backward) {t_eng:.1f} us, with torch's softmax {t_tor:.1f} us ({t_tor / t_eng:.2f}x)")
        del op


def probe_fused(name, a):
    gen = torch.Generator(device="cuda").manual_seed(2)
    for k in (32, 128):
        op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True)
        plan = op.plan
        i = plan.attention_info()
        Q, K, V = (torch.rand((r, k), device="cuda", generator=gen) * 2 - 1 for r in (a.m, a.n, a.n))
        scale = k ** -0.5
        out, s, alpha = torch.empty((a.m, k), device="cuda"), torch.empty(a.nnz, device="cuda"), torch.empty(a.nnz, device="cuda")

        def four_calls():
            plan.sddmm(Q, K, out=s)
            plan.edge_softmax(s, scale, out=alpha)
            plan.set_values(alpha)
            plan(V, out=out)

        fns = {"four calls": four_calls, "fused": lambda: plan.attention(Q, K, V, scale, out=out),
               "fused + dP": lambda: plan.attention(Q, K, V, scale, out=out, p=alpha)}
        n = max(3, min(100, int(2e8 / max(1, a.nnz * k))))
        rounds = {key: [] for key in fns}
        for _ in range(3):  # alternating: every round times each of the three once
            for key, fn in fns.items():
                rounds[key].append(best_us(fn, n, rounds=1))
        best = {key: min(v) for key, v in rounds.items()}
        spread = {key: 100 * (max(v) - min(v)) / min(v) for key, v in rounds.items()}
        say(f"{name} k={k} forward (slot {i['rows_slot']} wave {i['rows_wave']} block {i['rows_block']} empty {i['rows_empty']} rows, {i['items']} items, "
            f"{i['groups']} groups of cost <= {i['group_budget']}, image {i['device_bytes'] / max(1, a.nnz):.2f} B/nnz): "
            + "  ".join(f"{key} {best[key]:.1f} us (+{spread[key]:.0f} % over 3 rounds)" for key in fns)
            + f"  four calls / fused {best['four calls'] / best['fused']:.2f}x, / fused + dP {best['four calls'] / best['fused + dP']:.2f}x"
            + f"  extra memory of a step: four calls {8 * a.nnz / 2 ** 20:.1f} MiB (s, alpha), fused + dP {4 * a.nnz / 2 ** 20:.1f} MiB, fused 0")
        del op, plan


def probe_backward(name, a):
    gen = torch.Generator(device="cuda").manual_seed(3)
    for k in (32, 128):
        chain = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True)
        fused = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
        i = fused.plan.attention_backward_info()
        Q, K, V = (torch.rand((r, k), device="cuda", generator=gen) * 2 - 1 for r in (a.m, a.n, a.n))
        g = torch.rand((a.m, k), device="cuda", generator=gen) * 2 - 1
        scale = k ** -0.5
        alpha = torch.empty(a.nnz, device="cuda")
        fused.plan.attention(Q, K, V, scale, p=alpha)
        gq, gk, gv = torch.empty((a.m, k), device="cuda"), torch.empty((a.n, k), device="cuda"), torch.empty((a.n, k), device="cuda")
        da, gs = torch.empty(a.nnz, device="cuda"), torch.empty(a.nnz, device="cuda")

        def eight_calls():  # _FusedAttention.backward without fused_backward
            chain.plan_t.set_values(alpha)
            chain.plan_t(g, out=gv)
            chain.plan.sddmm(g, V, out=da)
            chain.plan.edge_softmax_backward(alpha, da, scale, out=gs)
            chain.plan.set_values(gs)
            chain.plan(K, out=gq)
            chain.plan_t.set_values(gs)
            chain.plan_t(Q, out=gk)

        Qg, Kg, Vg = (x.clone().requires_grad_() for x in (Q, K, V))

        def step(op):
            for x in (Qg, Kg, Vg):
                x.grad = None
            op.attention(Qg, Kg, Vg, scale).backward(g)

        fns = {"eight calls": eight_calls,
               "fused backward": lambda: fused.plan.attention_backward(Q, K, V, alpha, g, scale, grad_q=gq, grad_k=gk, grad_v=gv, work=gs),
               "step, chain backward": lambda: step(chain), "step, fused backward": lambda: step(fused)}
        n = max(3, min(100, int(1e8 / max(1, a.nnz * k))))
        rounds = {key: [] for key in fns}
        for _ in range(3):  # alternating: every round times each contender once
            for key, fn in fns.items():
                rounds[key].append(best_us(fn, n, rounds=1))
        best = {key: min(v) for key, v in rounds.items()}
        spread = {key: 100 * (max(v) - min(v)) / min(v) for key, v in rounds.items()}
        say(f"{name} k={k} backward (columns: slot {i['columns_slot']} wave {i['columns_wave']} block {i['columns_block']} empty {i['columns_empty']}, {i['items']} items, "
            f"{i['groups']} groups of cost <= {i['group_budget']}, second part of the image {i['device_bytes'] / max(1, a.nnz):.2f} B/nnz): "
            + "  ".join(f"{key} {best[key]:.1f} us (+{spread[key]:.0f} % over 3 rounds)" for key in fns)
            + f"  eight calls / fused backward {best['eight calls'] / best['fused backward']:.2f}x"
            + f"  step / step with the fused backward {best['step, chain backward'] / best['step, fused backward']:.2f}x")
        del chain, fused


def probe_heads(name, a):
    gen = torch.Generator(device="cuda").manual_seed(4)
    st = torch.cuda.current_stream().cuda_stream
    for k, H in ((64, 4), (128, 4), (128, 8)):
        d = k // H
        multi = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
        one = flex_amd.SparseOperator(a, d, learn_values=True, fused_attention=True, fused_backward=True)  # the step of the loop
        strided = flex_amd.Plan(a, d, ldb=k, ldc=k, attention=True, attention_backward=True)               # the calls of the loop
        Q, K, V = (torch.rand((r, k), device="cuda", generator=gen) * 2 - 1 for r in (a.m, a.n, a.n))
        g = torch.rand((a.m, k), device="cuda", generator=gen) * 2 - 1
        scale = d ** -0.5
        out, gq, gk, gv = (torch.empty((r, k), device="cuda") for r in (a.m, a.m, a.n, a.n))
        P, W = torch.empty((a.nnz, H), device="cuda"), torch.empty((a.nnz, H), device="cuda")    # entry-major: the one call
        P1, W1 = torch.empty((H, a.nnz), device="cuda"), torch.empty((H, a.nnz), device="cuda")  # a vector per head: the loop
        ptr = lambda t, h: t.data_ptr() + 4 * h * d  # noqa: E731

        def loop_forward():
            for h in range(H):
                strided.attention_ptr(ptr(Q, h), ptr(K, h), ptr(V, h), scale, ptr(out, h), P1[h].data_ptr(), st)

        def loop_backward():
            for h in range(H):
                strided.attention_backward_ptr(ptr(Q, h), ptr(K, h), ptr(V, h), P1[h].data_ptr(), ptr(g, h), scale, ptr(gq, h), ptr(gk, h), ptr(gv, h),
                                               W1[h].data_ptr(), st)

        Qg, Kg, Vg = (x.clone().requires_grad_() for x in (Q, K, V))

        def clear():
            for x in (Qg, Kg, Vg):
                x.grad = None

        def loop_step():
            clear()
            torch.cat([one.attention(Qg[:, h * d:(h + 1) * d], Kg[:, h * d:(h + 1) * d], Vg[:, h * d:(h + 1) * d], scale) for h in range(H)], 1).backward(g)

        def heads_step():
            clear()
            multi.attention(Qg, Kg, Vg, scale, heads=H).backward(g)

        loop_forward()
        multi.plan.attention(Q, K, V, scale, out=out, p=P, heads=H)
        fns = {"forward, loop": loop_forward, "forward, heads": lambda: multi.plan.attention(Q, K, V, scale, out=out, p=P, heads=H),
               "backward, loop": loop_backward,
               "backward, heads": lambda: multi.plan.attention_backward(Q, K, V, P, g, scale, grad_q=gq, grad_k=gk, grad_v=gv, work=W, heads=H),
               "step, loop": loop_step, "step, heads": heads_step}
        n = max(3, min(100, int(1e8 / max(1, a.nnz * k))))
        rounds = {key: [] for key in fns}
        for _ in range(3):  # alternating: every round times each contender once
            for key, fn in fns.items():
                rounds[key].append(best_us(fn, n, rounds=1))
        best = {key: min(v) for key, v in rounds.items()}
        spread = {key: 100 * (max(v) - min(v)) / min(v) for key, v in rounds.items()}
        say(f"{name} k={k} H={H} d={d} heads: " + "  ".join(f"{key} {best[key]:.1f} us (+{spread[key]:.0f} % over 3 rounds)" for key in fns)
            + "  loop / heads: " + "  ".join(f"{w} {best[w + ', loop'] / best[w + ', heads']:.2f}x" for w in ("forward", "backward", "step"))
            + f"  edge arrays of a step: {8 * a.nnz * H / 2 ** 20:.1f} MiB (P and work, nnz x H floats each) either way")
        del multi, one, strided


def probe_gat(name, a):
    import numpy as np
    gen = torch.Generator(device="cuda").manual_seed(5)
    rp = a.rowPtr.astype(np.int64)
    rows = torch.from_numpy(np.repeat(np.arange(a.m), np.diff(rp))).cuda()
    cols = torch.from_numpy(a.col.astype(np.int64)).cuda()
    slope = 0.2
    for k, H in ((64, 8), (128, 4), (256, 8)):
        d = k // H
        fused = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
        one = flex_amd.SparseOperator(a, d, learn_values=True)  # what a user had: one head at a time on a column slice
        el, er = (torch.rand((r, H), device="cuda", generator=gen) * 4 - 2 for r in (a.m, a.n))
        V = torch.rand((a.n, k), device="cuda", generator=gen) * 2 - 1
        g = torch.rand((a.m, k), device="cuda", generator=gen) * 2 - 1
        out, gv = torch.empty((a.m, k), device="cuda"), torch.empty((a.n, k), device="cuda")
        gel, ger = torch.empty((a.m, H), device="cuda"), torch.empty((a.n, H), device="cuda")
        P, W = torch.empty((a.nnz, H), device="cuda"), torch.empty((a.nnz, H), device="cuda")
        elg, erg, Vg = (x.clone().requires_grad_() for x in (el, er, V))

        def loop(el, er, V):
            outs = []
            for h in range(H):
                s = torch.nn.functional.leaky_relu(el[rows, h] + er[cols, h], slope)
                outs.append(one(V[:, h * d:(h + 1) * d].contiguous(), values=one.edge_softmax(s)))
            return torch.cat(outs, 1)

        def loop_forward():
            with torch.no_grad():
                loop(el, er, V)

        def clear():
            for x in (elg, erg, Vg):
                x.grad = None

        kept = loop(elg, erg, Vg)

        def loop_backward():
            clear()
            kept.backward(g, retain_graph=True)

        def loop_step():
            clear()
            loop(elg, erg, Vg).backward(g)

        def fused_step():
            clear()
            fused.gat_attention(elg, erg, Vg, slope).backward(g)

        fused.plan.gat_attention(el, er, V, slope, out=out, p=P)
        fns = {"forward, loop": loop_forward, "forward, fused": lambda: fused.plan.gat_attention(el, er, V, slope, out=out, p=P),
               "backward, loop": loop_backward,
               "backward, fused": lambda: fused.plan.gat_attention_backward(el, er, V, P, g, slope, grad_el=gel, grad_er=ger, grad_v=gv, work=W),
               "step, loop": loop_step, "step, fused": fused_step}
        n = max(3, min(100, int(1e8 / max(1, a.nnz * k))))
        rounds = {key: [] for key in fns}
        for _ in range(3):  # alternating: every round times each contender once
            for key, fn in fns.items():
                rounds[key].append(best_us(fn, n, rounds=1))
        best = {key: min(v) for key, v in rounds.items()}
        spread = {key: 100 * (max(v) - min(v)) / min(v) for key, v in rounds.items()}
        say(f"{name} k={k} H={H} d={d} gat: " + "  ".join(f"{key} {best[key]:.1f} us (+{spread[key]:.0f} % over 3 rounds)" for key in fns)
            + "  loop / fused: " + "  ".join(f"{w} {best[w + ', loop'] / best[w + ', fused']:.2f}x" for w in ("forward", "backward", "step"))
            + f"  edge arrays of a step: {8 * a.nnz * H / 2 ** 20:.1f} MiB (P and work, nnz x H floats each)")
        del fused, one, kept


def probe_bf16(name, a):
    gen = torch.Generator(device="cuda").manual_seed(6)
    for k, H in ((64, 8), (128, 4), (256, 8)):
        d = k // H
        op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)  # one plan serves both element types
        plan = op.plan
        Q, K, V = (torch.rand((r, k), device="cuda", generator=gen) * 2 - 1 for r in (a.m, a.n, a.n))
        g = torch.rand((a.m, k), device="cuda", generator=gen) * 2 - 1
        Qb, Kb, Vb, gb = (x.bfloat16() for x in (Q, K, V, g))
        scale = d ** -0.5
        out, gq, gk, gv = (torch.empty((r, k), device="cuda") for r in (a.m, a.m, a.n, a.n))
        outb, gqb, gkb, gvb = (torch.empty((r, k), device="cuda", dtype=torch.bfloat16) for r in (a.m, a.m, a.n, a.n))
        P, W = torch.empty((a.nnz, H), device="cuda"), torch.empty((a.nnz, H), device="cuda")
        Pb, Wb = torch.empty((a.nnz, H), device="cuda"), torch.empty((a.nnz, H), device="cuda")
        leaves = {torch.float32: tuple(x.clone().requires_grad_() for x in (Q, K, V)), torch.bfloat16: tuple(x.clone().requires_grad_() for x in (Qb, Kb, Vb))}

        def step(dtype, grad):
            for x in leaves[dtype]:
                x.grad = None
            op.attention(*leaves[dtype], scale, heads=H).backward(grad)

        plan.attention(Q, K, V, scale, out=out, p=P, heads=H)
        plan.attention_bf16(Qb, Kb, Vb, scale, heads=H, out=outb, p=Pb)
        fns = {"forward, fp32": lambda: plan.attention(Q, K, V, scale, out=out, p=P, heads=H),
               "forward, bf16": lambda: plan.attention_bf16(Qb, Kb, Vb, scale, heads=H, out=outb, p=Pb),
               "backward, fp32": lambda: plan.attention_backward(Q, K, V, P, g, scale, grad_q=gq, grad_k=gk, grad_v=gv, work=W, heads=H),
               "backward, bf16": lambda: plan.attention_bf16_backward(Qb, Kb, Vb, Pb, gb, scale, heads=H, grad_q=gqb, grad_k=gkb, grad_v=gvb, work=Wb),
               "step, fp32": lambda: step(torch.float32, g), "step, bf16": lambda: step(torch.bfloat16, gb)}
        n = max(3, min(100, int(1e8 / max(1, a.nnz * k))))
        rounds = {key: [] for key in fns}
        for _ in range(3):  # alternating: every round times each contender once
            for key, fn in fns.items():
                rounds[key].append(best_us(fn, n, rounds=1))
        best = {key: min(v) for key, v in rounds.items()}
        spread = {key: 100 * (max(v) - min(v)) / min(v) for key, v in rounds.items()}
        say(f"{name} k={k} H={H} d={d} bf16: " + "  ".join(f"{key} {best[key]:.1f} us (+{spread[key]:.0f} % over 3 rounds)" for key in fns)
            + "  fp32 / bf16: " + "  ".join(f"{w} {best[w + ', fp32'] / best[w + ', bf16']:.2f}x" for w in ("forward", "backward", "step"))
            + f"  row operands of a step: {2 * (2 * a.m + 2 * a.n) * k * 2 / 2 ** 20:.1f} MiB in bf16, twice that in fp32 (Q, K, V, Out and their gradients);"
            + f" edge arrays {8 * a.nnz * H / 2 ** 20:.1f} MiB either way")
        del op, plan


def _alternate(fns, n):
    """best of 3 rounds and the spread over them, every round timing each contender once"""
    rounds = {key: [] for key in fns}
    for _ in range(3):
        for key, fn in fns.items():
            rounds[key].append(best_us(fn, n, rounds=1))
    return {key: min(v) for key, v in rounds.items()}, {key: 100 * (max(v) - min(v)) / min(v) for key, v in rounds.items()}


def probe_bias(name, a):
    gen = torch.Generator(device="cuda").manual_seed(7)
    for k, H in ((64, 8), (128, 4), (256, 8), (64, 1)):
        d = k // H
        op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)  # one plan serves every contender
        plan = op.plan
        Q, K, V, g = (torch.rand((r, k), device="cuda", generator=gen) * 2 - 1 for r in (a.m, a.n, a.n, a.m))
        b = torch.rand((a.nnz, H), device="cuda", generator=gen) * 8 - 4
        scale = d ** -0.5
        rows = {torch.float32: (Q, K, V, g), torch.bfloat16: tuple(x.bfloat16() for x in (Q, K, V, g))}
        outs = {dt: tuple(torch.empty((r, k), device="cuda", dtype=dt) for r in (a.m, a.m, a.n, a.n)) for dt in rows}
        P, W, GB = (torch.empty((a.nnz, H), device="cuda") for _ in range(3))
        leaves = {dt: tuple(x.clone().requires_grad_() for x in r[:3]) for dt, r in rows.items()}
        bl = b.clone().requires_grad_()

        def step(dt, biased):
            for x in leaves[dt] + (bl,):
                x.grad = None
            op.attention(*leaves[dt], scale, heads=H, bias=bl if biased else None).backward(rows[dt][3])

        fns = {}
        for dt, tag, plain, plain_b, biased, biased_b in (
                (torch.float32, "fp32", plan.attention, plan.attention_backward, plan.attention_bias, plan.attention_bias_backward),
                (torch.bfloat16, "bf16", plan.attention_bf16, plan.attention_bf16_backward, plan.attention_bf16_bias, plan.attention_bf16_bias_backward)):
            # one head in fp32 is flex_attention itself, whose edge arrays are [nnz]
            Pp, Wp = (P.view(-1), W.view(-1)) if H == 1 and dt == torch.float32 else (P, W)
            (q, kk, v, gg), (o, gq, gk, gv) = rows[dt], outs[dt]
            fns[f"forward, {tag}"] = lambda q=q, kk=kk, v=v, o=o, f=plain, Pp=Pp: f(q, kk, v, scale, out=o, p=Pp, heads=H)
            fns[f"forward, {tag} bias"] = lambda q=q, kk=kk, v=v, o=o, f=biased: f(q, kk, v, b, scale, heads=H, out=o, p=P)
            fns[f"backward, {tag}"] = lambda q=q, kk=kk, v=v, gg=gg, gq=gq, gk=gk, gv=gv, f=plain_b, Pp=Pp, Wp=Wp: f(q, kk, v, Pp, gg, scale, grad_q=gq, grad_k=gk, grad_v=gv, work=Wp, heads=H)
            fns[f"backward, {tag} bias"] = lambda q=q, kk=kk, v=v, gg=gg, gq=gq, gk=gk, gv=gv, f=biased_b: f(q, kk, v, P, gg, scale, heads=H, grad_q=gq, grad_k=gk, grad_v=gv, grad_bias=GB, work=W)
            fns[f"step, {tag}"] = lambda dt=dt: step(dt, False)
            fns[f"step, {tag} bias"] = lambda dt=dt: step(dt, True)
        if H == 1:  # what a user needed before: four calls and a torch add, with their autograd
            b1 = b[:, 0].clone().requires_grad_()

            def composed():
                for x in leaves[torch.float32] + (b1,):
                    x.grad = None
                q, kk, v = leaves[torch.float32]
                return op(v, values=op.edge_softmax(scale * op.sddmm(q, kk) + b1, 1.0))

            def composed_forward():
                with torch.no_grad():
                    composed()

            fns["forward, four calls and an add"] = composed_forward
            fns["step, four calls and an add"] = lambda: composed().backward(g)
        plan.attention_bias(Q, K, V, b, scale, heads=H, out=outs[torch.float32][0], p=P)  # P holds probabilities for every backward
        n = max(3, min(100, int(1e8 / max(1, a.nnz * k))))
        best, spread = _alternate(fns, n)
        say(f"{name} k={k} H={H} d={d} bias: " + "  ".join(f"{key} {best[key]:.1f} us (+{spread[key]:.0f} % over 3 rounds)" for key in fns)
            + "  bias / no bias: " + "  ".join(f"{w} {t} {best[f'{w}, {t} bias'] / best[f'{w}, {t}']:.2f}x" for t in ("fp32", "bf16") for w in ("forward", "backward", "step"))
            + ("  four calls / fused: " + "  ".join(f"{w} {best[w + ', four calls and an add'] / best[w + ', fp32 bias']:.2f}x" for w in ("forward", "step")) if H == 1 else "")
            + f"  bias and gBias: {4 * a.nnz * H / 2 ** 20:.1f} MiB each (nnz x H floats), beside P and work of the same size")
        del op, plan


def probe_dropout(name, a):
    gen = torch.Generator(device="cuda").manual_seed(8)
    seed = 0x0123456789ABCDEF
    for k, H in ((64, 8), (128, 4), (256, 8)):
        d = k // H
        plan = flex_amd.Plan(a, k, attention=True, attention_backward=True)  # one plan serves every contender
        Q, K, V, g = (torch.rand((r, k), device="cuda", generator=gen) * 2 - 1 for r in (a.m, a.n, a.n, a.m))
        scale = d ** -0.5
        rows = {torch.float32: (Q, K, V, g), torch.bfloat16: tuple(x.bfloat16() for x in (Q, K, V, g))}
        outs = {dt: tuple(torch.empty((r, k), device="cuda", dtype=dt) for r in (a.m, a.m, a.n, a.n)) for dt in rows}
        P, W = (torch.empty((a.nnz, H), device="cuda") for _ in range(2))
        fns = {}
        for dt, tag, plain, plain_b, drop, drop_b in (
                (torch.float32, "fp32", plan.attention, plan.attention_backward, plan.attention_dropout, plan.attention_dropout_backward),
                (torch.bfloat16, "bf16", plan.attention_bf16, plan.attention_bf16_backward, plan.attention_bf16_dropout, plan.attention_bf16_dropout_backward)):
            (q, kk, v, gg), (o, gq, gk, gv) = rows[dt], outs[dt]
            fns[f"forward, {tag}"] = lambda q=q, kk=kk, v=v, o=o, f=plain: f(q, kk, v, scale, out=o, p=P, heads=H)
            fns[f"backward, {tag}"] = lambda q=q, kk=kk, v=v, gg=gg, gq=gq, gk=gk, gv=gv, f=plain_b: f(q, kk, v, P, gg, scale, grad_q=gq, grad_k=gk, grad_v=gv, work=W, heads=H)
            for p_ in (0.1, 0.6):
                fns[f"forward, {tag} p={p_}"] = lambda q=q, kk=kk, v=v, o=o, f=drop, p_=p_: f(q, kk, v, scale, p_, seed, heads=H, out=o, probs=P)
                fns[f"backward, {tag} p={p_}"] = lambda q=q, kk=kk, v=v, gg=gg, gq=gq, gk=gk, gv=gv, f=drop_b, p_=p_: f(q, kk, v, P, gg, scale, p_, seed, heads=H, grad_q=gq, grad_k=gk, grad_v=gv, work=W)
        plan.attention(Q, K, V, scale, out=outs[torch.float32][0], p=P, heads=H)  # P holds probabilities for every backward
        n = max(3, min(100, int(1e8 / max(1, a.nnz * k))))
        best, spread = _alternate(fns, n)
        say(f"{name} k={k} H={H} d={d} dropout: " + "  ".join(f"{key} {best[key]:.1f} us (+{spread[key]:.0f} % over 3 rounds)" for key in fns)
            + "  dropout / no dropout: " + "  ".join(f"{w} {t} p={p_} {best[f'{w}, {t} p={p_}'] / best[f'{w}, {t}']:.2f}x"
                                                      for t in ("fp32", "bf16") for w in ("forward", "backward") for p_ in (0.1, 0.6))
            + "  extra memory: none (the mask is recomputed from the seed)")
        del plan


def probe_gat_dropout(name, a):
    gen = torch.Generator(device="cuda").manual_seed(9)
    seed, slope = 0x0123456789ABCDEF, 0.2
    for k, H in ((64, 8), (128, 4), (256, 8)):
        d = k // H
        plan = flex_amd.Plan(a, k, attention=True, attention_backward=True)  # one plan serves every contender
        el, er = (torch.rand((r, H), device="cuda", generator=gen) * 4 - 2 for r in (a.m, a.n))
        V, g = (torch.rand((r, k), device="cuda", generator=gen) * 2 - 1 for r in (a.n, a.m))
        out, gv = torch.empty((a.m, k), device="cuda"), torch.empty((a.n, k), device="cuda")
        gel, ger = torch.empty((a.m, H), device="cuda"), torch.empty((a.n, H), device="cuda")
        P, W = (torch.empty((a.nnz, H), device="cuda") for _ in range(2))
        fns = {"forward": lambda: plan.gat_attention(el, er, V, slope, out=out, p=P),
               "backward": lambda: plan.gat_attention_backward(el, er, V, P, g, slope, grad_el=gel, grad_er=ger, grad_v=gv, work=W)}
        for p_ in (0.1, 0.6):
            fns[f"forward p={p_}"] = lambda p_=p_: plan.gat_attention_dropout(el, er, V, slope, p_, seed, out=out, probs=P)
            fns[f"backward p={p_}"] = lambda p_=p_: plan.gat_attention_dropout_backward(el, er, V, P, g, slope, p_, seed, grad_el=gel, grad_er=ger,
                                                                                       grad_v=gv, work=W)
        plan.gat_attention(el, er, V, slope, out=out, p=P)  # P holds probabilities for every backward
        n = max(3, min(100, int(1e8 / max(1, a.nnz * k))))
        best, spread = _alternate(fns, n)
        say(f"{name} k={k} H={H} d={d} gat dropout: " + "  ".join(f"{key} {best[key]:.1f} us (+{spread[key]:.0f} % over 3 rounds)" for key in fns)
            + "  dropout / no dropout: " + "  ".join(f"{w} p={p_} {best[f'{w} p={p_}'] / best[w]:.2f}x" for w in ("forward", "backward") for p_ in (0.1, 0.6))
            + "  extra memory: none (the mask is recomputed from the seed)")
        del plan


def probe_gat_bf16(name, a):
    gen = torch.Generator(device="cuda").manual_seed(10)
    seed, slope, p_ = 0x0123456789ABCDEF, 0.2, 0.6
    for k, H in ((64, 8), (128, 4), (256, 8)):
        d = k // H
        op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)  # one plan serves every contender
        plan = op.plan
        el, er = (torch.rand((r, H), device="cuda", generator=gen) * 4 - 2 for r in (a.m, a.n))
        V, g = (torch.rand((r, k), device="cuda", generator=gen) * 2 - 1 for r in (a.n, a.m))
        rows = {torch.float32: (V, g), torch.bfloat16: (V.bfloat16(), g.bfloat16())}
        outs = {dt: (torch.empty((a.m, k), device="cuda", dtype=dt), torch.empty((a.n, k), device="cuda", dtype=dt)) for dt in rows}
        gel, ger = torch.empty((a.m, H), device="cuda"), torch.empty((a.n, H), device="cuda")
        P, W = (torch.empty((a.nnz, H), device="cuda") for _ in range(2))
        leaves = {dt: (el.clone().requires_grad_(), er.clone().requires_grad_(), r[0].clone().requires_grad_()) for dt, r in rows.items()}

        def step(dt, dropped):
            for x in leaves[dt]:
                x.grad = None
            op.gat_attention(*leaves[dt], slope, **(dict(dropout=p_, seed=seed) if dropped else {})).backward(rows[dt][1])

        fns = {}
        for dt, tag, plain, plain_b, drop, drop_b in (
                (torch.float32, "fp32", plan.gat_attention, plan.gat_attention_backward, plan.gat_attention_dropout, plan.gat_attention_dropout_backward),
                (torch.bfloat16, "bf16", plan.gat_attention_bf16, plan.gat_attention_bf16_backward, plan.gat_attention_bf16_dropout,
                 plan.gat_attention_bf16_dropout_backward)):
            (v, gg), (o, gv) = rows[dt], outs[dt]
            fns[f"forward, {tag}"] = lambda v=v, o=o, f=plain: f(el, er, v, slope, out=o, p=P)
            fns[f"backward, {tag}"] = lambda v=v, gg=gg, gv=gv, f=plain_b: f(el, er, v, P, gg, slope, grad_el=gel, grad_er=ger, grad_v=gv, work=W)
            fns[f"step, {tag}"] = lambda dt=dt: step(dt, False)
            fns[f"forward, {tag} p={p_}"] = lambda v=v, o=o, f=drop: f(el, er, v, slope, p_, seed, out=o, probs=P)
            fns[f"backward, {tag} p={p_}"] = lambda v=v, gg=gg, gv=gv, f=drop_b: f(el, er, v, P, gg, slope, p_, seed, grad_el=gel, grad_er=ger, grad_v=gv, work=W)
            fns[f"step, {tag} p={p_}"] = lambda dt=dt: step(dt, True)
        plan.gat_attention(el, er, V, slope, out=outs[torch.float32][0], p=P)  # P holds probabilities for every backward
        n = max(3, min(100, int(1e8 / max(1, a.nnz * k))))
        best, spread = _alternate(fns, n)
        say(f"{name} k={k} H={H} d={d} gat bf16: " + "  ".join(f"{key} {best[key]:.1f} us (+{spread[key]:.0f} % over 3 rounds)" for key in fns)
            + "  fp32 / bf16: " + "  ".join(f"{w}{t} {best[f'{w}, fp32{t}'] / best[f'{w}, bf16{t}']:.2f}x" for t in ("", f" p={p_}") for w in ("forward", "backward", "step"))
            + f"  row operands of a step: {2 * (a.m + a.n) * k * 2 / 2 ** 20:.1f} MiB in bf16, twice that in fp32 (V, Out and their gradients);"
            + f" el, er, their gradients and the edge arrays ({8 * a.nnz * H / 2 ** 20:.1f} MiB) are fp32 either way")
        del op, plan


def probe_gatv2(name, a):
    import numpy as np
    gen = torch.Generator(device="cuda").manual_seed(13)
    rp = a.rowPtr.astype(np.int64)
    rows = torch.from_numpy(np.repeat(np.arange(a.m), np.diff(rp))).cuda()
    cols = torch.from_numpy(a.col.astype(np.int64)).cuda()
    slope = 0.2
    for k, H in ((64, 8), (128, 4), (256, 8)):
        d = k // H
        fused = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
        one = flex_amd.SparseOperator(a, d, learn_values=True)  # what a user had: one head at a time on a column slice
        xt, xs = (torch.rand((r, k), device="cuda", generator=gen) * 4 - 2 for r in (a.m, a.n))
        att = torch.rand((H, d), device="cuda", generator=gen) * 2 - 1
        g = torch.rand((a.m, k), device="cuda", generator=gen) * 2 - 1
        out, gxt, gxs, gatt = torch.empty((a.m, k), device="cuda"), torch.empty((a.m, k), device="cuda"), torch.empty((a.n, k), device="cuda"), torch.empty((H, d), device="cuda")
        P, W = torch.empty((a.nnz, H), device="cuda"), torch.empty((a.nnz, H), device="cuda")
        att_floats = fused.plan.gatv2_attention_work_size()
        AW = torch.empty(max(1, att_floats), device="cuda")
        xtg, xsg, attg = (x.clone().requires_grad_() for x in (xt, xs, att))

        def loop(xt, xs, att):
            s = (torch.nn.functional.leaky_relu((xt[rows] + xs[cols]).view(-1, H, d), slope) * att).sum(-1)  # the [nnz, k] tensor
            return torch.cat([one(xs[:, h * d:(h + 1) * d].contiguous(), values=one.edge_softmax(s[:, h].contiguous())) for h in range(H)], 1)

        def loop_forward():
            with torch.no_grad():
                loop(xt, xs, att)

        def clear():
            for x in (xtg, xsg, attg):
                x.grad = None

        kept = loop(xtg, xsg, attg)

        def loop_backward():
            clear()
            kept.backward(g, retain_graph=True)

        def loop_step():
            clear()
            loop(xtg, xsg, attg).backward(g)

        def fused_step():
            clear()
            fused.gatv2_attention(xtg, xsg, attg, slope).backward(g)

        fused.plan.gatv2_attention(xt, xs, att, slope, out=out, p=P)
        fns = {"forward, loop": loop_forward, "forward, fused": lambda: fused.plan.gatv2_attention(xt, xs, att, slope, out=out, p=P),
               "backward, loop": loop_backward,
               "backward, fused": lambda: fused.plan.gatv2_attention_backward(xt, xs, att, P, g, slope, grad_xt=gxt, grad_xs=gxs, grad_att=gatt, work=W, att_work=AW),
               "step, loop": loop_step, "step, fused": fused_step}
        n = max(3, min(100, int(1e8 / max(1, a.nnz * k))))
        rounds = {key: [] for key in fns}
        for _ in range(3):  # alternating: every round times each contender once
            for key, fn in fns.items():
                rounds[key].append(best_us(fn, n, rounds=1))
        best = {key: min(v) for key, v in rounds.items()}
        spread = {key: 100 * (max(v) - min(v)) / min(v) for key, v in rounds.items()}
        say(f"{name} k={k} H={H} d={d} gatv2: " + "  ".join(f"{key} {best[key]:.1f} us (+{spread[key]:.0f} % over 3 rounds)" for key in fns)
            + "  loop / fused: " + "  ".join(f"{w} {best[w + ', loop'] / best[w + ', fused']:.2f}x" for w in ("forward", "backward", "step"))
            + f"  edge arrays of a step: fused {8 * a.nnz * H / 2 ** 20:.1f} MiB (P and work) + {4 * att_floats / 2 ** 20:.2f} MiB (gAtt partials), "
              f"loop {4 * a.nnz * k / 2 ** 20:.1f} MiB for Xt[row] + Xs[col] alone")
        del fused, one, kept


def probe_gatv2_dropout(name, a):
    gen = torch.Generator(device="cuda").manual_seed(14)
    seed, slope = 0x0123456789ABCDEF, 0.2
    for k, H in ((64, 8), (128, 4), (256, 8)):
        d = k // H
        plan = flex_amd.Plan(a, k, attention=True, attention_backward=True)  # one plan serves every contender
        xt, xs = (torch.rand((r, k), device="cuda", generator=gen) * 4 - 2 for r in (a.m, a.n))
        att = torch.rand((H, d), device="cuda", generator=gen) * 2 - 1
        g = torch.rand((a.m, k), device="cuda", generator=gen) * 2 - 1
        out, gxt, gxs, gatt = torch.empty((a.m, k), device="cuda"), torch.empty((a.m, k), device="cuda"), torch.empty((a.n, k), device="cuda"), torch.empty((H, d), device="cuda")
        P, W = (torch.empty((a.nnz, H), device="cuda") for _ in range(2))
        AW = torch.empty(max(1, plan.gatv2_attention_work_size()), device="cuda")
        fns = {"forward": lambda: plan.gatv2_attention(xt, xs, att, slope, out=out, p=P),
               "backward": lambda: plan.gatv2_attention_backward(xt, xs, att, P, g, slope, grad_xt=gxt, grad_xs=gxs, grad_att=gatt, work=W, att_work=AW)}
        for p_ in (0.1, 0.6):
            fns[f"forward p={p_}"] = lambda p_=p_: plan.gatv2_attention_dropout(xt, xs, att, slope, p_, seed, out=out, probs=P)
            fns[f"backward p={p_}"] = lambda p_=p_: plan.gatv2_attention_dropout_backward(xt, xs, att, P, g, slope, p_, seed, grad_xt=gxt, grad_xs=gxs,
                                                                                         grad_att=gatt, work=W, att_work=AW)
        plan.gatv2_attention(xt, xs, att, slope, out=out, p=P)  # P holds probabilities for every backward
        n = max(3, min(100, int(1e8 / max(1, a.nnz * k))))
        best, spread = _alternate(fns, n)
        say(f"{name} k={k} H={H} d={d} gatv2 dropout: " + "  ".join(f"{key} {best[key]:.1f} us (+{spread[key]:.0f} % over 3 rounds)" for key in fns)
            + "  dropout / no dropout: " + "  ".join(f"{w} p={p_} {best[f'{w} p={p_}'] / best[w]:.2f}x" for w in ("forward", "backward") for p_ in (0.1, 0.6))
            + "  extra memory: none (the mask is recomputed from the seed)")
        del plan


def probe_gat_edge(name, a):
    import numpy as np
    gen = torch.Generator(device="cuda").manual_seed(15)
    rp = a.rowPtr.astype(np.int64)
    rows = torch.from_numpy(np.repeat(np.arange(a.m), np.diff(rp))).cuda()
    cols = torch.from_numpy(a.col.astype(np.int64)).cuda()
    slope = 0.2
    for k, H in ((64, 8), (128, 4), (256, 8)):
        d = k // H
        fused = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
        one = flex_amd.SparseOperator(a, d, learn_values=True)  # what a user had: one head at a time on a column slice
        el, er = (torch.rand((r, H), device="cuda", generator=gen) * 4 - 2 for r in (a.m, a.n))
        ee = torch.rand((a.nnz, H), device="cuda", generator=gen) * 4 - 2
        V = torch.rand((a.n, k), device="cuda", generator=gen) * 2 - 1
        g = torch.rand((a.m, k), device="cuda", generator=gen) * 2 - 1
        out, gv = torch.empty((a.m, k), device="cuda"), torch.empty((a.n, k), device="cuda")
        gel, ger = torch.empty((a.m, H), device="cuda"), torch.empty((a.n, H), device="cuda")
        P, W, gee = (torch.empty((a.nnz, H), device="cuda") for _ in range(3))
        elg, erg, eeg, Vg = (x.clone().requires_grad_() for x in (el, er, ee, V))

        def loop(el, er, ee, V):
            outs = []
            for h in range(H):
                s = torch.nn.functional.leaky_relu(el[rows, h] + er[cols, h] + ee[:, h], slope)
                outs.append(one(V[:, h * d:(h + 1) * d].contiguous(), values=one.edge_softmax(s)))
            return torch.cat(outs, 1)

        def loop_forward():
            with torch.no_grad():
                loop(el, er, ee, V)

        def clear():
            for x in (elg, erg, eeg, Vg):
                x.grad = None

        kept = loop(elg, erg, eeg, Vg)

        def loop_backward():
            clear()
            kept.backward(g, retain_graph=True)

        def loop_step():
            clear()
            loop(elg, erg, eeg, Vg).backward(g)

        def edge_step():
            clear()
            fused.gat_attention(elg, erg, Vg, slope, edge=eeg).backward(g)

        def plain_step():
            clear()
            fused.gat_attention(elg, erg, Vg, slope).backward(g)

        plan = fused.plan
        plan.gat_edge_attention(el, er, ee, V, slope, out=out, probs=P)
        fns = {"forward, loop": loop_forward, "forward, edge": lambda: plan.gat_edge_attention(el, er, ee, V, slope, out=out, probs=P),
               "forward, no edge": lambda: plan.gat_attention(el, er, V, slope, out=out, p=P),
               "backward, loop": loop_backward,
               "backward, edge": lambda: plan.gat_edge_attention_backward(el, er, ee, V, P, g, slope, grad_el=gel, grad_er=ger, grad_ee=gee, grad_v=gv),
               "backward, no edge": lambda: plan.gat_attention_backward(el, er, V, P, g, slope, grad_el=gel, grad_er=ger, grad_v=gv, work=W),
               "step, loop": loop_step, "step, edge": edge_step, "step, no edge": plain_step}
        n = max(3, min(100, int(1e8 / max(1, a.nnz * k))))
        best, spread = _alternate(fns, n)
        say(f"{name} k={k} H={H} d={d} gat edge: " + "  ".join(f"{key} {best[key]:.1f} us (+{spread[key]:.0f} % over 3 rounds)" for key in fns)
            + "  loop / edge: " + "  ".join(f"{w} {best[w + ', loop'] / best[w + ', edge']:.2f}x" for w in ("forward", "backward", "step"))
            + "  edge / no edge: " + "  ".join(f"{w} {best[w + ', edge'] / best[w + ', no edge']:.2f}x" for w in ("forward", "backward", "step"))
            + f"  edge arrays of a step: {12 * a.nnz * H / 2 ** 20:.1f} MiB (ee, P and gEe = the work array, nnz x H floats each)")
        del fused, one, kept


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "attention_probe.txt")
    if args[:1] == ["--out"]:
        out, args = args[1], args[2:]
    (fused_only, backward_only, heads_only, gat_only, bf16_only, bias_only, dropout_only, gat_dropout_only, gat_bf16_only, gatv2_only, gatv2_dropout_only,
     gat_edge_only) = (args[:1] == [flag] for flag in ("--fused", "--backward", "--heads", "--gat", "--bf16", "--bias", "--dropout", "--gat-dropout",
                                                       "--gat-bf16", "--gatv2", "--gatv2-dropout", "--gat-edge"))
    only = (fused_only or backward_only or heads_only or gat_only or bf16_only or bias_only or dropout_only or gat_dropout_only or gat_bf16_only or gatv2_only
            or gatv2_dropout_only or gat_edge_only)
    if only:
        args = args[1:]
    else:
        exp_error()
    hbm = flex_amd.hbm_probe(0, 2048, 10)
    say(f"flex_hbm_probe: read {hbm['read_GBps']:.0f} GB/s, copy {hbm['copy_GBps']:.0f} GB/s")
    for name in args or ["pubmed.csv", "flickr", "reddit", "soc-sign-epinions"]:
        a = load(name)
        if not only:
            probe(name, a, hbm["copy_GBps"])
        if fused_only or not only:
            probe_fused(name, a)
        if backward_only or not only:
            probe_backward(name, a)
        if heads_only or not only:
            probe_heads(name, a)
        if gat_only or not only:
            probe_gat(name, a)
        if bf16_only or not only:
            probe_bf16(name, a)
        if bias_only or not only:
            probe_bias(name, a)
        if dropout_only or not only:
            probe_dropout(name, a)
        if gat_dropout_only or not only:
            probe_gat_dropout(name, a)
        if gat_bf16_only or not only:
            probe_gat_bf16(name, a)
        if gatv2_only or not only:
            try:
                probe_gatv2(name, a)
            except torch.cuda.OutOfMemoryError:  # the loop's [nnz, k] tensors and their autograd copies
                say(f"{name} gatv2: the torch composition ran out of device memory")
        if gatv2_dropout_only or not only:
            probe_gatv2_dropout(name, a)
        if gat_edge_only or not only:
            probe_gat_edge(name, a)
    with open(out, "a" if only else "w") as f:  # a part is appended, the whole run starts the file
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

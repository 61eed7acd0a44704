#!/usr/bin/env python3
"""GEMM half of the A*X*W layer in isolation: time per order for a shape, library chosen by FLEX_AXW_LIB (ablations).
    probe_axw.py NAME DIM C      the fp32 layer on one shape
    probe_axw.py --bf16          the bf16 layer (FLEX_AXW_BF16) against the fp32 one, alternated in this process, on flickr and reddit at
                                 dim = c = 128 and dim = 256, c = 64: per-stage times, the bf16 GEMM against its streaming floor
                                 (n dim + n cp) 2 bytes / HBM_RATE, the cancellation case's worst err / bound at the probe's n, and what the
                                 bf16 MFMA does with subnormal operands and results.
    probe_axw.py --bf16-backward the bf16 backward (flex_axw_backward_bf16) against the fp32 one on the same graphs and shapes, alternated
                                 in this process: medians of event times of the whole call, of the call without dW and of the call without
                                 dX; the stages are their differences (A^T dOut = no-dW + no-dX - both, dX = both - no-dX, dW = both - no-dW),
                                 the dense ones against their streaming floor (n dim + n cp) 2 bytes / HBM_RATE.
    probe_axw.py --bf16-wide     both tables at input-layer widths (axw_bf16_wide_kernels.hip): flickr at dim 512 and reddit at dim 608 (602
                                 padded), c = 128 and 64, in the order AUTO picks there, A (X W); the fp32 handle runs rocBLAS at dim > 256.
    probe_axw.py --bf16-root     the layer with a root term, A X W + X R + b (flex_axw_run_root_bf16), in both orders against what a handle
                                 without FLEX_AXW_ROOT offers -- Axw.run(X, W) in its AUTO order, then torch's bf16 X @ R, the add and the
                                 bias -- alternated in this process on flickr at (128, 128), (512, 128) and reddit at (128, 128), (608, 128):
                                 medians of event times of the whole calls and of the new call's stages, the dual-source stage of (A X) W
                                 against its streaming floor (2 n dim + n cp) 2 bytes / HBM_RATE.
    probe_axw.py --bf16-root-backward  the backward of that layer (flex_axw_backward_root_bf16) against what the handle offered before it --
                                 Axw.backward, then torch's bf16 dOut @ R.T and the add into dX, X.T @ dOut and dOut.sum(0) -- alternated in
                                 this process: medians of event times of the whole calls, of the new call without dW / dR and without dX
                                 (the stages are their differences, as for --bf16-backward), the one-pass dW / dR / db launcher against two
                                 launches of the one-product dW launcher, and the dense stages against their streaming floors
                                 (2 n cp + n dim) 2 bytes / HBM_RATE.
    probe_axw.py --bf16-root-act the hidden layer dropout(relu(A X W + X R + b)): run_root, torch.relu and F.dropout(p = 0.5), and the backward
                                 of root_layer through those torch ops, against flex_axw_run_root_act_bf16 and flex_axw_backward_root_act_bf16
                                 at p = 0 and p = 0.5, alternated in this process on flickr (128, 128) and reddit (128, 128), (608, 128): medians of
                                 event times of the whole calls.
    probe_axw.py --bf16-fused    order FLEX_AXW_AX_W_FUSED (one launch, no n x dim intermediate) against orders FLEX_AXW_AX_W and FLEX_AXW_AUTO
                                 of the same handle, for run and run_root_act (p = 0.5), alternated in this process on pubmed.csv (128, 64),
                                 flickr (128, 128), reddit (128, 128) and flickr (256, 256): medians of event times of the whole calls, and
                                 the bytes each path moves at the least, computed from the shapes."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flex_amd  # noqa: E402
import tools._knobs  # noqa: E402,F401  (FLEX_* environment knobs -> plan descriptor)
from flex_amd import axw  # noqa: E402

HBM_RATE = 8e12  # bytes / s: the roofline peak of DESIGN.md 3.4 (flex_hbm_probe measures 5.9e12 reading and 4.7e12 copying on this card)
REPS = 30


def timed(h, X, W, order):
    """(gemm_us, spmm_us) of one more run"""
    _, (g, s) = h.run(X, W, order, timed=True)
    return g * 1e3, s * 1e3


NARROW = {name: ((128, 128), (256, 64)) for name in ("flickr", "reddit")}  # graph -> (dim, c)
WIDE = {"flickr": ((512, 128), (512, 64)), "reddit": ((608, 128), (608, 64))}


def bf16_table(shapes=NARROW, orders=(axw.FLEX_AXW_A_XW, axw.FLEX_AXW_AX_W)):
    print(f"| graph | dim | c | order | fp32 gemm | fp32 spmm | fp32 layer | bf16 gemm | bf16 spmm | bf16 layer | bf16 / fp32 | gemm floor | gemm / floor |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for name in shapes:
        a = flex_amd.synth_graph(name)
        for dim, c in shapes[name]:
            h32, h16 = axw.Axw(a, dim, c), axw.Axw(a, dim, c, bf16=True)
            X = torch.rand((a.n, dim), device="cuda") * 2 - 1
            W = torch.rand((dim, c), device="cuda")
            Xb, Wb = X.bfloat16(), W.bfloat16()
            for order in orders:
                t32, t16 = [], []
                for i in range(REPS + 5):  # alternated; the first five of each are warm-up
                    r32, r16 = timed(h32, X, W, order), timed(h16, Xb, Wb, order)
                    if i >= 5:
                        t32.append(r32)
                        t16.append(r16)
                (g32, s32), (g16, s16) = np.median(t32, axis=0), np.median(t16, axis=0)
                l32, l16 = np.median(np.sum(t32, axis=1)), np.median(np.sum(t16, axis=1))
                floor = (a.n * dim + a.n * h16.ld) * 2 / HBM_RATE * 1e6
                print(f"| {name} | {dim} | {c} | {'A(XW)' if order == axw.FLEX_AXW_A_XW else '(AX)W'} | {g32:.1f} | {s32:.1f} | {l32:.1f} | "
                      f"{g16:.1f} | {s16:.1f} | {l16:.1f} | {l16 / l32:.2f} | {floor:.1f} | {g16 / floor:.2f} |", flush=True)
            h32.destroy()
            h16.destroy()


def _gemm(L, Wp, c):
    n, dim = L.shape
    out = torch.empty((n, Wp.shape[1]), dtype=torch.bfloat16, device="cuda")
    rc = axw._gemm_bf16_launch(L.data_ptr(), Wp.data_ptr(), out.data_ptr(), n, dim, c, Wp.shape[1],
                               torch.cuda.get_device_properties(0).multi_processor_count, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return out


def cancellation(n=100000, dim=256, c=64):
    """err / (gamma(dim) |L||W| + dim 2^-149 + the bf16 rounding's share) of the GEMM on rows of pairs (x, -x (1 + 2^-7)), in float64"""
    g = torch.Generator(device="cuda").manual_seed(3)
    L = torch.exp2(torch.rand((n, dim), device="cuda", generator=g) * 8 - 4).bfloat16()
    L[:, 1::2] = -(L[:, 0::2].float() * (1 + 2.0 ** -7)).bfloat16()
    W = torch.exp2(torch.rand((1, c), device="cuda", generator=g) * 8 - 4).bfloat16().repeat(dim, 1).contiguous()
    out = _gemm(L, W, c).double()
    ref, s = L.double() @ W.double(), L.double().abs() @ W.double().abs()
    u = 2.0 ** -24
    b32 = dim * u / (1 - dim * u) * s + dim * 2.0 ** -149
    ratio = ((out - ref).abs() / (b32 + 2.0 ** -8 * (ref.abs() + b32) + 2.0 ** -134)).max().item()
    print(f"cancellation, n={n} dim={dim} c={c}: worst err / bound {ratio:.4f} under gamma(dim); median |ref| / bound32 {(ref.abs() / b32).median().item():.1f}")


def subnormals():
    """the bf16 MFMA on a subnormal bf16 operand (2^-130 x 2^20 = 2^-110, a normal result) and on a subnormal sum (2^-65 x 2^-65 = 2^-130,
    subnormal in fp32 and exactly representable as a bf16 subnormal)"""
    for what, xbits, x, w in (("subnormal operand", 0x0008, 2.0 ** -130, 2.0 ** 20), ("subnormal fp32 sum", 0x1F00, 2.0 ** -65, 2.0 ** -65)):
        L = torch.zeros((32, 16), dtype=torch.bfloat16, device="cuda")
        L.view(torch.int16)[:, 0] = xbits  # the bits, not a conversion that might flush
        W = torch.zeros((16, 64), dtype=torch.bfloat16, device="cuda")
        W[0, :] = w
        out = _gemm(L, W, 64)
        print(f"{what}: {x:g} x {w:g} -> bits {out.view(torch.int16)[0, 0].item() & 0xFFFF:#06x} = {out.float()[0, 0].item():g} (exact {x * w:g})")


def backward_table(shapes=NARROW):
    def once(h, g, X, W, need_x, need_w):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h.backward(g, X, W, need_x=need_x, need_w=need_w)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    print("| graph | dim | c | fp32 A^T dOut | fp32 dX | fp32 dW | fp32 all | bf16 A^T dOut | bf16 dX | bf16 dW | bf16 all | bf16 / fp32 | floor | dX / floor | dW / floor |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for name in shapes:
        a = flex_amd.synth_graph(name)
        for dim, c in shapes[name]:
            h32, h16 = axw.Axw(a, dim, c, backward=True), axw.Axw(a, dim, c, backward=True, bf16=True)
            X, W = torch.rand((a.n, dim), device="cuda") * 2 - 1, torch.rand((dim, c), device="cuda")
            g32, g16 = torch.zeros((a.n, h32.ld), device="cuda"), torch.zeros((a.n, h16.ld), dtype=torch.bfloat16, device="cuda")
            g32[:, :c] = torch.rand((a.n, c), device="cuda") * 2 - 1
            g16[:, :c] = g32[:, :c].bfloat16()
            ops = {32: (h32, g32, X, W), 16: (h16, g16, X.bfloat16(), W.bfloat16())}
            t = {(k, v): [] for k in ops for v in range(3)}
            for i in range(REPS + 5):  # alternated; the first five of each are warm-up
                for v, (nx, nw) in enumerate(((True, True), (True, False), (False, True))):
                    for k in ops:
                        us = once(*ops[k], nx, nw)
                        if i >= 5:
                            t[k, v].append(us)
            cells = []
            for k in (32, 16):
                both, no_dw, no_dx = (float(np.median(t[k, v])) for v in range(3))
                cells += [no_dw + no_dx - both, both - no_dx, both - no_dw, both]
            floor = (a.n * dim + a.n * h16.ld) * 2 / HBM_RATE * 1e6
            print(f"| {name} | {dim} | {c} | " + " | ".join(f"{x:.1f}" for x in cells) + f" | {cells[7] / cells[3]:.2f} | {floor:.1f} | "
                  f"{cells[5] / floor:.2f} | {cells[6] / floor:.2f} |", flush=True)
            h32.destroy()
            h16.destroy()


ROOT = {"flickr": ((128, 128), (512, 128)), "reddit": ((128, 128), (608, 128))}


def root_table(shapes=ROOT):
    def whole(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    orders = (axw.FLEX_AXW_A_XW, axw.FLEX_AXW_AX_W)
    print("| graph | dim | c | run + X@R + add + bias | A(XW) gemm | A(XW) spmm | A(XW) call | (AX)W gemm | (AX)W spmm | (AX)W call | "
          "A(XW) / parent | (AX)W / parent | dual floor | (AX)W gemm / floor |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for name in shapes:
        a = flex_amd.synth_graph(name)
        for dim, c in shapes[name]:
            h = axw.Axw(a, dim, c, bf16=True, root=True)
            X = (torch.rand((a.n, dim), device="cuda") * 2 - 1).bfloat16()
            W, R = (torch.rand((dim, c), device="cuda").bfloat16() for _ in range(2))
            bias = torch.rand(c, device="cuda")
            bias16 = bias.bfloat16()
            parent = lambda: h.run(X, W)[:, :c] + X @ R + bias16  # noqa: E731  (the flag changes nothing in run())
            t = {k: [] for k in ("parent", *orders, *((o, "stages") for o in orders))}
            for i in range(REPS + 5):  # alternated; the first five of each are warm-up
                got = {"parent": whole(parent)}
                for o in orders:
                    got[o] = whole(lambda: h.run_root(X, W, R, bias, o))
                    g, s = h.run_root(X, W, R, bias, o, timed=True)[1]
                    got[o, "stages"] = (g * 1e3, s * 1e3)
                if i >= 5:
                    for k, v in got.items():
                        t[k].append(v)
            par, c1, c2 = (float(np.median(t[k])) for k in ("parent", *orders))
            (g1, s1), (g2, s2) = (np.median(t[o, "stages"], axis=0) for o in orders)
            floor = (2 * a.n * dim + a.n * h.ld) * 2 / HBM_RATE * 1e6
            print(f"| {name} | {dim} | {c} | {par:.1f} | {g1:.1f} | {s1:.1f} | {c1:.1f} | {g2:.1f} | {s2:.1f} | {c2:.1f} | {c1 / par:.2f} | "
                  f"{c2 / par:.2f} | {floor:.1f} | {g2 / floor:.2f} |", flush=True)
            h.destroy()


ROOT_BACKWARD = {"flickr": ((128, 128), (512, 128)), "reddit": ((128, 128), (608, 128), (256, 64))}


def root_backward_table(shapes=ROOT_BACKWARD):
    def whole(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    print("| graph | dim | c | parent composition | new call | new / parent | A^T dOut | dX | dW dR db | two dW launches | dual dW launch | "
          "dual / two | dX / floor | dW / floor |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for name in shapes:
        a = flex_amd.synth_graph(name)
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        for dim, c in shapes[name]:
            h = axw.Axw(a, dim, c, bf16=True, backward=True, root=True)
            n, cp = a.n, h.ld
            X = (torch.rand((n, dim), device="cuda") * 2 - 1).bfloat16()
            W, R = (torch.rand((dim, c), device="cuda").bfloat16() for _ in range(2))
            d = torch.zeros((n, cp), dtype=torch.bfloat16, device="cuda")
            d[:, :c] = (torch.rand((n, c), device="cuda") * 2 - 1).bfloat16()
            G = d.clone()  # any finite right operand times the same for the launchers
            dW, dR, db = torch.empty_like(W), torch.empty_like(R), torch.empty(c, device="cuda")
            part = torch.empty(max(axw._dw_bf16_root_slices(n, dim, c, cus) * (2 * dim * c + c),
                                   (axw._dw_bf16_wide_slices(n, dim, c, cus) if dim > 256 else axw.lib().flex_axw_dw_bf16_slices(n, cus)) * dim * c),
                               device="cuda")
            one = axw._dw_bf16_wide_launch if dim > 256 else axw._dw_bf16_launch
            s = torch.cuda.current_stream().cuda_stream
            p = lambda t: t.data_ptr()  # noqa: E731

            def parent():
                gx, gw = h.backward(d, X, W)
                gx += d[:, :c] @ R.T
                return gx, gw, X.T @ d[:, :c], d.sum(0)

            def two():
                for right, out in ((G, dW), (d, dR)):
                    assert one(p(X), p(right), p(out), p(part), n, dim, c, cp, cus, s) == 0

            runs = {"parent": parent, "new": lambda: h.backward_root(d, X, W, R), "no_w": lambda: h.backward_root(d, X, W, R, need_w=False, need_b=False),
                    "no_x": lambda: h.backward_root(d, X, W, R, need_x=False), "two": two,
                    "dual": lambda: axw._dw_bf16_root_launch(p(X), p(G), p(d), p(dW), p(dR), p(db), p(part), n, dim, c, cp, cus, s)}
            t = {k: [] for k in runs}
            for i in range(REPS + 5):  # alternated; the first five of each are warm-up
                for k, f in runs.items():
                    us = whole(f)
                    if i >= 5:
                        t[k].append(us)
            m = {k: float(np.median(v)) for k, v in t.items()}
            dx, dw = m["new"] - m["no_x"], m["new"] - m["no_w"]
            fx, fw = (2 * n * cp + n * dim) * 2 / HBM_RATE * 1e6, (n * dim + 2 * n * cp) * 2 / HBM_RATE * 1e6
            print(f"| {name} | {dim} | {c} | {m['parent']:.1f} | {m['new']:.1f} | {m['new'] / m['parent']:.2f} | {m['no_w'] + m['no_x'] - m['new']:.1f} | "
                  f"{dx:.1f} | {dw:.1f} | {m['two']:.1f} | {m['dual']:.1f} | {m['dual'] / m['two']:.2f} | {dx / fx:.2f} | {dw / fw:.2f} |", flush=True)
            h.destroy()


ROOT_ACT = {"flickr": ((128, 128),), "reddit": ((128, 128), (608, 128))}


def root_act_table(shapes=ROOT_ACT):
    import torch.nn.functional as F

    def whole(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    print("| graph | dim | c | forward: run_root + relu + dropout | act p = 0 | act p = 0.5 | p = 0 / parent | p = 0.5 / parent | "
          "backward: through torch's ops | act p = 0 | act p = 0.5 | p = 0 / parent | p = 0.5 / parent |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for name in shapes:
        a = flex_amd.synth_graph(name)
        for dim, c in shapes[name]:
            h = axw.Axw(a, dim, c, bf16=True, backward=True, root=True)
            X = (torch.rand((a.n, dim), device="cuda") * 2 - 1).bfloat16()
            W, R = ((torch.rand((dim, c), device="cuda") - 0.5).bfloat16() for _ in range(2))
            bias = torch.rand(c, device="cuda") - 0.5
            d = torch.zeros((a.n, h.ld), dtype=torch.bfloat16, device="cuda")
            d[:, :c] = (torch.rand((a.n, c), device="cuda") * 2 - 1).bfloat16()
            leaves = [t.clone().requires_grad_() for t in (X, W, R, bias)]
            loss = F.dropout(torch.relu(h.root_layer(*leaves)), 0.5)  # the parent's graph, kept for its backward
            out = {p: h.run_root_act(X, W, R, bias, p, 7) for p in (0.0, 0.5)}
            runs = {"f": lambda: F.dropout(torch.relu(h.run_root(X, W, R, bias)), 0.5),
                    "f0": lambda: h.run_root_act(X, W, R, bias, 0.0, 7), "f5": lambda: h.run_root_act(X, W, R, bias, 0.5, 7),
                    "b": lambda: torch.autograd.grad(loss, leaves, d[:, :c], retain_graph=True),
                    "b0": lambda: h.backward_root_act(d, out[0.0], X, W, R, 0.0), "b5": lambda: h.backward_root_act(d, out[0.5], X, W, R, 0.5)}
            t = {k: [] for k in runs}
            for i in range(REPS + 5):  # alternated; the first five of each are warm-up
                for k, f in runs.items():
                    us = whole(f)
                    if i >= 5:
                        t[k].append(us)
            m = {k: float(np.median(v)) for k, v in t.items()}
            print(f"| {name} | {dim} | {c} | {m['f']:.1f} | {m['f0']:.1f} | {m['f5']:.1f} | {m['f0'] / m['f']:.2f} | {m['f5'] / m['f']:.2f} | "
                  f"{m['b']:.1f} | {m['b0']:.1f} | {m['b5']:.1f} | {m['b0'] / m['b']:.2f} | {m['b5'] / m['b']:.2f} |", flush=True)
            h.destroy()


FUSED = (("pubmed", 128, 64), ("flickr", 128, 128), ("reddit", 128, 128), ("flickr", 256, 256))


def fused_table(shapes=FUSED):
    def whole(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    print("| graph | dim | c | call | (AX)W us | AUTO us | fused us | fused / (AX)W | fused / AUTO | (AX)W MB | fused MB |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for name, dim, c in shapes:
        a = (flex_amd.csv_load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "pubmed.csv"))
             if name == "pubmed" else flex_amd.synth_graph(name))
        root = 2 * dim * flex_amd.axw.lib().flex_axw_ld_bf16(c) * 2 <= 128 * 1024  # [W; R] fits beside a tile
        h = axw.Axw(a, dim, c, bf16=True, root=root, fused=True)
        X = (torch.rand((a.n, dim), device="cuda") * 2 - 1).bfloat16()
        W, R = ((torch.rand((dim, c), device="cuda") - 0.5).bfloat16() for _ in range(2))
        bias = torch.rand(c, device="cuda") - 0.5
        nnz = int(a.rowPtr[-1])
        # at the least: every nonzero's X row, column and value once, Out once; the unfused order writes and reads T = A X as well;
        # the root forms read X once more
        least = nnz * (2 * dim + 8) + a.n * h.ld * 2
        calls = {"run": (lambda o: h.run(X, W, o), 0)}
        if root:
            calls["run_root_act p=0.5"] = (lambda o: h.run_root_act(X, W, R, bias, 0.5, 7, o), a.n * dim * 2)
        for what, (f, extra) in calls.items():
            orders = (axw.FLEX_AXW_AX_W, axw.FLEX_AXW_AUTO, axw.FLEX_AXW_AX_W_FUSED)
            t = {o: [] for o in orders}
            for i in range(REPS + 5):  # alternated; the first five of each are warm-up
                for o in orders:
                    us = whole(lambda: f(o))
                    if i >= 5:
                        t[o].append(us)
            m = [float(np.median(t[o])) for o in orders]
            print(f"| {name} | {dim} | {c} | {what} | {m[0]:.1f} | {m[1]:.1f} | {m[2]:.1f} | {m[2] / m[0]:.2f} | {m[2] / m[1]:.2f} | "
                  f"{(least + extra + 2 * a.n * dim * 2) / 1e6:.1f} | {(least + extra) / 1e6:.1f} |", flush=True)
        h.destroy()


if "--bf16-fused" in sys.argv[1:]:
    fused_table()
    sys.exit(0)

if "--bf16-root-act" in sys.argv[1:]:
    root_act_table()
    sys.exit(0)

if "--bf16-root-backward" in sys.argv[1:]:
    root_backward_table()
    sys.exit(0)

if "--bf16-root" in sys.argv[1:]:
    root_table()
    sys.exit(0)

if "--bf16-wide" in sys.argv[1:]:
    bf16_table(WIDE, (axw.FLEX_AXW_A_XW,))
    backward_table(WIDE)
    sys.exit(0)

if "--bf16-backward" in sys.argv[1:]:
    backward_table()
    sys.exit(0)

if "--bf16" in sys.argv[1:]:
    bf16_table()
    cancellation()
    subnormals()
    sys.exit(0)

name, dim, c = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
a = flex_amd.synth_graph(name)
h = axw.Axw(a, dim, c)
X = torch.rand((a.n, dim), device="cuda") * 2 - 1
W = torch.rand((dim, c), device="cuda")
for order in (axw.FLEX_AXW_A_XW, axw.FLEX_AXW_AX_W):
    best = (1e9, 1e9)
    for _ in range(15):
        _, (g, s) = h.run(X, W, order, timed=True)
        best = min(best, (g, s))
    print(f"{name} dim={dim} c={c} order={order}: gemm {best[0]*1e3:7.1f} us  spmm {best[1]*1e3:7.1f} us", flush=True)

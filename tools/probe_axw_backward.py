#!/usr/bin/env python3
"""The backward pass of the A*X*W layer, stage by stage: device-event medians, the paths alternated round by round.

  forward (flex_axw_run, AUTO order) | G = A^T dOut (the transposed plan) | dGradX = G W^T | dGradW = X^T G (the MFMA kernel) |
  dGradW on rocBLAS (same operands) | the whole flex_axw_backward
on the flickr and reddit stand-ins at dim = 128, c in {100, 128}, and the transposed against the forward SpMM on the epinions stand-in.
Usage: probe_axw_backward.py [graph ...]   (default: flickr reddit)"""
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flex_amd  # noqa: E402
from flex_amd import axw  # noqa: E402

ROUNDS, REPS = 15, 5


def median_us(fns):
    """{name: median over ROUNDS of the mean of REPS back-to-back calls}, the functions taken in turn every round."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = {k: [] for k in fns}
    for f in fns.values():
        f()
    for _ in range(ROUNDS):
        for k, f in fns.items():
            ev[0].record()
            for _ in range(REPS):
                f()
            ev[1].record()
            ev[1].synchronize()
            out[k].append(ev[0].elapsed_time(ev[1]) * 1e3 / REPS)
    return {k: statistics.median(v) for k, v in out.items()}


def layer(name, dim, c):
    a = flex_amd.synth_graph(name)
    L = axw.lib()
    h = axw.Axw(a, dim, c, backward=True)
    hb = axw.Axw(a, dim, c, order=flex_amd.FLEX_ORDER_CLUSTER | axw.FLEX_AXW_USE_BLAS, backward=True)
    X = torch.rand((a.n, dim), device="cuda") * 2 - 1
    W = torch.rand((dim, c), device="cuda") * 2 - 1
    dOut = torch.rand((a.n, h.ld), device="cuda") * 2 - 1
    out = torch.empty((a.n, h.ld), device="cuda")
    gx = torch.empty((a.n, dim), device="cuda")
    gw = torch.empty((dim, c), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    pt = flex_amd.Plan(a, c, order=flex_amd.FLEX_ORDER_CLUSTER, ldb=h.ld, ldc=h.ld, transpose=True)
    G = torch.zeros((a.n, h.ld), device="cuda")
    pt.spmm(dOut.data_ptr(), G.data_ptr(), s)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    slices = L.flex_axw_dw_slices(a.n, n_cus)
    part = torch.empty((slices * dim * c,), device="cuda")
    Wt = torch.zeros((h.ld, dim), device="cuda")
    Wt[:c] = W.t()
    ok = lambda rc: rc == 0 or sys.exit(f"call failed: {rc}")  # noqa: E731
    fns = {
        "forward": lambda: ok(L.flex_axw_run(h._h, 0, X.data_ptr(), W.data_ptr(), out.data_ptr(), s, None, None)),
        "G=A^T dOut": lambda: pt.spmm(dOut.data_ptr(), G.data_ptr(), s),
        "dX=G W^T": lambda: ok(L.flex_axw_gemm_launch(G.data_ptr(), Wt.data_ptr(), gx.data_ptr(), a.n, h.ld, dim, dim, n_cus, s)),
        "dW=X^T G": lambda: ok(L.flex_axw_dw_launch(X.data_ptr(), G.data_ptr(), gw.data_ptr(), part.data_ptr(), a.n, dim, c, h.ld, n_cus, s)),
        "dW rocBLAS": lambda: ok(L.flex_axw_backward(hb._h, X.data_ptr(), None, dOut.data_ptr(), None, gw.data_ptr(), s)),
        "backward": lambda: ok(L.flex_axw_backward(h._h, X.data_ptr(), W.data_ptr(), dOut.data_ptr(), gx.data_ptr(), gw.data_ptr(), s)),
    }
    r = median_us(fns)
    r["dW rocBLAS"] -= r["G=A^T dOut"]  # that call runs the SpMM too
    flop = 2.0 * a.n * dim * c
    print(f"{name} n={a.n} nnz={a.nnz} dim={dim} c={c}: " + "  ".join(f"{k} {v:.1f} us" for k, v in r.items())
          + f"  | dW kernel {flop / r['dW=X^T G'] / 1e6:.1f} TF/s", flush=True)


def transposed_spmm(name, k=32):
    a = flex_amd.synth_graph(name)
    p, pt = flex_amd.Plan(a, k), flex_amd.Plan(a, k, transpose=True)
    B = torch.rand((a.n, k), device="cuda")
    Bt = torch.rand((a.m, k), device="cuda")
    Cf, Ct = torch.empty((a.m, k), device="cuda"), torch.empty((a.n, k), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    r = median_us({"A B": lambda: p.spmm(B.data_ptr(), Cf.data_ptr(), s), "A^T B": lambda: pt.spmm(Bt.data_ptr(), Ct.data_ptr(), s)})
    print(f"{name} n={a.n} nnz={a.nnz} k={k}: " + "  ".join(f"{k_} {v:.1f} us" for k_, v in r.items()), flush=True)


if __name__ == "__main__":
    axw.lib().flex_axw_dw_slices.argtypes = [C.c_int, C.c_int]
    axw.lib().flex_axw_dw_launch.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p]
    for g in sys.argv[1:] or ["flickr", "reddit"]:
        for c in (100, 128):
            layer(g, 128, c)
    transposed_spmm("soc-sign-epinions")

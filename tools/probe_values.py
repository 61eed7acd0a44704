#!/usr/bin/env python3
"""Learnable edge values (FLEX_PLAN_MUTABLE_VALUES), timed on one plan: flex_plan_set_values, flex_sddmm and flex_spmm of the same
mutable plan, the SpMM of the plan made without the flag (what the flag costs), and a torch SDDMM (index_select of both row sets,
multiply, sum) where its two nnz x k temporaries fit in memory.  HIP events on torch's stream, warm-up, best of 3 (tools/_timing.py).

Bytes are computed from counts, every gather counted in full (no reuse, the model of flex_plan_stats.gather_bytes):
  set_values  records x (4 map + 4 copy + 8 record line) + nnz x 4 values   (the pass over the padded runs re-reads what the first
              pass wrote, mostly from the L2: not counted)
  sddmm       nnz x (4k B row + 8 record + 4 map + 4 out) + m x 4k G rows   (the 16-byte work items: not counted)
  spmm        nnz x 4k B row + records x 8 + m x 4k C rows
and the refresh is set against the copy rate of flex_hbm_probe.
Usage: probe_values.py [graph ...]   (default: pubmed.csv flickr reddit soc-sign-epinions; k = 32 and 128)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flex_amd  # noqa: E402


def best_us(fn, n, rounds=3, warm=3):
    best = 1e18
    for _ in range(rounds):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / n * 1e3)
    return best


def load(name):
    if name.endswith(".csv"):
        return flex_amd.csv_load(os.path.join(ROOT, "tests", "golden", name))
    return flex_amd.synth_graph(name)


def probe(name, a, k, copy_gbps):
    p = flex_amd.Plan(a, k, mutable_values=True)
    q = flex_amd.Plan(a, k)
    pi, qi = p.info(), q.info()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(k)
    B = torch.rand((a.n, k), device="cuda", generator=g) * 2 - 1
    G = torch.rand((a.m, k), device="cuda", generator=g) * 2 - 1
    v = torch.rand(a.nnz, device="cuda", generator=g) * 2 - 1
    out = torch.empty(a.nnz, device="cuda")
    C = torch.empty((a.m, k), device="cuda")
    n = max(5, min(200, int(2e8 / max(1, a.nnz * k))))
    t_set = best_us(lambda: p.set_values(v), n)
    t_sd = best_us(lambda: p.sddmm_ptr(G.data_ptr(), B.data_ptr(), out.data_ptr(), s), n)
    t_mut = best_us(lambda: p.spmm(B.data_ptr(), C.data_ptr(), s), n)
    t_plain = best_us(lambda: q.spmm(B.data_ptr(), C.data_ptr(), s), n)
    rec, nnz = pi["n_records"], a.nnz
    extra = pi["device_bytes"] - qi["device_bytes"]
    b_set = rec * 16 + nnz * 4
    b_sd = nnz * (4 * k + 16) + a.m * 4 * k
    b_mm = nnz * 4 * k + rec * 8 + a.m * 4 * k
    t_ref = None
    need = 2 * nnz * k * 4 + 2 * nnz * 8
    if need < 0.6 * torch.cuda.mem_get_info()[0]:
        rows = torch.repeat_interleave(torch.arange(a.m, device="cuda"), torch.from_numpy(a.rowPtr.astype("int64")).diff().cuda())
        cols = torch.from_numpy(a.col.astype("int64")).cuda()
        ref = lambda: (G.index_select(0, rows) * B.index_select(0, cols)).sum(1)  # noqa: E731
        t_ref = best_us(ref, max(3, n // 4))
        err = (ref() - out).abs().max().item()
        del rows, cols
    line = (f"{name} m={a.m} nnz={nnz} k={k}: set_values {t_set:.1f} us ({b_set / t_set / 1e3:.0f} GB/s, {100 * b_set / t_set / 1e3 / copy_gbps:.0f} % of copy)"
            f"  sddmm {t_sd:.1f} us ({b_sd / t_sd / 1e3:.0f} GB/s)  spmm {t_mut:.1f} us ({b_mm / t_mut / 1e3:.0f} GB/s)"
            f"  sddmm/spmm {t_sd / t_mut:.2f}  spmm without the flag {t_plain:.1f} us"
            + (f"  torch sddmm {t_ref:.1f} us ({t_ref / t_sd:.1f}x; max |diff| {err:.2g})" if t_ref is not None else "  torch sddmm: does not fit")
            + f"  | extra device bytes {extra} ({extra / max(1, nnz):.2f} per nnz)")
    print(line, flush=True)


def main():
    names = sys.argv[1:] or ["pubmed.csv", "flickr", "reddit", "soc-sign-epinions"]
    hbm = flex_amd.hbm_probe(0, 2048, 10)
    print(f"flex_hbm_probe: read {hbm['read_GBps']:.0f} GB/s, copy {hbm['copy_GBps']:.0f} GB/s", flush=True)
    for name in names:
        a = load(name)
        for k in (32, 128):
            probe(name, a, k, hbm["copy_GBps"])


if __name__ == "__main__":
    main()

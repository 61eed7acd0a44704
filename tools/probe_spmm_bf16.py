#!/usr/bin/env python3
"""flex_spmm_bf16 (FLEX_PLAN_BF16) against flex_spmm on the same graph, order, process and commit, and against the chain
a bf16 caller needs without it (widen B to fp32, flex_spmm, narrow C), with the protocol of DESIGN.md 3.11: the contenders alternate
round by round, best of 3 rounds after warm-up and the spread over the rounds, flex_hbm_probe's copy rate from the same run.  k = 32 and
128 on pubmed.csv and the flickr, reddit and amazon stand-ins (community order, as bench.py's headline).  Appends to
profiles/spmm_bf16_probe.txt.
Usage: probe_spmm_bf16.py [graph ...]   (default: pubmed.csv flickr reddit amazon)"""
import os
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


def probe(name, a, k, copy_gbps):
    order = flex_amd.FLEX_ORDER_CLUSTER
    p32, p16 = flex_amd.Plan(a, k, order=order), flex_amd.Plan(a, k, order=order, bf16=True)
    i32, i16 = p32.info(), p16.info()
    gen = torch.Generator(device="cuda").manual_seed(k)
    B16 = (torch.rand((a.n, k), device="cuda", generator=gen) * 2 - 1).to(torch.bfloat16)
    B32 = B16.float()
    C16 = torch.empty((a.m, k), dtype=torch.bfloat16, device="cuda")
    C32 = torch.empty((a.m, k), device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def chain():  # what a bf16 caller does today: two extra passes over n x k and m x k
        p32.spmm(B16.float().data_ptr(), C32.data_ptr(), s)
        C16.copy_(C32)

    fns = {"flex_spmm fp32": lambda: p32.spmm(B32.data_ptr(), C32.data_ptr(), s),
           "flex_spmm_bf16": lambda: p16.spmm_bf16(B16.data_ptr(), C16.data_ptr(), s),
           "widen + flex_spmm + narrow": chain}
    n = max(5, min(200, int(2e8 / max(1, a.nnz * k))))
    rounds = {key: [] for key in fns}
    for _ in range(3):  # the contenders alternate round by round
        for key, fn in fns.items():
            rounds[key].append(best_us(fn, n, rounds=1))
    best = {key: min(v) for key, v in rounds.items()}
    spread = {key: 100 * (max(v) - min(v)) / min(v) for key, v in rounds.items()}
    # the model of DESIGN.md 8: a launch is its cold nonzeros x the bytes of a B row; all nonzeros x row bytes is its upper end
    rows32, rows16 = a.nnz * 4.0 * k, a.nnz * 2.0 * k
    say(f"{name} n={a.n} nnz={a.nnz} k={k}: tile fp32 G={i32['lanes_per_nz']} bf16 G={i16['lanes_per_nz']}, records {i32['n_records']} / {i16['n_records']}, "
        f"bf16 partials {i16['n_partials']}")
    for key in fns:
        say(f"    {key:28s} {best[key]:9.1f} us  (spread over 3 rounds {spread[key]:.1f} %)")
    say(f"    bf16 / fp32 {best['flex_spmm_bf16'] / best['flex_spmm fp32']:.3f}, bf16 / chain {best['flex_spmm_bf16'] / best['widen + flex_spmm + narrow']:.3f}; "
        f"all nonzeros x row bytes: fp32 {rows32 / best['flex_spmm fp32'] / 1e3:.0f} GB/s, bf16 {rows16 / best['flex_spmm_bf16'] / 1e3:.0f} GB/s "
        f"(copy rate {copy_gbps:.0f} GB/s)")


def main(args):
    torch.cuda.set_device(0)
    hbm = flex_amd.hbm_probe(0, 2048, 10)
    say(f"flex_hbm_probe: read {hbm['read_GBps']:.0f} GB/s, copy {hbm['copy_GBps']:.0f} GB/s")
    for name in args or ["pubmed.csv", "flickr", "reddit", "amazon"]:
        a = load(name)
        for k in (32, 128):
            probe(name, a, k, hbm["copy_GBps"])
    out = os.path.join(ROOT, "profiles", "spmm_bf16_probe.txt")
    with open(out, "a") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])

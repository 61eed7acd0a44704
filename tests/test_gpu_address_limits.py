"""Every SpMM kernel at the 2 and 4 GiB address marks, against the float64 bound of tests/f64ref.py.

B side: one B of 2^22 + 8192 rows x ldb 256 (4.3 GB).  Plans over its first 2^22 rows are the largest with 32-bit B offsets
(n ldb 4 = 2^32 exactly, "top32"), their columns mostly past 2 GiB and up to row 2^22 - 1; plans over all of it are 64-bit ("wide64"),
their columns in the window past 4 GiB together with those columns' aliases c - 2^22, which hold other values.  C side: one C of
2^20 + 4096 rows x ldc 1024 (4.3 GB), B small; the rows of A sit below 2 GiB, past it, and past 4 GiB together with their aliases
r - 2^20.  f64ref.block_map places the scenario's 32-blocks, so dense tiles and hot blocks survive the embedding.

Each operand starts 2 GiB into an allocation whose front is poisoned (NaN in front of B, a sentinel in front of C), and every B row or
C column a case does not use is poisoned too.  So a 32-bit wrap reads another used row or writes another row, a sign-extended offset
reads NaN or writes the guard: the float64 bound, the class check or the guard check fails -- the GPU never faults
(tests/test_kernel_routes.py shows on the CPU that each of these faults fails the checks).  The kernels each route launches are
declared in f64ref.ADDRESS_TABLES and checked on the host simulator there.  C is checked on the device: nothing of 4 GiB is copied."""
import time

import numpy as np
import pytest

import flex_amd
from f64ref import (ADDRESS_TABLES, BIG_LDB, BIG_LDC, C_ROWS, GUARD_BYTES, SCENARIOS, TOP32_N, WIDE64_N, address_case, address_plans,
                    assert_within_f64_bound, block_map)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT = -7.0
GUARD = GUARD_BYTES // 4  # floats in front of the operand
B_FLOATS = GUARD + WIDE64_N * BIG_LDB + 4  # + room for the one-float shift of the unaligned route
C_FLOATS = GUARD + C_ROWS * BIG_LDC
NEED = 16 << 30  # the larger of the two allocations is 6.5 GB; they never coexist


class _Buffers:
    """At most one of the two big allocations at a time: the B side's is freed before the C side's is made."""

    def __init__(self):
        self.kind, self.buf = None, None

    def get(self, kind):
        if self.kind != kind:
            self.buf = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            free, _ = torch.cuda.mem_get_info()
            if free < NEED:
                pytest.skip(f"needs {NEED >> 30} GiB of free HBM, {free >> 30} GiB free")
            self.buf = torch.full((B_FLOATS if kind == "B" else C_FLOATS,), float("nan") if kind == "B" else SENT, device="cuda")
            self.kind = kind
        return self.buf


@pytest.fixture(scope="module")
def bufs():
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    b = _Buffers()
    yield b
    b.buf = None
    torch.cuda.synchronize()
    print(f"\naddress-limit module: {time.time() - t0:.1f} s, peak HBM allocated {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB")
    torch.cuda.empty_cache()


def _route_is_taken(table, route, plans):
    i = plans[0].info()
    if route.startswith("mfma"):
        assert i["n_tiles"] > 0, i
    if route.startswith("bundles"):
        assert i["n_bundles"] > 0, i
    if route.startswith("split"):
        assert i["n_split_rows"] > 0, i
    if route == "two_d":
        assert i["two_d"] == 1, i
    if route.startswith("blocks"):
        assert (i["n_blocks"] > 0) == (table != "wide64"), (table, i)  # 64-bit plans have no hot blocks
    if route.startswith("stamped"):
        assert i["lanes_per_nz"] == ADDRESS_TABLES[table][route]["tuning"]["lanes_per_nz"], i


# ---- B side -------------------------------------------------------------------------------------------------------------------

B_CASES = [(t, r) for t in ("top32", "wide64") for r in ADDRESS_TABLES[t]]


@pytest.mark.parametrize("table,route", B_CASES)
def test_b_side_within_the_float64_bound(bufs, table, route):
    buf = bufs.get("B")
    spec = ADDRESS_TABLES[table][route]
    k = spec["k"]
    n_big = TOP32_N if table == "top32" else WIDE64_N
    assert (n_big * BIG_LDB * 4 <= 1 << 32) == (table == "top32")  # plan_build.cpp: 32-bit B offsets exactly when n ldb 4 <= 2^32
    shift = 1 if spec.get("unaligned") else 0
    Bbig = buf[GUARD + shift:GUARD + shift + WIDE64_N * BIG_LDB].view(WIDE64_N, BIG_LDB)
    stream = torch.cuda.current_stream().cuda_stream
    for name in SCENARIOS:
        a, B, a_big = address_case(table, route, name)
        cols = torch.from_numpy(block_map(a.n, table)).cuda()
        assert int(cols.max()) < n_big
        plans = address_plans(table, route, a_big)
        _route_is_taken(table, route, plans)
        for p in plans:
            p.self_check()
        Bbig[cols, :k] = torch.from_numpy(B).cuda()
        Cbuf = torch.full((a.m * k + 4,), SENT, device="cuda")  # one float of room for the unaligned route
        C = Cbuf[shift:shift + a.m * k]
        try:
            for p in plans:
                dC = C.data_ptr() + 4 * _shard_begin(plans, p) * k  # a row-shard plan writes its rows slice-local
                if spec.get("stamped"):
                    p.measure_imbalance(Bbig.data_ptr(), dC, stream)
                else:
                    p.spmm(Bbig.data_ptr(), dC, stream)
            torch.cuda.synchronize()
            got = C.view(a.m, k).cpu().numpy()
            assert float(Cbuf[shift + a.m * k:].sum()) == SENT * (4 - shift) and (shift == 0 or float(Cbuf[0]) == SENT)
        finally:
            Bbig[cols] = float("nan")  # back to the poison of every unused row
        assert_within_f64_bound(a, B, got, route=f"{table}/{route}/{name}")


def _shard_begin(plans, p):
    """First row of a row-shard plan (the shards tile the rows in order)."""
    r0 = 0
    for q in plans:
        if q is p:
            return r0
        r0 += q.info()["m"]
    raise AssertionError("not a plan of the route")


# ---- C side -------------------------------------------------------------------------------------------------------------------

def _sub_rows(a, rows):
    """The rows `rows` of a as a CSR of their own (the scenario rows a row-shard plan writes)."""
    rp = a.rowPtr.astype(np.int64)
    deg = np.diff(rp)[rows]
    rp2 = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(deg, out=rp2[1:])
    e = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows] + [np.zeros(0, np.int64)])
    return flex_amd.HostCsr(rp2.astype(np.uint32), a.col[e], a.vals[e], n=a.n)


def _count_bad(Cbig, k, lo, hi, chunk=1 << 16):
    """Device counts over C rows [lo, hi): entries of columns < k that are not 0, entries of columns >= k that are not the sentinel."""
    zero_bad = torch.zeros((), dtype=torch.int64, device="cuda")
    sent_bad = torch.zeros((), dtype=torch.int64, device="cuda")
    for r in range(lo, hi, chunk):
        blk = Cbig[r:min(hi, r + chunk)]
        zero_bad += (blk[:, :k] != 0).sum()
        sent_bad += (blk[:, k:] != SENT).sum()
    return zero_bad, sent_bad


def _count_not_sent(x, chunk=1 << 26):
    bad = torch.zeros((), dtype=torch.int64, device="cuda")
    for i in range(0, x.numel(), chunk):
        bad += (x[i:i + chunk] != SENT).sum()
    return bad


@pytest.mark.parametrize("route", list(ADDRESS_TABLES["c_side"]))
def test_c_side_within_the_float64_bound(bufs, route):
    buf = bufs.get("C")
    spec = ADDRESS_TABLES["c_side"][route]
    k = spec["k"]
    Cbig = buf[GUARD:].view(C_ROWS, BIG_LDC)
    lo, hi = spec.get("rows", (0, C_ROWS))
    stream = torch.cuda.current_stream().cuda_stream
    for name in SCENARIOS:
        a, B, a_big = address_case("c_side", route, name)
        rmap = block_map(a.m, "c_side")
        plans = address_plans("c_side", route, a_big)
        _route_is_taken("c_side", route, plans)
        (p,) = plans
        p.self_check()
        buf.fill_(SENT)
        Bd = torch.from_numpy(B).cuda()
        p.spmm(Bd.data_ptr(), Cbig.data_ptr() + 4 * lo * BIG_LDC, stream)
        mine = np.nonzero((rmap >= lo) & (rmap < hi))[0]
        assert len(mine) > 0
        rows_t = torch.from_numpy(rmap[mine]).cuda()
        got = Cbig[rows_t, :k].cpu().numpy()
        Cbig[rows_t, :k] = 0.0  # now every row the plan writes must hold exactly 0 in columns < k
        zero_bad, sent_bad = _count_bad(Cbig, k, lo, hi)
        outside = sum(_count_not_sent(Cbig[r0:r1].reshape(-1)) for r0, r1 in ((0, lo), (hi, C_ROWS)) if r1 > r0)
        guard_bad = _count_not_sent(buf[:GUARD])
        torch.cuda.synchronize()
        where = f"c_side/{route}/{name}"
        assert int(zero_bad) == 0, f"[{where}] {int(zero_bad)} entries of rows without nonzeros are not 0"
        assert int(sent_bad) == 0, f"[{where}] {int(sent_bad)} entries of columns k..ldc-1 changed"
        assert int(outside) == 0, f"[{where}] {int(outside)} entries outside the plan's rows changed"
        assert int(guard_bad) == 0, f"[{where}] {int(guard_bad)} entries of the guard in front of C changed"
        a_mine = a if len(mine) == a.m else _sub_rows(a, mine)
        assert_within_f64_bound(a_mine, B, got, route=where)

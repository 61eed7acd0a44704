"""flex_sddmm, flex_plan_set_values and the edge softmax at the 2 and 4 GiB address marks, against their float64 references.

The sibling of tests/test_gpu_address_limits.py for the kernels of flex::values and flex::softmax; the cases, and the instantiations
each launches, are declared in tests/values_marks.py (CASES below) and checked on the host simulator by tests/test_kernel_routes.py,
which also shows on the CPU that each fault targeted here fails the checks used here.

  B side      one B of 2^22 + 8192 rows x ldb 256: every sddmm_slots<W, OFF32, VEC> on "top32" plans (32-bit byte offsets up to
              2^32 - 1 KiB; most columns past 2 GiB) and on "wide64" plans (column ids; columns past 4 GiB and their aliases c - 2^22).
  G side      one G of 2^20 + 4096 rows x ldc 1024, B small: G rows below 2 GiB, past it, past 4 GiB and their aliases r - 2^20; once
              through a transposed plan.
  entry side  shard plans whose entries start near entry 2^29 (byte 2 GiB) and 2^30 (byte 4 GiB) of the caller's CSR: the softmax
              forward and backward (aligned, one float off, in place), flex_sddmm's out[e], flex_plan_set_values's vals[e].

Every big operand starts 2 GiB into an allocation.  What is read is NaN wherever a case does not use it (the front included), with other
finite values at the aliases; what is written holds a sentinel everywhere, checked on the device after every call.  So a 32-bit wrap or
a sign extension gives a wrong value, a wrong class or a touched sentinel -- never a GPU fault.  One allocation set is alive at a time."""
import os
import time

import numpy as np
import pytest

import flex_amd
from f64ref import BIG_LDB, BIG_LDC, C_ROWS, GUARD_BYTES, TOP32_N, WIDE64_N, assert_within_f64_bound, f64_bound, spmm_f64
from sddmm_ref import _gb, assert_sddmm_within_bound, sddmm64
from softmax_ref import check_backward, check_forward, expected_classes, scores
from values_marks import (ENTRY_ALIAS, ENTRY_K, ENTRY_MARKS, ENTRY_OPS, ENTRY_PLANS, ENTRY_SCALE, SCORE_KINDS, SDDMM_TABLES, VALUE_KINDS,
                          declared_kernels, entry_csr, entry_filler, entry_graph, entry_launch, entry_plan, sddmm_case, sddmm_launch,
                          sddmm_plan)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = {"sddmm": SDDMM_TABLES, "entry": ENTRY_OPS, "kernels": declared_kernels}  # what runs here, for tests/test_kernel_routes.py
SENT = -7.0
GUARD = GUARD_BYTES // 4
B_FLOATS = GUARD + WIDE64_N * BIG_LDB + 4
G_FLOATS = GUARD + C_ROWS * BIG_LDC + 4
E_TAIL = 1 << 16  # floats behind the last entry
E_FLOATS = GUARD + (1 << 30) + (1 << 15) + E_TAIL  # the 4 GiB plans hold fewer than 2^15 entries past the mark
NEED = 24 << 30  # the entry side's three arrays are 19.3 GB
WORST = {}  # part -> worst err / bound


def _worst(part, ratio):
    WORST[part] = max(WORST.get(part, 0.0), float(ratio))


class _Buffers:
    """One allocation set at a time: B (NaN), G (NaN), or the entry side's x, y (NaN) and o (sentinel)."""

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
            nan = float("nan")
            if kind == "E":
                self.buf = tuple(torch.full((E_FLOATS,), f, device="cuda") for f in (nan, nan, SENT))
            else:
                self.buf = torch.full((B_FLOATS if kind == "B" else G_FLOATS,), nan, device="cuda")
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
    print(f"\nvalues address-limit module: {time.time() - t0:.1f} s, peak HBM allocated {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB; "
          f"worst err / bound {', '.join(f'{k} {v:.3g}' for k, v in sorted(WORST.items()))}")
    torch.cuda.empty_cache()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _same_bits(x, y):
    return bool(np.array_equal(np.asarray(x, np.float32).view(np.uint32), np.asarray(y, np.float32).view(np.uint32)))


def _count(x, pred, chunk=1 << 26):
    """Device count of the floats of x for which pred holds, chunked: nothing of 4 GiB is copied or made whole."""
    bad = torch.zeros((), dtype=torch.int64, device="cuda")
    for i in range(0, x.numel(), chunk):
        bad += pred(x[i:i + chunk]).sum()
    return int(bad)


def _not_sent_outside(buf, lo, hi):
    """Floats of buf outside [lo, hi) that do not hold the sentinel (the guard in front and the tail included)."""
    return _count(buf[:lo], lambda t: t != SENT) + _count(buf[hi:], lambda t: t != SENT)


# ---- 1, 2. SDDMM: the B side and the G side ------------------------------------------------------------------------------------------

SDDMM_CASES = [(t, c) for t in ("top32", "wide64", "g_side") for c in SDDMM_TABLES[t]]


@pytest.mark.parametrize("table,case", SDDMM_CASES)
def test_sddmm_at_the_marks_within_the_float64_bound(bufs, table, case):
    g_side = table == "g_side"
    buf = bufs.get("G" if g_side else "B")
    spec = SDDMM_TABLES[table][case]
    k, shift = spec["k"], spec.get("shift", 0)
    a, a_big, rows, cols, big_rows = sddmm_case(table, case)
    if g_side:
        big = buf[GUARD + shift:GUARD + shift + C_ROWS * BIG_LDC].view(C_ROWS, BIG_LDC)
        assert big_rows.max() >= 1 << 20 and ((big_rows >= 1 << 19) & (big_rows < 1 << 20)).any() and (big_rows < 1 << 19).any()
    else:
        n_big = TOP32_N if table == "top32" else WIDE64_N
        assert (n_big * BIG_LDB * 4 <= 1 << 32) == (table == "top32")  # plan_build.cpp: 32-bit B offsets exactly when n ldb 4 <= 2^32
        assert int(big_rows.max()) < n_big
        if table == "top32":
            assert (big_rows >= 1 << 21).mean() > 0.8 and big_rows.max() == TOP32_N - 1
        big = buf[GUARD + shift:GUARD + shift + WIDE64_N * BIG_LDB].view(WIDE64_N, BIG_LDB)
    plan = sddmm_plan(table, case, a_big)
    plan.self_check()
    assert plan.info()["nnz"] == a.nnz
    where_t = torch.from_numpy(big_rows).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    # rows of G and of B: the big operand has one per entry of big_rows; a transposed plan pairs A's columns (G) with A's rows (B)
    mg, nb = (len(big_rows), a.m if spec.get("transposed") else a.n) if g_side else (a.m, len(big_rows))
    base = buf[GUARD:].data_ptr()
    for i, kind in enumerate(VALUE_KINDS):
        G, B = _gb(kind, mg, nb, k, 20 + i)
        ref, T = sddmm64(rows, cols, G, B)
        small = _dev(B if g_side else G)
        big[where_t, :k] = _dev(G if g_side else B)
        out = torch.full((a.nnz + 1,), SENT, device="cuda")
        try:
            runs = []
            for _ in range(2):
                out.fill_(SENT)
                dG, dB = (base, small.data_ptr()) if g_side else (small.data_ptr(), base)
                sddmm_launch(table, case, plan, dG, dB, out.data_ptr(), stream)
                torch.cuda.synchronize()
                runs.append(out.cpu().numpy())
        finally:
            big[where_t] = float("nan")  # back to the poison of every unused row
        what = f"{table}/{case}/{kind}"
        assert runs[0][a.nnz] == SENT, f"[{what}] the float after the last entry changed"
        _worst("sddmm " + table, assert_sddmm_within_bound(runs[0][:a.nnz], ref, T, k, what))
        assert _same_bits(runs[0], runs[1]), f"[{what}] a second run gave other bits"


# ---- 3. the entry side ------------------------------------------------------------------------------------------------------------------

def _host_memory_or_skip(nnz):
    need = 2 * 4 * nnz + (6 << 30)  # the two zero arrays, were they ever touched, and room for the rest
    avail = os.sysconf("SC_AVPHYS_PAGES") * os.sysconf("SC_PAGE_SIZE")
    if avail < need:
        pytest.skip(f"needs {need >> 30} GiB of free host memory, {avail >> 30} GiB available")


def _rss_gib():
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * os.sysconf("SC_PAGE_SIZE") / 2**30


class _Placed:
    """data at entries [e0, e0 + len) of a per-entry array (one float off with shift), other finite values at their aliases e - 2^30 where
    those lie in the array; restore() puts the poison back."""

    def __init__(self, buf, shift, e0, data, alias):
        self.buf, self.fill = buf, float("nan")
        data = np.asarray(data, np.float32)
        self.lo = GUARD + shift + e0
        self.hi = self.lo + len(data)
        buf[self.lo:self.hi] = _dev(data)
        first = max(e0, ENTRY_ALIAS)  # aliases of the entries from 2^30 on
        self.alo, self.ahi = (self.lo - ENTRY_ALIAS + first - e0, self.hi - ENTRY_ALIAS) if e0 + len(data) > first else (0, 0)
        self.alias = _dev(alias[first - e0:]) if self.ahi > self.alo else None
        if self.alias is not None:
            assert self.alo >= GUARD + shift and self.ahi < self.lo
            buf[self.alo:self.ahi] = self.alias

    def untouched_outside(self):
        """Nothing outside the entries changed: NaN everywhere but the aliases, which keep their bits."""
        other = _count(self.buf[:self.lo], lambda t: ~torch.isnan(t)) + _count(self.buf[self.hi:], lambda t: ~torch.isnan(t))
        if self.alias is None:
            return other == 0
        return other == self.ahi - self.alo and bool(torch.equal(self.buf[self.alo:self.ahi].view(torch.int32), self.alias.view(torch.int32)))

    def restore(self):
        self.buf[self.lo:self.hi] = self.fill
        if self.alias is not None:
            self.buf[self.alo:self.ahi] = self.fill


@pytest.mark.parametrize("mark,where", ENTRY_PLANS)
def test_entry_indexed_arrays_at_the_marks(bufs, mark, where):
    g = entry_graph()
    F = entry_filler(g, mark, where)
    _host_memory_or_skip(F + g.nnz)
    xbuf, ybuf, obuf = bufs.get("E")
    rss0 = _rss_gib()
    a_big = entry_csr(g, F)
    e0, e1 = F, F + g.nnz
    assert e0 < ENTRY_MARKS[mark] < e1 and e1 - ENTRY_MARKS[mark] > ENTRY_MARKS[mark] - e0  # most of the shard's entries lie past the mark
    assert GUARD + 1 + e1 + E_TAIL <= E_FLOATS
    t0 = time.time()
    plan = entry_plan(a_big)
    t_plan = time.time() - t0
    rss1 = _rss_gib()
    plan.self_check()
    rp = a_big.rowPtr.astype(np.int64)[1:]  # the shard's row pointer, in entries of the whole CSR
    i = plan.softmax_info()
    assert (i["rows"], i["entries"]) == (g.m, g.nnz), i
    assert (i["rows_empty"], i["rows_packed"], i["rows_wave"], i["rows_block"]) == expected_classes(rp), (i, expected_classes(rp))
    print(f"\nentry side {mark}/{where}: F = {F}, shard plan of {g.nnz} entries behind {F} made in {t_plan:.2f} s "
          f"(info plan_ms {plan.info().get('plan_ms', float('nan')):.0f}); host RSS {rss0:.2f} -> {rss1:.2f} GiB over two zero arrays of {4 * (F + g.nnz) / 2**30:.2f} GiB")
    stream = torch.cuda.current_stream().cuda_stream
    x0, y0, o0 = (b[GUARD:].data_ptr() for b in (xbuf, ybuf, obuf))
    rng = np.random.default_rng([F % 1000, 3])
    other = lambda: rng.uniform(-3, 3, g.nnz).astype(np.float32)  # noqa: E731  what the aliases hold
    G, B = _gb("wide", g.m, g.n, ENTRY_K, 31)
    Gd, Bd = _dev(G), _dev(B)
    C = torch.full((g.m * ENTRY_K + 1,), SENT, device="cuda")
    tag = f"{mark}/{where}"

    def run(op):
        entry_launch(op, plan, x0, y0, o0, Gd.data_ptr(), Bd.data_ptr(), C.data_ptr(), stream)
        torch.cuda.synchronize()

    def output(op, shift):
        """The shard's slice of o after op; everything else of o must still hold the sentinel.  The slice is reset."""
        lo, hi = GUARD + shift + e0, GUARD + shift + e1
        got = obuf[lo:hi].cpu().numpy()
        bad = _not_sent_outside(obuf, lo, hi)
        obuf[lo:hi] = SENT
        assert bad == 0, f"[{tag} {op}] {bad} floats outside the shard's entries changed"
        return got

    for kind in SCORE_KINDS:
        s = scores(kind, rp, seed=41)
        gp = rng.uniform(-2, 2, g.nnz).astype(np.float32)
        ops = [("softmax", "softmax_backward", 0)]
        if kind == SCORE_KINDS[0]:
            ops += [("softmax_unaligned", "softmax_backward_unaligned", 1), ("softmax_in_place", "softmax_backward_in_place", 0)]
        for fwd, bwd, shift in ops:
            in_place = fwd.endswith("in_place")
            ps = _Placed(xbuf, shift, e0, s, other())
            try:
                run(fwd)
                assert ps.untouched_outside(), f"[{tag} {fwd}] the scores outside the shard's entries changed"
                p = xbuf[ps.lo:ps.hi].cpu().numpy() if in_place else output(fwd, shift)
            finally:
                ps.restore()
            assert not in_place or _not_sent_outside(obuf, 0, 0) == 0, f"[{tag} {fwd}] wrote to an array it was not given"
            _worst("softmax forward", check_forward(rp, s, ENTRY_SCALE, p, f"{tag} {fwd} {kind}"))
            pp, pg = _Placed(xbuf, shift, e0, p, other()), _Placed(ybuf, shift, e0, gp, other())
            try:
                run(bwd)
                assert pp.untouched_outside() and pg.untouched_outside(), f"[{tag} {bwd}] p or its gradient changed outside the shard's entries"
                gs = ybuf[pg.lo:pg.hi].cpu().numpy() if in_place else output(bwd, shift)
            finally:
                pp.restore()
                pg.restore()
            assert not in_place or _not_sent_outside(obuf, 0, 0) == 0, f"[{tag} {bwd}] wrote to an array it was not given"
            _worst("softmax backward", check_backward(rp, p, gp, ENTRY_SCALE, gs, f"{tag} {bwd} {kind}"))

    # flex_sddmm: out[e] of the shard's entries, slice-local G rows
    rows = np.repeat(np.arange(g.m, dtype=np.int64), np.diff(g.rowPtr.astype(np.int64)))
    ref, T = sddmm64(rows, g.col.astype(np.int64), G, B)
    run("sddmm")
    _worst("sddmm entry side", assert_sddmm_within_bound(output("sddmm", 0), ref, T, ENTRY_K, f"{tag} sddmm"))

    # flex_plan_set_values from vals[e], then one SpMM with them
    v = (rng.choice([-1.0, 1.0], g.nnz) * np.exp2(rng.uniform(-60, 60, g.nnz))).astype(np.float32)
    pv = _Placed(xbuf, 0, e0, v, other())
    try:
        run("set_values_then_spmm")
        assert pv.untouched_outside()
    finally:
        pv.restore()
    plan.self_check()
    got = C[:g.m * ENTRY_K].view(g.m, ENTRY_K).cpu().numpy()
    assert float(C[g.m * ENTRY_K]) == SENT
    sub = flex_amd.HostCsr(g.rowPtr, g.col, v, n=g.n)
    assert_within_f64_bound(sub, B, got, route=f"{tag} set_values + spmm")
    _worst("set_values + spmm", _spmm_ratio(sub, B, got))
    del plan, a_big


def _spmm_ratio(a, B, C):
    """The worst err / bound of an SpMM result that passed assert_within_f64_bound (for the report)."""
    ref = spmm_f64(a, B)
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        return float(np.where(fin, np.abs(C.astype(np.float64) - ref) / f64_bound(a, B), 0.0).max())

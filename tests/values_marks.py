"""The cases of tests/test_gpu_values_address_limits.py -- flex_sddmm, flex_plan_set_values and the edge softmax at the 2 and 4 GiB
address marks -- with the kernel instantiations each case launches, and numpy models of the faults those cases target.

No GPU is needed to import this module: tests/test_kernel_routes.py launches every case on the host simulator and compares the launch
log with the declaration, asserts that the declarations cover every kernel of flex::values and flex::softmax that libflex_spmm.so
ships, and shows that each fault model fails the checker the GPU test relies on.

Three operand sides (geometry of tests/f64ref.py):
  B side      B is the 2^22 + 8192 rows x ldb 256 buffer: "top32" plans (n = 2^22, records hold 32-bit byte offsets up to 2^32 - 1 KiB) and
              "wide64" plans (records hold column ids, the kernel forms B + size_t(col) ldb).  Every sddmm_slots<W, OFF32, VEC> runs here.
  G side      G is the 2^20 + 4096 rows x ldc 1024 buffer, B small: G rows below 2 GiB, past it, past 4 GiB with their aliases r - 2^20.
  entry side  out[e], vals[e], scores, p and gradients are indexed by entry numbers of the caller's whole CSR.  Row 0 of a host CSR is a
              filler of F entries (zeros that are never written), the rows behind it a test graph; only the shard rows (1, m) is planned,
              so its entries start at F, chosen so that entry 2^29 (byte 2 GiB) or 2^30 (byte 4 GiB) falls inside the shard."""
import numpy as np

from f64ref import BIG_LDB, BIG_LDC, C_MARK4, C_ROWS, TOP32_N, WIDE64_N, block_map, embed_cols, embed_rows, flat, scenario
from flex_amd import HostCsr
from softmax_ref import boundary_graph, long_rows_graph

VALUE_KINDS = ("uniform", "wide", "nonfinite")  # of sddmm_ref._gb


def sddmm(W, off32=True, vec=True):
    """sddmm_slots<W, OFF32, VEC> as `nm -C` prints it."""
    return f"sddmm_slots<{W}, {str(off32).lower()}, {str(vec).lower()}>"


def softmax(vec, bwd):
    return f"edge_softmax_rows<{str(vec).lower()}, {str(bwd).lower()}>"


REFRESH = ["refresh_records", "refresh_padding"]

# ---- SDDMM, B side and G side ------------------------------------------------------------------------------------------------------
# W = sddmm_lanes(k); VEC needs k % 4 == 0 and 16-byte aligned operands ("shift": the big operand starts one float off).
_WK = [(4, 16, 15), (8, 32, 30), (16, 64, 62), (32, 128, 126), (64, 256, 254)]


def _b_cases(o):
    c = {}
    for W, k_vec, k_odd in _WK:
        c[f"w{W}_vec"] = {"k": k_vec, "kernels": [sddmm(W, o, True)]}
        c[f"w{W}_odd_k"] = {"k": k_odd, "kernels": [sddmm(W, o, False)]}
    c["w8_unaligned"] = {"k": 32, "shift": 1, "kernels": [sddmm(8, o, False)]}
    return c


SDDMM_TABLES = {
    "top32": _b_cases(True),
    "wide64": _b_cases(False),
    "g_side": {
        "w8_vec": {"k": 32, "kernels": [sddmm(8, True, True)]},
        "w32_odd_k": {"k": 126, "kernels": [sddmm(32, True, False)]},
        "w16_unaligned": {"k": 64, "shift": 1, "kernels": [sddmm(16, True, False)]},
        "w16_vec_transposed": {"k": 64, "transposed": True, "kernels": [sddmm(16, True, True)]},
    },
}


def sddmm_case(table, case, seed=0):
    """(a, a_big, rows, cols, big_rows): the scenario pattern a, its embedding, and per entry OF THE EMBEDDED CSR the small G row and the
    small B row it pairs (embed_rows reorders the entries); big_rows: where each small row of the big operand sits in it."""
    spec = SDDMM_TABLES[table][case]
    a, _ = scenario("wide", k=spec["k"], m=512, seed=seed)
    if table != "g_side":
        cmap = block_map(a.n, table)
        a_big = embed_cols(a, cmap, TOP32_N if table == "top32" else WIDE64_N)
        rows = np.repeat(np.arange(a.m, dtype=np.int64), np.diff(a.rowPtr.astype(np.int64)))
        return a, a_big, rows, a.col.astype(np.int64), cmap
    if spec.get("transposed"):  # the plan of A^T: G has the rows of A^T (A's columns, embedded), B has A's rows
        cmap = block_map(a.n, "c_side")
        a_big = embed_cols(a, cmap, C_ROWS)
        rows = np.repeat(np.arange(a.m, dtype=np.int64), np.diff(a.rowPtr.astype(np.int64)))
        return a, a_big, a.col.astype(np.int64), rows, cmap
    rmap = block_map(a.m, "c_side")
    a_big = embed_rows(a, rmap, C_ROWS)
    inv = np.full(C_ROWS, -1, np.int64)
    inv[rmap] = np.arange(a.m)
    rows = inv[np.repeat(np.arange(C_ROWS, dtype=np.int64), np.diff(a_big.rowPtr.astype(np.int64)))]
    return a, a_big, rows, a_big.col.astype(np.int64), rmap


def sddmm_plan(table, case, a_big):
    import flex_amd
    spec = SDDMM_TABLES[table][case]
    k = spec["k"]
    if table == "g_side":
        return flex_amd.Plan(a_big, k, ldb=k, ldc=BIG_LDC, transpose=bool(spec.get("transposed")), mutable_values=True)
    return flex_amd.Plan(a_big, k, ldb=BIG_LDB, ldc=k, mutable_values=True)


def sddmm_launch(table, case, plan, dG, dB, dOut, stream=0):
    """flex_sddmm of a case on device pointers of G, B (16-byte aligned, each at its row 0) and out: the big operand of a "shift" case
    starts one float further."""
    off = 4 * SDDMM_TABLES[table][case].get("shift", 0)
    plan.sddmm_ptr(dG + (off if table == "g_side" else 0), dB + (off if table != "g_side" else 0), dOut, stream)


# ---- the entry side ---------------------------------------------------------------------------------------------------------------
ENTRY_K = 32
ENTRY_SCALE = 0.125
ENTRY_MARKS = {"2GiB": 1 << 29, "4GiB": 1 << 30}   # the entry whose byte offset is the mark
ENTRY_ALIAS = 1 << 30                              # entry e - 2^30: what a 32-bit (wrapped or sign-extended) byte offset of e reaches
ENTRY_PLANS = [(mark, where) for mark in ENTRY_MARKS for where in ("packed", "block")]
SCORE_KINDS = ("spread80", "masked30", "poisoned")
# The calls made on every entry-side plan, in this order.  x, y: the per-entry inputs, o: the per-entry output (device pointers of entry
# 0); "shift": every per-entry array of the call starts one float off 16 bytes.
ENTRY_OPS = {
    "softmax": {"kernels": [softmax(True, False)]},
    "softmax_backward": {"kernels": [softmax(True, True)]},
    "softmax_unaligned": {"shift": 1, "kernels": [softmax(False, False)]},
    "softmax_backward_unaligned": {"shift": 1, "kernels": [softmax(False, True)]},
    "softmax_in_place": {"kernels": [softmax(True, False)]},
    "softmax_backward_in_place": {"kernels": [softmax(True, True)]},
    "sddmm": {"kernels": [sddmm(8, True, True)]},
    "set_values_then_spmm": {"kernels": REFRESH + [flat(8)]},
}


def entry_graph():
    """long_rows_graph (packed rows, a wave row, a 2 600- and a 9 000-entry block row) followed by boundary_graph (rows of 256 / 257)."""
    g1, g2 = long_rows_graph(), boundary_graph()
    rp = np.concatenate([g1.rowPtr.astype(np.int64), g1.nnz + g2.rowPtr.astype(np.int64)[1:]])
    return HostCsr(rp.astype(np.uint32), np.concatenate([g1.col, g2.col]), np.concatenate([g1.vals, g2.vals]), n=max(g1.n, g2.n))


def entry_filler(g, mark, where):
    """F such that entry `mark` of the CSR with an F-entry filler row lies strictly inside a packed row near the front of g ("packed":
    the mark is inside that row's packed window) or 1000 entries into g's longest row ("block"); most of g's entries lie past it."""
    rp = g.rowPtr.astype(np.int64)
    deg = np.diff(rp)
    if where == "packed":
        r = int(np.flatnonzero((deg >= 2) & (deg <= 16))[2])
        off = int(rp[r]) + 1
    else:
        r = int(np.argmax(deg))
        off = int(rp[r]) + 1000
    assert rp[r] < off < rp[r + 1] and 2 * off < g.nnz
    F = ENTRY_MARKS.get(mark, mark) - off  # mark: a name of ENTRY_MARKS, or an entry number (small stand-ins on the CPU)
    span = (F + rp[r]) % 4 + deg[r]
    assert (span <= 256) == (where == "packed") and (span > 1024) == (where == "block")
    return F


def entry_csr(g, F):
    """Row 0: F entries (column 0, value 0) in pages that are never written (np.zeros; HostCsr does not copy arrays of its dtypes);
    rows 1 ..: g.  Returns the HostCsr; the shard to plan is rows (1, m)."""
    nnz = F + g.nnz
    assert nnz < 1 << 32
    rp = np.concatenate([[0], F + g.rowPtr.astype(np.int64)]).astype(np.uint32)
    col, vals = np.zeros(nnz, np.uint32), np.zeros(nnz, np.float32)
    col[F:], vals[F:] = g.col, g.vals
    a = HostCsr(rp, col, vals, n=g.n)
    assert a.col is col and a.vals is vals
    return a


def entry_plan(a_big):
    import flex_amd
    return flex_amd.Plan(a_big, ENTRY_K, rows=(1, a_big.m), mutable_values=True)


def entry_launch(op, plan, x, y, o, dG, dB, dC, stream=0):
    """The library calls of ENTRY_OPS[op] on device pointers: x, y, o of entry 0 of the per-entry arrays (16-byte aligned; a "shift" op
    moves all three one float), dG [m - 1, k] slice-local, dB [n, k], dC [m - 1, k]."""
    from flex_amd import binding
    off = 4 * ENTRY_OPS[op].get("shift", 0)
    x, y, o = x + off, y + off, o + off
    if op in ("softmax", "softmax_unaligned"):
        plan.edge_softmax_ptr(x, ENTRY_SCALE, o, stream)
    elif op in ("softmax_backward", "softmax_backward_unaligned"):
        plan.edge_softmax_backward_ptr(x, y, ENTRY_SCALE, o, stream)
    elif op == "softmax_in_place":
        plan.edge_softmax_ptr(x, ENTRY_SCALE, x, stream)
    elif op == "softmax_backward_in_place":
        plan.edge_softmax_backward_ptr(x, y, ENTRY_SCALE, y, stream)
    elif op == "sddmm":
        plan.sddmm_ptr(dG, dB, o, stream)
    elif op == "set_values_then_spmm":
        binding._check(binding._values_fn("flex_plan_set_values")(plan._h, x, stream), "flex_plan_set_values")
        plan.spmm(dB, dC, stream)
    else:
        raise ValueError(op)


def declared_kernels():
    """Every instantiation some case of this module launches."""
    k = {n for cases in SDDMM_TABLES.values() for spec in cases.values() for n in spec["kernels"]}
    return k | {n for spec in ENTRY_OPS.values() for n in spec["kernels"]}


# ---- numpy models of the big arrays and of the faults ---------------------------------------------------------------------------------

class EntryArray:
    """A model of a per-entry device array of the GPU test without its gigabytes: `fill` everywhere (the guard in front, negative
    indices, included), except where values were put."""

    def __init__(self, fill):
        self.fill, self.at = np.float32(fill), {}

    def write(self, idx, vals):
        for i, v in zip(np.asarray(idx, np.int64).tolist(), np.asarray(vals, np.float32)):
            self.at[i] = v

    def read(self, idx):
        return np.array([self.at.get(i, self.fill) for i in np.asarray(idx, np.int64).tolist()], np.float32)

    def changed_outside(self, e0, e1):
        """What the GPU test counts on the device: entries outside [e0, e1) that do not hold the fill."""
        same = lambda v: v == self.fill or (np.isnan(v) and np.isnan(self.fill))  # noqa: E731
        return sum(1 for i, v in self.at.items() if not (e0 <= i < e1) and not same(v))


def alias_entry(e):
    """Where a per-entry access lands if its byte offset 4 e is kept in 32 bits (e >= 2^30 wraps) or sign-extended (e >= 2^29 goes
    negative): entry e - 2^30 in both cases."""
    e = np.asarray(e, np.int64)
    return np.where(e >= 1 << 30, e - ENTRY_ALIAS, e)


def alias_row(r):
    """A G row whose byte offset r ldc 4 is kept in 32 bits: r >= 2^20 reads r - 2^20."""
    r = np.asarray(r, np.int64)
    return np.where(r >= C_MARK4, r - C_MARK4, r)


def sddmm_model(rows_big, cols_big, big_g, big_b, read_g=lambda r: r, read_b=lambda c: c):
    """flex_sddmm of an engine that is exact up to its order, reading the big operands (f64ref.BigB models) through addressing models."""
    G = big_g.rows(read_g(np.asarray(rows_big, np.int64))).astype(np.float64)
    B = big_b.rows(read_b(np.asarray(cols_big, np.int64))).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.einsum("ek,ek->e", G, B).astype(np.float32)

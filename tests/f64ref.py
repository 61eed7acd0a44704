"""A float64 reference of C = A B with an error bound per element, and seeded value scenarios that span the fp32 range.

resCheck (util.assert_matches_oracle) compares against an fp32 CSR-order oracle with a tolerance made for values near 1; it cannot
judge results that cancel, scaled inputs or subnormals.  This module can:

    C64[r, j] = sum_e a_e b_{c_e, j}      in float64 (every product of two fp32 values is exact there, none overflows)
    S[r, j]   = sum_e |a_e| |b_{c_e, j}|
    |C - C64| <= gamma(n_r) S + n_r 2^-149,    gamma(n) = n u / (1 - n u),  u = 2^-24,  n_r = nnz(row r) + P

for every entry whose reference is finite (and C must be finite there), and EXACTLY the reference's class where it is not: NaN where
C64 is NaN, +inf / -inf with the same sign.  Without fp32 overflow that class does not depend on the order of the sum, so every
scenario keeps S < 2^120 over its finite terms (asserted).  The second term is the underflow floor: a rounding in the subnormal range
costs up to half of 2^-149, whatever the magnitudes.

P, the planner's extra roundings.  The engine sums a row as a tree: every record slot of a task runs an fma chain over its records
(one per step, padding records included), the slots meet in a tree of log2(S) levels (S = 64 / lanes_per_nz <= 16 records per step),
the partial sums of a split row's pieces (1-D pieces or 2-D column panels) are added in a last pass, and a dense tile's MFMA sum
meets the vector kernel's in one more addition.  The padding that fills a task's last step splits ONE product into up to
steps - len + 1 exact parts (plan_build.cpp, pad_row), so sum |terms| is still S[r, j]; what it costs is depth.  A term's error is at
most gamma(d) |term| with d the roundings on its path to the result, and for a row of n records in q pieces:
    chain     <= ceil(len_piece / S) <= len_piece   (padding included: a piece's last step holds at most S - 1 of it)
    tree      <= log2(16) = 4
    pieces    <= q, and the q pieces hold n records, so len_piece + q <= n + 1
    product   <= 1 (a product rounded before it is added: the oracle, an MFMA)
    merges    <= 1 (the tile route's sum and the vector kernel's)
so d <= n + 7 on a task.  A row bundle has no tree and no pieces: d <= steps + 1 <= bundle_len + 1 <= 17 (bundle_len <= 16 on every
tile, tests use the rule).  P = 32 covers both with room; the float32 emulation of tests/test_f64_bound.py runs the planner's order
with it."""
import numpy as np

from flex_amd import HostCsr

U = 2.0 ** -24
TINY = 2.0 ** -149     # the smallest fp32 subnormal
P = 32                 # the planner's extra roundings (derivation above)
S_LIMIT = 2.0 ** 120   # finite terms of every scenario stay below this: no fp32 overflow anywhere


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def _row_sum(a, terms):
    """Per-row sums of a (nnz, k) float64 array of terms (rows contiguous as in CSR), IEEE semantics (inf - inf = NaN)."""
    rp = a.rowPtr.astype(np.int64)
    out = np.zeros((a.m, terms.shape[1]), dtype=np.float64)
    nonempty = np.nonzero(np.diff(rp) > 0)[0]
    if len(nonempty):
        with np.errstate(invalid="ignore", over="ignore"):
            out[nonempty] = np.add.reduceat(terms, rp[nonempty], axis=0)
    return out


def spmm_f64(a, B):
    """C = A B in float64 from the fp32 inputs; stored zeros are multiplied like any value (0 x inf = NaN)."""
    B64 = np.asarray(B, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        terms = a.vals.astype(np.float64)[:, None] * B64[a.col.astype(np.int64)]
    return _row_sum(a, terms)


def abs_sum_f64(a, B, finite_only=False):
    """S = |A| |B| in float64; finite_only: non-finite values of A and B count as 0 (the finite terms' magnitude)."""
    av = np.abs(a.vals.astype(np.float64))
    B64 = np.abs(np.asarray(B, dtype=np.float32).astype(np.float64))
    if finite_only:
        av = np.where(np.isfinite(av), av, 0.0)
        B64 = np.where(np.isfinite(B64), B64, 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        terms = av[:, None] * B64[a.col.astype(np.int64)]
    return _row_sum(a, terms)


def f64_bound(a, B, extra=P):
    nr = np.diff(a.rowPtr.astype(np.int64)) + extra
    S = abs_sum_f64(a, B)
    return gamma(nr)[:, None] * S + (nr * TINY)[:, None]


def check_f64_bound(a, B, C, route="", extra=P):
    """None if C passes, else a message naming the worst entry: err / bound, row, column, nnz(row), route."""
    C = np.asarray(C, dtype=np.float32)
    assert C.shape == (a.m, B.shape[1]), (C.shape, a.m, B.shape)
    s_fin = abs_sum_f64(a, B, finite_only=True)
    assert np.all(s_fin < S_LIMIT), f"scenario leaves the checked range: max S over finite terms {s_fin.max():g} >= 2^120"
    ref = spmm_f64(a, B)
    deg = np.diff(a.rowPtr.astype(np.int64))
    fin = np.isfinite(ref)
    C64 = C.astype(np.float64)
    # non-finite reference: exactly the same class
    nan_ref, pinf_ref, ninf_ref = np.isnan(ref), ref == np.inf, ref == -np.inf
    bad_class = (nan_ref & ~np.isnan(C64)) | (pinf_ref & (C64 != np.inf)) | (ninf_ref & (C64 != -np.inf))
    bad_class |= fin & ~np.isfinite(C64)
    if bad_class.any():
        r, j = np.argwhere(bad_class)[0]
        return (f"[{route}] {int(bad_class.sum())} entries of the wrong class; first at row {r} col {j} (nnz(row) {deg[r]}): "
                f"got {C[r, j]!r}, reference {ref[r, j]!r}")
    bound = f64_bound(a, B, extra)
    with np.errstate(invalid="ignore"):
        ratio = np.where(fin, np.abs(C64 - ref) / bound, 0.0)
    if ratio.size and ratio.max() > 1.0:
        r, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        return (f"[{route}] {int((ratio > 1).sum())} entries beyond the float64 bound; worst err/bound {ratio[r, j]:.3g} at row {r} "
                f"col {j} (nnz(row) {deg[r]}): got {C[r, j]!r}, reference {ref[r, j]!r}, bound {bound[r, j]:.3g}")
    return None


def assert_within_f64_bound(a, B, C, route="", extra=P):
    msg = check_f64_bound(a, B, C, route, extra)
    assert msg is None, msg


# ---- scenarios --------------------------------------------------------------------------------------------------------------

def _logu(rng, lo, hi, size):
    """Random signs, magnitudes 2^U(lo, hi)."""
    return (rng.choice([-1.0, 1.0], size=size) * np.exp2(rng.uniform(lo, hi, size=size))).astype(np.float32)


def _subnormal(rng, size, min_sig=1 << 10):
    """Random-sign subnormals: integer significand in [min_sig, 2^23) times 2^-149."""
    return (rng.choice([-1.0, 1.0], size=size) * rng.integers(min_sig, 1 << 23, size=size) * TINY).astype(np.float32)


def _pattern(kind, m, rng):
    """(rowPtr int64, col int64, n).  random: ~9 per row, 10 % empty rows, three long rows (split when the tuning cuts rows),
    columns unsorted.  block: 32-row diagonal blocks at fill 0.8 plus two random columns per row (dense tiles for the MFMA
    route, columns with reuse inside a block of rows for the hot-block route)."""
    n = m
    if kind == "random":
        deg = rng.poisson(9, size=m)
        deg[rng.random(m) < 0.1] = 0
        deg[3], deg[m // 5], deg[m - 1] = min(400, n), min(200, n), min(97, n)
        cols = [rng.permutation(n)[:d] for d in deg]
    elif kind == "block":
        cols = []
        for r in range(m):
            b0 = r // 32 * 32
            blk = b0 + np.nonzero(rng.random(min(32, n - b0)) < 0.8)[0]
            noise = rng.integers(0, n, size=2)
            c = np.unique(np.concatenate([blk, noise]))
            cols.append(rng.permutation(c))
    else:
        raise ValueError(kind)
    deg = np.array([len(c) for c in cols], dtype=np.int64)
    rp = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(deg, out=rp[1:])
    col = np.concatenate(cols).astype(np.int64) if rp[-1] else np.zeros(0, np.int64)
    return rp, col, n


def _last_of_rows(rp):
    d = np.diff(rp)
    return rp[1:][d > 0] - 1


def _sc_wide(rng, rp, col, n, k):
    return _logu(rng, -60, 60, rp[-1]), _logu(rng, -30, 30, (n, k))


def _sc_subnormal_A_large_B(rng, rp, col, n, k):
    return _subnormal(rng, rp[-1]), _logu(rng, 90, 110, (n, k))


def _sc_large_A_subnormal_B(rng, rp, col, n, k):
    return _logu(rng, 90, 110, rp[-1]), _subnormal(rng, (n, k))


def _sc_products_underflow(rng, rp, col, n, k):
    return _logu(rng, -80, -60, rp[-1]), _logu(rng, -90, -68, (n, k))


def _sc_huge(rng, rp, col, n, k):
    vals = (rng.choice([-1.0, 1.0], rp[-1]) * rng.uniform(0.5, 1.0, rp[-1]) * 2.0 ** 60).astype(np.float32)
    B = (rng.choice([-1.0, 1.0], (n, k)) * rng.uniform(0.5, 1.0, (n, k))).astype(np.float32)
    a = HostCsr(rp.astype(np.uint32), col.astype(np.uint32), vals, n=n)
    smax = abs_sum_f64(a, B).max()
    if smax > 0:  # scale B by a power of two so that the largest S lands in [2^119, 2^120)
        B = (B.astype(np.float64) * 2.0 ** (119 - int(np.floor(np.log2(smax))))).astype(np.float32)
    return vals, B


def _sc_zeros(rng, rp, col, n, k):
    vals = rng.uniform(-1, 1, rp[-1]).astype(np.float32)
    z = rng.random(rp[-1]) < 0.3
    vals[z] = np.where(rng.random(z.sum()) < 0.5, 0.0, -0.0).astype(np.float32)
    deg = np.diff(rp)
    rows = np.nonzero(deg > 0)[0]
    zero_rows = rows[rng.random(len(rows)) < 0.25]
    for r in zero_rows:  # every stored value zero, some against a non-finite B row
        vals[rp[r]:rp[r + 1]] = np.where(rng.random(deg[r]) < 0.5, 0.0, -0.0)
    B = rng.uniform(-1, 1, (n, k)).astype(np.float32)
    for r in zero_rows[::3]:
        B[col[rp[r + 1] - 1], rng.integers(0, k)] = np.inf
    return vals, B


def _sc_nonfinite_A(rng, rp, col, n, k):
    vals = rng.uniform(-1, 1, rp[-1]).astype(np.float32)
    pick = rng.random(rp[-1]) < 0.04
    last = _last_of_rows(rp)
    pick[last[rng.random(len(last)) < 0.3]] = True  # the record a task's padding is made from
    vals[pick] = rng.choice(np.array([np.inf, -np.inf, np.nan], np.float32), pick.sum())
    return vals, rng.uniform(-1, 1, (n, k)).astype(np.float32)


def _sc_tiny_vs_inf_B(rng, rp, col, n, k):
    vals = rng.uniform(-1, 1, rp[-1]).astype(np.float32)
    B = rng.uniform(-1, 1, (n, k)).astype(np.float32)
    deg = np.diff(rp)
    rows = np.nonzero(deg % 2 == 1)[0]  # odd lengths: never a whole number of steps, so every such task is padded
    rows = rows[rng.random(len(rows)) < 0.3]
    for i, r in enumerate(rows):
        e0, e1 = rp[r], rp[r + 1]
        if i % 2:
            vals[e0:e1] = _subnormal(rng, e1 - e0)
        else:
            vals[e0:e1] = _logu(rng, -122, -118, e1 - e0)
        c = col[e1 - 1]  # the B row of the record the padding is made from
        if i % 3 == 0:
            B[c, :] = np.inf if i % 2 else -np.inf
        else:
            B[c, rng.integers(0, k, size=max(1, k // 4))] = np.inf
    return vals, B


def _sc_inf_A_vs_inf_B(rng, rp, col, n, k):
    vals = rng.uniform(-1, 1, rp[-1]).astype(np.float32)
    B = rng.uniform(-1, 1, (n, k)).astype(np.float32)
    pick = np.zeros(rp[-1], bool)
    last = _last_of_rows(rp)
    pick[last[rng.random(len(last)) < 0.3]] = True
    pick |= rng.random(rp[-1]) < 0.02
    e = np.nonzero(pick)[0]
    vals[e] = rng.choice(np.array([np.inf, -np.inf], np.float32), len(e))
    for i, c in enumerate(col[e][::2]):  # half of them meet an inf in B: whole rows and single entries
        if i % 2:
            B[c, :] = np.inf
        else:
            B[c, rng.integers(0, k)] = -np.inf
    return vals, B


def _sc_nonfinite_B_wide_A(rng, rp, col, n, k):
    vals = _logu(rng, -60, 60, rp[-1])
    B = _logu(rng, -30, 30, (n, k))
    rows = rng.choice(n, size=max(3, n // 20), replace=False)
    for i, c in enumerate(rows):
        if i % 3 == 0:
            B[c, :] = np.inf
        elif i % 3 == 1:
            B[c, rng.integers(0, k)] = np.nan
        else:
            B[c, rng.integers(0, k, size=max(1, k // 3))] = -np.inf
    return vals, B


def _cancel(rng, m, k):
    """Rows of (c, v) + (c + h, -v) pairs over B rows c and c + h that hold the same values, and (c, w) + (c, -w) pairs on one
    column (duplicate columns inside a row); one small leftover term per row, columns unsorted.  Three long rows."""
    n = m - m % 2
    h = n // 2
    deg = rng.poisson(12, size=m)
    deg[rng.random(m) < 0.1] = 0
    deg[3], deg[m // 5], deg[m - 1] = 401, 201, 97
    cols, vals = [], []
    for d in deg:
        c, v = [], []
        for _ in range(d // 2):
            x = float(rng.uniform(-1, 1) * 2.0 ** rng.integers(-10, 11))
            i = int(rng.integers(0, h))
            if rng.random() < 0.25:
                c += [i, i]
            else:
                c += [i, i + h] if rng.random() < 0.5 else [i + h, i]
            v += [x, -x]
        if d % 2:
            c.append(int(rng.integers(0, n)))
            v.append(float(rng.uniform(-1, 1) * 2.0 ** -20))
        perm = rng.permutation(len(c))
        cols.append(np.array(c, np.int64)[perm])
        vals.append(np.array(v, np.float32)[perm])
    B = rng.uniform(-1, 1, (n, k)).astype(np.float32)
    B[h:] = B[:h]
    rp = np.zeros(m + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cols], out=rp[1:])
    return HostCsr(rp.astype(np.uint32), np.concatenate(cols).astype(np.uint32), np.concatenate(vals), n=n), B


def _cancel_block(rng, m, k):
    """"cancel" on the block pattern (dense tiles): B row c + 16 equals B row c in every 32-row block, and a row's entries on two such
    columns get v and -v; the rest small values."""
    rp, col, n = _pattern("block", m - m % 32, rng)
    B = rng.uniform(-1, 1, (n, k)).astype(np.float32)
    for b0 in range(0, n, 32):
        B[b0 + 16:b0 + 32] = B[b0:b0 + 16]
    vals = (rng.uniform(-1, 1, rp[-1]) * 2.0 ** -20).astype(np.float32)
    for r in range(len(rp) - 1):
        pos = {int(c): e for e, c in enumerate(col[rp[r]:rp[r + 1]], start=int(rp[r]))}
        for c, e in pos.items():
            if c % 32 < 16 and c + 16 in pos:
                x = np.float32(rng.uniform(-1, 1) * 2.0 ** rng.integers(-10, 11))
                vals[e], vals[pos[c + 16]] = x, -x
    return HostCsr(rp.astype(np.uint32), col.astype(np.uint32), vals, n=n), B


_VALUES = {
    "wide": _sc_wide,
    "subnormal_A_large_B": _sc_subnormal_A_large_B,
    "large_A_subnormal_B": _sc_large_A_subnormal_B,
    "products_underflow": _sc_products_underflow,
    "huge": _sc_huge,
    "zeros": _sc_zeros,
    "nonfinite_A": _sc_nonfinite_A,
    "tiny_vs_inf_B": _sc_tiny_vs_inf_B,
    "inf_A_vs_inf_B": _sc_inf_A_vs_inf_B,
    "nonfinite_B_wide_A": _sc_nonfinite_B_wide_A,
}
SCENARIOS = ["wide", "subnormal_A_large_B", "large_A_subnormal_B", "products_underflow", "huge", "cancel", "zeros", "nonfinite_A",
             "tiny_vs_inf_B", "inf_A_vs_inf_B", "nonfinite_B_wide_A"]


def scenario(name, k=32, m=512, seed=0, pattern="random"):
    """(HostCsr, B) of the named scenario, seeded; pattern "random" or "block" (ignored by "cancel", which has its own)."""
    rng = np.random.default_rng([seed, SCENARIOS.index(name), k, m])
    if name == "cancel":
        return _cancel(rng, m, k) if pattern == "random" else _cancel_block(rng, m, k)
    rp, col, n = _pattern(pattern, m, rng)
    vals, B = _VALUES[name](rng, rp, col, n, k)
    return HostCsr(rp.astype(np.uint32), col.astype(np.uint32), np.asarray(vals, np.float32), n=n), np.ascontiguousarray(B, np.float32)


def with_uniform_values(a, seed=0):
    """The same sparsity pattern with uniform(-1, 1) values."""
    vals = np.random.default_rng(seed).uniform(-1, 1, a.nnz).astype(np.float32)
    return HostCsr(a.rowPtr, a.col, vals, n=a.n)


# ---- routes -----------------------------------------------------------------------------------------------------------------
# Every way the engine can sum a row, forced by flex_plan_tuning knobs (k picks the column tile; "pattern" the input a route needs:
# dense 32 x 32 tiles for the MFMA route, columns reused inside a block of rows for the hot-block route).  "ld": strided B / C;
# "unaligned": B and C one float off 16-byte alignment (the generic kernels); "mapped": a CSR permuted by RCM planned with its map;
# "shards": three row shards concatenated.
# "kernels": the kernel instantiations every plan of the route launches, in launch order, named as `nm -C` prints them.
# tests/test_kernel_routes.py checks each declaration against the host simulator's launch log, on every scenario, and that every
# SpMM kernel of libflex_spmm.so is declared by some route (here or in tests/test_gpu_address_limits.py).


def flat(G, off32=True, unroll=None, stamped=False):
    """spmm_flat_kernel<G, OFF32, U, waves per workgroup, STAMP>: U = 4 on G <= 16, 8 on G >= 32, unless the unroll knob asks for 8."""
    U = unroll or (4 if G <= 16 else 8)
    return f"spmm_flat_kernel<{G}, {str(off32).lower()}, {U}, 4, {str(stamped).lower()}>"


def generic(off32=True):
    return f"spmm_generic_kernel<{str(off32).lower()}>"


def tile(off32=True):
    return f"spmm_tile_kernel<{str(off32).lower()}>"


def hot(rounds, vec4=True):
    return f"spmm_hot_kernel<{rounds}>" if vec4 else f"spmm_hot_generic_kernel<{rounds}>"


FIXUP = "spmm_fixup_kernel"
SPLIT = {"long_row": 24, "piece_records": 16}
ROUTES = {
    "flat_g4": {"k": 16, "tuning": {"lanes_per_nz": 4, "bundle": 2}, "kernels": [flat(4)]},
    "flat_g8": {"k": 32, "tuning": {"lanes_per_nz": 8, "bundle": 2}, "kernels": [flat(8)]},
    "flat_g16": {"k": 64, "tuning": {"lanes_per_nz": 16, "bundle": 2}, "kernels": [flat(16)]},
    "flat_g32": {"k": 128, "tuning": {"lanes_per_nz": 32}, "kernels": [flat(32)]},
    "flat_g64": {"k": 256, "tuning": {"lanes_per_nz": 64}, "kernels": [flat(64)]},
    "generic_odd_k": {"k": 7, "tuning": {}, "kernels": [generic(), FIXUP]},
    "generic_unaligned": {"k": 32, "tuning": {}, "unaligned": True, "kernels": [generic(), FIXUP]},
    "bundles_g4": {"k": 16, "tuning": {"lanes_per_nz": 4, "bundle": 1}, "kernels": [flat(4)]},
    "bundles_g8": {"k": 32, "tuning": {"lanes_per_nz": 8, "bundle": 1}, "kernels": [flat(8)]},
    "bundles_g16": {"k": 64, "tuning": {"lanes_per_nz": 16, "bundle": 1}, "kernels": [flat(16)]},
    "split_rows1": {"k": 32, "tuning": dict(SPLIT, split_rows=1, bundle=2), "kernels": [flat(8)]},
    "split_rows2": {"k": 32, "tuning": dict(SPLIT, split_rows=2, bundle=1), "kernels": [flat(8), FIXUP]},
    "split_g4": {"k": 12, "tuning": dict(SPLIT, split_rows=2, lanes_per_nz=4), "kernels": [flat(4), FIXUP]},
    "two_d": {"k": 32, "tuning": {"two_d": 1, "panel_kb": 1}, "kernels": [flat(8)]},
    "far_first": {"k": 32, "tuning": {"far_first": 8}, "kernels": [flat(8)]},
    "order_cluster": {"k": 32, "tuning": {}, "order": 2, "kernels": [flat(8)]},
    "order_rcm": {"k": 64, "tuning": dict(SPLIT), "order": 1, "kernels": [flat(16)]},
    "mapped": {"k": 32, "tuning": {}, "mapped": True, "kernels": [flat(8)]},
    "shards": {"k": 32, "tuning": dict(SPLIT), "shards": 3, "kernels": [flat(8)]},
    "strided": {"k": 20, "tuning": {}, "ld": (28, 24), "kernels": [flat(8)]},
    "mfma": {"k": 32, "tuning": {"mfma": 1, "mfma_fill_pct": 50}, "pattern": "block", "kernels": [flat(8), tile()]},
    "mfma_k100": {"k": 100, "tuning": {"mfma": 1, "mfma_fill_pct": 50}, "pattern": "block", "kernels": [flat(16), tile()]},
    "blocks": {"k": 64, "tuning": {"blocks": 1}, "pattern": "block", "kernels": [flat(16), hot(2)]},  # 2 rounds: the rule on few blocks
    # the other hot-block instantiations: 4 and 8 rounds on the vector kernel, and the generic hot kernel (unaligned operands) at each
    "blocks_r4": {"k": 64, "tuning": {"blocks": 1, "block_rounds": 4}, "pattern": "block", "kernels": [flat(16), hot(4)]},
    "blocks_r8": {"k": 64, "tuning": {"blocks": 1, "block_rounds": 8}, "pattern": "block", "kernels": [flat(16), hot(8)]},
    "blocks_generic_r2": {"k": 64, "tuning": {"blocks": 1, "block_rounds": 2}, "pattern": "block", "unaligned": True,
                          "kernels": [generic(), hot(2, vec4=False)]},
    "blocks_generic_r4": {"k": 64, "tuning": {"blocks": 1, "block_rounds": 4}, "pattern": "block", "unaligned": True,
                          "kernels": [generic(), hot(4, vec4=False)]},
    "blocks_generic_r8": {"k": 64, "tuning": {"blocks": 1, "block_rounds": 8}, "pattern": "block", "unaligned": True,
                          "kernels": [generic(), hot(8, vec4=False)]},
    # launch and grid-decode variants: the grouped 1-D grid (tile_group) with its short last group, the unroll-8 narrow tiles, the
    # dealt XCD stretches, non-temporal record loads with an occupancy throttle; "stamped": through flex_plan_measure_imbalance (the
    # stamped twin of the vector kernel, then the split-row fix-up and the MFMA tiles), which must leave the ordinary result in C.
    # "m": rows of the scenario where 512 does not reach the route: the XCD slices of the grouped grid end in a short group of 3 at
    # these sizes, and stretches are dealt only from 256 chunks on.
    "tile_group_g16": {"k": 128, "tuning": {"lanes_per_nz": 16, "tile_group": 3}, "kernels": [flat(16)]},
    "tile_group_rcm": {"k": 128, "tuning": {"lanes_per_nz": 16, "tile_group": 3}, "order": 1, "m": 448, "kernels": [flat(16)]},
    "tile_group_split": {"k": 128, "tuning": dict(SPLIT, lanes_per_nz=16, tile_group=3, split_rows=1), "m": 640, "kernels": [flat(16)]},
    "unroll8_g8": {"k": 32, "tuning": {"unroll": 8}, "kernels": [flat(8, unroll=8)]},
    "unroll8_g16": {"k": 64, "tuning": {"unroll": 8}, "kernels": [flat(16, unroll=8)]},
    "xcd_dealt": {"k": 32, "tuning": {"xcd_slices": 3, "xcd_stretch": 1}, "m": 2048, "kernels": [flat(8)]},
    "rec_nt_lds": {"k": 64, "tuning": {"rec_nt": 1, "lds_extra": 16384}, "kernels": [flat(16)]},
    "stamped": {"k": 128, "tuning": dict(SPLIT, split_rows=1), "stamped": True, "kernels": [flat(16, stamped=True)]},
    "stamped_g4": {"k": 16, "tuning": dict(SPLIT, lanes_per_nz=4, split_rows=2), "stamped": True, "kernels": [flat(4, stamped=True), FIXUP]},
}

# fake device addresses for the host simulator's launch log: 16-byte aligned, and one float off for the unaligned routes
FAKE_B, FAKE_C = 0x7F0000000000, 0x7F4000000000


def fake_launch(plans, unaligned=False, stamped=False):
    """Launch every plan once on fake operands (host simulator with its launch log on: nothing is read or written)."""
    off = 4 if unaligned else 0
    for p in plans:
        if stamped:
            p.measure_imbalance(FAKE_B + off, FAKE_C + off)
        else:
            p.spmm(FAKE_B + off, FAKE_C + off)


def plan_for_route(route, a):
    """The plan(s) of `route` for `a`: a list (one plan, or one per row shard)."""
    import flex_amd
    spec = ROUTES[route]
    k, tn = spec["k"], spec["tuning"]
    if spec.get("mapped"):
        vo, ap = flex_amd.perm_csr(a, flex_amd.order_rcm(a))
        return [flex_amd.Plan(ap, k, vo_mp=vo, tuning=tn)]
    if spec.get("shards"):
        b = flex_amd.shard_rows(a, k, spec["shards"])
        return [flex_amd.Plan(a, k, rows=(int(b[i]), int(b[i + 1])), tuning=tn) for i in range(spec["shards"])]
    ldb, ldc = spec.get("ld", (None, None))
    return [flex_amd.Plan(a, k, order=spec.get("order", 0), ldb=ldb, ldc=ldc, tuning=tn)]


# ---- the 2 and 4 GiB address marks (tests/test_gpu_address_limits.py) -------------------------------------------------------------
# A scenario's columns (B side) or rows (C side) are embedded into a large operand by a map that keeps every 32-aligned block of 32
# contiguous and 32-aligned, so the "block" pattern still yields dense tiles and hot blocks; the arithmetic does not change, so the result
# is judged against the scenario's own small (a, B).  Everything the map does not use is poisoned (NaN in B, a sentinel in C), and the
# operand sits 2 GiB into an allocation whose front is poisoned too: a wrapped 32-bit offset lands on a used row that holds other values,
# a sign-extended one in the guard in front -- a wrong value or class, never a fault.
#
# B side, ldb = 256 (1 KiB a row): row 2^21 starts at 2 GiB, row 2^22 at 4 GiB.  n = 2^22 is the largest plan with 32-bit B offsets
# (n ldb 4 = 2^32 exactly, plan_build.cpp); n = 2^22 + 8192 makes every plan 64-bit.
# C side, ldc = 1024 (4 KiB a row): row 2^19 starts at 2 GiB, row 2^20 at 4 GiB.
BIG_LDB = 256
TOP32_N = 1 << 22
WIDE64_N = (1 << 22) + 8192
BIG_LDC = 1024
C_MARK2, C_MARK4 = 1 << 19, 1 << 20
C_ROWS = (1 << 20) + 4096
GUARD_BYTES = 1 << 31  # a sign-extended 32-bit byte offset reaches at most 2 GiB below the operand


def _spread(lo, hi, count):
    """count distinct 32-aligned block starts in [lo, hi - 32], the first at lo and the last at hi - 32."""
    s = np.unique(np.linspace(lo // 32, hi // 32 - 1, count).astype(np.int64)) * 32
    assert len(s) == count, (lo, hi, count)
    return s


def block_slots(table, blocks):
    """Where each 32-block of a scenario's columns (B side) or rows (C side) goes, by table:
    top32:  two blocks below the 2 GiB mark (one ends at it), the rest in [2^21, 2^22) up to row 2^22 - 1;
    wide64: half in the window [2^22, 2^22 + 8192) above 4 GiB, the other half on their aliases c - 2^22;
    c_side: a quarter in the window [2^20, 2^20 + 4096) above 4 GiB with the next quarter on their aliases r - 2^20, the rest in
            [2^19, 2^20) (past 2 GiB)."""
    if table == "top32":
        assert blocks >= 4
        return np.concatenate([[0, (1 << 21) - 32], _spread(1 << 21, TOP32_N, blocks - 2)])
    if table == "wide64":
        assert blocks % 2 == 0
        win = _spread(TOP32_N, WIDE64_N, blocks // 2)
        return np.concatenate([win, np.roll(win, 1) - TOP32_N])  # rolled: "cancel" repeats B's first half in its second
    if table == "c_side":
        q = blocks // 4
        win = _spread(C_MARK4, C_ROWS, q)
        return np.concatenate([win, win - C_MARK4, _spread(C_MARK2, C_MARK4, blocks - 2 * q)])
    raise ValueError(table)


def block_map(count, table):
    """index -> big index for `count` scenario columns or rows: 32-block b goes to block_slots(table)[b], order kept inside a block."""
    i = np.arange(count, dtype=np.int64)
    return block_slots(table, -(-count // 32))[i // 32] + i % 32


def embed_cols(a, cmap, n_big):
    """The scenario's A with column c renamed cmap[c], over n_big columns."""
    return HostCsr(a.rowPtr, cmap[a.col.astype(np.int64)].astype(np.uint32), a.vals, n=n_big)


def embed_rows(a, rmap, m_big):
    """The scenario's A with row r moved to row rmap[r] of an m_big-row matrix; every other row empty."""
    rp = a.rowPtr.astype(np.int64)
    deg = np.zeros(m_big, np.int64)
    deg[rmap] = np.diff(rp)
    rp_big = np.zeros(m_big + 1, np.int64)
    np.cumsum(deg, out=rp_big[1:])
    order = np.argsort(rmap)
    e = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in order] + [np.zeros(0, np.int64)])
    return HostCsr(rp_big.astype(np.uint32), a.col[e], a.vals[e], n=a.n)


class BigB:
    """A model of the large B the GPU test builds, without its 4 GiB: row cmap[c] holds B[c], every other row -- and the guard in front
    of row 0 (negative rows) -- holds NaN.  rows(big) returns those rows."""

    def __init__(self, B, cmap):
        self.B, self.cmap = np.asarray(B, np.float32), np.asarray(cmap, np.int64)
        self.where = dict(zip(self.cmap.tolist(), range(len(self.cmap))))

    def rows(self, big):
        small = np.array([self.where.get(int(r), -1) for r in np.asarray(big).ravel()], np.int64)
        out = np.full((len(small), self.B.shape[1]), np.nan, np.float32)
        out[small >= 0] = self.B[small[small >= 0]]
        return out


def spmm_big_b(a_big, big_b, read=lambda c: c):
    """C of the embedded A read through the model, in float64 rounded to fp32 (an engine that is exact up to its order); read: the B row
    an addressing model makes of a column id (identity = right)."""
    col = read(a_big.col.astype(np.int64))
    uniq, inv = np.unique(col, return_inverse=True)
    Bu = big_b.rows(uniq)
    a_u = HostCsr(a_big.rowPtr, inv.astype(np.uint32), a_big.vals, n=len(uniq))
    return spmm_f64(a_u, Bu).astype(np.float32)


def wrap32(c, ldb=BIG_LDB):
    """A 64-bit plan's B row, had the byte offset c ldb 4 been kept in 32 bits: c >= 2^22 reads c - 2^22."""
    return ((np.asarray(c, np.int64) * ldb * 4) & 0xFFFFFFFF) // (ldb * 4)


def sign_extend32(c, ldb=BIG_LDB):
    """A 32-bit plan's B row, had its byte offset been sign-extended: offsets >= 2^31 land up to 2 GiB in front of B (negative rows)."""
    off = np.asarray(c, np.int64) * ldb * 4
    return np.where(off >= 1 << 31, off - (1 << 32), off) // (ldb * 4)


def _b_routes(o):
    """The B-side routes at ldb = 256; o: the plans have 32-bit B offsets (top32) or not (wide64).  "shards": three row shards;
    "stamped": through flex_plan_measure_imbalance; "unaligned": B and C one float off (the generic kernels)."""
    r = {
        "flat_g4": {"k": 16, "tuning": {"lanes_per_nz": 4, "bundle": 2}, "kernels": [flat(4, o)]},
        "flat_g8": {"k": 32, "tuning": {"lanes_per_nz": 8, "bundle": 2}, "kernels": [flat(8, o)]},
        "flat_g16": {"k": 64, "tuning": {"lanes_per_nz": 16, "bundle": 2}, "kernels": [flat(16, o)]},
        "flat_g32": {"k": 128, "tuning": {"lanes_per_nz": 32}, "kernels": [flat(32, o)]},
        "flat_g64": {"k": 256, "tuning": {"lanes_per_nz": 64}, "kernels": [flat(64, o)]},  # k = ldb: the last float4 ends the row
        "unroll8_g8": {"k": 32, "tuning": {"lanes_per_nz": 8, "unroll": 8}, "kernels": [flat(8, o, unroll=8)]},
        "unroll8_g16": {"k": 64, "tuning": {"lanes_per_nz": 16, "unroll": 8}, "kernels": [flat(16, o, unroll=8)]},
        "bundles_g4": {"k": 16, "tuning": {"lanes_per_nz": 4, "bundle": 1}, "kernels": [flat(4, o)]},
        "bundles_g8": {"k": 32, "tuning": {"lanes_per_nz": 8, "bundle": 1}, "kernels": [flat(8, o)]},
        "bundles_g16": {"k": 64, "tuning": {"lanes_per_nz": 16, "bundle": 1}, "kernels": [flat(16, o)]},
        "split_rows1": {"k": 32, "tuning": dict(SPLIT, split_rows=1, bundle=2), "kernels": [flat(8, o)]},
        "split_rows2": {"k": 32, "tuning": dict(SPLIT, split_rows=2, bundle=1), "kernels": [flat(8, o), FIXUP]},
        "generic_odd_k": {"k": 7, "tuning": {}, "kernels": [generic(o), FIXUP]},
        "generic_unaligned": {"k": 32, "tuning": {}, "unaligned": True, "kernels": [generic(o), FIXUP]},
        "two_d": {"k": 32, "tuning": {"two_d": 1, "panel_kb": 1}, "kernels": [flat(8, o)]},
        "tile_group": {"k": 128, "tuning": {"lanes_per_nz": 16, "tile_group": 3}, "kernels": [flat(16, o)]},
        "mfma": {"k": 32, "tuning": {"mfma": 1, "mfma_fill_pct": 50}, "pattern": "block", "kernels": [flat(8, o), tile(o)]},
        "mfma_k100": {"k": 100, "tuning": {"mfma": 1, "mfma_fill_pct": 50}, "pattern": "block", "kernels": [flat(16, o), tile(o)]},
        "shards": {"k": 32, "tuning": dict(SPLIT), "shards": 3, "kernels": [flat(8, o)]},
        "stamped_g4": {"k": 16, "tuning": dict(SPLIT, lanes_per_nz=4, split_rows=2), "stamped": True,
                       "kernels": [flat(4, o, stamped=True), FIXUP]},
        "stamped_g8": {"k": 32, "tuning": dict(SPLIT, lanes_per_nz=8, split_rows=1), "stamped": True, "kernels": [flat(8, o, stamped=True)]},
        "stamped_g16": {"k": 64, "tuning": {"lanes_per_nz": 16}, "stamped": True, "kernels": [flat(16, o, stamped=True)]},
        "stamped_g32": {"k": 128, "tuning": dict(SPLIT, lanes_per_nz=32, split_rows=2), "stamped": True,
                        "kernels": [flat(32, o, stamped=True), FIXUP]},
        "stamped_g64": {"k": 256, "tuning": {"lanes_per_nz": 64}, "stamped": True, "kernels": [flat(64, o, stamped=True)]},
    }
    for rounds in (2, 4, 8):  # hot blocks need 32-bit B offsets: a 64-bit plan must stay flat (and right)
        r[f"blocks_r{rounds}"] = {"k": 64, "tuning": {"blocks": 1, "block_rounds": rounds}, "pattern": "block",
                                  "kernels": [flat(16, o), hot(rounds)] if o else [flat(16, o)]}
    return r


B_TOP32 = _b_routes(True)
B_WIDE64 = _b_routes(False)
# C side: B small (32-bit plans), ldc = 1024, every row of the 2^20 + 4096 planned; "rows": a row shard above the 4 GiB mark
C_ROUTES = {
    "flat_g4": {"k": 16, "tuning": {"lanes_per_nz": 4, "bundle": 2}, "kernels": [flat(4)]},
    "flat_g8": {"k": 32, "tuning": {"lanes_per_nz": 8, "bundle": 2}, "kernels": [flat(8)]},
    "flat_g16": {"k": 64, "tuning": {"lanes_per_nz": 16, "bundle": 2}, "kernels": [flat(16)]},
    "flat_g32": {"k": 128, "tuning": {"lanes_per_nz": 32}, "kernels": [flat(32)]},
    "flat_g64": {"k": 256, "tuning": {"lanes_per_nz": 64}, "kernels": [flat(64)]},
    "bundles_g8": {"k": 32, "tuning": {"lanes_per_nz": 8, "bundle": 1}, "kernels": [flat(8)]},
    "split_rows1": {"k": 32, "tuning": dict(SPLIT, split_rows=1, bundle=2), "kernels": [flat(8)]},
    "split_rows2": {"k": 32, "tuning": dict(SPLIT, split_rows=2, bundle=1), "kernels": [flat(8), FIXUP]},
    "generic_odd_k": {"k": 7, "tuning": {}, "kernels": [generic(), FIXUP]},
    "two_d": {"k": 32, "tuning": {"two_d": 1, "panel_kb": 1}, "kernels": [flat(8)]},
    "mfma": {"k": 32, "tuning": {"mfma": 1, "mfma_fill_pct": 50}, "pattern": "block", "kernels": [flat(8), tile()]},
    "blocks": {"k": 64, "tuning": {"blocks": 1}, "pattern": "block", "kernels": [flat(16), hot(8)]},  # 8 rounds: the rule on 2^20 rows
    "rows_above_4GiB": {"k": 64, "tuning": {}, "rows": (C_MARK4, C_ROWS), "kernels": [flat(16)]},
}
ADDRESS_TABLES = {"top32": B_TOP32, "wide64": B_WIDE64, "c_side": C_ROUTES}


def address_case(table, route, name, seed=0):
    """(small a, B, big A) of scenario `name` for a route of an address table: the scenario's columns embedded into the 4 GiB B (B side),
    or its rows into the 4 GiB C (c_side)."""
    spec = ADDRESS_TABLES[table][route]
    a, B = scenario(name, k=spec["k"], m=512, seed=seed, pattern=spec.get("pattern", "random"))
    if table == "c_side":
        return a, B, embed_rows(a, block_map(a.m, table), C_ROWS)
    return a, B, embed_cols(a, block_map(a.n, table), TOP32_N if table == "top32" else WIDE64_N)


def address_plans(table, route, a_big):
    """The plans of an address-table route for the embedded A."""
    import flex_amd
    spec = ADDRESS_TABLES[table][route]
    k, tn = spec["k"], spec["tuning"]
    if table == "c_side":
        rows = spec.get("rows")
        return [flex_amd.Plan(a_big, k, ldb=k, ldc=BIG_LDC, rows=rows, tuning=tn)]
    if spec.get("shards"):
        b = flex_amd.shard_rows(a_big, k, spec["shards"])
        return [flex_amd.Plan(a_big, k, rows=(int(b[i]), int(b[i + 1])), ldb=BIG_LDB, ldc=k, tuning=tn) for i in range(spec["shards"])]
    return [flex_amd.Plan(a_big, k, ldb=BIG_LDB, ldc=k, tuning=tn)]


# ---- A*X*W (libflex_axw.so) -----------------------------------------------------------------------------------------------------
# Out = A X W in either association order (include/flex_axw.h).  The float64 reference follows the order of the call, since non-finite
# classes can differ between the orders: X[s,k] = 0 against W[k,j] = inf gives NaN in A (X W), and +-inf in (A X) W when another neighbour
# of the row carries a nonzero in column k.  The bound composes flex_spmm's with that of a length-dim dot product:
#
#   GEMM   Y = fl(L W):    |Y - L W| <= gamma(dim) |L||W| + dim 2^-149    (an fp32 dot product of dim terms, fma or mul + add, in any
#                                                                          order; each rounding in the subnormal range costs < 2^-149)
#   SpMM   C = fl(A B):    |C - A B| <= gamma(n_r) |A||B| + n_r 2^-149,   n_r = nnz(row r) + P   (above)
#
# A (X W): |Out - A X W| <= |A| |Y - X W| + |fl(A Y) - A Y|
#                         <= gamma(dim) S + dim 2^-149 sum_s |A_rs| + gamma(n_r) |A| |Y| + n_r 2^-149,
#          and |A||Y| <= (1 + gamma(dim)) S + dim 2^-149 sum_s |A_rs|, with S = |A| (|X| |W|), so
#          |Out - ref| <= (gamma(n_r) + gamma(dim) + gamma(n_r) gamma(dim)) S + 2^-149 (n_r + dim (1 + gamma(n_r)) sum_s |A_rs|).
# (A X) W: the same with the stages swapped: (gamma(n_r) + gamma(dim) + gamma(n_r) gamma(dim)) S + 2^-149 (dim + n_r (1 + gamma(dim)) sum_k |W_kj|).
# gamma(a) + gamma(b) + gamma(a) gamma(b) <= gamma(a + b), and (1 + gamma) <= 2 while every n u < 1/2, so both are covered by
#
#   |Out - ref| <= gamma(n_r + dim) S + 2^-149 (n_r + dim) (1 + sum_s |A_rs| + sum_k |W_kj|)
#
# for every entry whose reference is finite; every other entry must be of exactly the reference's class.  Two range guards keep that
# class argument sound, and the checker asserts both, as S_LIMIT above: every stage's sum of finite |terms| stays below 2^120 (no fp32
# overflow), and no finite intermediate of the first stage that fp32 may round to zero or to the other sign -- nonzero terms and
# |Y64| <= its stage bound, or |Y64| < 2^-126 -- meets an inf or NaN operand of the second stage (fp32 would give inf x 0 = NaN or an inf
# of the other sign there without being wrong).  The padding columns c .. cp-1 of Out must be +0.0 bit for bit.

NORMAL_MIN = 2.0 ** -126


def gemm_f64(L, W):
    """L @ W in float64 by an explicit multiply-add over k, so 0 x inf = NaN is kept (a BLAS dgemm may skip zero operands).  fp32 inputs
    give exact products."""
    L, W = np.asarray(L, np.float64), np.asarray(W, np.float64)
    out = np.zeros((L.shape[0], W.shape[1]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(L.shape[1]):
            out += L[:, k, None] * W[None, k, :]
    return out


def spmm64(a, B, absolute=False):
    """A B in float64 with B kept in float64 (an intermediate of the other stage is not rounded to fp32); absolute: |A| |B|.  Rows in
    chunks of about 2^24 terms, so that n = 60 000 at k = 260 fits in memory."""
    B = np.asarray(B, np.float64)
    vals = a.vals.astype(np.float64)
    if absolute:
        vals, B = np.abs(vals), np.abs(B)
    rp = a.rowPtr.astype(np.int64)
    col = a.col.astype(np.int64)
    out = np.zeros((a.m, B.shape[1]), dtype=np.float64)
    step = max(1, (1 << 24) // max(1, B.shape[1]))
    r0 = 0
    while r0 < a.m:
        r1 = int(np.searchsorted(rp, rp[r0] + step, side="right")) - 1
        r1 = min(a.m, max(r1, r0 + 1))
        e0, e1 = rp[r0], rp[r1]
        if e1 > e0:
            with np.errstate(invalid="ignore", over="ignore"):
                terms = vals[e0:e1, None] * B[col[e0:e1]]
            d = np.diff(rp[r0:r1 + 1])
            nonempty = np.nonzero(d > 0)[0]
            with np.errstate(invalid="ignore", over="ignore"):
                out[r0 + nonempty] = np.add.reduceat(terms, (rp[r0:r1] - e0)[nonempty], axis=0)
        r0 = r1
    return out


A_XW, AX_W = 1, 2  # FLEX_AXW_A_XW, FLEX_AXW_AX_W


def axw_f64(a, X, W, order):
    """float64 A (X W) (order A_XW) or (A X) W (order AX_W) of the fp32 inputs: n x c."""
    return spmm64(a, gemm_f64(X, W)) if order == A_XW else gemm_f64(spmm64(a, X), W)


def gemm_bound(L, W):
    """gamma(dim) |L||W| + dim 2^-149: the bound of one fp32 dot product of length dim, per entry."""
    dim = L.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        return gamma(dim) * gemm_f64(np.abs(L), np.abs(W)) + dim * TINY


def axw_bound(a, X, W, extra=P):
    dim = X.shape[1]
    nr = np.diff(a.rowPtr.astype(np.int64)) + extra
    with np.errstate(invalid="ignore", over="ignore"):
        S = spmm64(a, gemm_f64(np.abs(X), np.abs(W)), absolute=True)
        a_sum = spmm64(a, np.ones((a.n, 1)), absolute=True)[:, 0]
        w_sum = np.abs(np.asarray(W, np.float64)).sum(axis=0)
    m = (nr + dim).astype(np.float64)
    return gamma(m)[:, None] * S + TINY * m[:, None] * (1.0 + a_sum[:, None] + w_sum[None, :])


def _finite(x):
    x = np.asarray(x, np.float64)
    return np.where(np.isfinite(x), np.abs(x), 0.0)


def axw_range_guard(a, X, W, order, extra=P):
    """None if (a, X, W) lies in the range where the composed bound and exact classes hold for `order`, else why not."""
    Xf, Wf = _finite(X), _finite(W)
    af = HostCsr(a.rowPtr, a.col, np.where(np.isfinite(a.vals), np.abs(a.vals), 0).astype(np.float32), n=a.n)
    s_xw = gemm_f64(Xf, Wf)
    for what, s in (("|X||W|", s_xw), ("|A||X|", spmm64(af, Xf)), ("|A||X||W|", spmm64(af, s_xw))):
        if s.size and s.max() >= S_LIMIT:
            return f"stage sum {what} reaches {s.max():g} >= 2^120: fp32 may overflow"
    dim = X.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        if order == A_XW:
            inter, s1 = gemm_f64(X, W), gemm_f64(np.abs(X), np.abs(W))
            b1 = gamma(dim) * s1 + dim * TINY
        else:
            inter, s1 = spmm64(a, X), spmm64(a, X, absolute=True)
            nr = (np.diff(a.rowPtr.astype(np.int64)) + extra)[:, None]
            b1 = gamma(nr) * s1 + nr * TINY
        ai = np.abs(inter)
        unsafe = np.isfinite(inter) & (s1 > 0) & ~((ai > b1) & (ai >= NORMAL_MIN))
    if order == A_XW:  # Y[s, :] meets A[r, s]
        bad_s = np.unique(a.col[~np.isfinite(a.vals)].astype(np.int64))
        hit = unsafe[bad_s].any(axis=1) if len(bad_s) else np.zeros(0, bool)
        if hit.any():
            return f"X W row {bad_s[np.argmax(hit)]} holds a value fp32 may flush or flip, and meets an inf / NaN of A"
    else:  # Z[r, k] meets W[k, :]
        bad_k = ~np.isfinite(np.asarray(W, np.float32)).all(axis=1)
        hit = unsafe[:, bad_k]
        if hit.any():
            return f"A X holds {int(hit.sum())} values fp32 may flush or flip that meet an inf / NaN row of W"
    return None


def _class_mismatch(ref, got):
    nan_ref, pinf_ref, ninf_ref = np.isnan(ref), ref == np.inf, ref == -np.inf
    bad = (nan_ref & ~np.isnan(got)) | (pinf_ref & (got != np.inf)) | (ninf_ref & (got != -np.inf))
    return bad | (np.isfinite(ref) & ~np.isfinite(got))


def axw_reference(a, X, W, order, route="", extra=P):
    """(float64 reference, composed bound) of `order`, after asserting the range guards; reusable across runs of one input."""
    guard = axw_range_guard(a, X, W, order, extra)
    assert guard is None, f"[{route}] scenario leaves the checked range: {guard}"
    return axw_f64(a, X, W, order), axw_bound(a, X, W, extra)


def check_axw(a, X, W, Out, order, route="", extra=P, ref=None):
    """None if Out (n x c, or n x cp with the padding columns) passes for `order`, else a message naming the first failure.
    ref: axw_reference(a, X, W, order) if already computed."""
    Out = np.asarray(Out, np.float32)
    c = W.shape[1]
    assert Out.shape[0] == a.m and Out.shape[1] >= c, (Out.shape, a.m, c)
    ref, bound = ref if ref is not None else axw_reference(a, X, W, order, route, extra)
    if Out.shape[1] > c:
        pad = np.ascontiguousarray(Out[:, c:]).view(np.uint32)
        if pad.any():
            r, j = np.argwhere(pad != 0)[0]
            return (f"[{route}] {int((pad != 0).sum())} padding entries are not +0.0; first at row {r} col {c + j}: "
                    f"{Out[r, c + j]!r}")
    got = Out[:, :c].astype(np.float64)
    deg = np.diff(a.rowPtr.astype(np.int64))
    bad = _class_mismatch(ref, got)
    if bad.any():
        r, j = np.argwhere(bad)[0]
        return (f"[{route}] {int(bad.sum())} entries of the wrong class; first at row {r} col {j} (nnz(row) {deg[r]}): "
                f"got {got[r, j]!r}, reference {ref[r, j]!r}")
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        ratio = np.where(fin, np.abs(got - ref) / bound, 0.0)
    if ratio.size and ratio.max() > 1.0:
        r, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        return (f"[{route}] {int((ratio > 1).sum())} entries beyond the composed float64 bound; worst err/bound {ratio[r, j]:.3g} at row "
                f"{r} col {j} (nnz(row) {deg[r]}): got {got[r, j]!r}, reference {ref[r, j]!r}, bound {bound[r, j]:.3g}")
    return None


def assert_axw_within_bound(a, X, W, Out, order, route="", extra=P, ref=None):
    msg = check_axw(a, X, W, Out, order, route, extra, ref)
    assert msg is None, msg


def check_gemm_bound(L, W, Out):
    """None if Out (= L W in fp32, n x c) is within gamma(dim) |L||W| + dim 2^-149 of the float64 product, classes exact; else a message."""
    ref = gemm_f64(L, W)
    got = np.asarray(Out, np.float32).astype(np.float64)
    bad = _class_mismatch(ref, got)
    if bad.any():
        r, j = np.argwhere(bad)[0]
        return f"{int(bad.sum())} entries of the wrong class; first at ({r}, {j}): got {got[r, j]!r}, reference {ref[r, j]!r}"
    with np.errstate(invalid="ignore"):
        ratio = np.where(np.isfinite(ref), np.abs(got - ref) / gemm_bound(L, W), 0.0)
    if ratio.size and ratio.max() > 1.0:
        r, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        return f"entry ({r}, {j}) beyond the GEMM bound: err/bound {ratio[r, j]:.3g}, got {got[r, j]!r}, reference {ref[r, j]!r}"
    return None


# ---- A*X*W value scenarios: (A, X, W), seeded -----------------------------------------------------------------------------------

def _axw_pattern(rng, n):
    """rowPtr, col of an n x n graph: Poisson(6) per row, 10 % empty rows, two long rows; columns unsorted, repeats allowed."""
    deg = rng.poisson(6, size=n)
    deg[rng.random(n) < 0.1] = 0
    deg[n // 3] = min(300, 4 * n)
    deg[n - 1] = min(97, 3 * n)
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=rp[1:])
    return rp, rng.integers(0, n, size=rp[-1]).astype(np.int64)


def _u(rng, lo, hi, size):
    return rng.uniform(lo, hi, size).astype(np.float32)


def _sprinkle(rng, x, frac, values=(np.inf, -np.inf, np.nan)):
    x = x.copy()
    flat = x.reshape(-1)
    pick = rng.random(flat.size) < frac
    if flat.size:
        pick[rng.integers(0, flat.size)] = True  # at least one
    flat[pick] = rng.choice(np.array(values, np.float32), pick.sum())
    return x


def _axw_values(name, rng, nnz, n, dim, c):
    if name == "uniform":
        return _u(rng, -1, 1, nnz), _u(rng, -1, 1, (n, dim)), _u(rng, -1, 1, (dim, c))
    if name == "wide":
        return _logu(rng, -20, 20, nnz), _logu(rng, -30, 30, (n, dim)), _logu(rng, -30, 30, (dim, c))
    if name == "subnormal_X_large_W":  # the products X W are normal: a kernel that flushed X would return 0
        return _u(rng, -1, 1, nnz), _subnormal(rng, (n, dim)), _logu(rng, 90, 110, (dim, c))
    if name == "large_X_subnormal_W":
        return _u(rng, -1, 1, nnz), _logu(rng, 90, 110, (n, dim)), _subnormal(rng, (dim, c))
    if name == "products_underflow":
        return _u(rng, -1, 1, nnz), _logu(rng, -80, -60, (n, dim)), _logu(rng, -90, -68, (dim, c))
    if name == "huge":
        return (_u(rng, 0.5, 1, nnz) * rng.choice([-1, 1], nnz)).astype(np.float32), _u(rng, 0.5, 1, (n, dim)), \
            (_u(rng, 0.5, 1, (dim, c)) * rng.choice([-1, 1], (dim, c))).astype(np.float32)
    if name == "cancel":  # X's columns h.. are its columns ..h, W's rows h.. the negated rows ..h: every k pair cancels exactly
        h = dim // 2
        X = _u(rng, -1, 1, (n, dim))
        X[:, h:2 * h] = X[:, :h]
        W = (_u(rng, -1, 1, (dim, c)) * np.exp2(rng.integers(-10, 11, (dim, c)))).astype(np.float32)
        W[h:2 * h] = -W[:h]
        if dim % 2:
            W[-1] *= np.float32(2.0 ** -20)
        return _u(rng, -1, 1, nnz), X, W
    if name == "zeros":  # stored +-0 in A, zeros in X and W, infs of W against zeros of X; A, X >= 0 so A X never cancels
        vals = _u(rng, 0.5, 1, nnz)
        z = rng.random(nnz) < 0.3
        vals[z] = np.where(rng.random(z.sum()) < 0.5, 0.0, -0.0)
        X = _u(rng, 0, 1, (n, dim))
        X[rng.random((n, dim)) < 0.3] = 0.0
        W = _u(rng, -1, 1, (dim, c))
        W[rng.random((dim, c)) < 0.3] = 0.0
        W = _sprinkle(rng, W, 0.02, (np.inf, -np.inf))
        return vals, X, W
    if name == "nonfinite_X":
        return _u(rng, -1, 1, nnz), _sprinkle(rng, _u(rng, -1, 1, (n, dim)), 0.01), _u(rng, -1, 1, (dim, c))
    if name == "nonfinite_W":  # A >= 0 and X > 0: A X is a sum of positive terms (or exactly 0) where it meets W's infs
        return _u(rng, 0, 1, nnz), _u(rng, 0.5, 1, (n, dim)), _sprinkle(rng, _u(rng, -1, 1, (dim, c)), 0.03)
    if name == "nonfinite_A":  # X, W > 0: X W is positive where it meets A's infs
        return _sprinkle(rng, _u(rng, -1, 1, nnz), 0.04), _u(rng, 0.5, 1, (n, dim)), _u(rng, 0.5, 1, (dim, c))
    raise ValueError(name)


AXW_SCENARIOS = ["uniform", "wide", "subnormal_X_large_W", "large_X_subnormal_W", "products_underflow", "huge", "cancel", "zeros",
                 "nonfinite_X", "nonfinite_W", "nonfinite_A"]


def axw_scenario(name, n, dim, c, seed=0):
    """(HostCsr A [n x n], X [n x dim], W [dim x c]) of the named scenario, seeded."""
    rng = np.random.default_rng([seed, AXW_SCENARIOS.index(name), n, dim, c])
    rp, col = _axw_pattern(rng, n)
    vals, X, W = _axw_values(name, rng, int(rp[-1]), n, dim, c)
    a = HostCsr(rp.astype(np.uint32), col.astype(np.uint32), np.asarray(vals, np.float32), n=n)
    if name == "huge":  # W scaled by a power of two so that the largest stage sum lands in [2^119, 2^120)
        af = HostCsr(a.rowPtr, a.col, np.abs(a.vals), n=n)
        s_xw = gemm_f64(np.abs(X), np.abs(W))
        smax = max(s_xw.max(initial=0), spmm64(af, s_xw).max(initial=0))
        sx = spmm64(af, np.abs(X)).max(initial=0)
        if sx >= 2.0 ** 119:  # |A||X| alone must stay below the limit too
            X = (X * np.float32(2.0 ** (100 - int(np.floor(np.log2(sx)))))).astype(np.float32)
            s_xw = gemm_f64(np.abs(X), np.abs(W))
            smax = max(s_xw.max(initial=0), spmm64(af, s_xw).max(initial=0))
        if smax > 0:
            W = (W.astype(np.float64) * 2.0 ** (119 - int(np.floor(np.log2(smax))))).astype(np.float32)
    return a, np.ascontiguousarray(X, np.float32), np.ascontiguousarray(W, np.float32)

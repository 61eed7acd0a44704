"""Reference, bound, checker and case table of the SpMM on bf16 operands (include/flex_spmm.h: FLEX_PLAN_BF16, flex_spmm_bf16), shared by
tests/test_spmm_bf16_host.py and tests/test_gpu_spmm_bf16.py.

Definition: read every bf16 element of B as the fp32 number it is; with x32 = what flex_spmm's contract allows for that fp32 input,
C = rn_bf16(x32), one rounding.  So with C64 = spmm_f64 and bound32 = f64_bound of tests/f64ref.py on the widened B (|x32 - C64| <= bound32),
    |C - C64| <= bound32 + 2^-8 (|C64| + bound32) + 2^-134
for every entry whose C64 is finite (attention_bf16_ref.bound_bf16: 2^-8 is the unit roundoff of bf16, 2^-134 half its smallest
subnormal).  Classes are check_f64_bound's, exactly: NaN, +inf and -inf where C64 has them and nowhere else -- except that the ROUNDING
may overflow: +-inf of C64's sign counts as finite-within-bound where |C64| + bound32 reaches bf16's largest finite value.  An empty row
is +0 bits.  B is rounded to bf16 before anything else, so the reference sees the kernel's inputs."""
import functools

import numpy as np

import f64ref
from attention_bf16_ref import bound_bf16, f64_to_bf16, from_bf16, rounded, to_bf16  # noqa: F401  (re-exported for the tests)
from flex_amd import HostCsr

BF16_MAX = float(from_bf16(np.array([0x7F7F], np.uint16))[0])


def reference(a, B, extra=f64ref.P):
    """(C64, bound32) of the widened B."""
    return f64ref.spmm_f64(a, B), f64ref.f64_bound(a, B, extra)


def check(a, B, C_bits, route="", extra=f64ref.P, ref=None):
    """(message or None, worst err / bound).  B: fp32 array of bf16 numbers; C_bits: uint16 [m, k]."""
    C_bits = np.asarray(C_bits)
    assert C_bits.dtype == np.uint16 and C_bits.shape == (a.m, B.shape[1]), (C_bits.dtype, C_bits.shape, a.m, B.shape)
    assert np.array_equal(rounded(B).view(np.uint32), np.ascontiguousarray(B, np.float32).view(np.uint32)), "B holds bf16 numbers"
    s_fin = f64ref.abs_sum_f64(a, B, finite_only=True)
    assert np.all(s_fin < f64ref.S_LIMIT), f"scenario leaves the checked range: max S over finite terms {s_fin.max():g} >= 2^120"
    c64, bound32 = ref if ref is not None else reference(a, B, extra)
    deg = np.diff(a.rowPtr.astype(np.int64))
    C = from_bf16(C_bits).astype(np.float64)
    empty = deg == 0
    if np.any(C_bits[empty] != 0):
        r = np.nonzero(empty)[0][np.argwhere(C_bits[empty] != 0)[0][0]]
        return f"[{route}] the empty row {r} is not +0 bits in every column", np.inf
    fin = np.isfinite(c64)
    nan_ref, pinf_ref, ninf_ref = np.isnan(c64), c64 == np.inf, c64 == -np.inf
    bad = (nan_ref & ~np.isnan(C)) | (pinf_ref & (C != np.inf)) | (ninf_ref & (C != -np.inf))
    # a finite reference: finite, or the rounding's own overflow to the infinity of C64's sign
    with np.errstate(invalid="ignore"):
        overflow = fin & np.isinf(C) & (np.sign(C) == np.sign(c64)) & (np.abs(c64) + bound32 >= BF16_MAX)
    bad |= fin & ~np.isfinite(C) & ~overflow
    if bad.any():
        r, j = np.argwhere(bad)[0]
        return (f"[{route}] {int(bad.sum())} entries of the wrong class; first at row {r} col {j} (nnz(row) {deg[r]}): "
                f"got {C[r, j]!r}, reference {c64[r, j]!r}"), np.inf
    judged = fin & ~overflow
    with np.errstate(invalid="ignore", over="ignore"):
        ratio = np.where(judged, np.abs(C - c64) / bound_bf16(np.where(fin, c64, 0.0), bound32), 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        r, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        return (f"[{route}] {int((ratio > 1).sum())} entries beyond the bf16 bound; worst err/bound {ratio[r, j]:.3g} at row {r} col {j} "
                f"(nnz(row) {deg[r]}): got {C[r, j]!r}, reference {c64[r, j]!r}, bound32 {bound32[r, j]:.3g}"), worst
    return None, worst


# ---- graphs ------------------------------------------------------------------------------------------------------------------

def _csr(cols, n):
    deg = np.array([len(c) for c in cols], np.int64)
    rp = np.zeros(len(cols) + 1, np.int64)
    np.cumsum(deg, out=rp[1:])
    col = np.concatenate([np.asarray(c, np.int64) for c in cols] + [np.zeros(0, np.int64)])
    return rp, col, n


def _fixed_degree(rng, m, n, d):
    return _csr([rng.permutation(n)[:d] for _ in range(m)], n)


def _graph(kind, rng):
    """(rowPtr, col, n), the tuning the graph asks for."""
    if kind == "deg3":       # short rows: bundles on the tiles that have them
        return _fixed_degree(rng, 512, 512, 3), {"bundle": 1}
    if kind == "deg40":      # every row a task of its own, several steps per slot
        return _fixed_degree(rng, 512, 512, 40), {"bundle": 2}
    if kind == "long":       # one row of 5 000 nonzeros among short ones: cut into pieces, summed by spmm_fixup_bf16_kernel
        n = 5120
        deg = rng.integers(1, 9, size=512)
        deg[7] = 5000
        return _csr([rng.permutation(n)[:d] for d in deg], n), {}
    if kind == "empty":      # empty rows, the first and the last among them
        deg = rng.integers(1, 12, size=640)
        deg[rng.random(640) < 0.3] = 0
        deg[0] = deg[1] = deg[-1] = 0
        return _csr([rng.permutation(640)[:d] for d in deg], 640), {}
    if kind in ("pack1", "pack2"):  # the f64ref pattern (rows of 400, 200 and 97 entries among ~9), 6-byte records forced on / off
        return f64ref._pattern("random", 512, rng), {"rec_pack": 1 if kind == "pack1" else 2}
    raise ValueError(kind)


GRAPHS = ["deg3", "deg40", "long", "empty", "pack1", "pack2"]
PACK_GRAPHS = ("pack1", "pack2")


def _cancel_values(rng, rp, col, n, k):
    """Every row of B the same vector, A's entries in pairs (x, -x (1 + 2^-12)): S is large, C64 small."""
    nnz = int(rp[-1])
    x = f64ref._logu(rng, -8, 8, nnz)
    vals = x.copy()
    for r in range(len(rp) - 1):
        e0, e1 = int(rp[r]), int(rp[r + 1])
        pairs = (e1 - e0) // 2
        vals[e0 + 1:e0 + 2 * pairs:2] = -(vals[e0:e0 + 2 * pairs:2] * np.float32(1 + 2.0 ** -12))
    B = np.repeat(f64ref._logu(rng, -4, 4, (1, k)), n, axis=0)
    return vals, B


VALUES = {"wide": f64ref._VALUES["wide"], "zeros": f64ref._VALUES["zeros"], "nonfinite_A": f64ref._VALUES["nonfinite_A"],
          "nonfinite_B": f64ref._VALUES["nonfinite_B_wide_A"], "cancel": _cancel_values}
VALUE_NAMES = list(VALUES)

# (k, tuning, lanes_per_nz the plan must report; None: whatever the rule picks): every form of spmm_flat_bf16_kernel with 32-bit
# offsets.  k is in ELEMENTS; a tile is 8 G elements wide.
PAIRS = {
    "k8_g4": (8, {"lanes_per_nz": 4}, 4),              # most lanes of a slot idle
    "k32_g4": (32, {"lanes_per_nz": 4}, 4),
    "k40_g8": (40, {"lanes_per_nz": 8}, 8),            # 20 words on the 32-word tile: lanes past the row's end
    "k64_g8": (64, {"lanes_per_nz": 8}, 8),
    "k128_g16": (128, {"lanes_per_nz": 16}, 16),
    "k256_g32": (256, {"lanes_per_nz": 32}, 32),
    "k512_rule": (512, {}, None),                       # the tile by rule (graphs this small get four tiles of G = 16)
    "k512_g32": (512, {"lanes_per_nz": 32}, 32),        # two tiles of G = 32
    "k512_g64": (512, {"lanes_per_nz": 64}, 64),
    "k256_group": (256, {"lanes_per_nz": 16, "tile_group": 3}, 16),  # two tiles walked group by group
}
CASES = [(p, g) for p in PAIRS for g in GRAPHS]


def values_of(pair, graph):
    """The value scenario of a case: they rotate, so that every pair and every graph meets every scenario."""
    return VALUE_NAMES[(list(PAIRS).index(pair) + GRAPHS.index(graph)) % len(VALUE_NAMES)]


@functools.lru_cache(maxsize=None)
def case(pair, graph, values=None):
    """(a, B, tuning, lanes) of a case; B is rounded to bf16 (an fp32 array of bf16 numbers).  Cached: treat as read-only."""
    k, tn, lanes = PAIRS[pair]
    values = values or values_of(pair, graph)
    rng = np.random.default_rng([17, list(PAIRS).index(pair), GRAPHS.index(graph), VALUE_NAMES.index(values)])
    (rp, col, n), gt = _graph(graph, rng)
    vals, B = VALUES[values](rng, rp, col, n, k)
    a = HostCsr(rp.astype(np.uint32), col.astype(np.uint32), np.asarray(vals, np.float32), n=n)
    return a, rounded(np.ascontiguousarray(B, np.float32)), {**tn, **gt}, lanes


@functools.lru_cache(maxsize=8)
def case_reference(pair, graph, values=None):
    a, B, _, _ = case(pair, graph, values)
    return reference(a, B)

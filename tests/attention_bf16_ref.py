"""bf16 conversions, operands, bound and checkers of the multi-head fused attention on bf16 row operands (include/flex_spmm.h:
flex_attention_bf16, flex_attention_bf16_backward), shared by tests/test_attention_bf16_host.py and tests/test_gpu_attention_bf16.py.

A bf16 is the upper 16 bits of an IEEE float, carried here as uint16.  The operands are multihead_attention_ref.operands rounded to bf16
and widened again, so the float64 reference and the fp32 bounds of multihead_attention_ref see exactly the numbers the kernel reads.  Out,
gQ, gK and gV are rounded once, at their store: for y = rn_bf16(x32), the reference's x64 and its fp32 bound bound32 (|x32 - x64| <= bound32),
    |y - x64| <= bound32 + 2^-8 (|x64| + bound32) + 2^-134
2^-8 being the unit roundoff of bf16 (|rn(x) - x| <= 2^-8 |x| on normal x, and |x32| <= |x64| + bound32) and 2^-134 half its smallest
subnormal (the rounding error below the normal range).  The classes are exact, as in the fp32 checks: +0 rows are +0 bits, NaN where the
reference is NaN and nowhere else, masked p = +0 bit for bit.  P and ds are fp32 and keep the fp32 bounds unchanged."""
import numpy as np

import multihead_attention_ref as mh
from fused_attention_ref import coo

U_BF16, HALF_SUBNORMAL = 2.0 ** -8, 2.0 ** -134


def to_bf16(x):
    """fp32 -> bf16 bits (uint16), round to nearest even, in integer arithmetic; +-inf stays, a NaN stays a NaN (quiet bit set)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def from_bf16(b):
    """bf16 bits -> the fp32 number they are (exact)."""
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def f64_to_bf16(x):
    """float64 -> bf16 bits, rounded ONCE (to nearest, ties to even): the nearest of the rounding through fp32 and its two neighbours."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        best = to_bf16(x.astype(np.float32)).astype(np.int64)
    fin = np.isfinite(x) & ((best & 0x7FFF) < 0x7F80)
    start = best.copy()
    for step in (-1, 1):
        mag = (start & 0x7FFF) + step
        cand = (start & 0x8000) | np.clip(mag, 0, 0x7F7F)
        with np.errstate(invalid="ignore"):
            eb, ec = np.abs(from_bf16(best.astype(np.uint16)).astype(np.float64) - x), np.abs(from_bf16(cand.astype(np.uint16)).astype(np.float64) - x)
        take = fin & (mag >= 0) & (mag <= 0x7F7F) & ((ec < eb) | ((ec == eb) & (cand % 2 == 0) & (best % 2 == 1)))
        best = np.where(take, cand, best)
    return best.astype(np.uint16)


def rounded(x):
    """x (fp32) rounded to bf16 and widened again: an fp32 array that holds bf16 numbers."""
    return from_bf16(to_bf16(x))


def operands(names, a, k, seed=0):
    """multihead_attention_ref.operands rounded to bf16 and widened: (Q, K, V) fp32 arrays of bf16 numbers.  Signs, infinities and NaN
    survive the rounding, so the masks and the poisoned rows of every scenario are the same."""
    return tuple(rounded(x) for x in mh.operands(names, a, k, seed=seed))


def bound_bf16(x64, bound32):
    return bound32 + U_BF16 * (np.abs(x64) + bound32) + HALF_SUBNORMAL


def _bits(x, shape, what):
    x = np.asarray(x)
    assert x.dtype == np.uint16 and x.shape == shape, f"{what}: bf16 bits (uint16) of shape {shape}; got {x.dtype} {x.shape}"
    return x


def check(a, Q, K, V, scale, heads, out_bits, p=None, rows=None, what="", ratios=None):
    """Out (bf16 bits [rows, k]) and, where given, P (fp32 [entries, heads]) against multihead_attention_ref.reference: per head the
    classes exactly (NaN in a poisoned head's d columns and nowhere else, +0 bits on a row without a live entry, non-finite values where
    float64 has them, masked p = +0 bit for bit), Out under the bf16 bound and P under the fp32 bound, on every element.  Returns the
    worst err / bound (ratios, a dict: the worst of "out" and "p")."""
    ref = mh.reference(a, Q, K, V, scale, heads, rows)
    k = Q.shape[1]
    bits = _bits(out_bits, ref["out"].shape, f"{what} Out")
    out = from_bf16(bits)
    row, col, rp = coo(a, rows)
    m = len(rp) - 1
    for h in range(heads):
        c = mh.head_columns(k, heads, h)
        poisoned, live, vfin = np.zeros(m, bool), np.zeros(m, bool), np.ones(m, bool)
        if row.size:
            poisoned[row[np.isnan(ref["p"][:, h])]] = True
            live[row[np.nan_to_num(ref["p"][:, h]) > 0]] = True
            vfin[row[~np.isfinite(np.asarray(V, np.float64)[col][:, c]).all(1)]] = False
        assert np.all(np.isnan(out[poisoned][:, c])), f"{what} head {h}: a row with a +inf or NaN score is not NaN in every column of the head"
        zero = ~poisoned & ~live & vfin
        assert np.all(bits[zero][:, c] == 0), f"{what} head {h}: a row without a live entry is not +0 in every column"
        want, got = ref["out"][~poisoned][:, c], out[~poisoned][:, c]
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), f"{what} head {h}: non-finite values not exactly where float64 has them"
    ok = np.isfinite(ref["out"])
    ratio = np.abs(out[ok].astype(np.float64) - ref["out"][ok]) / bound_bf16(ref["out"][ok], ref["out_bound"][ok])
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} elements of Out beyond the bf16 bound, worst err / bound {worst:.3g}"
    if ratios is not None:
        ratios["out"] = max(worst, ratios.get("out", 0.0))
    if p is not None:
        p = np.asarray(p)
        assert p.dtype == np.float32 and p.shape == ref["p"].shape, f"{what}: P is fp32 [entries, heads], entry-major; got {p.dtype} {p.shape}"
        nan_ref = np.isnan(ref["p"])
        assert np.array_equal(np.isnan(p), nan_ref), f"{what}: P is NaN exactly on the poisoned rows of each head"
        masked = ~nan_ref & (ref["s"] == -np.inf)
        assert np.all(p[masked].view(np.uint32) == 0), f"{what}: a masked entry is not +0 bit for bit"
        r = np.abs(p[~nan_ref].astype(np.float64) - ref["p"][~nan_ref]) / ref["p_bound"][~nan_ref]
        wp = float(r.max()) if r.size else 0.0
        assert wp <= 1.0, f"{what}: {int((r > 1).sum())} entries of P beyond the fp32 bound, worst err / bound {wp:.3g}"
        if ratios is not None:
            ratios["p"] = max(wp, ratios.get("p", 0.0))
        worst = max(worst, wp)
    return worst


def check_backward(a, Q, K, V, p, g, scale, heads, gQ=None, gK=None, gV=None, ds=None, what="", ratios=None):
    """gQ, gK, gV (bf16 bits) and ds (fp32 [nnz, heads]) against multihead_attention_ref.backward_reference on the same p: for every
    output given, +0 bits on rows without entries, NaN and infinities where float64 has them, the bf16 bound on every other element of a
    gradient; ds under the fp32 checker unchanged.  Returns the worst err / bound (ratios: the worst of each output)."""
    ref = mh.backward_reference(a, Q, K, V, np.asarray(p, np.float32), g, scale, heads)
    row, col, rp = coo(a)
    empty = {"gq": np.diff(rp) == 0, "gk": np.bincount(col, minlength=a.n) == 0}
    empty["gv"] = empty["gk"]
    worst = 0.0
    for key, got in (("gq", gQ), ("gk", gK), ("gv", gV)):
        if got is None:
            continue
        want, bound = ref[key], ref[key + "_bound"]
        bits = _bits(got, want.shape, f"{what} {key}")
        got = from_bf16(bits)
        assert np.all(bits[empty[key]] == 0), f"{what}: a row of {key} without entries is not +0 in every column"
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: {key} is NaN where float64 is, and nowhere else ({int((np.isnan(got) != np.isnan(want)).sum())} differ)"
        inf = np.isinf(want)
        assert np.array_equal(got[inf].astype(np.float64), want[inf]) and not np.isinf(got[~inf]).any(), f"{what}: {key}: infinities as float64 gives them"
        fin = np.isfinite(want)
        ratio = np.abs(got[fin].astype(np.float64) - want[fin]) / bound_bf16(want[fin], bound[fin])
        w = float(ratio.max()) if ratio.size else 0.0
        assert w <= 1.0, f"{what}: {int((ratio > 1).sum())} elements of {key} beyond the bf16 bound, worst err / bound {w:.3g}"
        worst = max(worst, w)
        if ratios is not None:
            ratios[key] = max(w, ratios.get(key, 0.0))
    if ds is not None:
        ds = np.asarray(ds)
        assert ds.dtype == np.float32, f"{what}: ds is fp32; got {ds.dtype}"
        worst = max(worst, mh.check_backward(a, Q, K, V, p, g, scale, heads, ds=ds, what=what, ratios=ratios))
    return worst

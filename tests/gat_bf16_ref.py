"""Operands and checkers of the fused GAT attention on bf16 V rows, with and without dropout (include/flex_spmm.h:
flex_gat_attention_bf16, flex_gat_attention_bf16_backward, flex_gat_attention_bf16_dropout, flex_gat_attention_bf16_dropout_backward),
shared by tests/test_gat_bf16_host.py and tests/test_gpu_gat_bf16.py.

Nothing here is new: the operands are gat_attention_ref.operands with V (and the test's g) passed through attention_bf16_ref.rounded and
el, er untouched, so the float64 references and the fp32 bounds of gat_attention_ref / gat_dropout_ref see exactly the numbers the
kernel reads.  Out and gV are bf16 bits (uint16), rounded once at their store: for y = rn_bf16(x32), the reference's x64 and its fp32
bound bound32,
    |y - x64| <= bound32 + 2^-8 (|x64| + bound32) + 2^-134                      (attention_bf16_ref.bound_bf16)
with the classes exact (+0 bits where nothing is summed, NaN in a poisoned head's columns and nowhere else, infinities where float64
has them).  P, dx, gEl and gEr are fp32 and go to the fp32 checkers unchanged.  `drop` is None for the undropped pair and (p, seed) for
the dropout pair."""
import hashlib

import numpy as np

import attention_bf16_ref as bf
import gat_attention_ref as gat
import gat_dropout_ref as gd
from attention_bf16_ref import f64_to_bf16, from_bf16, rounded, to_bf16  # noqa: F401
from attention_dropout_ref import _check_edge, _check_rows
from fused_attention_ref import coo
from multihead_attention_ref import head_columns

SLOPE = gat.SLOPE


def operands(names, a, k, seed=0):
    """(el, er, V): gat_attention_ref.operands with V rounded to bf16 and widened again; el and er as they are."""
    el, er, V = gat.operands(names, a, k, seed=seed)
    return el, er, rounded(V)


# ---- the references: gat_attention_ref's and gat_dropout_ref's, by `drop`

_last = {}


def _once(kind, fn, arrays, values):
    """fn(), or what the last call of this kind returned when it had the same array objects with the same contents and the same
    values: result() and the checker that follows it on the same inputs share one float64 evaluation (seconds at 64 heads).  The
    arrays are held, so no id is reused, and a digest of their bytes is part of the key, so an operand changed in place is evaluated
    again (milliseconds beside the evaluation it saves)."""
    values = values + tuple(hashlib.blake2b(np.ascontiguousarray(x).view(np.uint8), digest_size=16).digest() for x in arrays if isinstance(x, np.ndarray))
    hit = _last.get(kind)
    if hit is not None and len(hit[0]) == len(arrays) and all(x is y for x, y in zip(hit[0], arrays)) and hit[1] == values:
        return hit[2]
    res = fn()
    _last[kind] = (arrays, values, res)
    return res


def reference(a, el, er, V, slope, drop=None, rows=None):
    fn = (lambda: gat.reference(a, el, er, V, slope, rows)) if drop is None else (lambda: gd.reference(a, el, er, V, slope, drop[0], drop[1], rows))
    return _once("forward", fn, (a, el, er, V), (slope, drop, rows))


def backward_reference(a, el, er, V, p, g, slope, drop=None, fault=None):
    if drop is None:
        assert fault is None
        fn = lambda: gat.backward_reference(a, el, er, V, p, g, slope)  # noqa: E731
    else:
        fn = lambda: gd.backward_reference(a, el, er, V, p, g, slope, drop[0], drop[1], fault=fault)  # noqa: E731
    return _once("backward", fn, (a, el, er, V, p, g), (slope, drop, fault))


def _kept(a, heads, drop, rows, entries):
    return np.ones((entries, heads), bool) if drop is None else gd.kept_entries(a, heads, drop[0], drop[1], rows)


# ---- the checkers

def check(a, el, er, V, slope, out_bits, p=None, rows=None, drop=None, what="", ratios=None):
    """Out (bf16 bits [rows, k]) against the float64 reference under the bf16 bound, the classes exact: +0 bits in a head of a row with
    no (kept) live entry where the (kept) V rows are finite, NaN in a poisoned head's columns and nowhere else, infinities where float64
    has them.  P (fp32 [entries, H], the UNDROPPED alpha), where given, under gat_attention_ref's classes and fp32 bound unchanged.
    Returns the worst err / bound (ratios, a dict: the worst of "out" and "p")."""
    ref = reference(a, el, er, V, slope, drop, rows)
    k, heads = V.shape[1], el.shape[1]
    row, col, rp = coo(a, rows)
    m = len(rp) - 1
    kp = _kept(a, heads, drop, rows, len(row))
    zero = np.zeros((m, k), bool)
    V64 = np.asarray(V, np.float64)
    for h in range(heads):
        cs, sel = head_columns(k, heads, h), kp[:, h]
        busy = np.zeros(m, bool)  # a (kept) entry that is live (p > 0 or NaN) or whose V is not finite; a poisoned head, kept or not
        if len(row):
            al = ref["p"][sel, h]
            busy[row[sel][~(al == 0) | ~np.isfinite(V64[col[sel]][:, cs]).all(1)]] = True
            busy[row[np.isnan(ref["p"][:, h])]] = True
        zero[:, cs] = ~busy[:, None]
    worst = _check_rows(out_bits, ref["out"], ref["out_bound"], what, "Out", True, zero_rows=zero)
    if ratios is not None:
        ratios["out"] = max(worst, ratios.get("out", 0.0))
    if p is not None:
        p = np.asarray(p)
        assert p.dtype == np.float32 and p.shape == ref["p"].shape, f"{what}: P is fp32 [entries, heads], entry-major; got {p.dtype} {p.shape}"
        nan_ref = np.isnan(ref["p"])
        assert np.array_equal(np.isnan(p), nan_ref), f"{what}: P is NaN exactly on the poisoned rows of each head"
        masked = ~nan_ref & (ref["s"] == -np.inf)
        assert np.all(p[masked].view(np.uint32) == 0), f"{what}: a masked entry of P is not +0 bit for bit"
        r = np.abs(p[~nan_ref].astype(np.float64) - ref["p"][~nan_ref]) / ref["p_bound"][~nan_ref]
        wp = float(r.max()) if r.size else 0.0
        assert wp <= 1.0, f"{what}: {int((r > 1).sum())} entries of P beyond the fp32 bound, worst err / bound {wp:.3g}"
        if ratios is not None:
            ratios["p"] = max(wp, ratios.get("p", 0.0))
        worst = max(worst, wp)
    return worst


def check_backward(a, el, er, V, p, g, slope, gEl=None, gEr=None, gV=None, dx=None, drop=None, what="", ratios=None):
    """gV (bf16 bits [n, k]) under the bf16 bound with its classes exact (+0 bits in a head of a column without a (kept) entry); gEl,
    gEr and dx (fp32) under the fp32 bounds of gat_attention_ref.backward_reference / gat_dropout_ref.backward_reference unchanged, with
    the classes of their checkers (+0 bits on rows of gEl and of gEr without entries, NaN and infinities where float64 has them).
    Returns the worst err / bound (ratios: the worst of each output)."""
    ref = backward_reference(a, el, er, V, np.asarray(p, np.float32), g, slope, drop)  # one evaluation for the four outputs
    _, col, rp = coo(a)
    k, heads = V.shape[1], el.shape[1]
    kp = _kept(a, heads, drop, None, a.nnz)
    empty_r = np.repeat((np.diff(rp) == 0)[:, None], heads, 1)
    empty_c = np.repeat((np.bincount(col, minlength=a.n) == 0)[:, None], heads, 1)
    none_kept = np.zeros((a.n, k), bool)
    for h in range(heads):
        any_kept = np.zeros(a.n, bool)
        any_kept[col[kp[:, h]]] = True
        none_kept[:, head_columns(k, heads, h)] = ~any_kept[:, None]
    worst = 0.0
    # gat_dropout_ref.check_backward's loop (and, with every entry kept, gat_attention_ref.check_backward's classes), gV as bf16 bits
    for key, got, zero, bf16 in (("gel", gEl, empty_r, False), ("ger", gEr, empty_c, False), ("gv", gV, none_kept, True)):
        if got is not None:
            w = _check_rows(np.asarray(got), ref[key], ref[key + "_bound"], what, key, bf16, zero_rows=zero)
            worst = max(worst, w)
            if ratios is not None:
                ratios[key] = max(w, ratios.get(key, 0.0))
    if dx is not None:
        w = _check_edge(dx, ref["dx"], ref["dx_bound"], what, "dx", (a.nnz, heads))
        worst = max(worst, w)
        if ratios is not None:
            ratios["dx"] = max(w, ratios.get("dx", 0.0))
    return worst


# ---- what a right kernel returns up to roundings, and the faults the checkers must reject

FORWARD_FAULTS = ("out_truncated", "out_rounded_twice", "p_bf16", "el_er_bf16", "poison_spreads")
BACKWARD_FAULTS = ("gv_terms_rounded", "gv_unmasked")
FAULTS = FORWARD_FAULTS + BACKWARD_FAULTS


def _round_bits(x, bits):
    """float64 rounded to `bits` significant bits, to nearest even."""
    m, e = np.frexp(x)
    return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e)


def result(a, el, er, V, slope, drop=None, g=None, p=None, rows=None, fault=None):
    """dict(out: bf16 bits, p: fp32; with g also gel, ger, dx: fp32 and gv: bf16 bits) from a float64 evaluation, every output rounded
    ONCE to its format; the backward starts from `p` (default: this forward's).  Faults:
      out_truncated      Out is cut to bf16, not rounded
      out_rounded_twice  Out is rounded to 11 significant bits and then to bf16
      p_bf16             P is rounded to bf16
      el_er_bf16         el and er are rounded to bf16 before the score
      poison_spreads     a row that one head poisons is NaN in every head's columns of Out
      gv_terms_rounded   every term p g of gV is rounded to bf16 before the sum
      gv_unmasked        with dropout: gV = sum p g"""
    assert fault in (None,) + FAULTS, fault
    eu, ru = (rounded(el), rounded(er)) if fault == "el_er_bf16" else (el, er)
    ref = reference(a, eu, ru, V, slope, drop, rows)
    with np.errstate(invalid="ignore", over="ignore"):
        out64 = ref["out"]
        if fault == "out_truncated":
            bits = (out64.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        elif fault == "out_rounded_twice":
            bits = f64_to_bf16(np.where(np.isfinite(out64), _round_bits(np.where(np.isfinite(out64), out64, 0.0), 11), out64))
        else:
            bits = f64_to_bf16(out64)
        if fault == "poison_spreads":
            bits = bits.copy()
            bits[np.isnan(out64).any(1)] = 0x7FC0
        p32 = ref["p"].astype(np.float32)
    got = dict(out=bits, p=rounded(p32) if fault == "p_bf16" else p32)
    if g is None:
        return got
    assert rows is None, "the backward is not defined on shards"
    pin = got["p"] if p is None else np.asarray(p, np.float32)
    b = backward_reference(a, el, er, V, pin, g, slope, drop, fault="gv_unmasked" if fault == "gv_unmasked" else None)
    with np.errstate(invalid="ignore", over="ignore"):
        got.update({key: b[key].astype(np.float32) for key in ("gel", "ger", "dx")})
        gv64 = b["gv"]
        if fault == "gv_terms_rounded":
            row, col, _ = coo(a)
            k, heads = V.shape[1], el.shape[1]
            kp = _kept(a, heads, drop, None, a.nnz)
            c = 1.0 if drop is None else gd.factor(drop[0])
            g64 = np.asarray(g, np.float64)
            gv64 = np.zeros((a.n, k))
            for h in range(heads):
                cs, sel = head_columns(k, heads, h), kp[:, h]
                terms = (c * pin[sel, h].astype(np.float64))[:, None] * g64[row[sel]][:, cs]
                np.add.at(gv64[:, cs], col[sel], from_bf16(f64_to_bf16(terms)).astype(np.float64))
        got["gv"] = f64_to_bf16(gv64)
    return got

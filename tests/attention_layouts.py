"""Where the row operands of a per-head attention call lie when they are not dense [rows, k] tensors, and the check of a run on such a
layout against the dense run (tests/test_gpu_attention_layouts.py; the check against modelled faults: tests/test_attention_layouts_host.py).

A plan carries two leading dimensions: ldb is the pitch of the K, V, gK and gV rows (side "b", n rows), ldc that of the Q, Out, g and gQ
rows (side "c", m rows); a row address is row * ld + column.  The layouts, beside "dense" (ldb = ldc = k, every operand a buffer of its
own):
  padded       ldb = k + 4, ldc = k + 8, every operand in a buffer of its own.  In bf16 the odd rows of side b are then 8-byte but not
               16-byte aligned
  padded_off4  the same with every row operand four elements into its buffer: in bf16, 8 bytes off a 16-byte mark (bf16 variants only)
  slab         ldb = ldc = 4 k + 4 and two buffers: Q | K | V | g at the column offsets 0, k, 2 k, 3 k of an input slab, Out | gQ | gK | gV
               at the same offsets of an output slab (GAT: V and g, Out and gV, at the offsets the dot-product operands have)
Every buffer holds its rows at the LARGER of the two leading dimensions and a guard tail of one such row and eight elements, so a kernel
that takes the other side's pitch, the pitch k or another operand's column offset stays inside the allocation (max_index) and shows as
wrong bits, as NaN read from the padding, or as a touched fill.  Input buffers are NaN where no operand lies, output buffers hold a fill.
numpy only: no GPU, no torch."""
from typing import NamedTuple

import numpy as np

from attention_forms import FORM_OF_K, FORMS
from attention_forms import LAYOUT_DOT_PAIRS as DOT_PAIRS
from attention_forms import LAYOUT_GAT_PAIRS as GAT_PAIRS

SENTINEL = np.float32(-12345.5)  # fp32 rows and the edge arrays start here, as in the family files
FILL = np.uint16(0x5A5A)         # bf16 bits no test computes
NAN16 = np.uint16(0x7FC0)

# the (k, H) of every (W, NS) form, all of them pairs of the *_PAIRS tables of tests/attention_forms.py
assert [FORM_OF_K[k] for k, _ in DOT_PAIRS] == FORMS and [FORM_OF_K[k] for k, _ in GAT_PAIRS] == FORMS


def _variant(gat, bf16, bias, drop, forward, backward):
    return {"gat": gat, "bf16": bf16, "bias": bias, "drop": drop, "entries": (forward, backward)}


# variant -> what it runs: the entry points are include/flex_spmm.h's names
VARIANTS = {
    "heads": _variant(False, False, False, False, "flex_attention_heads", "flex_attention_heads_backward"),
    "bf16": _variant(False, True, False, False, "flex_attention_bf16", "flex_attention_bf16_backward"),
    "bias_fp32": _variant(False, False, True, False, "flex_attention_bias", "flex_attention_bias_backward"),
    "bias_bf16": _variant(False, True, True, False, "flex_attention_bf16_bias", "flex_attention_bf16_bias_backward"),
    "dropout_fp32": _variant(False, False, False, True, "flex_attention_dropout", "flex_attention_dropout_backward"),
    "dropout_bf16": _variant(False, True, False, True, "flex_attention_bf16_dropout", "flex_attention_bf16_dropout_backward"),
    "dropout_bias_fp32": _variant(False, False, True, True, "flex_attention_dropout", "flex_attention_dropout_backward"),
    "dropout_bias_bf16": _variant(False, True, True, True, "flex_attention_bf16_dropout", "flex_attention_bf16_dropout_backward"),
    "gat": _variant(True, False, False, False, "flex_gat_attention", "flex_gat_attention_backward"),
    "gat_dropout": _variant(True, False, False, True, "flex_gat_attention_dropout", "flex_gat_attention_dropout_backward"),
    "gat_bf16": _variant(True, True, False, False, "flex_gat_attention_bf16", "flex_gat_attention_bf16_backward"),
    "gat_bf16_dropout": _variant(True, True, False, True, "flex_gat_attention_bf16_dropout", "flex_gat_attention_bf16_dropout_backward"),
}
LAYOUTS = ("padded", "padded_off4", "slab")


def layouts_of(variant):
    return LAYOUTS if VARIANTS[variant]["bf16"] else ("padded", "slab")


def pair_of(variant, form):
    return (GAT_PAIRS if VARIANTS[variant]["gat"] else DOT_PAIRS)[FORMS.index(form)]


# (variant, form, layout): what tests/test_gpu_attention_layouts.py runs against the dense run of the same (variant, form)
TRIPLES = [(v, form, layout) for v in VARIANTS for form in FORMS for layout in layouts_of(v)]

# ---- places

SLAB_ORDER = {"in": ("Q", "K", "V", "g"), "out": ("out", "gq", "gk", "gv")}
SIDE = {"Q": "c", "g": "c", "out": "c", "gq": "c", "K": "b", "V": "b", "gk": "b", "gv": "b"}


class Place(NamedTuple):
    buf: str   # the buffer the operand lies in
    off: int   # elements from the buffer's start to element (0, 0)
    ld: int    # elements from a row to the next
    rows: int


def inputs_of(gat):
    return ("V", "g") if gat else ("Q", "K", "V", "g")


def outputs_of(gat):
    return ("out", "gv") if gat else ("out", "gq", "gk", "gv")


def leading(k, layout):
    """(ldb, ldc) of the plan of a layout"""
    return {"dense": (k, k), "slab": (4 * k + 4, 4 * k + 4)}.get(layout, (k + 4, k + 8))


def places(gat, k, m, n, layout):
    """(name -> Place of every row operand, buffer -> its size in elements, guard: the elements of every buffer's tail)"""
    ldb, ldc = leading(k, layout)
    top = max(ldb, ldc)
    guard = top + 8
    pl, sizes = {}, {}
    for name in inputs_of(gat) + outputs_of(gat):
        rows, ld = (m, ldc) if SIDE[name] == "c" else (n, ldb)
        if layout == "slab":
            buf = "in" if name in SLAB_ORDER["in"] else "out"
            pl[name] = Place(buf, SLAB_ORDER[buf].index(name) * k, ld, rows)
            sizes[buf] = max(m, n) * top + guard
        else:
            pl[name] = Place(name, 4 if layout == "padded_off4" else 0, ld, rows)
            sizes[name] = rows * top + guard
    return pl, sizes, guard


def max_index(place, k):
    """the last element an access of rows x k at the place touches"""
    return place.off + (place.rows - 1) * place.ld + k - 1


def _rows_view(flat, place, k):
    assert flat.ndim == 1 and flat.flags.c_contiguous and 0 <= place.off and max_index(place, k) < flat.size
    return np.lib.stride_tricks.as_strided(flat[place.off:], shape=(place.rows, k), strides=(place.ld * flat.itemsize, flat.itemsize))


def scatter(flat, place, x):
    """x [rows, k] to its place in the flat buffer"""
    _rows_view(flat, place, x.shape[1])[...] = x


def gather(flat, place, k):
    """the [rows, k] at a place of the flat buffer, as a copy"""
    return _rows_view(flat, place, k).copy()


def fill_of(dtype):
    return FILL if np.dtype(dtype) == np.uint16 else SENTINEL


def input_buffers(pl, sizes, ins):
    """buffer -> flat array: NaN (in bf16: NaN bits) with every operand of `ins` (name -> [rows, k], float32 or uint16 bits) at its place"""
    bufs = {}
    for name, x in ins.items():
        p = pl[name]
        if p.buf not in bufs:
            bufs[p.buf] = np.full(sizes[p.buf], NAN16 if x.dtype == np.uint16 else np.float32(np.nan), x.dtype)
        scatter(bufs[p.buf], p, x)
    return bufs


def output_buffers(pl, sizes, names, dtype):
    """buffer -> flat array of the fill, for the outputs `names`"""
    return {pl[name].buf: np.full(sizes[pl[name].buf], fill_of(dtype), dtype) for name in names}


# ---- the check

def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and bool(np.array_equal(x.view(np.uint8), y.view(np.uint8)))


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def check(what, dense, bufs, pl, k, guard, edges=None):
    """A run on a layout against the dense run.  dense: name -> [rows, k] of the dense run for every row output of the call, None where
    the output was not wanted (its pointer was NULL); bufs: buffer -> the flat output buffer after the run; edges: name -> (what the run
    left, the dense run's or None = not wanted) for P, dWork and the dense gradients (the bias gradient; GAT: gEl, gEr).
    Asserts: every wanted output has the dense run's bits; every edge array that is not wanted holds the sentinel; every element of an
    output buffer outside the columns of the wanted outputs holds the fill, the guard tail first."""
    for name, (got, want) in (edges or {}).items():
        if want is None:
            assert bool(np.all(_bits(got) == _bits(np.float32(SENTINEL)))), f"{what}: {name} was not wanted and does not hold its fill"
        else:
            differ = np.argwhere(_bits(got) != _bits(want))
            assert got.shape == want.shape and not len(differ), f"{what}: {name} has not the bits of the dense run in {len(differ)} elements, first at {tuple(int(i) for i in differ[0])}"
    written = {buf: np.zeros(flat.size, bool) for buf, flat in bufs.items()}
    for name, want in dense.items():
        if want is None:
            continue
        p = pl[name]
        got = gather(bufs[p.buf], p, k)
        assert got.dtype == want.dtype and got.shape == want.shape, (what, name, got.dtype, want.dtype, got.shape, want.shape)
        differ = np.argwhere(_bits(got) != _bits(want))
        assert not len(differ), (f"{what}: {name} has not the bits of the dense run in {len(differ)} elements, first at row {differ[0][0]}, column {differ[0][1]}"
                                 f" ({got[tuple(differ[0])]!r} for {want[tuple(differ[0])]!r})")
        _rows_view(written[p.buf], p, k)[...] = True
    for buf, flat in bufs.items():
        touched = np.flatnonzero((_bits(flat) != _bits(fill_of(flat.dtype))) & ~written[buf])
        tail = touched[touched >= flat.size - guard]
        assert not len(tail), f"{what}: the guard tail of buffer {buf} is touched in {len(tail)} elements, first at {tail[0] - (flat.size - guard)} of {guard}"
        assert not len(touched), f"{what}: buffer {buf} lost its fill outside the written columns in {len(touched)} elements, first at element {touched[0]}"

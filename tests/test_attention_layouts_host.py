"""The check of tests/test_gpu_attention_layouts.py (tests/attention_layouts.py: check) against numpy models of the three address faults
it targets, and the table of that file.  No GPU.

The model kernel reads its row operands at `row * ld + column` from the input buffers of a layout and writes its row outputs the same
way: Out = Q + g, gQ = Q - g, gK = K + V, gV = K - V (GAT: Out = 2 g, gV = 2 V), in bf16 rounded once.  A fault changes the places it
reads from, or the places it writes to:
  other_pitch  ldc where ldb is meant and ldb where ldc is meant
  pitch_k      k where the leading dimension is meant
  rotated      the column offset of the next operand of the slab (Q reads K's columns, Out is written to gQ's, ...)
With ldb == ldc == k all three give the dense run's bits.  The padded layouts show the first two, the slab the last two (its two leading
dimensions are equal, and the operands of a padded layout have no column offsets): between them the layouts show each."""
import re

import numpy as np
import pytest

import attention_bf16_ref as bf
import attention_layouts as lay
from attention_forms import FORMS

M, N = 37, 41
FAULTS = ("other_pitch", "pitch_k", "rotated")
SHOWS = {"other_pitch": ("padded", "padded_off4"), "pitch_k": ("padded", "padded_off4", "slab"), "rotated": ("slab",)}


def faulty(pl, k, layout, fault):
    ldb, ldc = lay.leading(k, layout)
    out = {}
    for name, p in pl.items():
        if fault == "other_pitch":
            p = p._replace(ld=ldc if lay.SIDE[name] == "b" else ldb)
        elif fault == "pitch_k":
            p = p._replace(ld=k)
        elif fault == "rotated" and layout == "slab":
            p = p._replace(off=(p.off // k + 1) % 4 * k)
        out[name] = p
    return out


def toy(gat, x):
    if gat:
        return {"out": 2 * x["g"], "gv": 2 * x["V"]}
    return {"out": x["Q"] + x["g"], "gq": x["Q"] - x["g"], "gk": x["K"] + x["V"], "gv": x["K"] - x["V"]}


def operands(gat, k, bf16):
    rng = np.random.default_rng([k, gat, bf16])
    x = {name: rng.uniform(-1, 1, (M if lay.SIDE[name] == "c" else N, k)).astype(np.float32) for name in lay.inputs_of(gat)}
    return {name: bf.rounded(v) for name, v in x.items()} if bf16 else x


def narrow(x, bf16):
    return bf.to_bf16(x) if bf16 else x.astype(np.float32)


def model_run(gat, k, layout, bf16, fault=None, where="reads", want=None):
    """(the output buffers a model kernel with `fault` leaves, the dense run: name -> [rows, k] or None where not wanted, places, guard)"""
    x = operands(gat, k, bf16)
    want = lay.outputs_of(gat) if want is None else want
    pl, sizes, guard = lay.places(gat, k, M, N, layout)
    ins = lay.input_buffers(pl, sizes, {name: narrow(v, bf16) for name, v in x.items()})
    outs = lay.output_buffers(pl, sizes, lay.outputs_of(gat), np.uint16 if bf16 else np.float32)
    rd = faulty(pl, k, layout, fault) if where == "reads" else pl
    wr = faulty(pl, k, layout, fault) if where == "writes" else pl
    got = {name: lay.gather(ins[pl[name].buf], rd[name], k) for name in lay.inputs_of(gat)}
    with np.errstate(invalid="ignore", over="ignore"):
        res = toy(gat, {name: bf.from_bf16(v) if bf16 else v for name, v in got.items()})
    for name in want:
        lay.scatter(outs[pl[name].buf], wr[name], narrow(res[name], bf16))
    dense = {name: narrow(v, bf16) if name in want else None for name, v in toy(gat, x).items()}
    return outs, dense, pl, guard


KS = (8, 48)  # W = 4 whole, and lanes past k


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("gat", [False, True], ids=["dot", "gat"])
@pytest.mark.parametrize("layout", lay.LAYOUTS)
def test_the_check_accepts_the_right_model_on_every_layout(layout, gat, bf16):
    for k in KS:
        outs, dense, pl, guard = model_run(gat, k, layout, bf16)
        lay.check("right", dense, outs, pl, k, guard)
        for name in lay.outputs_of(gat):  # one output alone: the others keep their fill
            outs, dense, pl, guard = model_run(gat, k, layout, bf16, want=(name,))
            assert [key for key, v in dense.items() if v is not None] == [name]
            lay.check("right", dense, outs, pl, k, guard)


@pytest.mark.parametrize("where", ["reads", "writes"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("gat", [False, True], ids=["dot", "gat"])
@pytest.mark.parametrize("fault", FAULTS)
def test_the_check_rejects_each_fault_on_the_layouts_that_show_it(fault, gat, bf16, where):
    why = r"has not the bits of the dense run|lost its fill outside the written columns|the guard tail of buffer \w+ is touched"
    for k in KS:
        for layout in lay.LAYOUTS:
            outs, dense, pl, guard = model_run(gat, k, layout, bf16, fault, where)
            if layout in SHOWS[fault]:
                with pytest.raises(AssertionError, match=why):
                    lay.check(fault, dense, outs, pl, k, guard)
            else:  # the layout cannot show it: equal leading dimensions, or no column offsets
                lay.check(fault, dense, outs, pl, k, guard)
        # and on the dense layout no fault shows at all: what a dense-only suite sees
        outs, dense, pl, guard = model_run(gat, k, "dense", bf16, fault, where)
        lay.check(fault, dense, outs, pl, k, guard)
    assert set().union(*SHOWS.values()) == set(lay.LAYOUTS) and all(SHOWS[f] for f in FAULTS)


def test_a_read_at_the_wrong_pitch_meets_the_nan_of_the_padding_and_a_write_touches_the_fill():
    k = 8
    outs, dense, pl, guard = model_run(False, k, "padded", False, "other_pitch", "reads")
    got = lay.gather(outs["gk"], pl["gk"], k)
    assert np.isnan(got).any() and not np.isnan(dense["gk"]).any()
    with pytest.raises(AssertionError, match="gk has not the bits of the dense run"):
        lay.check("nan", {"gk": dense["gk"]}, {"gk": outs["gk"]}, pl, k, guard)
    for fault in ("other_pitch", "pitch_k"):  # the values are right and lie elsewhere: in the padding, never past the rows of the larger pitch
        outs, dense, pl, guard = model_run(False, k, "padded", False, fault, "writes")
        with pytest.raises(AssertionError, match="buffer gk lost its fill outside the written columns"):
            lay.check("padding", {"gk": None}, {"gk": outs["gk"]}, pl, k, guard)
    # a write past the last row (no pitch does that: a row index would) lands in the guard tail
    outs, dense, pl, guard = model_run(False, k, "padded", False)
    lay.scatter(outs["gk"], pl["gk"]._replace(off=pl["gk"].off + pl["gk"].ld, ld=lay.leading(k, "padded")[1]), dense["gk"])
    with pytest.raises(AssertionError, match="the guard tail of buffer gk is touched"):
        lay.check("tail", {"gk": None}, {"gk": outs["gk"]}, pl, k, guard)


def test_an_output_that_was_not_wanted_must_keep_its_fill_and_the_edge_arrays_are_held_to_the_dense_run():
    k = 8
    outs, dense, pl, guard = model_run(False, k, "padded", False)
    with pytest.raises(AssertionError, match="buffer gq lost its fill"):
        lay.check("unwanted", dict(dense, gq=None), outs, pl, k, guard)
    p = np.arange(12, dtype=np.float32).reshape(6, 2)
    lay.check("edges", dense, outs, pl, k, guard, edges={"p": (p, p.copy()), "work": (np.full((6, 2), lay.SENTINEL), None)})
    with pytest.raises(AssertionError, match="p has not the bits of the dense run in 1 elements, first at \\(4, 1\\)"):
        other = p.copy()
        other[4, 1] = -other[4, 1]
        lay.check("edges", dense, outs, pl, k, guard, edges={"p": (other, p)})
    with pytest.raises(AssertionError, match="work was not wanted and does not hold its fill"):
        lay.check("edges", dense, outs, pl, k, guard, edges={"work": (p, None)})
    zero = np.zeros((3, 2), np.float32)
    with pytest.raises(AssertionError, match="has not the bits"):  # -0 is not +0
        lay.check("edges", dense, outs, pl, k, guard, edges={"gb": (-zero, zero)})


def test_no_fault_leaves_the_allocation_at_any_shape_of_the_gpu_file():
    """The sizes of places() hold every access of every fault model at the shapes the GPU file runs (890 x 890)."""
    m = n = 890
    for gat, pairs in ((False, lay.DOT_PAIRS), (True, lay.GAT_PAIRS)):
        for k, _ in pairs:
            for layout in lay.LAYOUTS + ("dense",):
                pl, sizes, guard = lay.places(gat, k, m, n, layout)
                assert guard >= max(lay.leading(k, layout)) + 8  # a row of fill, and room for the four elements of padded_off4
                for fault in (None,) + FAULTS:
                    for name, p in (faulty(pl, k, layout, fault) if fault else pl).items():
                        assert lay.max_index(p, k) < sizes[p.buf] - (guard if fault is None else 0), (gat, k, layout, fault, name)


def test_the_table_meets_every_variant_form_and_layout_and_all_twenty_per_head_entry_points():
    import os
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "flex_spmm.h")).read()
    declared = set(re.findall(r"^int (flex_(?:gat_)?attention\w*)\(", header, re.M))
    assert len(declared) == 22
    # the single-head pair has no per-head form; tests/test_gpu_fused_attention.py runs it padded, odd and one float off
    per_head = declared - {"flex_attention", "flex_attention_backward"}
    reached = {e for v in lay.VARIANTS.values() for e in v["entries"]}
    assert reached == per_head and len([e for e in reached if "gat" not in e]) == 12 and len([e for e in reached if "gat" in e]) == 8
    for v in lay.VARIANTS:
        for layout in lay.layouts_of(v):
            assert {form for vv, form, ll in lay.TRIPLES if (vv, ll) == (v, layout)} == set(FORMS)
    assert len(lay.TRIPLES) == len(set(lay.TRIPLES)) == 7 * (6 * 2 + 6 * 3)
    for gat, pairs in ((False, lay.DOT_PAIRS), (True, lay.GAT_PAIRS)):
        for k, H in pairs:
            d = k // H
            assert k % H == 0 and 4 <= d <= 256 and d & (d - 1) == 0
            for layout in lay.LAYOUTS:
                ldb, ldc = lay.leading(k, layout)
                assert ldb % 4 == 0 and ldc % 4 == 0 and min(ldb, ldc) > k  # what the vector form needs, and never dense
    # bf16: the odd rows of side b of the padded layout are 8 bytes off a 16-byte mark (at k = 4 those of side c)
    for k, _ in lay.DOT_PAIRS + lay.GAT_PAIRS:
        assert (2 * lay.leading(k, "padded")[0 if k > 4 else 1]) % 16 == 8

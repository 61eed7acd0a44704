"""The per-head attention calls on the GPU on rows that are not dense [rows, k] tensors: the twelve dot-product entry points
(flex_attention_heads, _bf16, _bias, _bf16_bias, _dropout, _bf16_dropout and their backward calls) and the eight GAT ones (fp32 and bf16 V
rows, with and without dropout), in every (W, NS) form, on the layouts of tests/attention_layouts.py: padded rows (ldb = k + 4,
ldc = k + 8), the same four elements further (bf16: 8 bytes off a 16-byte mark), and Q | K | V | g and Out | gQ | gK | gV as column blocks
of two slabs of pitch 4 k + 4.

Every run is held to the dense run of the same operands (ldb = ldc = k, contiguous rows) bit for bit -- Out, P, dWork, every gradient and
the bias gradient -- and every element of an output buffer outside the written columns, the guard tail included, to its fill.  No float64
reference and no tolerance: the family files hold the dense runs to float64, the walk and the fp32 expressions do not depend on the pitch,
and the dropout mask and the edge arrays are indexed by e * H + h alone.  With ldb == ldc == k a kernel that takes ldc for ldb, k for a
leading dimension or a column offset from the wrong place gives the right answer; here it gives other bits, reads the NaN of the input
padding or touches a fill (tests/test_attention_layouts_host.py holds the check to models of these faults).

Graph: both_sides(threshold_graph()), 890 x 890: the slot, wave and block classes and their boundaries in rows and in columns.  Both runs
go through the pointer forms of binding.Plan; a different score scenario in every head."""
import numpy as np
import pytest

import attention_bf16_ref as bf
import attention_bias_ref as ab
import attention_layouts as lay
import flex_amd
import gat_attention_ref as gat
import multihead_attention_ref as mh
from attention_forms import FORMS
from fused_attention_backward_ref import both_sides
from fused_attention_ref import threshold_graph
from test_attention_dropout_host import SEED

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SCALE, SLOPE, DROP = 0.25, gat.SLOPE, 0.5
_cache = {}


def graph():
    if "graph" not in _cache:
        _cache["graph"] = both_sides(threshold_graph())
    return _cache["graph"]


def plan(k, layout):
    key = ("plan", k) + lay.leading(k, layout)
    if key not in _cache:
        ldb, ldc = lay.leading(k, layout)
        _cache[key] = flex_amd.Plan(graph(), k, attention=True, attention_backward=True, **({} if layout == "dense" else {"ldb": ldb, "ldc": ldc}))
        _cache[key].self_check()
    return _cache[key]


def operands(variant, form):
    """The host operands of a (variant, form), made once and left unchanged: the generators of the family files' ref modules, the scenario
    of head h rotated by the form.  rows: name -> [rows, k] (float32, or bf16 bits); edge: the dense float32 inputs (bias; GAT: el, er)."""
    v = lay.VARIANTS[variant]
    k, H = lay.pair_of(variant, form)
    key = ("operands", v["gat"], v["bias"], v["bf16"], k, H)
    if key not in _cache:
        a, shift = graph(), FORMS.index(form)
        g = np.random.default_rng([1, k, 82]).uniform(-1, 1, (a.m, k)).astype(np.float32)
        edge = {}
        if v["gat"]:
            edge["el"], edge["er"], V = gat.operands(gat.scenarios_of(H, shift=shift), a, k, seed=1)
            rows = {"V": V, "g": g}
        elif v["bias"]:
            Q, K, V, edge["bias"] = ab.operands(ab.scenarios_of(H, shift=shift), a, k, seed=1, bf16=v["bf16"])
            rows = {"Q": Q, "K": K, "V": V, "g": g}
        else:
            Q, K, V = mh.operands(mh.scenarios_of(H, shift=shift), a, k, seed=1)
            rows = {"Q": Q, "K": K, "V": V, "g": g}
        rows = {name: bf.to_bf16(x) if v["bf16"] else np.ascontiguousarray(x, np.float32) for name, x in rows.items()}
        _cache[key] = (rows, {name: np.ascontiguousarray(x, np.float32) for name, x in edge.items()})
    return _cache[key]


def _dev(x):
    """a host array on the device, bf16 bits as int16"""
    return torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).cuda()


def _host(t):
    x = t.cpu().numpy()
    return x.view(np.uint16) if x.dtype == np.int16 else x


def run(variant, form, layout, want=None):
    """The forward and the backward of a variant on a layout.  want: the gradients asked for, (gQ, gK, gV, gBias) (GAT: (gEl, gEr, gV));
    None: all the variant has.  (the output buffers on the host, edges: name -> what P, dWork and the dense gradients hold, places, guard)"""
    v = lay.VARIANTS[variant]
    k, H = lay.pair_of(variant, form)
    a, p = graph(), plan(k, layout)
    rows, edge = operands(variant, form)
    pl, sizes, guard = lay.places(v["gat"], k, a.m, a.n, layout)
    es = 2 if v["bf16"] else 4
    ins = {buf: _dev(x) for buf, x in lay.input_buffers(pl, sizes, rows).items()}
    outs = {buf: _dev(x) for buf, x in lay.output_buffers(pl, sizes, lay.outputs_of(v["gat"]), np.uint16 if v["bf16"] else np.float32).items()}
    for name, q in pl.items():  # every access of the call lies inside its buffer, whichever of the pitches a kernel takes
        assert lay.max_index(q._replace(ld=max(lay.leading(k, layout))), k) < (ins if name in rows else outs)[q.buf].numel()
    at = {name: (ins if name in rows else outs)[q.buf].data_ptr() + es * q.off for name, q in pl.items()}
    assert all(ptr % (4 * es) == 0 for ptr in at.values())
    if layout == "padded_off4":
        assert all(ptr % 16 == 8 for ptr in at.values())
    dense_in = {name: _dev(x) for name, x in edge.items()}
    shapes = {"p": (a.nnz, H), "work": (a.nnz, H)}
    if v["gat"]:
        shapes |= {"gel": (a.m, H), "ger": (a.n, H)}
        if want is None:
            want = (True, True, True)
        wanted = dict(zip(("gel", "ger", "gv"), want))
    else:
        if v["bias"]:
            shapes["gb"] = (a.nnz, H)
        if want is None:
            want = (True, True, True, v["bias"])
        assert v["bias"] or not want[3]
        wanted = dict(zip(("gq", "gk", "gv", "gb"), want))
    e = {name: torch.full(shape, float(lay.SENTINEL), device="cuda") for name, shape in shapes.items()}
    ptr = lambda name: (e[name].data_ptr() if name in e else at[name]) if wanted.get(name, True) else None
    s = torch.cuda.current_stream().cuda_stream
    drop = (DROP, SEED) if v["drop"] else ()
    if v["gat"]:
        tail = "_bf16" * v["bf16"] + "_dropout" * v["drop"]
        el, er = dense_in["el"].data_ptr(), dense_in["er"].data_ptr()
        getattr(p, f"gat_attention{tail}_ptr")(H, el, er, at["V"], SLOPE, *drop, at["out"], e["p"].data_ptr(), s)
        getattr(p, f"gat_attention{tail}_backward_ptr")(H, el, er, at["V"], e["p"].data_ptr(), at["g"], SLOPE, *drop, ptr("gel"), ptr("ger"), ptr("gv"),
                                                         e["work"].data_ptr(), s)
    else:
        q, kk, vv = at["Q"], at["K"], at["V"]
        bias = dense_in["bias"].data_ptr() if v["bias"] else None
        grads = (ptr("gq"), ptr("gk"), ptr("gv"))
        gb = ptr("gb") if v["bias"] else None
        if v["drop"]:
            tail = "_bf16" * v["bf16"] + "_dropout"
            getattr(p, f"attention{tail}_ptr")(q, kk, vv, bias, SCALE, *drop, at["out"], e["p"].data_ptr(), s, heads=H)
            getattr(p, f"attention{tail}_backward_ptr")(q, kk, vv, e["p"].data_ptr(), at["g"], SCALE, *drop, *grads, gb, e["work"].data_ptr(), s, heads=H)
        elif v["bias"]:
            tail = "_bf16" * v["bf16"] + "_bias"
            getattr(p, f"attention{tail}_ptr")(q, kk, vv, bias, SCALE, at["out"], e["p"].data_ptr(), s, heads=H)
            getattr(p, f"attention{tail}_backward_ptr")(q, kk, vv, e["p"].data_ptr(), at["g"], SCALE, *grads, gb, e["work"].data_ptr(), s, heads=H)
        else:
            tail = "_bf16" * v["bf16"]
            kw = {"heads": H}
            getattr(p, f"attention{tail}_ptr")(q, kk, vv, SCALE, at["out"], e["p"].data_ptr(), s, **kw)
            getattr(p, f"attention{tail}_backward_ptr")(q, kk, vv, e["p"].data_ptr(), at["g"], SCALE, *grads, e["work"].data_ptr(), s, **kw)
    torch.cuda.synchronize()
    for buf, before in lay.input_buffers(pl, sizes, rows).items():  # no call writes an input
        assert lay.same_bits(_host(ins[buf]), before), f"{variant} {form} {layout}: input buffer {buf} changed"
    return {buf: _host(t) for buf, t in outs.items()}, {name: _host(t) for name, t in e.items()}, pl, guard, wanted


def dense(variant, form):
    """The dense run of a (variant, form), once: (name -> [rows, k] of every row output, name -> the edge arrays)."""
    key = ("dense", variant, form)
    if key not in _cache:
        k, _ = lay.pair_of(variant, form)
        outs, edges, pl, guard, wanted = run(variant, form, "dense")
        rows = {name: lay.gather(outs[pl[name].buf], pl[name], k) for name in lay.outputs_of(lay.VARIANTS[variant]["gat"])}
        lay.check(f"{variant} {form} dense", rows, outs, pl, k, guard)  # the tails of the dense buffers
        fill = lay.fill_of(rows["out"].dtype)
        for name, x in {**rows, **edges}.items():  # every output is written: what is compared below is no fill
            assert not bool(np.any(x == (fill if x.dtype == np.uint16 else lay.SENTINEL))), f"{variant} {form}: the dense run left fill in {name}"
        _cache[key] = (rows, edges)
    return _cache[key]


def _id(x):
    return f"w{x[0]}ns{x[1]}" if isinstance(x, tuple) else str(x)


@pytest.mark.parametrize("variant,form,layout", lay.TRIPLES, ids=_id)
def test_every_output_has_the_bits_of_the_dense_run_and_nothing_else_is_written(variant, form, layout):
    k, H = lay.pair_of(variant, form)
    rows, edges = dense(variant, form)
    outs, got, pl, guard, _ = run(variant, form, layout)
    ldb, ldc = lay.leading(k, layout)
    lay.check(f"{variant} k={k} H={H} {layout} (ldb {ldb}, ldc {ldc})", rows, outs, pl, k, guard, edges={name: (got[name], edges[name]) for name in edges})


def test_the_parametrisation_meets_every_variant_form_and_layout():
    """What ran above is the table, whole: every (W, NS) form of every variant on every layout it has, nothing skipped."""
    marks = test_every_output_has_the_bits_of_the_dense_run_and_nothing_else_is_written.pytestmark
    ran = [m.args[1] for m in marks if m.name == "parametrize"][0]
    assert list(ran) == lay.TRIPLES
    want = {(v, form, layout) for v in lay.VARIANTS for form in FORMS for layout in ("padded", "slab") + (("padded_off4",) if lay.VARIANTS[v]["bf16"] else ())}
    assert set(ran) == want and len(ran) == len(want) == 210
    assert all(not getattr(t, "marks", ()) for t in ran)  # no skip, no xfail
    entries = {e for v, _, _ in ran for e in lay.VARIANTS[v]["entries"]}
    assert len(entries) == 20 and sum("gat" in e for e in entries) == 8


# ---- subsets of the gradients on the padded layout

ROW_ALONE, COLUMN_ALONE, BIAS_ALONE = "row kernel alone", "column kernel alone", "bias gradient alone"
SUBSETS = [(v, FORMS[(3 * i + j) % len(FORMS)], which) for i, v in enumerate(lay.VARIANTS)
           for j, which in enumerate((ROW_ALONE, COLUMN_ALONE) + ((BIAS_ALONE,) if lay.VARIANTS[v]["bias"] else ()))]


@pytest.mark.parametrize("variant,form,which", SUBSETS, ids=_id)
def test_a_subset_of_the_gradients_on_padded_rows_leaves_the_unwanted_outputs_at_their_fill(variant, form, which):
    """gQ alone (GAT: gEl alone) runs the row launch alone, gV alone the column launch alone, the bias gradient alone the row launch
    without gQ.  What is wanted has the dense full run's bits; gQ, gK, gV, the bias gradient (gEl, gEr) that are not wanted keep their
    fill, and dWork keeps it where the row launch is skipped."""
    v = lay.VARIANTS[variant]
    k, H = lay.pair_of(variant, form)
    n = 3 if v["gat"] else 4
    want = tuple(i == {ROW_ALONE: 0, COLUMN_ALONE: 2, BIAS_ALONE: 3}[which] for i in range(n))
    rows, edges = dense(variant, form)
    outs, got, pl, guard, wanted = run(variant, form, "padded", want=want)
    assert sum(wanted.values()) == 1
    held = {name: x if wanted.get(name, True) else None for name, x in rows.items()}
    row_launch = which != COLUMN_ALONE
    e = {name: (got[name], edges[name] if wanted.get(name, name != "work" or row_launch) else None) for name in edges}
    lay.check(f"{variant} k={k} H={H} padded, {which}", held, outs, pl, k, guard, edges=e)

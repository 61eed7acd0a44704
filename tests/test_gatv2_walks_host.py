"""Host side of tests/test_gpu_gatv2_walks.py: the kernels of the fused GATv2 attention and of its dropout twin (flex::gatv2,
flex::gatv2_dropout) on walks whose group budget is above the floor of 64 and on unsorted rows with repeated (row, column) pairs, and
the two-stage check of gAtt (tests/gatv2_attention_ref.py: att_work_layout, att_partials_reference, att_reduce32, check_att).

Here: the table of the GPU file's cases; the budget, the items per group and the classes each case claims, held to the plans of the host
simulator; att_work_layout's row count against flex_gatv2_attention_work_size at every (T, k) of the table, under the default plan
(the XCD remap) and under tuning={"xcd_slices": 2}, the knob that turns the remap off on an attention plan (it reaches them:
plan.tuning()["xcd_slices"] reads 2 and the row count is no longer rounded up to a multiple of 8; order=FLEX_ORDER_RCM gives the same
plan and is held to it); the fp32 evaluations against check, check_backward and check_att on the operands of every float64 case (the
inputs are fair); numpy models of five faults of gAtt's two stages against check_att, of the four multi-item faults of
tests/test_attention_walks_host.py in GATv2's own outputs against the check of the copies, and of a dropout mask taken at entries off by
the group's first item, in each of the three launches, against the float64 checkers; the references on the multi-edge graph against an
independent float64 torch autograd evaluation.  No GPU."""
import numpy as np
import pytest

import attention_dropout_ref as ad
import flex_amd
import gatv2_attention_ref as v2
import gatv2_dropout_ref as vd
from attention_walk_graphs import BUDGETS, MIN_ITEMS_PER_GROUP, assert_copies, multi_edge_graph, tile_rows, walk_graph, walk_places
from flex_amd import binding
from fused_attention_ref import coo
from multihead_attention_ref import head_columns
from test_attention_walks_host import FAULTS, ITEMS_PER_GROUP
from test_gat_walks_host import DROP, KERNELS, RANGE_COPY, SEED, SENTINEL, _sum_by, case_id, grad, repeats_that_differ_in_the_mask  # noqa: F401
from test_gatv2_entry_host import _build as build_gatv2_simulator

hostsim = pytest.importorskip("hostsim")

SLOPE = v2.SLOPE
KEYS = ("out", "p", "gxt", "gxs", "dz")  # what the check of the copies holds; gAtt and dAttWork are check_att's

# ---- the table.  A case is (section, family, k, H, T); every row is dense (ldb = ldc = k)
FAMILIES = ("gatv2", "gatv2_dropout")
DROPOUT_FAMILIES = ("gatv2_dropout",)
# (a) budget 128 against float64: W = 4 and W = 8 in both families, W = 16 under dropout
A_PAIRS = {"gatv2": [(8, 2), (32, 4)], "gatv2_dropout": [(8, 2), (32, 4), (64, 8)]}
# (b) budgets 512 and 2048 by copies: W = 4, 16 and 64 at T = 7, W = 4 at T = 30.  gatv2: every output; gatv2_dropout: P
B_PAIRS = {"gatv2": [(8, 2), (64, 8), (256, 1)], "gatv2_dropout": [(8, 2), (64, 8), (256, 1)]}
# (c) dropout at budget 512 against float64: every output at W = 4; the forward over the rows of copy 3 at W = 16
C_PAIRS = {"gatv2_dropout": [(8, 2)]}
C_RANGE_PAIRS = {"gatv2_dropout": [(64, 8)]}
# (d) the multi-edge graph against float64
MULTI_EDGE_PAIRS = {"gatv2": [(32, 4), (256, 1)], "gatv2_dropout": [(32, 4), (256, 1)]}
# (e) the branch without the remap; (f) a captured graph, a forward without P and a backward without gAtt
E_CASES = [("gatv2", 8, 2, 1), ("gatv2_dropout", 8, 2, 1)]
F_CASE = ("gatv2_dropout", 8, 2, 7)
NO_REMAP = {"xcd_slices": 2}
CASES = ([("a", f, k, H, 1) for f in FAMILIES for k, H in A_PAIRS[f]]
         + [("b", f, k, H, 7) for f in FAMILIES for k, H in B_PAIRS[f]] + [("b", f, *B_PAIRS[f][0], 30) for f in FAMILIES]
         + [("c", f, k, H, 7) for f in DROPOUT_FAMILIES for k, H in C_PAIRS[f]]
         + [("c_range", f, k, H, 7) for f in DROPOUT_FAMILIES for k, H in C_RANGE_PAIRS[f]] + [("e",) + c for c in E_CASES] + [("f",) + F_CASE])


def launches(c):
    """The kernels of its family that a case of the table launches: written down beside the GPU file's tests.  (b) under dropout and
    the range case of (c) run the forward alone."""
    section, family = c[:2]
    return KERNELS[:1] if section == "c_range" or (section == "b" and family in DROPOUT_FAMILIES) else KERNELS


def drop_of(family):
    """check_att's `drop` of a family: None, or (p, seed)."""
    return (DROP, SEED) if family in DROPOUT_FAMILIES else None


def shift_of(family, k, H):
    """The scenario rotation of a pair: its place in the family's lists, so that the pairs of a family differ."""
    pairs = A_PAIRS[family] + B_PAIRS[family] + MULTI_EDGE_PAIRS[family]
    return pairs.index((k, H)) + len(family)


_operands = {}


def operands(family, k, H, a, shift, seed=1):
    """dict(xt, xs, att, g) of a call on graph a: a scenario per head, rotated by `shift`.  Made once per (k, H, graph, shift) and left
    unchanged; both families take the same arrays."""
    key = (k, H, id(a), shift, seed)
    if key not in _operands:
        xt, xs, att = v2.operands(v2.scenarios_of(H, shift=shift), a, k, seed=seed)
        _operands[key] = (a, dict(xt=xt, xs=xs, att=att, g=grad(a, k, seed)))
    return _operands[key][1]


def tiled_operands(o, T):
    """The row operands repeated for the T copies; att is one [H, d] for all of them."""
    return {key: x if key == "att" else tile_rows(x, T) for key, x in o.items()}


def layout_of(a, k, budget, remap=True):
    return v2.att_work_layout(a.rowPtr, k, budget, remap)


def check64(family, a, o, got, what, rows=None, backward=True, layout=None):
    """Every output of a run (host arrays) against the float64 reference under the bounds and the checkers of the family, gAtt by the
    whole-graph bound of check_backward and, where a layout is given, by check_att on got["att_work"]: the worst err / bound of each,
    printed.  rows = (r0, r1): the forward of those rows alone, o["xt"], got["out"] and got["p"] holding those rows and their entries; the
    mask is taken at the entries of the whole of a."""
    each = {}
    xt, xs, att = o["xt"], o["xs"], o["att"]
    if family == "gatv2":
        each["out_p"] = v2.check(a, xt, xs, att, SLOPE, got["out"], got["p"], rows=rows, what=what)
        if backward:
            v2.check_backward(a, xt, xs, att, got["p"], o["g"], SLOPE, got["gxt"], got["gxs"], got["gatt"], got["dz"], what=what, ratios=each)
    else:
        vd.check(a, xt, xs, att, SLOPE, DROP, SEED, got["out"], got["p"], rows=rows, what=what, ratios=each)
        if backward:
            vd.check_backward(a, xt, xs, att, got["p"], o["g"], SLOPE, DROP, SEED, got["gxt"], got["gxs"], got["gatt"], got["dz"], what=what, ratios=each)
    if backward and layout is not None:
        v2.check_att(a, xt, xs, att, got["p"], o["g"], SLOPE, got["att_work"], got["gatt"], layout, drop=drop_of(family), what=what, ratios=each)
    print(f"{what}: worst err / bound " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))
    return each


def fp32_run(family, a, o, layout):
    """The family's evaluation in fp32 arithmetic with the rows of dAttWork under the layout."""
    if family == "gatv2":
        return v2.fp32_result(a, o["xt"], o["xs"], o["att"], SLOPE, g=o["g"], partials=layout)
    return vd.fp32_result(a, o["xt"], o["xs"], o["att"], SLOPE, DROP, SEED, g=o["g"], partials=layout)


@pytest.fixture(scope="module")
def sim():
    """The host simulator with the GATv2 entry points (tests/hostsim_gatv2): flex_gatv2_attention_work_size is among them."""
    so = build_gatv2_simulator()
    old_so, old_lib = binding._SO, binding._lib
    binding._SO, binding._lib = so, None
    yield binding.lib()
    binding._SO, binding._lib = old_so, old_lib


# ---- 1. what the cases claim

def test_the_table_holds_what_it_is_meant_to():
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids) == 5 + 8 + 1 + 1 + 2 + 1
    assert {c[4] for c in CASES if c[0] == "a"} == {1} and {c[4] for c in CASES if c[0] == "b"} == {7, 30} and {c[4] for c in CASES if c[0][0] in "cf"} == {7}
    assert {c[4] for c in CASES if c[0] == "e"} == {1} and [c[2:4] for c in CASES if c[4] == 30] == [(8, 2), (8, 2)]
    assert A_PAIRS == {"gatv2": [(8, 2), (32, 4)], "gatv2_dropout": [(8, 2), (32, 4), (64, 8)]}
    for f in FAMILIES:
        assert B_PAIRS[f] == [(8, 2), (64, 8), (256, 1)] and MULTI_EDGE_PAIRS[f] == [(32, 4), (256, 1)]
        shifts = [shift_of(f, k, H) for k, H in dict.fromkeys(A_PAIRS[f] + B_PAIRS[f] + MULTI_EDGE_PAIRS[f])]
        assert len(set(shifts)) == len(shifts)
        assert len({tuple(v2.scenarios_of(H, shift=shift_of(f, k, H))) for k, H in dict.fromkeys(A_PAIRS[f] + B_PAIRS[f] + MULTI_EDGE_PAIRS[f]) if H > 1}) >= 3
    assert C_PAIRS == {"gatv2_dropout": [(8, 2)]} and C_RANGE_PAIRS == {"gatv2_dropout": [(64, 8)]} and (DROP, RANGE_COPY) == (0.5, 3)


def test_every_case_plans_at_the_budget_the_items_per_group_and_the_classes_it_declares(sim):
    assert BUDGETS == {1: 128, 7: 512, 30: 2048} and MIN_ITEMS_PER_GROUP == {1: 1.5, 7: 7.5, 30: 33.0}
    seen = {}
    above = {(f, kern): [] for f in FAMILIES for kern in KERNELS}  # the cases that run a kernel on more than 7.5 items per group
    for c in CASES:
        _, family, k, H, T = c
        if (T, k) not in seen:
            p = flex_amd.Plan(walk_graph(T), k, attention=True, attention_backward=True)
            p.self_check()
            seen[(T, k)] = (p.attention_info(), p.attention_backward_info())
            p.destroy()
        fwd, bwd = seen[(T, k)]
        assert fwd["group_budget"] == bwd["group_budget"] == BUDGETS[T], f"{case_id(c)} declares budget {BUDGETS[T]}: the plan has {fwd['group_budget']}, {bwd['group_budget']}"
        want = ITEMS_PER_GROUP[(T, k)]
        assert want >= MIN_ITEMS_PER_GROUP[T]
        per_group = []
        for i, blocks in ((fwd, fwd["rows_block"]), (bwd, bwd["columns_block"])):
            per_group.append((i["items"] - blocks) / i["groups"])
            assert per_group[-1] >= want, f"{case_id(c)} declares {want} items per group: the plan has {per_group[-1]:.3g}"
        for i, keys in ((fwd, ("rows_empty", "rows_slot", "rows_wave", "rows_block")), (bwd, ("columns_empty", "columns_slot", "columns_wave", "columns_block"))):
            assert min(i[x] for x in keys) > 0, (case_id(c), i)  # every class in both walks
        assert fwd["rows_block"] == bwd["columns_block"] == 4 * T and fwd["rows_wave"] == bwd["columns_wave"]
        for kern in launches(c):  # the forward and the row backward walk the rows, the column backward the columns
            if per_group[kern == "columns_backward"] > 7.5:
                above[(family, kern)].append(case_id(c))
    for (family, kern), ids in above.items():
        assert ids, f"no case launches {family}'s {kern} on a plan of more than 7.5 items per group"
    print("\n".join(f"{f} {kern}: {', '.join(ids)}" for (f, kern), ids in above.items()))


def test_the_multi_edge_cases_plan_at_the_floor_with_every_class(sim):
    a, _ = multi_edge_graph()
    for k in sorted({k for f in FAMILIES for k, _ in MULTI_EDGE_PAIRS[f]}):
        p = flex_amd.Plan(a, k, attention=True, attention_backward=True)
        p.self_check()
        fwd, bwd = p.attention_info(), p.attention_backward_info()
        assert (fwd["group_budget"], bwd["group_budget"]) == (64, 64), k
        assert min(fwd[x] for x in ("rows_empty", "rows_slot", "rows_wave", "rows_block")) > 0
        assert min(bwd[x] for x in ("columns_empty", "columns_slot", "columns_wave", "columns_block")) > 0
        assert layout_of(a, k, 64)[1] * k == p.gatv2_attention_work_size()
        p.destroy()


def test_the_layout_has_the_row_count_of_the_work_size_with_and_without_the_remap(sim):
    """tuning={"xcd_slices": 2} reaches an attention plan: its tuning() reads 2 where the default plan's reads 1, and the grid of the
    grouped items is ceil(groups / 4) workgroups where the default plan rounds it up to a multiple of 8.  order=FLEX_ORDER_RCM, which
    the planner treats as interleaved, gives the same count.  At T = 1, k = 8 the two grids differ: ceil(2945 / 4) = 737 = 92 * 8 + 1."""
    counts = {}
    for T, k in sorted({(c[4], c[2]) for c in CASES}):
        a = walk_graph(T)
        for remap, tuning in ((True, None), (False, NO_REMAP)):
            p = flex_amd.Plan(a, k, attention=True, attention_backward=True, tuning=tuning)
            i = p.attention_info()
            assert p.tuning()["xcd_slices"] == (1 if remap else 2) and i["group_budget"] == BUDGETS[T]
            row_of, n_rows = layout_of(a, k, BUDGETS[T], remap)
            wgs = -(-i["groups"] // 4)
            assert n_rows == i["rows_block"] + (-(-wgs // 8) * 8 if remap else wgs), (T, k, remap)
            assert n_rows * k == p.gatv2_attention_work_size(), (T, k, remap, n_rows, p.gatv2_attention_work_size() // k)
            used = np.bincount(row_of, minlength=n_rows) > 0
            assert used[:i["rows_block"]].all() and int(used.sum()) == i["rows_block"] + wgs and len(row_of) == a.nnz
            counts[(T, k, remap)] = n_rows
            p.destroy()
    assert -(-2945 // 4) % 8 != 0 and (counts[(1, 8, True)], counts[(1, 8, False)]) == (748, 741)
    p = flex_amd.Plan(walk_graph(1), 8, attention=True, attention_backward=True, order=flex_amd.FLEX_ORDER_RCM)
    assert p.tuning()["xcd_slices"] == 2 and p.gatv2_attention_work_size() == 741 * 8
    p.destroy()


# ---- 2. the inputs are fair: the fp32 evaluations pass every checker, check_att among them, on every float64 case

FAIR_CASES = ([("a", f, k, H, 1) for f in FAMILIES for k, H in A_PAIRS[f]] + [("c", f, k, H, 7) for f in DROPOUT_FAMILIES for k, H in C_PAIRS[f]]
              + [("d", f, k, H, "multi") for f in FAMILIES for k, H in MULTI_EDGE_PAIRS[f]])


@pytest.mark.parametrize("c", FAIR_CASES, ids=case_id)
def test_the_fp32_evaluation_passes_every_checker_on_the_inputs_of_every_float64_case(c):
    """A condition on the inputs, not a measurement.  The rows of dAttWork are chains of fmas in entry order; measured here, the worst
    err / bound of the partial rows is about 0.011 on the undropped k = 8 case."""
    section, family, k, H, T = c
    if section == "d":
        a, first = multi_edge_graph()
        o = operands(family, k, H, a, shift_of(family, k, H))
        layout = layout_of(a, k, 64)
    else:
        o = operands(family, k, H, walk_graph(1), shift_of(family, k, H))
        a, o = walk_graph(T), (o if T == 1 else tiled_operands(o, T))
        layout = layout_of(a, k, BUDGETS[T])
    res = fp32_run(family, a, o, layout)
    each = check64(family, a, o, res, case_id(c), layout=layout)
    assert max(each.values()) <= 1.0 and {"gxt", "gxs", "gatt", "dz", "att_work"} <= set(each)
    if section == "d" and family in DROPOUT_FAMILIES:
        share, count = repeats_that_differ_in_the_mask(a, first, H, live=res["p"] > 0)
        print(f"{case_id(c)}: {share:.3f} of {count} live repeats differ in the mask")
        assert count > 100 and 0.3 < share < 0.7


# ---- 3. the two stages of gAtt: five faults against check_att

_model = {}


def _one_copy():
    """The one-copy operands at k = 8, H = 2 (every head uniform4: all finite), a right float64 result of the undropped calls on them
    and what the models of the faults need beside it: the scores s, da = <g, Xs>, delta = sum p da, L and w per head."""
    if not _model:
        a, k, H = walk_graph(1), 8, 2
        xt, xs, att = v2.operands(["uniform4"] * H, a, k, seed=2)
        g = grad(a, k, 2)
        ref = v2.reference(a, xt, xs, att, SLOPE)
        p32 = ref["p"].astype(np.float32)
        refb = v2.backward_reference(a, xt, xs, att, p32, g, SLOPE)
        row, col, _ = coo(a)
        terms = [v2.head_terms(a, xt, xs, att, SLOPE, h) for h in range(H)]
        da = np.stack([(g.astype(np.float64)[row][:, head_columns(k, H, h)] * xs.astype(np.float64)[col][:, head_columns(k, H, h)]).sum(1) for h in range(H)], axis=1)
        base64 = dict(out=ref["out"], p=ref["p"], gxt=refb["gxt"], gxs=refb["gxs"], dz=refb["dz"])
        assert all(np.isfinite(x).all() for x in base64.values())
        _model.update(a=a, o=dict(xt=xt, xs=xs, att=att, g=g), s=ref["s"], p32=p32, da=da, delta=_sum_by(p32 * da, row, a.m), base64=base64,
                      L=np.concatenate([t[2] for t in terms], 1), w=np.concatenate([t[3] for t in terms], 1))
    return _model


def _partial_rows(m, layout, keep=None):
    """The float64 rows of dAttWork of the one-copy model, rounded once; keep (bool [nnz]): the entries that reach their row."""
    row_of, n_rows = layout
    k, H = 8, 2
    terms = np.repeat(m["base64"]["dz"], k // H, axis=1) * m["L"]
    if keep is not None:
        terms = terms[keep]
        row_of = row_of[keep]
    return _sum_by(terms, row_of, n_rows).astype(np.float32)


def _check_att(m, layout, att_work, gatt, what):
    o = m["o"]
    return v2.check_att(m["a"], o["xt"], o["xs"], o["att"], m["p32"], o["g"], SLOPE, att_work, gatt, layout, what=what)


@pytest.mark.parametrize("remap", [True, False], ids=["remap", "no_remap"])
def test_check_att_accepts_the_right_model_and_rejects_the_faults_of_the_partial_rows(remap):
    """partial_restarts_per_item: a lane's partial starts from zero at every item, so only the last item of each group reaches the row.
    partial_row_of_an_idle_workgroup_unwritten: a workgroup without a group returns before the store and its row keeps the sentinel
    (the padded grid of the remap has such workgroups; without the remap there is none, and nothing to reject).
    rows_stored_at_the_unremapped_id: the row is stored at the workgroup's id after the remap, not at blockIdx.x.
    What the whole-graph bound of check_backward makes of the first is printed, not asserted: it is why check_att exists."""
    m = _one_copy()
    a, o, k = m["a"], m["o"], 8
    layout = layout_of(a, k, BUDGETS[1], remap)
    row_of, n_rows = layout
    right = _partial_rows(m, layout)
    worst = _check_att(m, layout, right, v2.att_reduce32(right), "right")
    print(f"right model, remap {remap}: worst err / bound of the partial rows {worst:.3g}")
    assert worst <= 1.0
    pl = walk_places(a.rowPtr.astype(np.int64), k, BUDGETS[1])
    row, _, _ = coo(a)
    item = pl["item"][row]
    last = np.where(item >= 0, pl["grp"][np.maximum(pl["group"][row], 0) + 1] - 1 == item, True)  # block lines keep every entry
    touched = np.zeros(n_rows, bool)
    touched[row_of[~last]] = True
    assert touched.sum() > 50
    bad = _partial_rows(m, layout, keep=last)
    assert np.array_equal(bad[~touched], right[~touched])
    with pytest.raises(AssertionError, match=r"restarts: \d+ elements in \d+ rows of dAttWork beyond the bound") as err:
        _check_att(m, layout, bad, v2.att_reduce32(bad), "restarts")
    print(f"partial_restarts_per_item, remap {remap}, {int(touched.sum())} rows touched: check_att says: {err.value}")
    for r in np.flatnonzero(touched)[::97]:  # and every row it touches is rejected on its own
        one = right.copy()
        one[r] = bad[r]
        with pytest.raises(AssertionError, match=r"elements in 1 rows of dAttWork beyond the bound"):
            _check_att(m, layout, one, v2.att_reduce32(one), "restarts, one row")
    try:
        old = v2.check_backward(a, o["xt"], o["xs"], o["att"], m["p32"], o["g"], SLOPE, gAtt=v2.att_reduce32(bad).reshape(2, 4), what="restarts")
        print(f"partial_restarts_per_item: the whole-graph check_backward ACCEPTS this gAtt, worst err / bound {old:.3g}")
    except AssertionError as e:
        print(f"partial_restarts_per_item: the whole-graph check_backward says: {e}")
    idle = np.bincount(row_of, minlength=n_rows) == 0
    assert int(idle.sum()) == (7 if remap else 0)
    if remap:
        bad = right.copy()
        bad[idle] = SENTINEL
        with pytest.raises(AssertionError, match="unwritten: 7 rows of dAttWork without entries are not \\+0"):
            _check_att(m, layout, bad, v2.att_reduce32(bad), "unwritten")
        n_b = 4
        per = (n_rows - n_b) // 8
        x = np.arange(n_rows - n_b)
        bad = right.copy()
        bad[n_b + (x % 8) * per + x // 8] = right[n_b + x]  # the row of id x lands at the id of the workgroup it runs
        assert (bad != right).any(1).sum() > 500
        with pytest.raises(AssertionError, match="unremapped: .*dAttWork"):
            _check_att(m, layout, bad, v2.att_reduce32(bad), "unremapped")


def test_the_bit_check_rejects_a_reduction_that_drops_rows_or_sums_in_one_chain():
    """reduce_drops_the_rows_past_a_multiple_of_four: the chains stop at floor(rows / 4) * 4 (741 rows without the remap: the last is
    lost).  reduce_in_one_chain: one chain over all rows.  The rows themselves are right, so only the bits of gAtt give them away."""
    m = _one_copy()
    layout = layout_of(m["a"], 8, BUDGETS[1], remap=False)
    rows = _partial_rows(m, layout)
    assert layout[1] == 741 and np.all(rows[740] != 0)
    right = v2.att_reduce32(rows)
    _check_att(m, layout, rows, right, "right")
    dropped = v2.att_reduce32(rows[:740])
    chain = np.zeros(8, np.float32)
    for r in rows:
        chain = chain + r
    for what, bad in (("drops", dropped), ("one chain", chain)):
        assert (bad.view(np.uint32) != right.view(np.uint32)).any()
        with pytest.raises(AssertionError, match=rf"{what}: gAtt has not the bits of gatt_reduce on the rows of dAttWork in \d of 8 columns"):
            _check_att(m, layout, rows, bad, what)
    nan = rows.copy()
    nan[5, 3] = np.nan  # NaN for NaN, whatever the payload
    got = v2.att_reduce32(nan)
    assert np.isnan(got[3]) and np.array_equal(got[np.arange(8) != 3], right[np.arange(8) != 3])


# ---- 4. the four multi-item faults in GATv2's own outputs, by copies

def check_copies(what, a, got, base, T):
    """Section (b) of the GPU file: Out, P, gXt, gXs and dz of the T-copy run, copy by copy, against the one-copy run; lines without
    entries +0."""
    _, col, rp = coo(a)
    empty = {"out": np.diff(rp) == 0, "gxt": np.diff(rp) == 0, "gxs": np.bincount(col, minlength=a.n) == 0}
    for key in base:
        assert_copies(what, key, got[key], base[key], T, empty=empty.get(key))


def faulty(fault, T=7, k=8, H=2):
    """The T copies of the right one-copy result as kernels with `fault` on the T-copy plan would leave them (outputs start at the
    sentinel); the faults are those of tests/test_attention_walks_host.py.  The row walk's show in Out, P, gXt and dz, the column
    walk's in gXs.  state_not_reset: the running maximum and sum of a slot are carried into the next item of the group (Out, P), and so
    is the slot's delta into gXt (dz is left right: the check tells them apart)."""
    m = _one_copy()
    a = walk_graph(T)
    x64 = {key: tile_rows(x, T) for key, x in m["base64"].items()}
    if fault is None:
        return {key: x.astype(np.float32) for key, x in x64.items()}
    row, col, rp = coo(a)
    cp = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=a.n))])
    rows, cols = walk_places(rp, k, BUDGETS[T]), walk_places(cp, k, BUDGETS[T])
    if fault == "state_not_reset":
        s = tile_rows(m["s"], T).astype(np.float64)
        M = np.full((a.m, H), -np.inf)
        np.maximum.at(M, row, s)
        L = _sum_by(np.exp(s - M[row]), row, a.m)
        items = rows["items"]
        r = np.flatnonzero(rows["later"])
        before = rows["item"][r] - 1
        slot = r - items[rows["item"][r], 2]
        has = slot < items[before, 3]
        r, rb = r[has], items[before[has], 2] + slot[has]
        live = (L[r] > 0) & (L[rb] > 0)
        factor = np.ones((a.m, H))
        with np.errstate(invalid="ignore"):
            top = np.maximum(M[r], M[rb])
            own, carried = L[r] * np.exp(M[r] - top), L[rb] * np.exp(M[rb] - top)
        factor[r] = np.where(live, own / np.where(live, own + carried, 1.0), 1.0)
        assert (factor < 0.99).sum() > 1000
        x64["p"] = x64["p"] * factor[row]
        x64["out"] = x64["out"] * np.repeat(factor, k // H, axis=1)
        carried_delta = np.zeros((a.m, H))
        carried_delta[r] = tile_rows(m["delta"], T)[rb]
        pw = _sum_by(np.repeat(tile_rows(m["p32"], T), k // H, axis=1) * tile_rows(m["w"], T), row, a.m)
        x64["gxt"] = x64["gxt"] - np.repeat(carried_delta, k // H, axis=1) * pw
        assert (np.abs(carried_delta) > 1e-3).sum() > 1000
        return {key: x.astype(np.float32) for key, x in x64.items()}
    got = {key: x.astype(np.float32) for key, x in x64.items()}
    if fault == "stops_after_the_first_item":
        for key in ("out", "gxt"):
            got[key][rows["later"]] = SENTINEL
        for key in ("p", "dz"):
            got[key][rows["later"][row]] = SENTINEL
        got["gxs"][cols["later"]] = SENTINEL
    elif fault == "last_slice_dropped":
        for pl, keys, edge in ((rows, ("out", "gxt"), ("p", "dz")), (cols, ("gxs",), ())):
            lost = pl["group"] >= 4 * 8 * (-(-pl["n_groups"] // 4) // 8)  # four groups a workgroup
            assert lost.any()
            for key in keys:
                got[key][lost] = SENTINEL
            for key in edge:
                got[key][lost[row]] = SENTINEL
    else:
        assert fault == "entries_off_by_the_first_item"
        at = np.arange(a.nnz) + rows["shift"][row]
        ok = at < a.nnz
        for key in ("p", "dz"):
            x = np.full_like(got[key], SENTINEL)
            x[at[ok]] = got[key][ok]
            got[key] = x
    return got


TOUCHED = {"stops_after_the_first_item": ("out", "p", "gxt", "dz", "gxs"), "state_not_reset": ("out", "p", "gxt"),
           "entries_off_by_the_first_item": ("p", "dz"), "last_slice_dropped": ("out", "p", "gxt", "dz", "gxs")}


def test_the_check_of_the_copies_accepts_the_right_model():
    m = _one_copy()
    base = faulty(None, T=1)
    assert set(base) == set(KEYS)
    check_copies("right", m["a"], faulty(None), base, 7)
    o = m["o"]  # the right model is a right result: both float64 checkers accept one copy of it
    assert v2.check(m["a"], o["xt"], o["xs"], o["att"], SLOPE, base["out"], base["p"]) <= 1.0
    assert v2.check_backward(m["a"], o["xt"], o["xs"], o["att"], base["p"], o["g"], SLOPE, base["gxt"], base["gxs"], dz=base["dz"]) <= 1.0


@pytest.mark.parametrize("fault", FAULTS)
def test_the_check_of_the_copies_rejects_each_fault_in_every_output_it_touches(fault):
    m = _one_copy()
    base, bad, right = faulty(None, T=1), faulty(fault), faulty(None)
    assert set(TOUCHED) == set(FAULTS)
    for key in KEYS:
        one = dict(right, **{key: bad[key]})
        if key in TOUCHED[fault]:
            with pytest.raises(AssertionError, match=rf"{fault}: {key} has not the bits of the one-copy run: first at copy \d+, row \d+, column \d+"):
                check_copies(fault, m["a"], one, base, 7)
        else:
            assert np.array_equal(bad[key], right[key])
            check_copies(fault, m["a"], one, base, 7)


# ---- 5. the dropout mask taken at entries off by the group's first item, in each of the three launches, against float64

def _dropout_model(a, o, alpha64, alpha32, kp_forward, kp_rows, kp_columns, layout):
    """fp32 (out, p, gxt, gxs, dz, att_work, gatt) of the dropout calls on finite scores, in float64 and rounded once, with the mask of
    the forward, of the row backward (da = w <g, Xs>) and of the column backward (the value term of gXs) given each on its own."""
    row, col, _ = coo(a)
    k, H = o["xs"].shape[1], o["att"].shape[0]
    c = ad.factor(DROP)
    V64, g64 = o["xs"].astype(np.float64), o["g"].astype(np.float64)
    p64 = alpha32.astype(np.float64)
    out, gxt, gxs, dz, rows_ = np.zeros((a.m, k)), np.zeros((a.m, k)), np.zeros((a.n, k)), np.zeros((a.nnz, H)), np.zeros((layout[1], k))
    for h in range(H):
        cs = head_columns(k, H, h)
        _, _, L, w = v2.head_terms(a, o["xt"], o["xs"], o["att"], SLOPE, h)
        Vh, gh = V64[col][:, cs], g64[row][:, cs]
        out[:, cs] = _sum_by((alpha64[:, h] * kp_forward[:, h] * c)[:, None] * Vh, row, a.m)
        da = kp_rows[:, h] * c * (gh * Vh).sum(1)
        dz[:, h] = p64[:, h] * (da - _sum_by(p64[:, h] * da, row, a.m)[row])
        gxt[:, cs] = _sum_by(dz[:, h, None] * w, row, a.m)
        gxs[:, cs] = _sum_by(dz[:, h, None] * w + (p64[:, h] * kp_columns[:, h] * c)[:, None] * gh, col, a.n)
        rows_[:, cs] = _sum_by(dz[:, h, None] * L, layout[0], layout[1])
    res = {key: x.astype(np.float32) for key, x in dict(out=out, p=alpha64, gxt=gxt, gxs=gxs, dz=dz, att_work=rows_).items()}
    res["gatt"] = v2.att_reduce32(res["att_work"]).reshape(H, k // H)
    return res


def test_the_float64_checks_reject_a_mask_taken_at_entries_off_by_the_first_item_in_each_launch():
    """Section (c): the mask is a hash of the entry's index in the whole graph (attention_gatv2_device.h: (pl.first + j0) * H).  A
    forward whose later items of a group take it at an entry that is off by the group's first item passes the check of P and fails that
    of Out; the row backward's first sweep then gives a wrong da, which dz, gXt and the rows of dAttWork show and the value term of gXs
    does not; the column launch reads the entry's index from its list, and one that takes the index of the entry as many places
    further in the column order as the column group's first item has gives a wrong gXs beside a right dz.  The right model passes
    everything."""
    m = _one_copy()
    T, k, H = 7, 8, 2
    a, o = walk_graph(T), tiled_operands(m["o"], T)
    layout = layout_of(a, k, BUDGETS[T])
    row, col, rp = coo(a)
    cp = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=a.n))])
    alpha64 = tile_rows(m["base64"]["p"], T)
    alpha32 = alpha64.astype(np.float32)
    e = np.arange(a.nnz, dtype=np.int64)
    right = ad.kept_entries(a, H, DROP, SEED)
    off_rows = ad.keep(SEED, DROP, (e + walk_places(rp, k, BUDGETS[T])["shift"][row]).astype(np.uint64)[:, None] * np.uint64(H) + np.arange(H, dtype=np.uint64)[None, :])
    by_column = np.argsort(col, kind="stable")  # the column launch's order of the entries
    place = np.empty(a.nnz, np.int64)
    place[by_column] = e
    off_columns = right[by_column[np.minimum(place + walk_places(cp, k, BUDGETS[T])["shift"][col], a.nnz - 1)]]
    assert (off_rows != right).mean() > 0.3 and (off_columns != right).mean() > 0.3
    xt, xs, att, g = o["xt"], o["xs"], o["att"], o["g"]
    args = (a, xt, xs, att)
    good = _dropout_model(a, o, alpha64, alpha32, right, right, right, layout)
    assert vd.check(*args, SLOPE, DROP, SEED, good["out"], good["p"], what="right") <= 1.0
    assert vd.check_backward(*args, good["p"], g, SLOPE, DROP, SEED, good["gxt"], good["gxs"], good["gatt"], good["dz"], what="right") <= 1.0
    assert v2.check_att(*args, good["p"], g, SLOPE, good["att_work"], good["gatt"], layout, drop=(DROP, SEED), what="right") <= 1.0
    bad = _dropout_model(a, o, alpha64, alpha32, off_rows, right, right, layout)  # the forward
    assert all(np.array_equal(bad[key], good[key]) for key in good if key != "out")
    with pytest.raises(AssertionError, match=r"forward: .*\bOut\b"):
        vd.check(*args, SLOPE, DROP, SEED, bad["out"], bad["p"], what="forward")
    bad = _dropout_model(a, o, alpha64, alpha32, right, off_rows, right, layout)  # the row backward
    assert np.array_equal(bad["out"], good["out"])
    with pytest.raises(AssertionError, match=r"rows: .*\bdz\b"):
        vd.check_backward(*args, bad["p"], g, SLOPE, DROP, SEED, dz=bad["dz"], what="rows")
    with pytest.raises(AssertionError, match=r"rows: .*\bgxt\b"):
        vd.check_backward(*args, bad["p"], g, SLOPE, DROP, SEED, gXt=bad["gxt"], what="rows")
    with pytest.raises(AssertionError, match=r"rows: .*\bgxs\b"):  # through the score term, which sums the dz it is given
        vd.check_backward(*args, bad["p"], g, SLOPE, DROP, SEED, gXs=bad["gxs"], what="rows")
    with pytest.raises(AssertionError, match=r"rows: .* rows of dAttWork beyond the bound"):
        v2.check_att(*args, bad["p"], g, SLOPE, bad["att_work"], bad["gatt"], layout, drop=(DROP, SEED), what="rows")
    bad = _dropout_model(a, o, alpha64, alpha32, right, right, off_columns, layout)  # the column backward: the rest is accepted, then gXs is refused
    assert all(np.array_equal(bad[key], good[key]) for key in good if key != "gxs")
    with pytest.raises(AssertionError, match=r"columns: .*\bgxs\b"):
        vd.check_backward(*args, bad["p"], g, SLOPE, DROP, SEED, gXt=bad["gxt"], gXs=bad["gxs"], dz=bad["dz"], what="columns")


# ---- 6. the references on unsorted rows and repeated pairs

@pytest.mark.parametrize("k,H", [(32, 4), (8, 1)])
def test_on_the_multi_edge_graph_the_references_agree_with_an_independent_float64_torch_evaluation(k, H):
    """gatv2_attention_ref's reference (the mask all ones, c = 1) and gatv2_dropout_ref's with the mask against torch autograd in float64
    with ad.kept_entries as a constant.  Xt and Xs are multiples of 1 / 64, att of 1 / 16 and the slope is 1 / 4, so that every score is
    exact in fp32 (tests/test_gatv2_dropout_host.py).  gAtt is the whole-graph sum, and the sum of the partial rows."""
    pytest.importorskip("torch")
    a, first = multi_edge_graph()
    slope = 0.25
    xt, xs, att = v2.operands(["uniform4", "att_signs", "spread80", "x_zero"][:H], a, k, seed=1)
    xt, xs = ((np.round(x * 64) / 64).astype(np.float32) for x in (xt, xs))
    att = (np.round(att * 16) / 16).astype(np.float32)
    g = grad(a, k, 3)
    kp, c = ad.kept_entries(a, H, DROP, SEED), ad.factor(DROP)
    share, count = repeats_that_differ_in_the_mask(a, first, H)
    assert count > 600 and 0.3 < share < 0.7
    layout = layout_of(a, k, 64)

    def agree(what, ref, refb, rows, want):
        got = (ref["out"], ref["p"], refb["gxt"], refb["gxs"], refb["gatt"], rows.sum(0).reshape(H, k // H))
        for key, x, y in zip(("Out", "P", "gXt", "gXs", "gAtt", "the rows of dAttWork"), got, want + (want[4],)):
            err = float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))
            assert err <= 1e-12, f"{what} k={k} H={H} {key}: {err:.3g}"

    ref = v2.reference(a, xt, xs, att, slope)
    agree("gatv2", ref, v2.backward_reference(a, xt, xs, att, ref["p"], g, slope), v2.att_partials_reference(a, xt, xs, att, ref["p"], g, slope, layout)[0],
          vd.torch_float64(a, xt, xs, att, slope, g, np.ones_like(kp), 1.0))
    ref = vd.reference(a, xt, xs, att, slope, DROP, SEED)
    agree("gatv2_dropout", ref, vd.backward_reference(a, xt, xs, att, ref["p"], g, slope, DROP, SEED),
          v2.att_partials_reference(a, xt, xs, att, ref["p"], g, slope, layout, drop=(DROP, SEED))[0], vd.torch_float64(a, xt, xs, att, slope, g, kp, c))

"""Host side of tests/test_gpu_gat_edge_walks.py: the kernels of the per-edge score term of the fused GAT attention (flex::gat_edge,
attention_gat_edge_kernels.hip) on walks whose group budget is above the floor of 64, on unsorted rows with repeated (row, column) pairs
and on the branch without the XCD remap.  Both kernels hold a copy of their own of the loop over a group's items, of the class pick and
of the remap, and the new operand ee is read at the entry's index in the whole matrix, which is what goes wrong on the later items of a
group; tests/test_gpu_gat_edge.py plans every graph at the floor.

Here: the table of the GPU file's cases with the kernels each launches; the budget, the items per group and the classes each case
claims, held to the plans of the host simulator; a float64 result rounded once against both checkers on the inputs of every float64 case
(the inputs are fair); numpy models of ee read at entries off by the group's first item, in the forward and in sweep 2 of the row
backward, against the float64 checkers and the check of the copies, of ee read a whole copy away, which the check of the copies accepts
on tiled operands (why section (c) of the GPU file draws its operands on the whole graph), and of P and gEe delivered in column order;
the references on the multi-edge graph against an independent float64 torch autograd evaluation.  No GPU."""
import numpy as np
import pytest

import attention_dropout_ref as ad
import flex_amd
import gat_attention_ref as gat
import gat_edge_ref as ge
from attention_forms import FORM_OF_K, FORMS
from attention_walk_graphs import BUDGETS, MIN_ITEMS_PER_GROUP, multi_edge_graph, tile_rows, walk_graph, walk_places
from flex_amd import binding
from fused_attention_ref import coo
from test_attention_walks_host import ITEMS_PER_GROUP, check_copies
from test_gat_walks_host import DROP, RANGE_COPY, SEED, case_id, grad, repeats_that_differ_in_the_mask  # noqa: F401
from test_gatv2_walks_host import NO_REMAP

hostsim = pytest.importorskip("hostsim")

SLOPE = ge.SLOPE
KEYS = ("out", "p", "gel", "ger", "gee", "gv")  # gee: what the work array holds afterwards

# ---- the table.  A case is (section, family, k, H, T); every row is dense (ldb = ldc = k)
FAMILIES = ("gat_edge", "gat_edge_dropout")  # drop_p = 0, and p = 0.5 under the seed of the sibling files
DROPOUT_FAMILIES = ("gat_edge_dropout",)
# (a) budget 128 against float64: W = 4, 8 and 16 in both families
A_PAIRS = {f: [(8, 2), (32, 4), (64, 8)] for f in FAMILIES}
# (b) budgets 512 and 2048 by copies: W = 4, 16 and 64 at T = 7, W = 4 at T = 30.  gat_edge: every output; gat_edge_dropout: P
B_PAIRS = {f: [(8, 2), (64, 8), (256, 1)] for f in FAMILIES}
# (b') ee = +0 at budget 512 against the GAT calls bit for bit: W = 16, and W = 64 (the only case that runs the row backward with DROP on
# at that width above the floor)
ZERO_PAIRS = {f: [(64, 8), (256, 1)] for f in FAMILIES}
# (c) budget 512 against float64 with the operands drawn on the whole 7-copy graph: every output at W = 4; the forward over the rows of
# copy 3 at W = 16
C_PAIRS = {f: [(8, 2)] for f in FAMILIES}
C_RANGE_PAIRS = {f: [(64, 8)] for f in FAMILIES}
# (d) the multi-edge graph against float64
MULTI_EDGE_PAIRS = {f: [(32, 4), (256, 1)] for f in FAMILIES}
# (e) the branch without the remap; (f) a captured graph, a forward without P and a backward whose work array is dWork
E_CASES = [(f, 8, 2, 1) for f in FAMILIES]
F_CASE = ("gat_edge_dropout", 8, 2, 7)
CASES = ([("a", f, k, H, 1) for f in FAMILIES for k, H in A_PAIRS[f]]
         + [("b", f, k, H, 7) for f in FAMILIES for k, H in B_PAIRS[f]] + [("b", f, *B_PAIRS[f][0], 30) for f in FAMILIES]
         + [("b0", f, k, H, 7) for f in FAMILIES for k, H in ZERO_PAIRS[f]]
         + [("c", f, k, H, 7) for f in FAMILIES for k, H in C_PAIRS[f]] + [("c_range", f, k, H, 7) for f in FAMILIES for k, H in C_RANGE_PAIRS[f]]
         + [("e",) + c for c in E_CASES] + [("f",) + F_CASE])
KERNELS = ("gat_edge_rows", "gat_edge_rows_backward")  # the column launch is the GAT family's (tests/test_gpu_gat_walks.py)
# the rotation of the ee scenarios of a pair (gat_edge_ref.edge_scenarios_of), written down: spread and cancel on the two heads of
# (8, 2), among the four of (32, 4) and the eight of (64, 8), and one each on the single head of (256, 1)
EDGE_SHIFTS = {"gat_edge": {(8, 2): 1, (32, 4): 0, (64, 8): 3, (256, 1): 1}, "gat_edge_dropout": {(8, 2): 1, (32, 4): 5, (64, 8): 4, (256, 1): 2}}


def launches(c):
    """The kernels of flex::gat_edge that a case of the table launches, as `nm -C` names them (tests/test_gat_edge_host.py: kernels_of):
    written down beside the GPU file's tests.  (b) under dropout and the range cases of (c) run the forward alone."""
    section, family, k = c[:3]
    W, NS = FORM_OF_K[k]
    drop = "true" if family in DROPOUT_FAMILIES else "false"
    names = KERNELS[:1] if section == "c_range" or (section == "b" and family in DROPOUT_FAMILIES) else KERNELS
    return [f"{kern}<{W}, {NS}, {drop}>" for kern in names]


def drop_of(family):
    """drop_p of a family's calls."""
    return DROP if family in DROPOUT_FAMILIES else 0.0


def pairs_of(family):
    return list(dict.fromkeys(A_PAIRS[family] + B_PAIRS[family] + MULTI_EDGE_PAIRS[family]))


def shift_of(family, k, H):
    """The rotation of the el / er scenarios of a pair: its place in the family's lists, so that the pairs of a family differ."""
    pairs = A_PAIRS[family] + B_PAIRS[family] + MULTI_EDGE_PAIRS[family]
    return pairs.index((k, H)) + len(family)


def scenarios(family, k, H):
    """(the el / er scenario, the ee scenario) of every head of a pair."""
    return gat.scenarios_of(H, shift=shift_of(family, k, H)), ge.edge_scenarios_of(H, shift=EDGE_SHIFTS[family][(k, H)])


_operands = {}


def operands(family, k, H, a, seed=1):
    """dict(el, er, ee, V, g) of a family's call on graph a, drawn on the whole of a.  Made once per (family, k, H, graph) and left
    unchanged."""
    key = (family, k, H, id(a), seed)
    if key not in _operands:
        el, er, ee, V = ge.operands(*scenarios(family, k, H), a, k, seed=seed)
        _operands[key] = (a, dict(el=el, er=er, ee=ee, V=V, g=grad(a, k, seed)))
    return _operands[key][1]


def tiled_operands(o, T):
    return {key: tile_rows(x, T) for key, x in o.items()}


def check64(family, a, o, got, what, rows=None, backward=True):
    """Every output of a run (host arrays) against the float64 reference under the bounds and the checkers of gat_edge_ref: the worst
    err / bound of each output, printed.  rows = (r0, r1): the forward of those rows alone, o["el"], got["out"] and got["p"] holding
    those rows and their entries; ee and the mask are taken at the entries of the whole of a."""
    each = {}
    p = drop_of(family)
    ge.check(a, o["el"], o["er"], o["ee"], o["V"], SLOPE, p, SEED, got["out"], got["p"], rows=rows, what=what, ratios=each)
    if backward:
        ge.check_backward(a, o["el"], o["er"], o["ee"], o["V"], got["p"], o["g"], SLOPE, p, SEED, got["gel"], got["ger"], got["gee"], got["gv"], what=what, ratios=each)
    print(f"{what}: worst err / bound " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))
    return each


def repeats_that_differ_in_p(p, first):
    """(differing, live): among the (entry, head) pairs of the repeated entries of the multi-edge graph with a positive P in both
    copies, how many hold other bits in the two."""
    p = np.ascontiguousarray(p, np.float32)
    rep = np.flatnonzero(first != np.arange(len(first)))
    both = (p[rep] > 0) & (p[first[rep]] > 0)
    return int((p[rep].view(np.uint32) != p[first[rep]].view(np.uint32))[both].sum()), int(both.sum())


@pytest.fixture(scope="module")
def sim():
    import os
    so = os.environ.get("FLEX_HOSTSIM_LIB") or hostsim.build()
    old_so, old_lib = binding._SO, binding._lib
    binding._SO, binding._lib = so, None
    yield binding.lib()
    binding._SO, binding._lib = old_so, old_lib


# ---- 1. what the cases claim

FLOAT64_CASES = ([("a", f, k, H, 1) for f in FAMILIES for k, H in A_PAIRS[f]] + [("c", f, k, H, 7) for f in FAMILIES for k, H in C_PAIRS[f]]
                 + [("c_range", f, k, H, 7) for f in FAMILIES for k, H in C_RANGE_PAIRS[f]] + [("d", f, k, H, "multi") for f in FAMILIES for k, H in MULTI_EDGE_PAIRS[f]])


def test_the_table_holds_what_it_is_meant_to():
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids) == 6 + 8 + 4 + 2 + 2 + 2 + 1
    assert {c[4] for c in CASES if c[0] == "a"} == {1} and {c[4] for c in CASES if c[0] == "b"} == {7, 30} and {c[4] for c in CASES if c[0] == "e"} == {1}
    assert {c[4] for c in CASES if c[0] in ("b0", "c", "c_range", "f")} == {7} and [c[2:4] for c in CASES if c[4] == 30] == [(8, 2), (8, 2)]
    assert (DROP, RANGE_COPY, NO_REMAP) == (0.5, 3, {"xcd_slices": 2}) and [drop_of(f) for f in FAMILIES] == [0.0, 0.5]
    shipped = {f"{kern}<{W}, {NS}, {drop}>" for W, NS in FORMS for kern in KERNELS for drop in ("false", "true")}  # tests/test_gat_edge_host.py: the 28
    for f in FAMILIES:
        assert A_PAIRS[f] == [(8, 2), (32, 4), (64, 8)] and B_PAIRS[f] == [(8, 2), (64, 8), (256, 1)] and MULTI_EDGE_PAIRS[f] == [(32, 4), (256, 1)]
        assert ZERO_PAIRS[f] == [(64, 8), (256, 1)] and C_PAIRS[f] == [(8, 2)] and C_RANGE_PAIRS[f] == [(64, 8)]
        rotations = [(shift_of(f, k, H) % 6, EDGE_SHIFTS[f][(k, H)]) for k, H in pairs_of(f)]
        assert len(set(rotations)) == len(rotations) == 4 and len({r[0] for r in rotations}) == 4  # they differ from pair to pair
        assert len({tuple(zip(*scenarios(f, k, H))) for k, H in pairs_of(f)}) == 4
    assert len({(shift_of(f, k, H) % 6, EDGE_SHIFTS[f][(k, H)]) for f in FAMILIES for k, H in pairs_of(f)}) == 8  # and from family to family
    # section, family, k, H and T -> the kernels: both of the family's form, the forward alone in (b) under dropout and in the range cases
    for c in CASES:
        names = launches(c)
        assert set(names) <= shipped and len(names) == (1 if c[0] == "c_range" or (c[0], c[1]) == ("b", "gat_edge_dropout") else 2), case_id(c)
        assert all(("true" in n) == (c[1] == "gat_edge_dropout") for n in names) and names[0].startswith("gat_edge_rows<")
    assert {FORM_OF_K[k][0] for k in (8, 32, 64, 256)} == {4, 8, 16, 64} and [FORM_OF_K[k] for k in (8, 32, 64, 256)] == [(4, 1), (8, 1), (16, 1), (64, 1)]
    assert {n for c in CASES for n in launches(c)} == {f"{kern}<{W}, 1, {drop}>" for W in (4, 8, 16, 64) for kern in KERNELS for drop in ("false", "true")}
    # across the float64 cases every ee scenario on some head, and spread and cancel at every W
    seen = {}
    for _, f, k, H, _ in FLOAT64_CASES:
        seen.setdefault(FORM_OF_K[k][0], set()).update(scenarios(f, k, H)[1])
    assert set().union(*seen.values()) == set(ge.EDGE_SCENARIOS) and len(ge.EDGE_SCENARIOS) == 6
    assert set(seen) == {4, 8, 16, 64} and all({"spread", "cancel"} <= names for names in seen.values()), seen


def test_every_case_plans_at_the_budget_the_items_per_group_and_the_classes_it_declares(sim):
    assert BUDGETS == {1: 128, 7: 512, 30: 2048} and MIN_ITEMS_PER_GROUP == {1: 1.5, 7: 7.5, 30: 33.0}
    seen = {}
    # (kernel, DROP, W) -> the cases at T >= 7 that run the kernel on more than 7.5 items per group
    above = {(kern, drop, W): [] for kern in KERNELS for drop in ("false", "true") for W in (4, 16, 64)}
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
        if T >= 7 and per_group[0] > 7.5:  # both kernels walk the rows
            for name in launches(c):
                kern, form = name.split("<")
                W, _, drop = form.rstrip(">").split(", ")
                above[(kern, drop, int(W))].append(case_id(c))
    for key, ids in above.items():
        assert ids, f"no case at T >= 7 launches {key[0]} with DROP {key[1]} at W = {key[2]} on a plan of more than 7.5 items per group"
    print("\n".join(f"{kern}<{W}, 1, {drop}>: {', '.join(ids)}" for (kern, drop, W), ids in above.items()))
    for f, k, H, T in E_CASES:  # (e): the knob reaches the plan and leaves the budget alone
        p = flex_amd.Plan(walk_graph(T), k, attention=True, attention_backward=True, tuning=NO_REMAP)
        assert p.tuning()["xcd_slices"] == 2 and p.attention_info()["group_budget"] == p.attention_backward_info()["group_budget"] == BUDGETS[T]
        p.destroy()


def test_the_multi_edge_cases_plan_at_the_floor_with_every_class(sim):
    a, _ = multi_edge_graph()
    for k in sorted({k for f in FAMILIES for k, _ in MULTI_EDGE_PAIRS[f]}):
        p = flex_amd.Plan(a, k, attention=True, attention_backward=True)
        p.self_check()
        fwd, bwd = p.attention_info(), p.attention_backward_info()
        assert (fwd["group_budget"], bwd["group_budget"]) == (64, 64), k
        assert min(fwd[x] for x in ("rows_empty", "rows_slot", "rows_wave", "rows_block")) > 0
        assert min(bwd[x] for x in ("columns_empty", "columns_slot", "columns_wave", "columns_block")) > 0
        p.destroy()


# ---- 2. the inputs are fair: a float64 result rounded once passes both checkers on every float64 case

FAIR_CASES = [c for c in FLOAT64_CASES if c[0] != "c_range"]  # the range cases hold the forward of (64, 8) on operands the same rule draws


@pytest.mark.parametrize("c", FAIR_CASES, ids=case_id)
def test_a_float64_result_rounded_once_passes_both_checkers_on_the_inputs_of_every_float64_case(c):
    """A condition on the inputs, not a measurement: the worst err / bound of the reference alone is at most 1.0 on all six keys (gV
    reaches the level of one rounding, 0.998, on a column of one entry where the bound is gamma(1) |p g|; halved under dropout, whose
    count is one higher).  (c) draws its operands on the whole 7-copy graph.  On the multi-edge graph the two copies of a repeated entry
    must differ in P in more than 100 live pairs, and under dropout in the mask in a share strictly between 0.3 and 0.7."""
    section, family, k, H, T = c
    first = None
    if section == "d":
        a, first = multi_edge_graph()
    else:
        a = walk_graph(T)
    o = operands(family, k, H, a)
    res = ge.fp32_result(a, o["el"], o["er"], o["ee"], o["V"], SLOPE, drop_of(family), SEED, g=o["g"])
    each = check64(family, a, o, res, case_id(c))
    assert max(each.values()) <= 1.0 and set(each) == set(KEYS)
    if section == "d":
        differ, live = repeats_that_differ_in_p(res["p"], first)
        print(f"{case_id(c)}: P differs in {differ} of {live} live repeat pairs")
        assert differ > 100
        if family in DROPOUT_FAMILIES:
            share, count = repeats_that_differ_in_the_mask(a, first, H, live=res["p"] > 0)
            print(f"{case_id(c)}: {share:.3f} of {count} live repeats differ in the mask")
            assert count > 100 and 0.3 < share < 0.7


# ---- 3. the checks have teeth: ee of the later items of a group read at other entries

_model = {}
MODEL_T, MODEL_K, MODEL_H = 7, 8, 2


def _one_copy():
    """The one-copy operands at k = 8, H = 2 -- every head uniform4 in el and er and spread in ee: all finite, and x = (el + er) + ee
    takes either sign with |ee| the larger part, so that another entry's ee moves the branch -- their tiling over the 7 copies, a right
    result of the undropped calls on both (float64 rounded once), and the row walk's places at budget 512."""
    if not _model:
        a1, a, k, H, T = walk_graph(1), walk_graph(MODEL_T), MODEL_K, MODEL_H, MODEL_T
        el, er, ee, V = ge.operands(["uniform4"] * H, ["spread"] * H, a1, k, seed=2)
        o1 = dict(el=el, er=er, ee=ee, V=V, g=grad(a1, k, 2))
        o = tiled_operands(o1, T)
        base = ge.fp32_result(a1, el, er, ee, V, SLOPE, g=o1["g"])
        right = {key: tile_rows(x, T) for key, x in base.items()}
        assert all(np.isfinite(x).all() for x in base.values()) and set(base) == set(KEYS)
        row, _, rp = coo(a)
        shift = walk_places(rp, k, BUDGETS[T])["shift"][row]
        assert (shift > 0).mean() > 0.5  # most entries lie on a later item of their group
        _model.update(a1=a1, a=a, o1=o1, o=o, base=base, right=right, shift=shift)
    return _model


def _ee_off_by_the_first_item(m, ee):
    """ee as the later items of a group would read it at entries off by the entries of the group's first item (clamped at the end)."""
    return ee[np.minimum(np.arange(len(ee)) + m["shift"], len(ee) - 1)]


def test_the_right_model_passes_both_checkers_and_the_check_of_the_copies():
    m = _one_copy()
    a, o, right = m["a"], m["o"], m["right"]
    each = check64("gat_edge", a, o, right, "right")
    assert max(each.values()) <= 1.0 and set(each) == set(KEYS)
    check_copies("right", m["a1"], right, m["base"], MODEL_T)


def test_the_forwards_ee_off_by_the_first_item_is_rejected_in_p_and_in_out_and_by_the_copies():
    """The forward loads ee at (pl.first + j0) H: a kernel whose later items of a group take pl.first off by the group's first item has
    the softmax of other scores on those rows.  gat_edge_ref.check rejects P, and Out beside the right P; on the tiled operands the
    check of the copies rejects P."""
    m = _one_copy()
    a, o, right = m["a"], m["o"], m["right"]
    bad = ge.fp32_result(a, o["el"], o["er"], _ee_off_by_the_first_item(m, o["ee"]), o["V"], SLOPE)
    args = (a, o["el"], o["er"], o["ee"], o["V"], SLOPE, 0.0, SEED)
    with pytest.raises(AssertionError, match=r"forward: .*\bP\b"):
        ge.check(*args, right["out"], bad["p"], what="forward")
    with pytest.raises(AssertionError, match=r"forward: .*\bOut\b"):
        ge.check(*args, bad["out"], right["p"], what="forward")
    for key in ("p", "out"):
        with pytest.raises(AssertionError, match=rf"forward: {key} has not the bits of the one-copy run: first at copy \d+, row \d+, column \d+"):
            check_copies("forward", m["a1"], dict(right, **{key: bad[key]}), m["base"], MODEL_T)


def test_sweep_twos_ee_off_by_the_first_item_is_rejected_in_gee_and_gel_and_leaves_gv():
    """Sweep 2 of the row backward forms x = (el + er) + Ee[e] for the branch alone: P, da and delta do not see it.  With ee of another
    entry the sign of x changes on the entries counted here, dx is dz where it should be slope dz or the reverse, and gEe and gEl show
    it (gEr sums the same dx); gV does not read dx and keeps its bits.  The heads hold spread: +-40 beside el + er within +-4."""
    m = _one_copy()
    a, o, right = m["a"], m["o"], m["right"]
    off = _ee_off_by_the_first_item(m, o["ee"])
    _, pos, _ = ge.scores(a, o["el"], o["er"], o["ee"], SLOPE)
    _, pos_off, _ = ge.scores(a, o["el"], o["er"], off, SLOPE)
    changed = int((pos != pos_off).sum())
    print(f"the sign of x changes on {changed} of {pos.size} (entry, head) pairs")
    assert changed > 1000
    bad = ge.fp32_result(a, o["el"], o["er"], off, o["V"], SLOPE, g=o["g"], probs=right["p"])  # the backward from the right P: the branch alone moves
    assert np.array_equal(bad["gv"], right["gv"]) and not np.array_equal(bad["gee"], right["gee"])
    args = (a, o["el"], o["er"], o["ee"], o["V"], right["p"], o["g"], SLOPE, 0.0, SEED)
    with pytest.raises(AssertionError, match=r"rows: .*\bgee\b"):
        ge.check_backward(*args, gEe=bad["gee"], gV=bad["gv"], what="rows")
    with pytest.raises(AssertionError, match=r"rows: .*\bgel\b"):
        ge.check_backward(*args, gEl=bad["gel"], gV=bad["gv"], what="rows")
    for key in ("gee", "gel"):
        with pytest.raises(AssertionError, match=rf"rows: {key} has not the bits of the one-copy run: first at copy \d+, row \d+, column \d+"):
            check_copies("rows", m["a1"], dict(right, **{key: bad[key]}), m["base"], MODEL_T)


def test_ee_read_a_whole_copy_away_passes_the_copies_on_tiled_operands_and_fails_float64_on_operands_of_the_whole_graph():
    """An index wrong by the entries of one copy (e + 213 658, wrapped): on tiled ee every copy holds the same numbers, the faulty kernel
    computes what the right one does, and the check of the copies ACCEPTS it -- asserted here; it is why section (c) of the GPU file
    draws ee on the whole 7-copy graph, where gat_edge_ref.check rejects the same fault."""
    m = _one_copy()
    a1, a, o = m["a1"], m["a"], m["o"]
    away = np.roll(o["ee"], -a1.nnz, axis=0)
    bad = ge.fp32_result(a, o["el"], o["er"], away, o["V"], SLOPE)
    check_copies("a copy away, tiled", a1, bad, {key: m["base"][key] for key in ("out", "p")}, MODEL_T)  # accepted
    el, er, ee, V = ge.operands(["uniform4"] * MODEL_H, ["spread"] * MODEL_H, a, MODEL_K, seed=2)  # drawn on the whole graph
    assert not np.array_equal(ee[:a1.nnz], ee[a1.nnz:2 * a1.nnz])
    args = (a, el, er, ee, V, SLOPE, 0.0, SEED)
    good = ge.fp32_result(a, el, er, ee, V, SLOPE)
    assert ge.check(*args, good["out"], good["p"], what="right") <= 1.0
    bad = ge.fp32_result(a, el, er, np.roll(ee, -a1.nnz, axis=0), V, SLOPE)
    with pytest.raises(AssertionError, match=r"a copy away: .*\bP\b"):
        ge.check(*args, good["out"], bad["p"], what="a copy away")
    with pytest.raises(AssertionError, match=r"a copy away: .*\bOut\b"):
        ge.check(*args, bad["out"], good["p"], what="a copy away")


def test_p_and_gee_ordered_by_column_within_the_row_are_rejected_and_the_csr_order_is_accepted():
    """With ee the two copies of a repeated (row, column) pair hold different scores, so "per entry, in CSR order" shows in P itself."""
    a, first = multi_edge_graph()
    k, H = 32, 4
    el, er, ee, V = ge.operands(["uniform4"] * H, ["spread", "cancel", "near_cancel", "spread"], a, k, seed=5)  # finite: every place holds a number of its own
    g = grad(a, k, 5)
    row, col, _ = coo(a)
    right = ge.fp32_result(a, el, er, ee, V, SLOPE, g=g)
    assert ge.check(a, el, er, ee, V, SLOPE, 0.0, SEED, right["out"], right["p"], what="right") <= 1.0
    assert ge.check_backward(a, el, er, ee, V, right["p"], g, SLOPE, 0.0, SEED, right["gel"], right["ger"], right["gee"], right["gv"], what="right") <= 1.0
    differ, live = repeats_that_differ_in_p(right["p"], first)
    assert differ > 100, (differ, live)
    by_column = np.lexsort((col, row))  # stable: the entries of a row by column, repeats in the order given
    assert (by_column != np.arange(a.nnz)).mean() > 0.5
    with pytest.raises(AssertionError, match=r"by column: .*\bP\b"):
        ge.check(a, el, er, ee, V, SLOPE, 0.0, SEED, right["out"], right["p"][by_column], what="by column")
    with pytest.raises(AssertionError, match=r"by column: .*\bgee\b"):
        ge.check_backward(a, el, er, ee, V, right["p"], g, SLOPE, 0.0, SEED, gEe=right["gee"][by_column], what="by column")


# ---- 4. the references on unsorted rows and repeated pairs

@pytest.mark.parametrize("p", [0.0, DROP])
@pytest.mark.parametrize("k,H", [(32, 4), (8, 1)])
def test_on_the_multi_edge_graph_the_references_agree_with_an_independent_float64_torch_evaluation(k, H, p):
    """gat_edge_ref's reference and backward_reference against torch autograd in float64, with ad.kept_entries as a constant under
    dropout.  el, er and ee are multiples of 1 / 64 and the slope is 1 / 4, so that every score is exact in fp32
    (tests/test_gat_edge_host.py).  The two copies of a repeated pair hold other ee: their P differs."""
    pytest.importorskip("torch")
    a, first = multi_edge_graph()
    slope = 0.25
    el, er, V = gat.operands(["uniform4"] * H, a, k, seed=1)
    ee = np.random.default_rng([k, H, 5]).uniform(-2, 2, (a.nnz, H))
    el, er, ee = ((np.round(x * 64) / 64 + np.float32(0)).astype(np.float32) for x in (el, er, ee))
    g = grad(a, k, 3)
    ref = ge.reference(a, el, er, ee, V, slope, p, SEED)
    refb = ge.backward_reference(a, el, er, ee, V, ref["p"], g, slope, p, SEED)  # on the float64 alpha, as torch keeps its own
    kp = ad.kept_entries(a, H, p, SEED) if p else None
    want = ge.torch_float64(a, el, er, ee, V, slope, g, kp, ad.factor(p) if p else 1.0)
    for what, x, y in zip(("Out", "P", "gEl", "gEr", "gEe", "gV"), (ref["out"], ref["p"], refb["gel"], refb["ger"], refb["gee"], refb["gv"]), want):
        err = float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))
        assert err <= 1e-12, f"multi-edge k={k} H={H} p={p} {what}: {err:.3g}"
    differ, live = repeats_that_differ_in_p(ref["p"].astype(np.float32), first)
    print(f"multi-edge k={k} H={H} p={p}: P differs in {differ} of {live} live repeat pairs")
    assert differ > 100

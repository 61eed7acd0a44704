"""Host side of tests/test_gpu_gat_walks.py: the dropout and bf16 kernels of the fused GAT attention (flex::gat_dropout, flex::gat_bf16)
on walks whose group budget is above the floor of 64 and on unsorted rows with repeated (row, column) pairs.  These kernels hold copies
of their own of the loop over a group's items, which tests/test_gpu_attention_walks.py (the undropped fp32 GAT calls) does not run.

Here: the table of the GPU file's cases; the budget, the items per group and the classes each case claims, held to the plans of the host
simulator; a float64 result rounded once against both checkers on the inputs of every float64 case (the inputs are fair) and what the
dropout cases rely on; numpy models of the four multi-item faults of tests/test_attention_walks_host.py in GAT's own outputs (Out, P,
gEl, gEr, gV, dx, fp32 and bf16 bits) against the check of the copies, and of a dropout mask taken at entries off by the group's first
item, in each of the three launches, against the float64 checkers; the references on the multi-edge graph against an independent
float64 torch autograd evaluation.  No GPU."""
import numpy as np
import pytest

import attention_dropout_ref as ad
import flex_amd
import gat_attention_ref as gat
import gat_bf16_ref as gb
import gat_dropout_ref as gd
from attention_walk_graphs import BUDGETS, MIN_ITEMS_PER_GROUP, multi_edge_graph, tile_rows, walk_graph, walk_places
from flex_amd import binding
from fused_attention_ref import coo
from multihead_attention_ref import head_columns
from test_attention_walks_host import FAULTS, ITEMS_PER_GROUP, check_copies

hostsim = pytest.importorskip("hostsim")

SLOPE = gat.SLOPE
SEED = 0x0123456789ABCDEF
DROP = 0.5
SENTINEL = np.float32(-12345.5)
FILL = np.uint16(0x5A5A)  # bf16 bits no test computes
KEYS = ("out", "p", "gel", "ger", "gv", "dx")

# ---- the table.  A case is (section, family, k, H, T); every row is dense (ldb = ldc = k)
FAMILIES = ("gat_dropout", "gat_bf16", "gat_bf16_dropout")
DROPOUT_FAMILIES = ("gat_dropout", "gat_bf16_dropout")
# (a) budget 128 against float64: W = 4 and W = 8 in every family, W = 16 where bf16 rows and the mask meet
A_PAIRS = {"gat_dropout": [(8, 2), (32, 4)], "gat_bf16": [(8, 2), (32, 4)], "gat_bf16_dropout": [(8, 2), (32, 4), (64, 8)]}
# (b) budgets 512 and 2048 by copies: W = 4, 16 and 64 at T = 7, W = 4 at T = 30.  gat_bf16: every output; the dropout families: P
B_PAIRS = {"gat_dropout": [(8, 2), (64, 8), (256, 1)], "gat_bf16": [(8, 2), (64, 8), (256, 1)], "gat_bf16_dropout": [(8, 2), (64, 8), (256, 1)]}
# (c) dropout at budget 512 against float64: every output at W = 4; the forward over the rows of copy 3 at W = 16
C_PAIRS = {"gat_dropout": [(8, 2)], "gat_bf16_dropout": [(8, 2)]}
C_RANGE_PAIRS = {"gat_dropout": [(64, 8)], "gat_bf16_dropout": [(64, 8)]}
RANGE_COPY = 3
# (d) the multi-edge graph against float64
MULTI_EDGE_PAIRS = {"gat_dropout": [(32, 4), (256, 1)], "gat_bf16": [(32, 4), (256, 1)], "gat_bf16_dropout": [(32, 4), (256, 1)]}
# (e) a captured graph and a forward without P
E_CASE = ("gat_bf16_dropout", 8, 2, 7)
CASES = ([("a", f, k, H, 1) for f in FAMILIES for k, H in A_PAIRS[f]]
         + [("b", f, k, H, 7) for f in FAMILIES for k, H in B_PAIRS[f]] + [("b", f, *B_PAIRS[f][0], 30) for f in FAMILIES]
         + [("c", f, k, H, 7) for f in DROPOUT_FAMILIES for k, H in C_PAIRS[f]]
         + [("c_range", f, k, H, 7) for f in DROPOUT_FAMILIES for k, H in C_RANGE_PAIRS[f]] + [("e",) + E_CASE])
KERNELS = ("rows", "rows_backward", "columns_backward")


def launches(c):
    """The kernels of its family that a case of the table launches: written down beside the GPU file's tests.  (b) of the dropout
    families and the range cases of (c) run the forward alone."""
    section, family = c[:2]
    return KERNELS[:1] if section == "c_range" or (section == "b" and family in DROPOUT_FAMILIES) else KERNELS


def case_id(c):
    return "-".join(str(x) for x in c[:2]) + f"-k{c[2]}-h{c[3]}-T{c[4]}"


def is_bf16(family):
    return "bf16" in family


def drop_of(family):
    """gat_bf16_ref's `drop` of a family: None, or (p, seed)."""
    return (DROP, SEED) if family in DROPOUT_FAMILIES else None


def shift_of(family, k, H):
    """The scenario rotation of a pair: its place in the family's lists, so that the pairs of a family differ."""
    pairs = A_PAIRS[family] + B_PAIRS[family] + MULTI_EDGE_PAIRS[family]
    return pairs.index((k, H)) + len(family)


def grad(a, k, seed, bf16=False):
    g = np.random.default_rng([seed, k, 80]).uniform(-1, 1, (a.m, k)).astype(np.float32)
    return gb.rounded(g) if bf16 else g


_operands = {}


def operands(family, k, H, a, shift, seed=1):
    """dict(el, er, V, g) of a family's call on graph a: a score scenario per head, rotated by `shift`; V and g hold bf16 numbers in the
    bf16 families, el and er stay float32.  Made once per (family, k, H, graph) and left unchanged."""
    key = (family, k, H, id(a), shift, seed)
    if key not in _operands:
        el, er, V = gat.operands(gat.scenarios_of(H, shift=shift), a, k, seed=seed)
        g = grad(a, k, seed, is_bf16(family))
        _operands[key] = (a, dict(el=el, er=er, V=gb.rounded(V) if is_bf16(family) else V, g=g))
    return _operands[key][1]


def tiled_operands(o, T):
    return {key: tile_rows(x, T) for key, x in o.items()}


def check64(family, a, o, got, what, rows=None, backward=True):
    """Every output of a run (host arrays; Out and gV bf16 bits in the bf16 families) against the float64 reference under the bounds and
    the checkers of the family: the worst err / bound of each output, printed.  rows = (r0, r1): the forward of those rows alone, o["el"],
    got["out"] and got["p"] holding those rows and their entries; the mask is taken at the entries of the whole of a."""
    each = {}
    el, er, V = o["el"], o["er"], o["V"]
    if family == "gat_dropout":
        gd.check(a, el, er, V, SLOPE, DROP, SEED, got["out"], got["p"], rows=rows, what=what, ratios=each)
        if backward:
            gd.check_backward(a, el, er, V, got["p"], o["g"], SLOPE, DROP, SEED, got["gel"], got["ger"], got["gv"], got["dx"], what=what, ratios=each)
    else:
        gb.check(a, el, er, V, SLOPE, got["out"], got["p"], rows=rows, drop=drop_of(family), what=what, ratios=each)
        if backward:
            gb.check_backward(a, el, er, V, got["p"], o["g"], SLOPE, got["gel"], got["ger"], got["gv"], got["dx"], drop=drop_of(family), what=what, ratios=each)
    print(f"{what}: worst err / bound " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))
    return each


def rounded_once(family, a, o):
    """A float64 evaluation with every output rounded once to its format."""
    if family == "gat_dropout":
        return gd.fp32_result(a, o["el"], o["er"], o["V"], SLOPE, DROP, SEED, g=o["g"])
    return gb.result(a, o["el"], o["er"], o["V"], SLOPE, drop_of(family), g=o["g"])


def repeats_that_differ_in_the_mask(a, first, H, live=None):
    """(share, count): among the (entry, head) pairs of the repeated entries of the multi-edge graph (those with live[e, h] and
    live[first[e], h] where given), the share whose two copies differ in kept / dropped under ad.kept_entries."""
    kp = ad.kept_entries(a, H, DROP, SEED)
    rep = np.flatnonzero(first != np.arange(a.nnz))
    use = np.ones((len(rep), H), bool) if live is None else live[rep] & live[first[rep]]
    return float((kp[rep] != kp[first[rep]])[use].mean()), int(use.sum())


@pytest.fixture(scope="module")
def sim():
    import os
    so = os.environ.get("FLEX_HOSTSIM_LIB") or hostsim.build()
    old_so, old_lib = binding._SO, binding._lib
    binding._SO, binding._lib = so, None
    yield binding.lib()
    binding._SO, binding._lib = old_so, old_lib


# ---- 1. what the cases claim

def test_the_table_holds_what_it_is_meant_to():
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids) == 7 + 9 + 3 + 2 + 2 + 1
    assert {c[4] for c in CASES if c[0] == "a"} == {1} and {c[4] for c in CASES if c[0] == "b"} == {7, 30} and {c[4] for c in CASES if c[0][0] in "ce"} == {7}
    assert [(k, H) for f in FAMILIES for k, H in A_PAIRS[f] if k == 64] == [(64, 8)] and A_PAIRS["gat_bf16_dropout"][-1] == (64, 8)
    for f in FAMILIES:
        assert A_PAIRS[f][:2] == [(8, 2), (32, 4)] and B_PAIRS[f] == [(8, 2), (64, 8), (256, 1)] and MULTI_EDGE_PAIRS[f] == [(32, 4), (256, 1)]
        shifts = [shift_of(f, k, H) for k, H in dict.fromkeys(A_PAIRS[f] + B_PAIRS[f] + MULTI_EDGE_PAIRS[f])]
        assert len(set(shifts)) == len(shifts)


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
        assert any("-T7" in i or "-T30" in i for i in ids)
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
        p.destroy()


# ---- 2. the inputs are fair: a float64 result rounded once passes both checkers of its family on every float64 case

FAIR_CASES = ([("a", f, k, H, 1) for f in FAMILIES for k, H in A_PAIRS[f]] + [("c", f, k, H, 7) for f in DROPOUT_FAMILIES for k, H in C_PAIRS[f]]
              + [("d", f, k, H, "multi") for f in FAMILIES for k, H in MULTI_EDGE_PAIRS[f]])


@pytest.mark.parametrize("c", FAIR_CASES, ids=case_id)
def test_a_float64_result_rounded_once_passes_both_checkers_on_the_inputs_of_every_float64_case(c):
    """A condition on the inputs, not a measurement: the worst err / bound of the reference alone is at most 1.0 (Out and gV near 0.996
    in bf16, the level of one rounding).  On the multi-edge graph the dropout families also need the two copies of a repeated entry to
    differ in the mask in a share of them strictly between 0.3 and 0.7, among the repeats with a positive P."""
    section, family, k, H, T = c
    if section == "d":
        a, first = multi_edge_graph()
        o = operands(family, k, H, a, shift_of(family, k, H))
    else:
        o = operands(family, k, H, walk_graph(1), shift_of(family, k, H))
        a, o = walk_graph(T), (o if T == 1 else tiled_operands(o, T))
    res = rounded_once(family, a, o)
    each = check64(family, a, o, res, case_id(c))
    assert max(each.values()) <= 1.0 and set(each) == set(KEYS)
    if section == "d" and family in DROPOUT_FAMILIES:
        share, count = repeats_that_differ_in_the_mask(a, first, H, live=res["p"] > 0)
        print(f"{case_id(c)}: {share:.3f} of {count} live repeats differ in the mask")
        assert count > 100 and 0.3 < share < 0.7


def test_the_dropout_cases_hold_fully_dropped_heads_and_long_rows_on_both_sides_of_the_mask():
    """On walk_graph(1) at H = 2, p = 0.5 and SEED, 20 746 of the 120 442 heads of rows with entries have every entry dropped (Out is
    +0 there, delta is 0): at least 1 000 are required.  A head whose entries are all kept exists among the rows of one entry and up
    (c alone scales it); among the rows of more than 32 entries (a wave's or a block's) a fully kept head has probability 2^-33 and
    does not occur at this p, so what is required of them is what the kernels meet there: every such head has kept and dropped entries,
    and the kept share of their entries lies within 0.45 .. 0.55."""
    a, H = walk_graph(1), 2
    row, _, rp = coo(a)
    kp = ad.kept_entries(a, H, DROP, SEED)
    kept, deg = np.zeros((a.m, H), np.int64), np.diff(rp)
    np.add.at(kept, row, kp)
    full = deg > 0
    dropped = int((kept[full] == 0).sum())
    print(f"{dropped} of {int(full.sum()) * H} heads of non-empty rows have every entry dropped; "
          f"{int((kept[full] == deg[full, None]).sum())} have every entry kept, the longest of {int(deg[full][(kept[full] == deg[full, None]).any(1)].max())} entries")
    assert (int(full.sum()) * H, dropped) == (120_442, 20_746)
    assert dropped >= 1000
    assert (kept[full] == deg[full, None]).sum() >= 1000
    long_ = deg > 32
    assert long_.sum() > 100 and np.all(kept[long_] > 0) and np.all(kept[long_] < deg[long_, None])
    assert 0.45 < kept[long_].sum() / (H * deg[long_].sum()) < 0.55


# ---- 3. the checks have teeth: the four multi-item faults in GAT's own outputs, by copies

_model = {}


def _sum_by(x, seg, n):
    """sum of the rows of x [entries] or [entries, j] by seg, in float64."""
    x = np.asarray(x, np.float64)
    if x.ndim == 1:
        return np.bincount(seg, weights=x, minlength=n)
    return np.stack([np.bincount(seg, weights=x[:, j], minlength=n) for j in range(x.shape[1])], axis=1)


def _one_copy():
    """The one-copy operands at k = 8, H = 2 (every head uniform4: all finite; V and g bf16 numbers, so that one set serves the fp32 and
    the bf16 bits) and a right float64 result of the undropped calls on them, with what the models of the faults need beside it: the
    scores s, the slope factor f, da = <g, V> and delta = sum p da."""
    if not _model:
        a, k, H = walk_graph(1), 8, 2
        el, er, V = gb.operands(["uniform4"] * H, a, k, seed=2)
        g = grad(a, k, 2, bf16=True)
        ref = gat.reference(a, el, er, V, SLOPE)
        p32 = ref["p"].astype(np.float32)
        refb = gat.backward_reference(a, el, er, V, p32, g, SLOPE)
        row, col, _ = coo(a)
        _, pos = gat.scores(a, el, er, SLOPE)
        f = np.where(pos, 1.0, np.float64(np.float32(SLOPE)))
        da = np.stack([(g.astype(np.float64)[row][:, head_columns(k, H, h)] * V.astype(np.float64)[col][:, head_columns(k, H, h)]).sum(1) for h in range(H)], axis=1)
        delta = _sum_by(p32 * da, row, a.m)
        base64 = dict(out=ref["out"], p=ref["p"], gel=refb["gel"], ger=refb["ger"], gv=refb["gv"], dx=refb["dx"])
        assert all(np.isfinite(x).all() for x in base64.values())
        _model.update(a=a, o=dict(el=el, er=er, V=V, g=g), s=ref["s"], f=f, p32=p32, da=da, delta=delta, base64=base64)
    return _model


def _as_run(x64, bf16):
    """A float64 result as the run's arrays: fp32 everywhere, or Out and gV as bf16 bits."""
    return {key: gb.f64_to_bf16(x) if bf16 and key in ("out", "gv") else x.astype(np.float32) for key, x in x64.items()}


def base_of(bf16):
    return _as_run(_one_copy()["base64"], bf16)


def faulty(fault, bf16, T=7, k=8, H=2):
    """The T copies of the right one-copy result as kernels with `fault` on the T-copy plan would leave them (outputs start at the
    sentinel: -12345.5, or the bf16 fill).  The row walk's faults show in Out, P, gEl and dx, the column walk's in gEr and gV:
      stops_after_the_first_item     a wave runs the first item of its group only: the lines of the later items keep the sentinel
      state_not_reset                the running maximum and sum of a slot are carried from the item before into the next of the group
                                     (Out, P), and so is the slot's delta into the sum of gEl (dx is left right: the check tells them apart)
      entries_off_by_the_first_item  P and dx of the later items of a group are written as many entries further as the group's first item has
      last_slice_dropped             the remap to XCD slices runs floor(workgroups / 8) workgroups per slice: the last groups are not run"""
    m = _one_copy()
    a = walk_graph(T)
    x64 = {key: tile_rows(x, T) for key, x in m["base64"].items()}
    if fault is None:
        return _as_run(x64, bf16)
    row, col, rp = coo(a)
    cp = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=a.n))])
    rows, cols = walk_places(rp, k, BUDGETS[T]), walk_places(cp, k, BUDGETS[T])
    if fault == "state_not_reset":  # slot s of an item starts from (M, L, delta) of slot s of the item before it in the group
        s = tile_rows(m["s"], T)
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
        x64["gel"] = x64["gel"] - carried_delta * _sum_by(tile_rows(m["f"] * m["p32"], T), row, a.m)
        assert (np.abs(carried_delta) > 1e-3).sum() > 1000
        return _as_run(x64, bf16)
    got = _as_run(x64, bf16)
    fill = {key: FILL if x.dtype == np.uint16 else SENTINEL for key, x in got.items()}
    if fault == "stops_after_the_first_item":
        for key in ("out", "gel"):
            got[key][rows["later"]] = fill[key]
        for key in ("p", "dx"):
            got[key][rows["later"][row]] = fill[key]
        for key in ("ger", "gv"):
            got[key][cols["later"]] = fill[key]
    elif fault == "last_slice_dropped":
        for pl, keys, edge in ((rows, ("out", "gel"), ("p", "dx")), (cols, ("ger", "gv"), ())):
            lost = pl["group"] >= 4 * 8 * (-(-pl["n_groups"] // 4) // 8)  # four groups a workgroup
            assert lost.any()
            for key in keys:
                got[key][lost] = fill[key]
            for key in edge:
                got[key][lost[row]] = fill[key]
    else:
        assert fault == "entries_off_by_the_first_item"
        at = np.arange(a.nnz) + rows["shift"][row]
        ok = at < a.nnz
        for key in ("p", "dx"):
            x = np.full_like(got[key], SENTINEL)
            x[at[ok]] = got[key][ok]
            got[key] = x
    return got


TOUCHED = {"stops_after_the_first_item": ("out", "p", "gel", "dx", "ger", "gv"), "state_not_reset": ("out", "p", "gel"),
           "entries_off_by_the_first_item": ("p", "dx"), "last_slice_dropped": ("out", "p", "gel", "dx", "ger", "gv")}
BITS = [False, True]
BITS_IDS = ["fp32", "bf16"]


@pytest.mark.parametrize("bf16", BITS, ids=BITS_IDS)
def test_the_check_of_the_copies_accepts_the_right_model(bf16):
    m, base = _one_copy(), base_of(bf16)
    assert base["out"].dtype == base["gv"].dtype == (np.uint16 if bf16 else np.float32) and set(base) == set(KEYS)
    check_copies("right", m["a"], faulty(None, bf16), base, 7)
    # the right model is a right result: both float64 checkers of the undropped calls accept one copy of it
    o = m["o"]
    if bf16:
        assert gb.check(m["a"], o["el"], o["er"], o["V"], SLOPE, base["out"], base["p"]) <= 1.0
        assert gb.check_backward(m["a"], o["el"], o["er"], o["V"], base["p"], o["g"], SLOPE, base["gel"], base["ger"], base["gv"], base["dx"]) <= 1.0
    else:
        assert gat.check(m["a"], o["el"], o["er"], o["V"], SLOPE, base["out"], base["p"]) <= 1.0
        assert gat.check_backward(m["a"], o["el"], o["er"], o["V"], base["p"], o["g"], SLOPE, base["gel"], base["ger"], base["gv"], base["dx"]) <= 1.0


@pytest.mark.parametrize("bf16", BITS, ids=BITS_IDS)
@pytest.mark.parametrize("fault", FAULTS)
def test_the_check_of_the_copies_rejects_each_fault_in_every_output_it_touches(fault, bf16):
    m, base = _one_copy(), base_of(bf16)
    bad, right = faulty(fault, bf16), faulty(None, bf16)
    assert set(TOUCHED) == set(FAULTS)
    for key in KEYS:
        one = dict(right, **{key: bad[key]})
        if key in TOUCHED[fault]:
            with pytest.raises(AssertionError, match=rf"{fault}: {key} has not the bits of the one-copy run: first at copy \d+, row \d+, column \d+"):
                check_copies(fault, m["a"], one, base, 7)
        else:
            assert np.array_equal(bad[key], right[key])
            check_copies(fault, m["a"], one, base, 7)
    if fault == "stops_after_the_first_item":  # the first copy's first group is whole: the report names a later place
        with pytest.raises(AssertionError, match="out has not the bits of the one-copy run: first at copy 0, row (1[6-9]|[2-9][0-9]|[1-9][0-9]{2,}),"):
            check_copies(fault, m["a"], bad, base, 7)


# ---- 4. the dropout mask taken at entries off by the group's first item, in each of the three launches, against float64

def _dropout_model(a, o, alpha64, alpha32, kp_forward, kp_rows, kp_columns):
    """fp32 (out, p, gel, ger, gv, dx) of the dropout calls on finite scores, in float64 and rounded once, with the mask of the forward,
    of the row backward (da = w <g, V>) and of the column backward (gV = sum p w g) given each on its own.  gEr sums the dx it is given,
    as the column launch sums dWork."""
    row, col, _ = coo(a)
    k, H = o["V"].shape[1], o["el"].shape[1]
    c = ad.factor(DROP)
    V64, g64 = o["V"].astype(np.float64), o["g"].astype(np.float64)
    _, pos = gat.scores(a, o["el"], o["er"], SLOPE)
    f = np.where(pos, 1.0, np.float64(np.float32(SLOPE)))
    p64 = alpha32.astype(np.float64)
    out, gv, dx = np.zeros((a.m, k)), np.zeros((a.n, k)), np.zeros((a.nnz, H))
    for h in range(H):
        cs = head_columns(k, H, h)
        Vh, gh = V64[col][:, cs], g64[row][:, cs]
        out[:, cs] = _sum_by((alpha64[:, h] * kp_forward[:, h] * c)[:, None] * Vh, row, a.m)
        da = kp_rows[:, h] * c * (gh * Vh).sum(1)
        dx[:, h] = f[:, h] * (p64[:, h] * (da - _sum_by(p64[:, h] * da, row, a.m)[row]))
        gv[:, cs] = _sum_by((p64[:, h] * kp_columns[:, h] * c)[:, None] * gh, col, a.n)
    res = dict(out=out, p=alpha64, gel=_sum_by(dx, row, a.m), ger=_sum_by(dx, col, a.n), gv=gv, dx=dx)
    return {key: x.astype(np.float32) for key, x in res.items()}


def test_the_float64_checks_reject_a_mask_taken_at_entries_off_by_the_first_item_in_each_launch():
    """Section (c): the mask is a hash of the entry's index in the whole graph.  A forward whose later items of a group take it at an
    entry that is off by the group's first item passes the check of P and fails that of Out; the row backward's first sweep then gives a
    wrong da, which dx and gEl show and gV does not; the column launch reads the entry's index from its list (ent.y), and one that takes
    the index of the entry as many places further in the column order as the column group's first item has gives a wrong gV beside a
    right gEr.  The right model passes everything."""
    m = _one_copy()
    T, k, H = 7, 8, 2
    a, o = walk_graph(T), tiled_operands(m["o"], T)
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
    el, er, V, g = o["el"], o["er"], o["V"], o["g"]
    args = (a, el, er, V)
    good = _dropout_model(a, o, alpha64, alpha32, right, right, right)
    assert gd.check(*args, SLOPE, DROP, SEED, good["out"], good["p"], what="right") <= 1.0
    assert gd.check_backward(*args, good["p"], g, SLOPE, DROP, SEED, good["gel"], good["ger"], good["gv"], good["dx"], what="right") <= 1.0
    bad = _dropout_model(a, o, alpha64, alpha32, off_rows, right, right)  # the forward
    assert all(np.array_equal(bad[key], good[key]) for key in KEYS if key != "out")
    with pytest.raises(AssertionError, match=r"forward: .*\bOut\b"):
        gd.check(*args, SLOPE, DROP, SEED, bad["out"], bad["p"], what="forward")
    with pytest.raises(AssertionError, match=r"forward: .*\bOut\b"):  # and as bf16 bits under the bf16 checker
        gb.check(*args, SLOPE, gb.to_bf16(bad["out"]), bad["p"], drop=(DROP, SEED), what="forward")
    bad = _dropout_model(a, o, alpha64, alpha32, right, off_rows, right)  # the row backward: gV is accepted, then dx is refused
    assert np.array_equal(bad["gv"], good["gv"]) and np.array_equal(bad["out"], good["out"])
    with pytest.raises(AssertionError, match=r"rows: .*\bdx\b"):
        gd.check_backward(*args, bad["p"], g, SLOPE, DROP, SEED, gV=bad["gv"], dx=bad["dx"], what="rows")
    with pytest.raises(AssertionError, match=r"rows: .*\bgel\b"):
        gd.check_backward(*args, bad["p"], g, SLOPE, DROP, SEED, gEl=bad["gel"], what="rows")
    bad = _dropout_model(a, o, alpha64, alpha32, right, right, off_columns)  # the column backward: gEr is accepted, then gV is refused
    assert all(np.array_equal(bad[key], good[key]) for key in KEYS if key != "gv")
    with pytest.raises(AssertionError, match=r"columns: .*\bgv\b"):
        gd.check_backward(*args, bad["p"], g, SLOPE, DROP, SEED, gEr=bad["ger"], gV=bad["gv"], what="columns")


# ---- 5. the references on unsorted rows and repeated pairs

@pytest.mark.parametrize("k,H", [(32, 4), (8, 1)])
def test_on_the_multi_edge_graph_the_references_agree_with_an_independent_float64_torch_evaluation(k, H):
    """gat_dropout_ref's reference with the mask, and gat_bf16_ref's on bf16 V and g with and without it, against torch autograd in
    float64 with ad.kept_entries as a constant.  el and er are multiples of 1 / 64 and the slope is 1 / 4: every score is exact in fp32
    (tests/test_gat_bf16_host.py)."""
    pytest.importorskip("torch")
    a, first = multi_edge_graph()
    slope = 0.25
    rng = np.random.default_rng([k, H, 8])
    el, er = (rng.integers(-256, 257, (r, H)).astype(np.float32) / 64 for r in (a.m, a.n))
    V = rng.uniform(-1, 1, (a.n, k)).astype(np.float32)
    g = grad(a, k, 3)
    kp, c = ad.kept_entries(a, H, DROP, SEED), ad.factor(DROP)
    share, count = repeats_that_differ_in_the_mask(a, first, H)
    assert count > 600 and 0.3 < share < 0.7

    def agree(what, ref, refb, want):
        for key, x, y in zip(("Out", "gEl", "gEr", "gV"), (ref["out"], refb["gel"], refb["ger"], refb["gv"]), want):
            err = float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))
            assert err <= 1e-12, f"{what} k={k} H={H} {key}: {err:.3g}"

    ref = gd.reference(a, el, er, V, slope, DROP, SEED)
    agree("gat_dropout", ref, gd.backward_reference(a, el, er, V, ref["p"], g, slope, DROP, SEED), gd.torch_float64(a, el, er, V, slope, g, kp, c))
    V16, g16 = gb.rounded(V), gb.rounded(g)
    for drop, mask, cc in ((None, np.ones_like(kp), 1.0), ((DROP, SEED), kp, c)):
        ref = gb.reference(a, el, er, V16, slope, drop)
        agree(f"gat_bf16 {drop}", ref, gb.backward_reference(a, el, er, V16, ref["p"], g16, slope, drop), gd.torch_float64(a, el, er, V16, slope, g16, mask, cc))

"""Host side of tests/test_gpu_attention_walks.py: the table of its cases with the group budget and the items per group each case claims,
held to the plans of the host simulator; every attention case of the older tables at the floor of 64; the check of the copies and the
float64 checkers against numpy models of four faults that only show in groups of several items; the references on a graph with unsorted
rows and repeated (row, column) pairs against independent float64 torch evaluations, and a model that delivers P and gBias ordered by
column against the checker.  No GPU."""
import numpy as np
import pytest

import attention_bf16_ref as bf
import attention_bias_ref as ab
import attention_dropout_ref as ad
import attention_forms
import flex_amd
import fused_attention_backward_ref as fb
import fused_attention_ref as fa
import gat_attention_ref as gat
import multihead_attention_ref as mh
from attention_walk_graphs import (BUDGETS, MIN_ITEMS_PER_GROUP, assert_copies, multi_edge_graph, tile_rows, walk_graph, walk_places)
from backward_ref import _directed
from flex_amd import binding
from fused_attention_backward_ref import both_sides
from fused_attention_ref import coo, threshold_graph
from softmax_ref import long_rows_graph

hostsim = pytest.importorskip("hostsim")

SCALE = 0.25
SEED = 0x0123456789ABCDEF
DROP = 0.5

# ---- the table.  A case is (section, family, k, H, T); ldb / ldc are k except in the single head's generic form (k = 30: k + 3, k + 1)
FAMILIES = ("single", "heads", "gat", "bf16", "bias_fp32", "bias_bf16")
DROPOUT_FAMILIES = ("dropout_fp32", "dropout_bf16", "dropout_bias_fp32", "dropout_bias_bf16")
# (a) budget 128 against float64: W = 4 and W = 8 in every family (the generic form at k = 30), W = 16 in the heads.  The other pairs of
# W = 16 and those of W = 32 and 64 (k = 64, 128, 256; dropout's (128, 8)) are cut: the float64 references at 213 658 entries grow with
# k, and the file is held to twice the time of tests/test_gpu_attention_dropout.py
A_PAIRS = {
    "single": [(8, 1), (32, 1)], "heads": [(8, 2), (32, 4), (64, 4)], "gat": [(8, 2), (32, 4)], "bf16": [(8, 2), (32, 4)], "bias_fp32": [(8, 2), (32, 4)],
    "bias_bf16": [(8, 2), (32, 4)], "single_generic": [(30, 1)],
    "dropout_fp32": [(8, 2)], "dropout_bf16": [(8, 2)], "dropout_bias_fp32": [(8, 2)], "dropout_bias_bf16": [(8, 2)],
}
# (b) budgets 512 and 2048 by copies: W = 4, 16 and 64 at T = 7, W = 4 at T = 30
B_PAIRS = {"single": [(8, 1), (64, 1), (256, 1)], "heads": [(8, 2), (64, 4), (256, 4)], "gat": [(8, 2), (64, 8), (256, 1)], "bf16": [(8, 2), (64, 1), (256, 4)],
           "bias_fp32": [(8, 2), (64, 1), (256, 4)], "bias_bf16": [(8, 2), (64, 1), (256, 4)]}
CASES = ([("a", f, k, H, 1) for f, pairs in A_PAIRS.items() for k, H in pairs]
         + [("b", f, k, H, 7) for f in FAMILIES for k, H in B_PAIRS[f]] + [("b", f, *B_PAIRS[f][0], 30) for f in FAMILIES]
         + [("c", f, 8, 2, 7) for f in DROPOUT_FAMILIES] + [("e", "heads", 8, 2, 7)])
# what a case claims, written down: the budget of its T (attention_walk_graphs.BUDGETS) and at least this many items per group (the grouped
# items: slot items and wave lines) in both walks, by (T, k).  Measured on the host simulator: 1.57, 3.57, 3.57, 7.55, 31.3; 7.87, 31.7,
# 126.8; 33.2
ITEMS_PER_GROUP = {(1, 8): 1.5, (1, 30): 3.5, (1, 32): 3.5, (1, 64): 7.5, (1, 256): 31.0, (7, 8): 7.5, (7, 64): 31.0, (7, 256): 126.0, (30, 8): 33.0}
MULTI_EDGE_PAIRS = {"single": [(32, 1), (256, 1)], "heads": [(32, 4), (256, 4)], "gat": [(32, 4), (256, 1)], "bf16": [(32, 4), (256, 4)],
                    "bias_fp32": [(32, 4), (256, 4)], "bias_bf16": [(32, 4), (256, 4)],
                    "dropout_fp32": [(32, 4), (256, 4)], "dropout_bf16": [(32, 4), (256, 4)], "dropout_bias_fp32": [(32, 4), (256, 4)],
                    "dropout_bias_bf16": [(32, 4), (256, 4)]}


def case_id(c):
    return "-".join(str(x) for x in c[:2]) + f"-k{c[2]}-h{c[3]}-T{c[4]}"


def leading(family, k):
    return (k + 3, k + 1) if family == "single_generic" else (k, k)


def grad(a, k, seed, bf16=False):
    g = np.random.default_rng([seed, k, 80]).uniform(-1, 1, (a.m, k)).astype(np.float32)
    return bf.rounded(g) if bf16 else g


def is_bf16(family):
    return family.endswith("bf16")


def operands(family, k, H, a, shift=0, seed=1):
    """dict of the host operands of a family's call on graph a: Q, K, V (el, er, V for GAT), g, and bias where the family has one; the
    scenario of head h rotates with `shift` as multihead_attention_ref.scenarios_of has it.  bf16 families hold bf16 numbers."""
    b16 = is_bf16(family)
    if family == "gat":
        el, er, V = gat.operands(gat.scenarios_of(H, shift=shift), a, k, seed=seed)
        return dict(el=el, er=er, V=V, g=grad(a, k, seed))
    if "bias" in family:
        Q, K, V, b = ab.operands(ab.scenarios_of(H, shift=shift), a, k, seed=seed, bf16=b16)
        return dict(Q=Q, K=K, V=V, bias=b, g=grad(a, k, seed, b16))
    if family.startswith("single"):
        Q, K, V = fa.operands(mh.scenarios_of(1, shift=shift)[0], a, k, seed=seed)
    else:
        Q, K, V = mh.operands(mh.scenarios_of(H, shift=shift), a, k, seed=seed)
    if b16:
        Q, K, V = (bf.rounded(x) for x in (Q, K, V))
    return dict(Q=Q, K=K, V=V, g=grad(a, k, seed, b16))


def shift_of(family, k, H):
    """The scenario rotation of a pair: its place in the family's lists, so that the pairs of a family differ."""
    pairs = A_PAIRS.get(family, []) + B_PAIRS.get(family, []) + MULTI_EDGE_PAIRS.get(family, [])
    return pairs.index((k, H)) + len(family)


@pytest.fixture(scope="module")
def sim():
    import os
    so = os.environ.get("FLEX_HOSTSIM_LIB") or hostsim.build()
    old_so, old_lib = binding._SO, binding._lib
    binding._SO, binding._lib = so, None
    yield binding.lib()
    binding._SO, binding._lib = old_so, old_lib


# ---- 1. what the cases claim

def test_every_case_plans_at_the_budget_and_the_items_per_group_it_declares(sim):
    assert BUDGETS == {1: 128, 7: 512, 30: 2048} and MIN_ITEMS_PER_GROUP == {1: 1.5, 7: 7.5, 30: 33.0}
    assert (walk_graph(1).m, walk_graph(1).n, walk_graph(1).nnz) == (70_000, 70_000, 213_658) and walk_graph(7).nnz == 1_495_606
    assert {c[4] for c in CASES if c[0] == "a"} == {1} and {c[4] for c in CASES if c[0] == "b"} == {7, 30} and {c[4] for c in CASES if c[0] == "c"} == {7}
    seen = {}
    for c in CASES:
        _, family, k, H, T = c
        key = (T, k) + leading(family, k)
        if key not in seen:
            a = walk_graph(T)
            p = flex_amd.Plan(a, k, attention=True, attention_backward=True, ldb=key[2], ldc=key[3])
            p.self_check()
            seen[key] = (p.attention_info(), p.attention_backward_info())
            p.destroy()
        fwd, bwd = seen[key]
        assert fwd["group_budget"] == bwd["group_budget"] == BUDGETS[T], f"{case_id(c)} declares budget {BUDGETS[T]}: the plan has {fwd['group_budget']}, {bwd['group_budget']}"
        want = ITEMS_PER_GROUP[(T, k)]
        assert want >= MIN_ITEMS_PER_GROUP[T]
        for i, blocks in ((fwd, fwd["rows_block"]), (bwd, bwd["columns_block"])):
            got = (i["items"] - blocks) / i["groups"]
            assert got >= want, f"{case_id(c)} declares {want} items per group: the plan has {got:.3g}"
        for i, keys in ((fwd, ("rows_empty", "rows_slot", "rows_wave", "rows_block")), (bwd, ("columns_empty", "columns_slot", "columns_wave", "columns_block"))):
            assert min(i[x] for x in keys) > 0, (case_id(c), i)  # every class in both walks
        assert fwd["rows_block"] == bwd["columns_block"] == 4 * T and fwd["rows_wave"] == bwd["columns_wave"]


OLD_GRAPHS = {"thresholds": threshold_graph, "thresholds_lifted": lambda: both_sides(threshold_graph()), "directed_empty": lambda: _directed(250, 260, seed=7),
              "long_rows": long_rows_graph}


def test_every_attention_case_of_the_older_tables_and_the_multi_edge_graph_are_at_the_floor(sim):
    forms = sorted({(c["k"], c["ldb"], c["ldc"]) for c in attention_forms.CASES if c["family"] != "spmm_bf16"})
    assert len(forms) >= 40
    graphs = {name: make() for name, make in OLD_GRAPHS.items()}
    graphs["multi_edge"] = multi_edge_graph()[0]
    for name, a in graphs.items():
        for k, ldb, ldc in forms:
            p = flex_amd.Plan(a, k, attention=True, attention_backward=True, ldb=ldb, ldc=ldc)
            assert (p.attention_info()["group_budget"], p.attention_backward_info()["group_budget"]) == (64, 64), (name, k)
            p.destroy()


def test_the_edge_softmax_plans_at_its_floor_on_the_older_graphs_and_at_512_on_the_seven_copies(sim):
    """flex_plan_softmax_info calls its budget group_entries (floor 256).  tests/test_gpu_attention.py runs the 7 copies for that reason."""
    for name, make in OLD_GRAPHS.items():
        assert flex_amd.Plan(make(), 32, mutable_values=True).softmax_info()["group_entries"] == 256, name
    i = flex_amd.Plan(walk_graph(7), 32, mutable_values=True).softmax_info()
    assert i["group_entries"] == 512 and i["items"] > 1.9 * i["groups"], i


def test_the_walk_model_is_the_planners_work_list(sim):
    """walk_places restates build_attention_walk; the models below stand on it."""
    for T, k in ((1, 8), (7, 8), (1, 64)):
        a = walk_graph(T)
        p = flex_amd.Plan(a, k, attention=True, attention_backward=True)
        cp = np.concatenate([[0], np.cumsum(np.bincount(a.col.astype(np.int64), minlength=a.n))])
        for i, ptr, blocks in ((p.attention_info(), a.rowPtr, "rows_block"), (p.attention_backward_info(), cp, "columns_block")):
            pl = walk_places(ptr, k, i["group_budget"])
            assert (len(pl["items"]) + i[blocks], pl["n_groups"]) == (i["items"], i["groups"])
            assert int((pl["item"] < 0).sum()) == i[blocks]
        p.destroy()


def test_the_multi_edge_graph_has_unsorted_rows_repeats_and_rows_that_cross_the_classes_by_them(sim):
    a, first = multi_edge_graph()
    base = both_sides(threshold_graph())
    row, col, rp = coo(a)
    assert (a.m, a.n) == (base.m, base.n) and 1.08 * base.nnz < a.nnz < 1.12 * base.nnz
    rep = np.flatnonzero(first != np.arange(a.nnz))
    assert len(rep) > 600 and np.all(first[rep] < rep) and np.array_equal(col[rep], col[first[rep]]) and np.array_equal(row[rep], row[first[rep]])
    unsorted = np.zeros(a.m, bool)
    unsorted[row[1:][(np.diff(col) < 0) & (np.diff(row) == 0)]] = True
    assert unsorted.sum() > 0.5 * (np.diff(rp) > 1).sum()
    deg, deg0 = np.diff(rp), np.diff(base.rowPtr.astype(np.int64))
    assert ((deg0 <= 32) & (deg > 32)).any() and ((deg0 <= 512) & (deg > 512)).any()
    cnt, cnt0 = np.bincount(col, minlength=a.n), np.bincount(base.col.astype(np.int64), minlength=a.n)
    assert ((cnt0 <= 32) & (cnt > 32)).any() and ((cnt0 <= 512) & (cnt > 512)).any()
    p = flex_amd.Plan(a, 32, attention=True, attention_backward=True)
    p.self_check()
    assert min(p.attention_info()[x] for x in ("rows_empty", "rows_slot", "rows_wave", "rows_block")) > 0
    assert min(p.attention_backward_info()[x] for x in ("columns_empty", "columns_slot", "columns_wave", "columns_block")) > 0


# ---- 2. the checks have teeth: four faults that only show in groups of several items

FAULTS = ("stops_after_the_first_item", "state_not_reset", "entries_off_by_the_first_item", "last_slice_dropped")
SENTINEL = np.float32(-12345.5)
_model = {}


def _one_copy():
    """The one-copy operands (every head uniform4: all finite) and a right fp32 result of them, at k = 8, H = 2."""
    if not _model:
        a, k, H = walk_graph(1), 8, 2
        Q, K, V = mh.operands(["uniform4"] * H, a, k, seed=2)
        g = grad(a, k, 2)
        ref = mh.reference(a, Q, K, V, SCALE, H)
        out, p = ref["out"].astype(np.float32), ref["p"].astype(np.float32)
        refb = mh.backward_reference(a, Q, K, V, p, g, SCALE, H)
        base = dict(out=out, p=p, **{key: refb[key].astype(np.float32) for key in ("gq", "gk", "gv", "ds")})
        _model.update(a=a, Q=Q, K=K, V=V, g=g, s=ref["s"], base=base)
    return _model


def faulty(fault, T=7, k=8, H=2):
    """The T copies of the right one-copy result as a kernel with `fault` on the T-copy plan would leave them (outputs start at the
    sentinel).  The row walk's faults show in Out and P, the column walk's in gK and gV:
      stops_after_the_first_item     a wave runs the first item of its group only: the lines of the later items keep the sentinel
      state_not_reset                the running maximum and sum of a slot are carried from the item before into the next of the group
      entries_off_by_the_first_item  P of the later items of a group is written as many entries further as the group's first item has
      last_slice_dropped             the remap to XCD slices runs floor(workgroups / 8) workgroups per slice: the last groups are not run"""
    m = _one_copy()
    a1, a = m["a"], walk_graph(T)
    got = {key: tile_rows(x, T) for key, x in m["base"].items()}
    if fault is None:
        return got
    row, col, rp = coo(a)
    cp = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=a.n))])
    rows, cols = walk_places(rp, k, BUDGETS[T]), walk_places(cp, k, BUDGETS[T])
    if fault == "stops_after_the_first_item":
        got["out"][rows["later"]] = SENTINEL
        got["p"][rows["later"][row]] = SENTINEL
        got["gk"][cols["later"]] = SENTINEL
        got["gv"][cols["later"]] = SENTINEL
    elif fault == "last_slice_dropped":
        for pl, keys in ((rows, ("out",)), (cols, ("gk", "gv"))):
            run = 4 * 8 * (-(-pl["n_groups"] // 4) // 8)  # four groups a workgroup
            lost = pl["group"] >= run
            assert lost.any()
            for key in keys:
                got[key][lost] = SENTINEL
        got["p"][(rows["group"] >= 4 * 8 * (-(-rows["n_groups"] // 4) // 8))[row]] = SENTINEL
    elif fault == "entries_off_by_the_first_item":
        at = np.arange(a.nnz) + rows["shift"][row]
        p = np.full_like(got["p"], SENTINEL)
        ok = at < a.nnz
        p[at[ok]] = got["p"][ok]
        got["p"] = p
    else:  # state_not_reset: slot s of an item starts from (M, L) of slot s of the item before it in the group
        s = tile_rows(m["s"], T).astype(np.float64)
        M = np.full((a.m, H), -np.inf)
        np.maximum.at(M, row, s)
        L = np.zeros((a.m, H))
        np.add.at(L, row, np.exp(SCALE * (s - M[row])))
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
            own, carried = L[r] * np.exp(SCALE * (M[r] - top)), L[rb] * np.exp(SCALE * (M[rb] - top))
        factor[r] = np.where(live, own / np.where(live, own + carried, 1.0), 1.0)
        assert (factor < 0.99).sum() > 1000
        got["p"] = (got["p"] * factor[row]).astype(np.float32)
        got["out"] = (got["out"] * np.repeat(factor, k // H, axis=1)).astype(np.float32)
    return got


def check_copies(what, a, got, base, T):
    """The check of section (b): every output of the T-copy run, copy by copy, against the one-copy run; lines without entries +0."""
    row, col, rp = coo(a)
    empty_r, empty_c = np.diff(rp) == 0, np.bincount(col, minlength=a.n) == 0
    for key in base:
        if base[key] is not None:
            assert_copies(what, key, got[key], base[key], T, empty=empty_r if key in ("out", "gq", "gel") else empty_c if key in ("gk", "gv", "ger") else None)


def test_the_check_of_the_copies_accepts_the_right_model():
    m = _one_copy()
    check_copies("right", m["a"], faulty(None), m["base"], 7)


@pytest.mark.parametrize("fault", FAULTS)
def test_the_check_of_the_copies_rejects_each_fault_in_every_output_it_touches(fault):
    m = _one_copy()
    bad, right = faulty(fault), faulty(None)
    touched = {"stops_after_the_first_item": ("out", "p", "gk", "gv"), "state_not_reset": ("out", "p"), "entries_off_by_the_first_item": ("p",),
               "last_slice_dropped": ("out", "p", "gk", "gv")}[fault]
    for key in m["base"]:
        one = dict(right, **{key: bad[key]})
        if key in touched:
            with pytest.raises(AssertionError, match=rf"{key} has not the bits of the one-copy run: first at copy \d+, row \d+, column \d+"):
                check_copies(fault, m["a"], one, m["base"], 7)
        else:
            check_copies(fault, m["a"], one, m["base"], 7)
    if fault == "stops_after_the_first_item":  # the first copy's first group is whole: the report names a later place
        with pytest.raises(AssertionError, match="first at copy 0, row (1[6-9]|[2-9][0-9]|[1-9][0-9]{2,}),"):
            check_copies(fault, m["a"], bad, m["base"], 7)


def test_the_check_of_the_copies_rejects_a_bias_read_at_entries_off_by_the_first_item():
    """The same index fault on the input side: the later items of a group read the bias as many entries further as the group's first item
    has.  P of those rows is then the softmax of other biases, which the copies give away."""
    m = _one_copy()
    T, k, H = 7, 8, 2
    a1, a = m["a"], walk_graph(T)
    bias = np.random.default_rng(9).uniform(-4, 4, (a1.nnz, H))

    def probs(g, t):
        row = coo(g)[0]
        M = np.full((g.m, H), -np.inf)
        np.maximum.at(M, row, t)
        e = np.exp(t - M[row])
        L = np.zeros((g.m, H))
        np.add.at(L, row, e)
        return (e / L[row]).astype(np.float32)

    base = probs(a1, SCALE * m["s"].astype(np.float64) + bias)
    row, _, rp = coo(a)
    shift = walk_places(rp, k, BUDGETS[T])["shift"][row]
    off = np.minimum(np.arange(a.nnz) + shift, a.nnz - 1)
    got = np.where((shift > 0)[:, None], probs(a, SCALE * tile_rows(m["s"], T).astype(np.float64) + tile_rows(bias, T)[off]), tile_rows(base, T))
    check_copies("right", a1, dict(p=tile_rows(base, T)), dict(p=base), T)
    with pytest.raises(AssertionError, match=r"p has not the bits of the one-copy run: first at copy 0, row \d+, column \d+"):
        check_copies("bias off", a1, dict(p=got), dict(p=base), T)


def test_the_float64_check_of_the_dropout_rejects_a_mask_taken_at_entries_off_by_the_first_item():
    """Section (c): the mask is a hash of the entry's index in the whole graph, so a kernel whose later items of a group index it by an
    entry that is off passes the check of P and fails the float64 check of Out."""
    m = _one_copy()
    T, k, H = 7, 8, 2
    a = walk_graph(T)
    Q, K, V = (tile_rows(m[x], T) for x in ("Q", "K", "V"))
    row, col, rp = coo(a)
    alpha = tile_rows(mh.reference(m["a"], m["Q"], m["K"], m["V"], SCALE, H)["p"], T)
    shift = walk_places(rp, k, BUDGETS[T])["shift"][row]
    e, h = np.arange(a.nnz, dtype=np.uint64)[:, None], np.arange(H, dtype=np.uint64)[None, :]
    V64 = V.astype(np.float64)
    for what, at in (("right", e), ("off", e + shift.astype(np.uint64)[:, None])):
        w = ad.keep(SEED, DROP, at * np.uint64(H) + h) * ad.factor(DROP)
        out = np.zeros((a.m, k))
        for hh in range(H):
            cs = mh.head_columns(k, H, hh)
            np.add.at(out[:, cs], row, (alpha[:, hh] * w[:, hh])[:, None] * V64[col][:, cs])
        if what == "right":
            assert ad.check(a, Q, K, V, None, SCALE, H, DROP, SEED, out.astype(np.float32), alpha.astype(np.float32), what=what) <= 1.0
        else:
            with pytest.raises(AssertionError, match="Out"):
                ad.check(a, Q, K, V, None, SCALE, H, DROP, SEED, out.astype(np.float32), alpha.astype(np.float32), what=what)


# ---- 3. unsorted rows and repeated pairs: the references, and the order of the edge arrays

def _exact_operands(a, k, H, seed):
    """Q and K multiples of 1 / 8 within +-1, the bias multiples of 1 / 64 within +-4, scale 1 / 4: every score is exact in fp32."""
    rng = np.random.default_rng([k, H, seed])
    Q, K = (rng.integers(-8, 9, (r, k)).astype(np.float32) / 8 for r in (a.m, a.n))
    V = rng.uniform(-1, 1, (a.n, k)).astype(np.float32)
    bias = rng.integers(-256, 257, (a.nnz, H)).astype(np.float32) / 64
    return Q, K, V, bias


def _agree(what, pairs):
    for key, x, y in pairs:
        if y is None:
            continue
        err = float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))
        assert err <= 1e-12, f"{what} {key}: {err:.3g}"


@pytest.mark.parametrize("k,H", [(32, 4), (8, 1)])
def test_on_the_multi_edge_graph_the_references_agree_with_independent_float64_torch_evaluations(k, H):
    """As the host files of the families have it on the sorted graphs: the biased reference, the unbiased one (a zero bias in torch), the
    single head's (H = 1), the dropout's with the mask as a constant, and GAT's."""
    torch = pytest.importorskip("torch")
    a, first = multi_edge_graph()
    Q, K, V, bias = _exact_operands(a, k, H, 7)
    g = grad(a, k, 3)
    rep = np.flatnonzero(first != np.arange(a.nnz))
    assert (bias[rep] != bias[first[rep]]).any(1).mean() > 0.9  # the two copies of a repeated entry hold different biases
    names = ("Out", "gQ", "gK", "gV", "gBias")
    ref = ab.reference(a, Q, K, V, bias, SCALE, H)
    refb = ab.backward_reference(a, Q, K, V, ref["p"], g, SCALE, H)
    _agree("bias", zip(names, (ref["out"], refb["gq"], refb["gk"], refb["gv"], refb["gb"]), ab.torch_float64(a, Q, K, V, bias, SCALE, H, g)))
    # the unbiased backward references round the p they are given to fp32: on the fp32 p they are the biased one to the last bit
    p32 = ref["p"].astype(np.float32)
    mine, theirs = ab.backward_reference(a, Q, K, V, p32, g, SCALE, H), mh.backward_reference(a, Q, K, V, p32, g, SCALE, H)
    assert all(np.array_equal(mine[key], theirs[key]) for key in ("gq", "gk", "gv", "ds"))
    plain = ab.torch_float64(a, Q, K, V, np.zeros_like(bias), SCALE, H, g)
    _agree("heads", [("Out", mh.reference(a, Q, K, V, SCALE, H)["out"], plain[0])])
    if H == 1:
        _agree("single", [("Out", fa.reference(a, Q, K, V, SCALE)["out"], plain[0])])
        one = fb.reference(a, Q, K, V, p32[:, 0], g, SCALE)
        assert all(np.array_equal(one[key], theirs[key].reshape(one[key].shape)) for key in ("gq", "gk", "gv", "ds"))
    for b in (None, bias):
        ref = ad.reference(a, Q, K, V, b, SCALE, H, 0.6, SEED)
        refb = ad.backward_reference(a, Q, K, V, ref["p"], g, SCALE, H, 0.6, SEED)
        kp = ad.kept_entries(a, H, 0.6, SEED)
        _agree("dropout", zip(names, (ref["out"], refb["gq"], refb["gk"], refb["gv"], refb["gb"]), ad.torch_float64(a, Q, K, V, b, SCALE, H, g, kp, ad.factor(0.6))))
    # GAT: el and er multiples of 1 / 64, slope 1 / 4 (tests/test_gat_attention_host.py)
    rng = np.random.default_rng([k, H, 8])
    el, er = (rng.integers(-256, 257, (r, H)).astype(np.float32) / 64 for r in (a.m, a.n))
    slope, d = 0.25, k // H
    ref = gat.reference(a, el, er, V, slope)
    refb = gat.backward_reference(a, el, er, V, ref["p"], g, slope)
    row, col, _ = coo(a)
    row_t, col_t = torch.from_numpy(row), torch.from_numpy(col)
    el_t, er_t, V_t = (torch.from_numpy(x).double().requires_grad_() for x in (el, er, V))
    s = torch.nn.functional.leaky_relu(el_t[row_t] + er_t[col_t], slope)
    M = torch.full((a.m, H), -np.inf, dtype=torch.float64).scatter_reduce(0, row_t[:, None].expand(-1, H), s.detach(), "amax")
    t = torch.exp(s - M[row_t])
    p = t / torch.zeros((a.m, H), dtype=torch.float64).index_add_(0, row_t, t)[row_t]
    out = torch.zeros((a.m, H, d), dtype=torch.float64).index_add_(0, row_t, p[:, :, None] * V_t.view(a.n, H, d)[col_t]).reshape(a.m, k)
    out.backward(torch.from_numpy(g).double())
    _agree("gat", (("Out", ref["out"], out.detach().numpy()), ("gEl", refb["gel"], el_t.grad.numpy()), ("gEr", refb["ger"], er_t.grad.numpy()),
                   ("gV", refb["gv"], V_t.grad.numpy())))


def test_p_and_gbias_ordered_by_column_within_the_row_are_rejected_and_the_csr_order_is_accepted():
    a, _ = multi_edge_graph()
    k, H = 32, 4
    o = operands("bias_fp32", k, H, a, shift=1)
    o["bias"] = np.where(np.isfinite(o["bias"]), o["bias"], np.float32(0.5))  # every entry live, so that every place holds a number of its own
    Q, K, V, bias, g = o["Q"], o["K"], o["V"], o["bias"], o["g"]
    row, col, _ = coo(a)
    right = ab.fp32_result(a, Q, K, V, bias, SCALE, H, g=g)
    assert ab.check(a, Q, K, V, bias, SCALE, H, right["out"], right["p"], what="right") <= 1.0
    assert ab.check_backward(a, Q, K, V, right["p"], g, SCALE, H, right["gq"], right["gk"], right["gv"], right["gb"], right["ds"], what="right") <= 1.0
    by_column = np.lexsort((col, row))  # stable: the entries of a row by column, repeats in the order given
    assert (by_column != np.arange(a.nnz)).mean() > 0.5
    with pytest.raises(AssertionError, match=r"\bP\b"):
        ab.check(a, Q, K, V, bias, SCALE, H, right["out"], right["p"][by_column], what="by column")
    with pytest.raises(AssertionError, match="gBias"):
        ab.check_backward(a, Q, K, V, right["p"], g, SCALE, H, gB=right["gb"][by_column], what="by column")
    with pytest.raises(AssertionError, match="ds"):
        ab.check_backward(a, Q, K, V, right["p"], g, SCALE, H, ds=right["ds"][by_column], what="by column")

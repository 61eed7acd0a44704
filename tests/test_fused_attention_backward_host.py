"""The fused attention backward's schedule on the host simulator (FLEX_PLAN_ATTENTION_BACKWARD, flex_plan_attention_backward_info): a plan
made with the flag uploads, after the forward's image, hostA's entries sorted by column and a work list over whole columns;
flex_plan_self_check verifies that second part against the input, and flex_plan_attention_backward_info accounts for every column and
entry.  Plans without the flag upload what they uploaded before.  The checker of tests/fused_attention_backward_ref.py is shown to have
teeth on numpy models of three faults."""
import ctypes as C

import numpy as np
import pytest

import flex_amd
from backward_ref import _directed
from f64ref import scenario
from flex_amd import binding
from fused_attention_backward_ref import both_sides, check, fp32_result
from fused_attention_ref import coo, expected_classes, lanes, operands, reference, threshold_graph
from softmax_ref import boundary_graph, long_rows_graph

hostsim = pytest.importorskip("hostsim")


@pytest.fixture(scope="module")
def sim():
    import os
    so = os.environ.get("FLEX_HOSTSIM_LIB") or hostsim.build()
    old_so, old_lib = binding._SO, binding._lib
    binding._SO, binding._lib = so, None
    L = binding.lib()
    L.hostsim_upload_hash.restype = C.c_uint64
    L.hostsim_upload_hash.argtypes = [C.c_int]
    yield L
    binding._SO, binding._lib = old_so, old_lib


def assert_accounts(p, a, k):
    """attention_backward_info of plan p accounts for every column and entry of a, by the classifier restated in numpy on bincount(col)."""
    i = p.attention_backward_info()
    cp = np.concatenate([[0], np.cumsum(np.bincount(a.col.astype(np.int64), minlength=a.n))])
    assert (i["columns"], i["entries"]) == (a.n, a.nnz), i
    assert (i["columns_empty"], i["columns_slot"], i["columns_wave"], i["columns_block"]) == expected_classes(cp), (i, expected_classes(cp))
    slots = 64 // lanes(k)
    short = i["columns_empty"] + i["columns_slot"]
    assert i["columns_wave"] + i["columns_block"] + -(-short // slots) <= i["items"] <= i["columns_wave"] + i["columns_block"] + short
    assert i["groups"] <= i["items"] - i["columns_block"] and (i["groups"] > 0) == (i["items"] > i["columns_block"])
    assert 64 <= i["group_budget"] <= 2048
    assert i["device_bytes"] >= 4 * (i["columns"] + 1) + 8 * i["entries"] + 16 * i["items"] + 4 * (i["groups"] + 1)
    return i


GRAPHS = {"dups": lambda: _directed(300, seed=6, dup=True), "empty_rows_cols": lambda: _directed(250, 260, seed=7), "long_rows": long_rows_graph,
          "rows_256_257": boundary_graph, "thresholds": threshold_graph, "wide_512": lambda: scenario("wide", k=32, m=512)[0],
          "thresholds_lifted": lambda: both_sides(threshold_graph()), "long_rows_lifted": lambda: both_sides(long_rows_graph())}


@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_the_flag_plans_on_every_accepted_form_and_the_image_checks(sim, graph):
    a = GRAPHS[graph]()
    for k in (8, 32, 100, 256):
        for kw in ({}, {"mutable_values": True}, {"ldb": k + 4, "ldc": k + 8}, {"tuning": {"host_threads": 1}}, {"tuning": {"host_threads": 3}},
                   {"tuning": {"host_threads": 8}}):
            p = flex_amd.Plan(a, k, attention=True, attention_backward=True, **kw)
            p.self_check()
            assert_accounts(p, a, k)


def test_the_lifted_graphs_have_every_class_in_their_columns(sim):
    for make in (threshold_graph, long_rows_graph, boundary_graph):
        a = both_sides(make())
        i = assert_accounts(flex_amd.Plan(a, 32, attention=True, attention_backward=True), a, 32)
        counts = np.bincount(a.col.astype(np.int64), minlength=a.n)
        assert np.array_equal(counts[:make().m], np.diff(make().rowPtr.astype(np.int64)))  # the columns take the rows' lengths
        if make is threshold_graph:
            assert {0, 1, 31, 32, 33, 511, 512, 513} <= set(counts.tolist()) and min(i["columns_empty"], i["columns_slot"], i["columns_wave"], i["columns_block"]) > 0


def _upload_hash(L, make):
    L.hostsim_upload_hash(1)
    p = make()
    return L.hostsim_upload_hash(1), p


def test_the_image_does_not_depend_on_the_host_threads(sim):
    for a in (both_sides(long_rows_graph()), both_sides(threshold_graph())):
        got = {t: _upload_hash(sim, lambda: flex_amd.Plan(a, 32, attention=True, attention_backward=True, tuning={"host_threads": t})) for t in (1, 3, 8)}
        assert len({h for h, _ in got.values()}) == 1
        assert len({tuple(sorted(p.attention_backward_info().items())) for _, p in got.values()}) == 1


def test_device_bytes_grow_by_what_the_info_reports_and_a_plan_without_the_flag_is_what_it_was(sim):
    for a in (long_rows_graph(), _directed(250, 260, seed=7)):
        for kw in ({}, {"mutable_values": True}):
            h0, fused = _upload_hash(sim, lambda: flex_amd.Plan(a, 32, attention=True, **kw))
            h1, both = _upload_hash(sim, lambda: flex_amd.Plan(a, 32, attention=True, attention_backward=True, **kw))
            h2, again = _upload_hash(sim, lambda: flex_amd.Plan(a, 32, attention=True, **kw))
            assert h0 == h2 and h1 != h0  # creating flag plans beside it changes nothing of a plan without the flag
            assert both.info()["device_bytes"] - both.attention_backward_info()["device_bytes"] == fused.info()["device_bytes"] == again.info()["device_bytes"]
            assert both.attention_backward_info()["device_bytes"] > 0
            assert both.attention_info() == fused.attention_info()
            for key in ("n_tasks", "n_chunks", "n_records", "n_slots", "lanes_per_nz"):
                assert both.info()[key] == fused.info()[key]
            with pytest.raises(binding.FlexError, match="invalid"):
                fused.attention_backward_info()


def test_the_flag_is_refused_without_attention_with_transpose_with_maps_and_with_a_row_range(sim):
    a = scenario("wide", k=32, m=600)[0]
    vo, ap = flex_amd.perm_csr(a, flex_amd.order_rcm(a))
    ident = np.arange(a.n, dtype=np.int32)
    for kw in ({}, {"mutable_values": True}, {"tuning": {"host_threads": 1}}):
        with pytest.raises(binding.FlexError, match="invalid"):
            flex_amd.Plan(a, 32, attention_backward=True, **kw)
    for kw in ({"transpose": True}, {"vo_mp": vo}, {"col_map": ident, "tuning": {"host_threads": 1}}, {"rows": (0, 100)}, {"rows": (0, a.m)},
               {"rows": (0, 100), "tuning": {"host_threads": 1}}, {"transpose": True, "mutable_values": True}):
        with pytest.raises(binding.FlexError, match="not supported"):
            flex_amd.Plan(ap if "vo_mp" in kw else a, 32, attention=True, attention_backward=True, **kw)


# ---- the checker has teeth

def _case(k=32, scale=0.125):
    a = both_sides(threshold_graph())
    Q, K, V = operands("uniform4", a, k, seed=3)
    p = reference(a, Q, K, V, scale)["p"].astype(np.float32)
    g = np.random.default_rng(4).uniform(-1, 1, (a.m, k)).astype(np.float32)
    return a, Q, K, V, p, g, scale


def test_the_checker_passes_a_float64_evaluation_rounded_to_fp32():
    a, Q, K, V, p, g, scale = _case()
    gq, gk, gv, ds = fp32_result(a, Q, K, V, p, g, scale)
    assert check(a, Q, K, V, p, g, scale, gq, gk, gv, ds, what="identity") < 1.0


@pytest.mark.parametrize("fault", ["entry_dropped", "unweighted_delta", "scale_left_out"])
def test_the_checker_fails_a_faulty_result(fault):
    a, Q, K, V, p, g, scale = _case()
    _, col, _ = coo(a)
    c = int(np.argmax(np.bincount(col, minlength=a.n)))  # a long column: 513 entries
    right = fp32_result(a, Q, K, V, p, g, scale)
    in_c = np.flatnonzero(col == c)
    e = int(in_c[np.argmax(np.abs(right[3][in_c]))])  # not one of a row with a single entry, whose ds is exactly 0: gK could not miss it
    kw = {"entry_dropped": dict(drop_entry=e), "unweighted_delta": dict(unweighted_delta=True),
          "scale_left_out": dict(no_scale=True)}[fault]
    gq, gk, gv, ds = fp32_result(a, Q, K, V, p, g, scale, **kw)
    for key, bad in (("gK", gk), ("gV", gv)) if fault == "entry_dropped" else (("gQ", gq), ("gK", gk), ("ds", ds)):
        with pytest.raises(AssertionError, match="beyond the bound"):  # each output the fault touches shows it on its own
            check(a, Q, K, V, p, g, scale, **{key: bad}, what=fault)
    with pytest.raises(AssertionError, match="beyond the bound"):
        check(a, Q, K, V, p, g, scale, gq, gk, gv, ds, what=fault)
    assert check(a, Q, K, V, p, g, scale, *right, what="right") < 1.0

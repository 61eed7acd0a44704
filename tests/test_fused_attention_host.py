"""The fused attention's schedule on the host simulator (FLEX_PLAN_ATTENTION, flex_plan_attention_info; internal.h, kAtPass): a plan made
with the flag uploads hostA's row pointer and columns for its rows and a work list over whole rows, flex_plan_self_check verifies that
image against the input, and flex_plan_attention_info accounts for every row and entry.  Plans without the flag upload nothing for it.
The checker of tests/fused_attention_ref.py is shown to have teeth on numpy models of three faults."""
import ctypes as C

import numpy as np
import pytest

import flex_amd
from backward_ref import _directed
from f64ref import scenario
from flex_amd import binding
from fused_attention_ref import check, expected_classes, fp32_result, lanes, operands, threshold_graph
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


def assert_accounts(p, rp, k):
    """attention_info of plan p accounts for every row and entry of the row pointer slice rp, by the classifier restated in numpy."""
    i = p.attention_info()
    rp = np.asarray(rp, np.int64)
    assert (i["rows"], i["entries"]) == (len(rp) - 1, int(rp[-1] - rp[0])), i
    assert (i["rows_empty"], i["rows_slot"], i["rows_wave"], i["rows_block"]) == expected_classes(rp), (i, expected_classes(rp))
    slots = 64 // lanes(k)
    short = i["rows_empty"] + i["rows_slot"]
    assert i["rows_wave"] + i["rows_block"] + -(-short // slots) <= i["items"] <= i["rows_wave"] + i["rows_block"] + short
    assert i["groups"] <= i["items"] - i["rows_block"] and (i["groups"] > 0) == (i["items"] > i["rows_block"])
    assert 64 <= i["group_budget"] <= 2048
    assert i["device_bytes"] >= 4 * (i["rows"] + 1) + 4 * i["entries"] + 16 * i["items"] + 4 * (i["groups"] + 1)
    return i


GRAPHS = {"dups": lambda: _directed(300, seed=6, dup=True), "empty_rows_cols": lambda: _directed(250, 260, seed=7), "long_rows": long_rows_graph,
          "rows_256_257": boundary_graph, "thresholds": threshold_graph, "wide_512": lambda: scenario("wide", k=32, m=512)[0]}


@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_the_flag_plans_on_every_accepted_form_and_the_image_checks(sim, graph):
    a = GRAPHS[graph]()
    for k in (8, 32, 100, 256):
        for kw in ({}, {"mutable_values": True}, {"ldb": k + 4, "ldc": k + 8}, {"tuning": {"host_threads": 2}}):
            p = flex_amd.Plan(a, k, attention=True, **kw)
            p.self_check()
            assert_accounts(p, a.rowPtr, k)
        cuts = [0, 17, 17, min(101, a.m), a.m]  # an empty shard among them
        seen = np.zeros(4, np.int64)
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            p = flex_amd.Plan(a, k, rows=(r0, r1), attention=True, mutable_values=True)
            p.self_check()
            i = assert_accounts(p, a.rowPtr[r0:r1 + 1], k)
            seen += [i["rows_empty"], i["rows_slot"], i["rows_wave"], i["rows_block"]]
        assert tuple(seen) == expected_classes(a.rowPtr)


def test_the_flag_is_refused_with_transpose_and_with_maps(sim):
    a = scenario("wide", k=32, m=600)[0]
    vo, ap = flex_amd.perm_csr(a, flex_amd.order_rcm(a))
    ident = np.arange(a.n, dtype=np.int32)
    for kw in ({"transpose": True}, {"vo_mp": vo}, {"rows": (0, 100), "col_map": ident}, {"col_map": ident, "tuning": {"host_threads": 1}},
               {"transpose": True, "mutable_values": True}):
        with pytest.raises(binding.FlexError, match="not supported"):
            flex_amd.Plan(ap if "vo_mp" in kw else a, 32, attention=True, **kw)
    plain = flex_amd.Plan(a, 32, mutable_values=True)
    with pytest.raises(binding.FlexError, match="invalid"):
        plain.attention_info()


def _upload_hash(L, make):
    L.hostsim_upload_hash(1)
    p = make()
    return L.hostsim_upload_hash(1), p


def test_the_image_does_not_depend_on_the_host_threads(sim):
    for a in (long_rows_graph(), threshold_graph()):
        got = {t: _upload_hash(sim, lambda: flex_amd.Plan(a, 32, attention=True, tuning={"host_threads": t})) for t in (1, 3, 8)}
        assert len({h for h, _ in got.values()}) == 1
        assert len({tuple(sorted(p.attention_info().items())) for _, p in got.values()}) == 1


def test_device_bytes_grow_by_what_the_info_reports_and_not_at_all_without_the_flag(sim):
    for a in (long_rows_graph(), _directed(250, 260, seed=7)):
        for kw in ({}, {"mutable_values": True}, {"rows": (10, 200)}):
            h0, plain = _upload_hash(sim, lambda: flex_amd.Plan(a, 32, **kw))
            h1, again = _upload_hash(sim, lambda: flex_amd.Plan(a, 32, **kw))
            h2, fused = _upload_hash(sim, lambda: flex_amd.Plan(a, 32, attention=True, **kw))
            assert h0 == h1 and h2 != h0
            assert fused.info()["device_bytes"] - plain.info()["device_bytes"] == fused.attention_info()["device_bytes"] > 0
            assert plain.info()["device_bytes"] == again.info()["device_bytes"]
            for key in ("n_tasks", "n_chunks", "n_records", "n_slots", "lanes_per_nz"):  # the SpMM's plan is what it is without the flag
                assert fused.info()[key] == plain.info()[key]


# ---- the checker has teeth

def _case(k=32):
    a = long_rows_graph()
    return (a,) + operands("uniform4", a, k, seed=3)


def test_the_checker_passes_a_float64_evaluation_rounded_to_fp32():
    a, Q, K, V = _case()
    for scale in (1.0, 0.125):
        out, p = fp32_result(a, Q, K, V, scale)
        assert check(a, Q, K, V, scale, out, p, what="identity") < 1.0
    r0, r1 = 90, 260
    out, p = fp32_result(a, Q[r0:r1], K, V, 0.125, rows=(r0, r1))
    assert check(a, Q[r0:r1], K, V, 0.125, out, p, rows=(r0, r1), what="shard") < 1.0


@pytest.mark.parametrize("fault", ["entry_dropped", "scale_left_out", "wrong_rows_sum"])
def test_the_checker_fails_a_faulty_result(fault):
    a, Q, K, V = _case()
    rp = a.rowPtr.astype(np.int64)
    r = int(np.flatnonzero(np.diff(rp) == 5)[0])
    kw = {"entry_dropped": dict(drop_entry=int(rp[r]) + 2), "scale_left_out": dict(no_scale=True), "wrong_rows_sum": dict(wrong_sum=(r, 17))}[fault]
    out, p = fp32_result(a, Q, K, V, 0.125, **kw)
    with pytest.raises(AssertionError, match="beyond the bound"):
        check(a, Q, K, V, 0.125, out, what=fault)  # Out alone shows it
    with pytest.raises(AssertionError, match="beyond the bound"):
        check(a, Q, K, V, 0.125, fp32_result(a, Q, K, V, 0.125)[0], p, what=fault)  # and so does P next to a right Out

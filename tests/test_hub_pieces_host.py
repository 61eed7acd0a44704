"""Hub rows cut by schedule window (flex_plan_tuning.hub_row; plan_build.cpp, cut_hub_rows) WITHOUT a GPU: the plans are created
through the host-simulated library and verified by flex_plan_self_check.  What moves is counted against the rule applied to the CSR in
numpy (tests/hub_graphs.py, expected_moves); the image does not depend on the host thread count; and the kinds of plan the cut is not
for -- a row shard, FLEX_PLAN_MUTABLE_VALUES, FLEX_PLAN_ATTENTION, FLEX_PLAN_TRANSPOSE, a plan whose hot blocks were taken, the 2-D
schedule -- upload the image they upload with the cut forced off."""
import ctypes as C
import os

import numpy as np
import pytest

import flex_amd
from flex_amd import binding
from hub_graphs import EMPTY_HOME, KNOBS, N, OFF, W, expected_moved_pieces, expected_moves, hub_graph

hostsim = pytest.importorskip("hostsim")


@pytest.fixture(scope="module")
def sim():
    so = os.environ.get("FLEX_HOSTSIM_LIB") or hostsim.build()
    old_so, old_lib = binding._SO, binding._lib
    binding._SO, binding._lib = so, None
    L = binding.lib()
    L.hostsim_upload_hash.restype = C.c_uint64
    L.hostsim_upload_hash.argtypes = [C.c_int]
    yield L
    binding._SO, binding._lib = old_so, old_lib


@pytest.fixture(scope="module")
def graph():
    return hub_graph()


def image_of(sim, *args, **kw):
    sim.hostsim_upload_hash(1)
    p = flex_amd.Plan(*args, **kw)
    image = sim.hostsim_upload_hash(1)
    p.self_check()
    return image, p


def test_what_moves_is_what_the_rule_says(sim, graph):
    runs, records, empty_home = expected_moves(graph)
    assert runs > 100 and empty_home >= 1  # EMPTY_HOME, at least
    rp = graph.rowPtr.astype(np.int64)
    assert rp[EMPTY_HOME + 1] - rp[EMPTY_HOME] == 300
    for k, extra in ((32, {}), (128, {}), (128, {"rec_pack": 1}), (100, {}), (102, {}), (16, {"lanes_per_nz": 8}), (32, {"bundle": 2})):
        p = flex_amd.Plan(graph, k, tuning=dict(KNOBS, **extra))
        p.self_check()
        i, t = p.info(), p.tuning()
        assert (t["hub_row"], t["hub_window"], t["hub_min_run"]) == (256, W, 4)
        assert i["moved_records"] == records and i["n_moved_pieces"] >= runs, (i, runs, records)
        # a run longer than one budget (LONG_RUN: 250 records against 128) is cut by length as well
        assert i["n_moved_pieces"] == expected_moved_pieces(graph, 64 // i["lanes_per_nz"]) > runs
        off = flex_amd.Plan(graph, k, tuning=dict(OFF, **extra))
        off.self_check()
        io, to = off.info(), off.tuning()
        assert (to["hub_row"], to["hub_window"], to["hub_min_run"]) == (1, 1, 1) and io["n_moved_pieces"] == 0 and io["moved_records"] == 0
        assert i["n_partials"] > io["n_partials"] and i["nnz"] == io["nnz"] == graph.nnz
    # without the knob the rule decides, and a graph that does not fill the chip is not cut
    rule = flex_amd.Plan(graph, 128)
    assert rule.tuning()["hub_row"] == 1 and rule.info()["n_moved_pieces"] == 0
    for knob in ("hub_row", "hub_window", "hub_min_run"):  # 1 in any of the three forces the cut off
        assert flex_amd.Plan(graph, 128, tuning=dict(KNOBS, **{knob: 1})).info()["n_moved_pieces"] == 0


def test_every_record_is_kept_once(sim, graph):
    """The stream of the cut plan names every B row at least as often as the CSR does, and what it names beyond that is exactly the
    padding (which repeats a B row of its task; the values, which the padding rule may spread over the padded records, are the GPU
    tests' business)."""
    want = np.bincount(graph.col, minlength=N)
    for tn in (dict(KNOBS, bundle=2), dict(KNOBS, rec_pack=1), dict(OFF, bundle=2)):
        p = flex_amd.Plan(graph, 128, tuning=tn)
        got = np.bincount(p.records()[:, 0] // 512, minlength=N)
        assert len(got) == N and np.all(got >= want) and got.sum() - want.sum() == p.info()["n_records"] - graph.nnz


def test_more_than_256_pieces_on_one_row(sim, graph):
    rp, col = graph.rowPtr.astype(np.int64), graph.col.astype(np.int64)
    w, cnt = np.unique(col[rp[5]:rp[6]] // W, return_counts=True)
    pieces = sum(-(-int(c) // 8) if c > 128 else 1 for c in cnt[w != 0])
    assert pieces > 256
    p = flex_amd.Plan(graph, 128, tuning=dict(KNOBS, piece_records=8))
    p.self_check()
    assert p.info()["n_partials"] > pieces and p.info()["n_moved_pieces"] == expected_moved_pieces(graph, 64 // p.info()["lanes_per_nz"], dict(KNOBS, piece_records=8)) > pieces


def test_tiny_pieces_among_empty_rows_respect_the_chunk_limit(sim):
    a = hub_graph(seed=1, tiny_pieces=True)
    for extra in ({"chunk_records": 512, "row_cost": 1}, {"chunk_records": 512, "row_cost": 1, "bundle": 2}, {}):
        tn = dict(KNOBS, **extra)
        p = flex_amd.Plan(a, 32, tuning=tn)
        p.self_check()  # at most 63 tasks per chunk, among much else
        assert p.info()["lanes_per_nz"] == 8 and p.info()["n_moved_pieces"] == expected_moved_pieces(a, 8, tn)
    assert expected_moves(a)[0] == expected_moves(hub_graph(seed=1))[0] + 100  # the hundred tiny pieces, one run each


def test_image_does_not_depend_on_the_thread_count(sim, graph):
    g = flex_amd.synth_graph(n=20000, nnz=20000 + 2 * 400000, community=256, p_in=0.6, p_near=0.25, seed=9)
    cases = [(graph, 128, flex_amd.FLEX_ORDER_NATURAL, KNOBS), (graph, 32, flex_amd.FLEX_ORDER_NATURAL, dict(KNOBS, rec_pack=1)),
             (g, 128, flex_amd.FLEX_ORDER_CLUSTER, {"hub_row": 64, "hub_window": 1024, "hub_min_run": 4})]
    for mat, k, order, tn in cases:
        shapes = []
        for threads in (1, 3, 8):
            image, p = image_of(sim, mat, k, order=order, tuning=dict(tn, host_threads=threads))
            i = p.info()
            assert i["n_moved_pieces"] > 0
            shapes.append((image, i["n_tasks"], i["n_chunks"], i["n_partials"], i["n_records"], i["n_moved_pieces"], i["moved_records"]))
        assert shapes[0] == shapes[1] == shapes[2], tn


def test_mapped_and_reordered_plans(sim, graph):
    """A mapped loader's ids are schedule positions (the windows are those of the permuted ids); under the community order the
    windows are cut in the schedule, not in the ids."""
    runs, records, _ = expected_moves(graph)
    vo = np.random.default_rng(3).permutation(N).astype(np.int32)
    p = flex_amd.Plan(graph, 128, vo_mp=vo, tuning=KNOBS)
    p.self_check()
    assert p.info()["moved_records"] == records
    c = flex_amd.Plan(graph, 128, order=flex_amd.FLEX_ORDER_CLUSTER, tuning=KNOBS)
    c.self_check()
    assert c.info()["moved_records"] > 0 and c.tuning()["hub_row"] == 256
    # BFS-like orders run round-robin over the XCDs: no window belongs to one L2, nothing is cut
    r = flex_amd.Plan(graph, 128, order=flex_amd.FLEX_ORDER_RCM, tuning=KNOBS)
    assert r.info()["n_moved_pieces"] == 0 and r.tuning()["hub_row"] == 1


EXCLUDED = {
    "shard": dict(rows=(0, N)),
    "mutable": dict(mutable_values=True),
    "attention": dict(attention=True),
    "transposed": dict(transpose=True),
    "two_d": dict(tuning={"two_d": 1}),
}


@pytest.mark.parametrize("kind", list(EXCLUDED))
def test_excluded_kinds_build_the_image_of_the_cut_forced_off(sim, graph, kind):
    kw = dict(EXCLUDED[kind])
    extra = kw.pop("tuning", {})
    k = 32 if kind == "attention" else 64
    on, p = image_of(sim, graph, k, tuning=dict(KNOBS, **extra), **kw)
    off, q = image_of(sim, graph, k, tuning=dict(OFF, **extra), **kw)
    assert on == off and p.info()["n_moved_pieces"] == 0 and p.tuning()["hub_row"] == 1
    assert p.info()["n_tasks"] == q.info()["n_tasks"]
    ctl, c = image_of(sim, graph, k, tuning=dict(KNOBS, **extra if kind != "two_d" else {}))  # the plain plan of the same input is cut
    assert c.info()["n_moved_pieces"] > 0 and ctl != off


def test_hot_blocks_taken_keep_their_rows_whole(sim):
    g = flex_amd.synth_graph(n=12000, nnz=12000 + 2 * 240000, community=300, p_in=0.6, p_near=0.25, seed=12)
    hub = {"hub_row": 64, "hub_window": 1024, "hub_min_run": 4}
    on, p = image_of(sim, g, 64, order=flex_amd.FLEX_ORDER_CLUSTER, tuning=dict(hub, blocks=1))
    off, _ = image_of(sim, g, 64, order=flex_amd.FLEX_ORDER_CLUSTER, tuning=dict(hub, blocks=1, hub_row=1))
    assert p.info()["n_blocks"] > 0 and on == off and p.info()["n_moved_pieces"] == 0
    _, flat = image_of(sim, g, 64, order=flex_amd.FLEX_ORDER_CLUSTER, tuning=dict(hub, blocks=2))
    assert flat.info()["n_moved_pieces"] > 0


def test_the_rule_without_knobs(sim):
    """No knob: the cut is on when the plan fills the chip (a chunk per wave slot of the card) and the rows of at least 1024 records
    hold a tenth of the nonzeros -- with the measured defaults 1024 / 8192 / 32 -- and off otherwise."""
    seen = set()
    for n, nnz, alpha in ((60000, 60000 + 2 * 2600000, 1.6), (60000, 60000 + 2 * 2600000, 2.6), (20000, 20000 + 2 * 400000, 1.6)):
        g = flex_amd.synth_graph(n=n, nnz=nnz, alpha=alpha, community=500, p_in=0.55, p_near=0.3, seed=6)
        deg = np.diff(g.rowPtr.astype(np.int64))
        fills = (g.nnz + 16.0 * g.m) / min(max(16.0 * g.nnz / g.m, 128.0), 512.0) >= 8192.0
        want = bool(fills and 10 * deg[deg >= 1024].sum() >= g.nnz)
        p = flex_amd.Plan(g, 128, order=flex_amd.FLEX_ORDER_CLUSTER)
        p.self_check()
        t, i = p.tuning(), p.info()
        assert (t["hub_row"], t["hub_window"], t["hub_min_run"]) == ((1024, 8192, 32) if want else (1, 1, 1)), (n, nnz, alpha, t)
        assert (i["n_moved_pieces"] > 0) == want
        seen.add(want)
    assert seen == {True, False}

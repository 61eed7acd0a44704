"""The packed record stream (flex_plan_tuning.rec_pack) WITHOUT a GPU: plans are created through the host-simulated
library with rec_pack = 1 and rec_pack = 2, the packed device image is decoded by the decoder of flex_plan_self_check
(flex_plan_read_records) and must give the unpacked plan's records exactly; the image must not depend on the host thread count."""
import ctypes as C
import os

import numpy as np
import pytest

import flex_amd
from flex_amd import binding
from util import random_csr

import hostsim  # tests/hostsim: the project's own module -- a failure to import it is a failure


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


def shrunk_preset(name, shrink):
    """bench.py --shrink: the preset's generator with n and nnz divided."""
    sp = flex_amd.synth_preset(name, 1)
    n = max(64, sp.n // shrink)
    nnz = max(n, sp.nnz // shrink)
    nnz -= (nnz - n) & 1
    return flex_amd.synth_graph(n=n, nnz=nnz, alpha=sp.alpha, community=sp.community, p_in=sp.p_in, p_near=sp.p_near,
                                near_window=sp.near_window, shuffle=False, gcn_norm=bool(sp.gcn_norm), directed=bool(sp.directed), seed=sp.seed)


def unsorted_with_duplicates():
    rng = np.random.default_rng(11)
    m, n, deg = 700, 900, 40
    col = rng.integers(0, n, size=(m, deg)).astype(np.uint32)
    col[:, 7] = col[:, 3]  # a duplicate (row, column) pair in every row, columns in no order
    rp = (np.arange(m + 1) * deg).astype(np.uint32)
    return flex_amd.HostCsr(rp, col.ravel(), rng.uniform(-1, 1, m * deg).astype(np.float32), n=n)


def graphs():
    return {
        # name: (matrix, k, order, knobs, what the packed plan must show)
        "amazon / 512": (shrunk_preset("amazon", 512), 128, flex_amd.FLEX_ORDER_CLUSTER, {}, lambda r: r["wide_records"] == 0),
        "unsorted, duplicates": (unsorted_with_duplicates(), 64, flex_amd.FLEX_ORDER_NATURAL, {"lanes_per_nz": 8}, lambda r: r["wide_records"] == 0),
        # n > 2^17: differences of 65 536 and more, in both directions (unsorted), several per chunk
        "wide columns": (random_csr(600, 300_000, 30, seed=5, sorted_cols=False), 128, flex_amd.FLEX_ORDER_NATURAL, {}, lambda r: r["exceptions"] > 1000),
        "far first": (shrunk_preset("reddit", 64), 128, flex_amd.FLEX_ORDER_CLUSTER, {"far_first": 300}, lambda r: r["records"] > 0),
        # short rows: chunks with a bundle keep 8-byte records, the long rows' chunks are packed
        "bundles": (random_csr(3000, 3000, 6, seed=6, long_rows={5: 900, 1500: 400, 2999: 2500}), 32, flex_amd.FLEX_ORDER_NATURAL, {"bundle": 1},
                    lambda r: 0 < r["wide_records"] < r["records"]),
    }


@pytest.mark.parametrize("name", list(graphs()))
def test_the_decoded_packed_image_is_the_unpacked_stream(sim, name):
    a, k, order, knobs, shows = graphs()[name]
    packed = flex_amd.Plan(a, k, order=order, tuning=dict(knobs, rec_pack=1))
    plain = flex_amd.Plan(a, k, order=order, tuning=dict(knobs, rec_pack=2))
    assert packed.tuning()["rec_pack"] == 1 and packed.info()["rec_packed"] == 1
    assert plain.tuning()["rec_pack"] == 2 and plain.info()["rec_packed"] == 0
    packed.self_check()
    plain.self_check()
    ri, pi = packed.record_info(), plain.record_info()
    assert shows(ri), ri
    assert ri["records"] == pi["records"] == plain.info()["n_records"] >= a.nnz
    for key in ("n_tasks", "n_chunks", "n_slots", "n_partials", "n_bundles", "lanes_per_nz"):
        assert packed.info()[key] == plain.info()[key], key
    assert ri["stream_bytes"] == 6 * (ri["records"] - ri["wide_records"]) + 8 * (ri["wide_records"] + ri["exceptions"])
    assert pi["stream_bytes"] == 8 * pi["records"] and pi["exceptions"] == 0 and pi["wide_records"] == 0
    got, want = packed.records(), plain.records()
    assert got.shape == want.shape and np.array_equal(got, want)
    # the 8-byte array is not there: the plan is smaller by two bytes per packed record, less the task columns and the tables
    if ri["wide_records"] == 0 and ri["exceptions"] * 8 < ri["records"]:
        assert packed.info()["device_bytes"] < plain.info()["device_bytes"]


@pytest.mark.parametrize("name", ["wide columns", "bundles", "far first"])
def test_the_packed_image_does_not_depend_on_the_thread_count(sim, name):
    a, k, order, knobs, _ = graphs()[name]
    images = []
    for threads in (1, 3, 8):
        sim.hostsim_upload_hash(1)
        p = flex_amd.Plan(a, k, order=order, tuning=dict(knobs, rec_pack=1, host_threads=threads))
        images.append(sim.hostsim_upload_hash(1))
        assert p.tuning()["host_threads"] == threads and p.info()["rec_packed"] == 1
    assert images[0] == images[1] == images[2]


def test_the_rule_and_the_plans_that_stay_unpacked(sim):
    a = random_csr(2000, 2000, 60, seed=9)
    # small streams and single-tile launches stay at 8 bytes by rule; the knob reports what was built
    assert flex_amd.Plan(a, 128).tuning()["rec_pack"] == 2
    # 2-D plans, the generic kernel's shapes, mutable values and attention keep the 8-byte records whatever the knob says
    assert flex_amd.Plan(a, 128, tuning={"rec_pack": 1, "two_d": 1, "panel_kb": 32}).info()["rec_packed"] == 0
    assert flex_amd.Plan(a, 102, tuning={"rec_pack": 1}).info()["rec_packed"] == 0
    assert flex_amd.Plan(a, 100, ldb=101, ldc=100, tuning={"rec_pack": 1}).info()["rec_packed"] == 0
    for kw in ({"mutable_values": True}, {"attention": True}):
        assert flex_amd.Plan(a, 64, **kw).info()["rec_packed"] == 0
        with pytest.raises(flex_amd.FlexError, match="not supported"):
            flex_amd.Plan(a, 64, tuning={"rec_pack": 1}, **kw)
    # a plan without records has nothing to pack
    empty = flex_amd.HostCsr(np.zeros(6, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=5)
    p = flex_amd.Plan(empty, 32, tuning={"rec_pack": 1})
    assert p.info()["rec_packed"] == 0 and p.records().shape == (0, 2)
    p.self_check()


def test_the_rule_packs_a_multi_tile_stream_of_32_mb(sim):
    """4.2 M records at k = 128 on the 8-lane tile (four column tiles): just above the rule's 32 MB."""
    rng = np.random.default_rng(2)
    m, deg = 16500, 256
    col = np.sort(rng.integers(0, m, size=(m, deg)).astype(np.uint32), axis=1)
    a = flex_amd.HostCsr((np.arange(m + 1) * deg).astype(np.uint32), col.ravel(), rng.uniform(-1, 1, m * deg).astype(np.float32), n=m)
    p = flex_amd.Plan(a, 128)
    t, ri = p.tuning(), p.record_info()
    assert t["lanes_per_nz"] == 8 and t["rec_pack"] == 1 and t["rec_nt"] == 1 and ri["packed"] == 1 and ri["wide_records"] == 0
    p.self_check()
    one_tile = flex_amd.Plan(a, 32)
    assert one_tile.tuning()["rec_pack"] == 2

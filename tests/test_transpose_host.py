"""FLEX_PLAN_TRANSPOSE on the host simulator: a transposed plan of A is exactly the plan of an explicitly built A^T.

A^T is built here by a stable sort of A's entries by column (row c of A^T lists A's rows in ascending order, duplicates in CSR order),
which is the order include/flex_spmm.h promises.  Each case compares the uploaded plan image (hostsim_upload_hash), info() but for the
planning time, self_check() and the kernels a launch would run (the launch log)."""
import ctypes as C

import numpy as np
import pytest

import flex_amd
from backward_ref import _directed, route_plans, transpose
from f64ref import ROUTES, SCENARIOS, fake_launch, scenario
from flex_amd import binding

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


def _image(L, make):
    """(upload hash, info without plan_ms, launch log) of the plans make() returns; every plan passes self_check()."""
    L.hostsim_upload_hash(1)
    plans = make()
    h = L.hostsim_upload_hash(1)
    infos = []
    for p in plans:
        p.self_check()
        i = p.info()
        i.pop("plan_ms")
        infos.append(i)
    log = hostsim.launch_log(L, lambda: fake_launch(plans))
    return h, infos, log


def assert_same_plan(L, make):
    """make(transpose) -> plans: with transpose=True it plans A with the flag, with False the explicit A^T."""
    got, want = _image(L, lambda: make(True)), _image(L, lambda: make(False))
    assert got[1] == want[1]
    assert got[2] == want[2]
    assert got[0] == want[0], "plan images differ"
    return got


def test_the_transpose_helper_is_stable():
    """Harness test: the explicit A^T every comparison here is made against has the promised order (no library call)."""
    a = binding.HostCsr(np.array([0, 3, 4, 6], np.uint32), np.array([2, 0, 2, 2, 0, 0], np.uint32),
                        np.arange(1, 7, dtype=np.float32), n=4)
    t = transpose(a)
    assert t.m == 4 and t.n == 3
    assert t.rowPtr.tolist() == [0, 3, 3, 6, 6]
    assert t.col.tolist() == [0, 2, 2, 0, 0, 1]
    assert t.vals.tolist() == [2, 5, 6, 1, 3, 4]


def test_info_reports_the_transposed_shape(sim):
    a = _directed(200, 90)
    p = flex_amd.Plan(a, 32, transpose=True)
    i = p.info()
    assert (i["m"], i["n"], i["nnz"]) == (a.n, a.m, a.nnz)


@pytest.mark.parametrize("case", ["natural", "rcm", "cluster", "vo_mp", "row_range", "ld", "tuning", "stats", "xcd"])
def test_transposed_plan_equals_the_plan_of_the_explicit_transpose(sim, case):
    a = _directed(400, seed=1)
    at = transpose(a)
    k = 32
    if case == "vo_mp":
        vo, ap = flex_amd.perm_csr(a, flex_amd.order_rcm(a))
        apt = transpose(ap)
        assert_same_plan(sim, lambda t: [flex_amd.Plan(ap if t else apt, k, vo_mp=vo, transpose=t)])
        return
    src = lambda t: a if t else at  # noqa: E731
    kw = {
        "natural": {}, "rcm": {"order": flex_amd.FLEX_ORDER_RCM}, "cluster": {"order": flex_amd.FLEX_ORDER_CLUSTER},
        "row_range": {"rows": (37, 311)}, "ld": {"ldb": 40, "ldc": 36},
        "tuning": {"tuning": {"lanes_per_nz": 4, "long_row": 24, "piece_records": 16, "split_rows": 2, "chunk_records": 40}},
        "stats": {"order": flex_amd.FLEX_PLAN_STATS | flex_amd.FLEX_ORDER_RCM},
        "xcd": {"order": flex_amd.FLEX_PLAN_XCD_INTERLEAVE},
    }[case]
    kk = 20 if case == "ld" else k
    assert_same_plan(sim, lambda t: [flex_amd.Plan(src(t), kk, transpose=t, **kw)])
    if case == "stats":
        st = [flex_amd.Plan(src(t), kk, transpose=t, **kw).stats() for t in (True, False)]
        assert st[0] == st[1]


def test_row_range_shards_of_the_transpose_cover_its_rows(sim):
    a = _directed(350, 500, seed=2)
    b = flex_amd.shard_rows(transpose(a), 32, 3)
    for i in range(3):
        r = (int(b[i]), int(b[i + 1]))
        assert_same_plan(sim, lambda t: [flex_amd.Plan(a if t else transpose(a), 32, rows=r, transpose=t)])
    with pytest.raises(binding.FlexError, match="invalid"):
        flex_amd.Plan(a, 32, rows=(0, a.n + 1), transpose=True)  # rows of A^T are columns of A


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_route_plans_the_transpose_as_the_explicit_one(sim, route):
    """Each route on a scenario of its pattern and, for the routes of the random pattern, on a directed graph."""
    spec = ROUTES[route]
    name = SCENARIOS[sorted(ROUTES).index(route) % len(SCENARIOS)]
    a, _ = scenario(name, k=spec["k"], m=spec.get("m", 512), pattern=spec.get("pattern", "random"))
    for src in (a, _directed(spec.get("m", 512), seed=3)) if spec.get("pattern", "random") == "random" else (a,):
        assert_same_plan(sim, lambda t: route_plans(route, src, t))


@pytest.mark.parametrize("shape", ["wide", "tall", "dups", "empty_rows_cols", "nnz0", "one_col"])
def test_edge_shapes(sim, shape):
    if shape == "nnz0":
        a = binding.HostCsr(np.zeros(41, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=17)
    elif shape == "one_col":
        a = binding.HostCsr(np.arange(0, 61, dtype=np.uint32), np.zeros(60, np.uint32), np.ones(60, np.float32), n=1)
    else:
        a = {"wide": lambda: _directed(120, 700, seed=4), "tall": lambda: _directed(700, 90, seed=5),
             "dups": lambda: _directed(300, seed=6, dup=True), "empty_rows_cols": lambda: _directed(250, 260, seed=7)}[shape]()
    for k in (16, 64):
        assert_same_plan(sim, lambda t: [flex_amd.Plan(a if t else transpose(a), k, transpose=t)])
    i = flex_amd.Plan(a, 16, transpose=True).info()
    assert (i["m"], i["n"]) == (a.n, a.m)


def test_the_image_does_not_depend_on_the_host_thread_count(sim):
    a = _directed(3000, seed=8, dup=True)
    images = []
    for threads in (1, 8):
        sim.hostsim_upload_hash(1)
        flex_amd.Plan(a, 64, order=flex_amd.FLEX_ORDER_CLUSTER, tuning={"host_threads": threads}, transpose=True)
        images.append(sim.hostsim_upload_hash(1))
    assert images[0] == images[1]


@pytest.mark.parametrize("flags", [0, flex_amd.FLEX_PLAN_TRANSPOSE])
@pytest.mark.parametrize("rows", [(0, -1), (1, -1), (5, 3), (-1, 4)])
def test_a_bad_row_range_is_still_refused(sim, flags, rows):
    """flex_plan_create_rows and flex_plan_create_ex with FLEX_PLAN_ROW_RANGE take the caller's range as given: a negative or
    reversed range is FLEX_ERR_INVALID, never a plan over some other rows (its C buffer is the shard's)."""
    a = _directed(60, seed=9)
    for tuning in (None, {"chunk_records": 40}):  # the first through flex_plan_create_rows, the second through flex_plan_create_ex
        with pytest.raises(binding.FlexError, match="invalid"):
            flex_amd.Plan(a, 32, order=flags, rows=rows, tuning=tuning)


def test_invalid_a_is_refused_before_the_transpose(sim):
    a = _directed(50)
    bad = binding.HostCsr(a.rowPtr, np.where(a.col == a.col[0], a.n, a.col).astype(np.uint32), a.vals, n=a.n)  # a column >= n
    with pytest.raises(binding.FlexError, match="invalid"):
        flex_amd.Plan(bad, 32, transpose=True)
    for bits in (0x400, 0x4000):  # the bits beside the flag stay refused
        with pytest.raises(binding.FlexError, match="invalid"):
            flex_amd.Plan(a, 32, order=bits | flex_amd.FLEX_PLAN_TRANSPOSE)

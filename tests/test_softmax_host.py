"""The edge softmax's schedule on the host simulator (flex_edge_softmax, flex_plan_softmax_info; internal.h, kSmWindow): every
FLEX_PLAN_MUTABLE_VALUES plan uploads hostA's row pointer for its rows and a work list made from it, flex_plan_self_check verifies that
list (every entry of the plan's rows in exactly one item, items hold whole rows of one class, groups within the promised balance), and
flex_plan_softmax_info accounts for every row and entry.  Plans without the flag upload nothing for it.  The bounds of
tests/softmax_ref.py are shown to be meetable: an fp32 numpy evaluation of the same formulas stays inside them on every score scenario."""
import ctypes as C

import numpy as np
import pytest

import flex_amd
from backward_ref import _directed
from f64ref import ROUTES, scenario
from flex_amd import binding
from softmax_ref import (SCALES, SCORE_SCENARIOS, boundary_graph, check_forward, csr_from_degrees, expected_classes, forward_fp32,
                         long_rows_graph, scores)

hostsim = pytest.importorskip("hostsim")

FLAT_ROUTES = sorted(r for r in ROUTES if not r.startswith(("mfma", "blocks")))


@pytest.fixture(scope="module")
def sim():
    import os
    so = os.environ.get("FLEX_HOSTSIM_LIB") or hostsim.build()
    old_so, old_lib = binding._SO, binding._lib
    binding._SO, binding._lib = so, None
    L = binding.lib()
    L.hostsim_live_allocations.restype = C.c_int64
    yield L
    binding._SO, binding._lib = old_so, old_lib


def route_plans(route, a, transposed, mutable=True):
    """The plan(s) of a route of tests/f64ref.py and, next to each, the row pointer slice whose softmax it computes (None: a transposed
    shard, which computes none)."""
    spec = ROUTES[route]
    k, kw = spec["k"], {"tuning": spec["tuning"], "transpose": transposed, "mutable_values": mutable}
    if spec.get("mapped"):
        vo, ap = flex_amd.perm_csr(a, flex_amd.order_rcm(a))
        return [(flex_amd.Plan(ap, k, vo_mp=vo, **kw), ap.rowPtr)]
    if spec.get("shards"):
        from backward_ref import transpose
        b = flex_amd.shard_rows(transpose(a) if transposed else a, k, spec["shards"])
        return [(flex_amd.Plan(a, k, rows=(int(b[i]), int(b[i + 1])), **kw), None if transposed else a.rowPtr[int(b[i]):int(b[i + 1]) + 1])
                for i in range(spec["shards"])]
    ldb, ldc = spec.get("ld", (None, None))
    return [(flex_amd.Plan(a, k, order=spec.get("order", 0), ldb=ldb, ldc=ldc, **kw), a.rowPtr)]


def assert_accounts(p, rp):
    """softmax_info of plan p accounts for every row and entry of the row pointer slice rp."""
    i = p.softmax_info()
    rp = np.asarray(rp, np.int64)
    assert (i["rows"], i["entries"]) == (len(rp) - 1, int(rp[-1] - rp[0])), i
    assert (i["rows_empty"], i["rows_packed"], i["rows_wave"], i["rows_block"]) == expected_classes(rp), (i, expected_classes(rp))
    assert i["rows_empty"] + i["rows_packed"] + i["rows_wave"] + i["rows_block"] == i["rows"]
    assert i["items"] >= i["rows_wave"] + i["rows_block"] + (1 if i["rows_packed"] else 0)
    assert i["groups"] <= i["items"] - i["rows_block"] and (i["groups"] > 0) == (i["items"] > i["rows_block"])
    assert 256 <= i["group_entries"] <= 2048
    assert i["device_bytes"] >= 4 * (i["rows"] + 1) + 16 * i["items"] + 4 * (i["groups"] + 1)
    assert p.info()["device_bytes"] > i["device_bytes"]
    return i


@pytest.mark.parametrize("route", FLAT_ROUTES)
@pytest.mark.parametrize("transposed", [False, True])
def test_every_flat_route_checks_and_accounts_for_its_softmax_schedule(sim, route, transposed):
    spec = ROUTES[route]
    for name in ("wide", "zeros"):
        a, _ = scenario(name, k=spec["k"], m=spec.get("m", 512))
        for p, rp in route_plans(route, a, transposed):
            p.self_check()
            if rp is None:
                with pytest.raises(binding.FlexError, match="not supported"):
                    p.softmax_info()
            else:
                assert_accounts(p, rp)
        if not spec.get("shards"):  # the schedule is made from hostA's row pointer alone: the same for the plan of A and of A^T
            (p, _), = route_plans(route, a, transposed)
            (q, _), = route_plans(route, a, not transposed)
            assert p.softmax_info() == q.softmax_info()


def edge_shape(shape):
    if shape == "nnz0":
        return binding.HostCsr(np.zeros(41, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=17)
    if shape == "one_col":
        return binding.HostCsr(np.arange(0, 61, dtype=np.uint32), np.zeros(60, np.uint32), np.full(60, 2.0 ** -148, np.float32), n=1)
    if shape == "long_rows":
        return long_rows_graph()
    if shape == "rows_256_257":
        return boundary_graph()
    if shape == "many_empty_rows":  # more rows than a packed item carries between two short rows
        deg = np.zeros(2000, np.int64)
        deg[[0, 3, 700, 701, 1999]] = [2, 1, 5, 250, 3]
        return csr_from_degrees(deg, 50, seed=8)
    return {"dups": lambda: _directed(300, seed=6, dup=True), "empty_rows_cols": lambda: _directed(250, 260, seed=7)}[shape]()


EDGE_SHAPES = ["dups", "empty_rows_cols", "nnz0", "one_col", "long_rows", "rows_256_257", "many_empty_rows"]


@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_edge_shapes(sim, shape):
    a = edge_shape(shape)
    for k in (7, 32):
        for t in (False, True):
            p = flex_amd.Plan(a, k, transpose=t, mutable_values=True)
            p.self_check()
            i = assert_accounts(p, a.rowPtr)
            if shape == "long_rows":
                assert i["rows_wave"] >= 1 and i["rows_block"] == 3, i
            if shape == "rows_256_257":
                assert i["rows_packed"] >= 1 and i["rows_wave"] >= 1 and i["rows_packed"] + i["rows_wave"] == a.m, i


def test_shards_account_for_their_own_rows_only(sim):
    a = long_rows_graph()
    cuts = [0, 17, 18, 101, 260, a.m]
    total = 0
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        p = flex_amd.Plan(a, 32, rows=(r0, r1), mutable_values=True)
        p.self_check()
        total += assert_accounts(p, a.rowPtr[r0:r1 + 1])["entries"]
        t = flex_amd.Plan(a, 32, rows=(r0, min(r1, a.n)), transpose=True, mutable_values=True)
        t.self_check()
        with pytest.raises(binding.FlexError, match="not supported"):
            t.softmax_info()
    assert total == a.nnz


def test_plans_without_the_flag_report_invalid_and_upload_nothing_for_it(sim):
    a = _directed(300, seed=6, dup=True)

    def allocations(**kw):
        before = sim.hostsim_live_allocations()
        p = flex_amd.Plan(a, 32, **kw)
        return p, sim.hostsim_live_allocations() - before

    plain, n_plain = allocations()
    with pytest.raises(binding.FlexError, match="invalid"):
        plain.softmax_info()
    _, n_mut = allocations(mutable_values=True)
    _, n_tshard = allocations(mutable_values=True, transpose=True, rows=(0, 100))
    _, n_plain_tshard = allocations(transpose=True, rows=(0, 100))
    # the value image is 5 arrays (record -> entry map, values, padded runs, SDDMM items and groups), the softmax schedule 3 more
    assert n_mut - n_plain == 8 and n_tshard - n_plain_tshard == 5, (n_plain, n_mut, n_tshard, n_plain_tshard)


@pytest.mark.parametrize("name", SCORE_SCENARIOS)
def test_an_fp32_evaluation_of_the_formulas_stays_within_the_bounds(name):
    """The forward bound is neither vacuous nor unmeetable: numpy in fp32 (sequential sums) passes check_forward on every scenario."""
    worst = 0.0
    for a in (long_rows_graph(), boundary_graph(), _directed(300, seed=6, dup=True)):
        s = scores(name, a.rowPtr, seed=3)
        for scale in SCALES:
            worst = max(worst, check_forward(a.rowPtr, s, scale, forward_fp32(a.rowPtr, s, scale), f"{name} scale {scale}"))
    print(f"{name}: worst err / bound {worst:.3g}")
    assert worst <= 1.0

"""FLEX_PLAN_MUTABLE_VALUES on the host simulator: every entry point and every flat route takes the flag, and the value image of each plan
passes flex_plan_self_check -- every entry held in exactly one real record, that record reading the entry's column (after col_map),
and every record's bits exactly what the padding rule shared with the GPU refresh (internal.h, pad_values) derives from the plan's
values.  The value scenarios of tests/f64ref.py reach every branch of that rule (halving, copies of +-inf / NaN / +-0, the split of a
significand, the (c_last, 0) residual).  Apart from the value image, a mutable plan is the plan of the same CSR made without the flag
and without the dense-tile and hot-block routes."""
import ctypes as C

import numpy as np
import pytest

import flex_amd
from backward_ref import _directed, transpose
from f64ref import ROUTES, SCENARIOS, fake_launch, scenario
from flex_amd import binding

hostsim = pytest.importorskip("hostsim")

MUT = flex_amd.FLEX_PLAN_MUTABLE_VALUES
FLAT_ROUTES = sorted(r for r in ROUTES if not r.startswith(("mfma", "blocks")))
NO_SPLIT_ROUTES = {"mfma": 2, "blocks": 2}


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


def route_plans(route, a, transposed=False, mutable=True, extra_tuning=None):
    """The plan(s) of a route of tests/f64ref.py for `a` (or, transposed, for A^T planned from `a`), made with or without the flag."""
    spec = ROUTES[route]
    k, tn = spec["k"], dict(spec["tuning"], **(extra_tuning or {}))
    kw = {"tuning": tn, "transpose": transposed, "mutable_values": mutable}
    if spec.get("mapped"):
        vo, ap = flex_amd.perm_csr(a, flex_amd.order_rcm(a))
        return [flex_amd.Plan(ap, k, vo_mp=vo, **kw)]
    if spec.get("shards"):
        b = flex_amd.shard_rows(transpose(a) if transposed else a, k, spec["shards"])
        return [flex_amd.Plan(a, k, rows=(int(b[i]), int(b[i + 1])), **kw) for i in range(spec["shards"])]
    ldb, ldc = spec.get("ld", (None, None))
    return [flex_amd.Plan(a, k, order=spec.get("order", 0), ldb=ldb, ldc=ldc, **kw)]


def _info(p):
    i = p.info()
    for f in ("plan_ms", "device_bytes"):
        i.pop(f)
    return i


@pytest.mark.parametrize("route", FLAT_ROUTES)
@pytest.mark.parametrize("transposed", [False, True])
def test_every_flat_route_takes_the_flag_and_checks_its_value_image(sim, route, transposed):
    spec = ROUTES[route]
    for name in SCENARIOS:
        a, _ = scenario(name, k=spec["k"], m=spec.get("m", 512))
        plans = route_plans(route, a, transposed)
        for p in plans:
            p.self_check()
            t = p.tuning()
            assert (t["mfma"], t["blocks"]) == (2, 2), (route, name, t)
        # apart from the value image: the plan without the flag (routes that are not taken anyway)
        plain = route_plans(route, a, transposed, mutable=False, extra_tuning=NO_SPLIT_ROUTES)
        assert [_info(p) for p in plans] == [_info(p) for p in plain], (route, name)
        assert all(p.info()["device_bytes"] > q.info()["device_bytes"] for p, q in zip(plans, plain) if p.info()["nnz"])
        log = hostsim.launch_log(sim, lambda: fake_launch(plans, unaligned=bool(spec.get("unaligned"))))
        assert log == hostsim.launch_log(sim, lambda: fake_launch(plain, unaligned=bool(spec.get("unaligned")))), (route, name)


@pytest.mark.parametrize("entry", ["create", "ld", "mapped", "rows", "ex", "ex_rows_mapped_ld"])
@pytest.mark.parametrize("transposed", [False, True])
def test_every_entry_point_takes_the_flag(sim, entry, transposed):
    a = _directed(300, seed=11, dup=True)
    src = transpose(a) if transposed else a  # the CSR the options refer to
    k = 32
    if entry == "create":
        p = flex_amd.Plan(a, k, transpose=transposed, mutable_values=True)
    elif entry == "ld":
        p = flex_amd.Plan(a, 20, ldb=28, ldc=24, transpose=transposed, mutable_values=True)
    elif entry == "mapped":
        sq, _ = scenario("wide", k=k, m=300)
        vo, ap = flex_amd.perm_csr(sq, flex_amd.order_rcm(sq))
        p = flex_amd.Plan(ap, k, vo_mp=vo, transpose=transposed, mutable_values=True)
    elif entry == "rows":
        p = flex_amd.Plan(a, k, rows=(37, 211), col_map=np.random.default_rng(0).permutation(src.n).astype(np.int32),
                          transpose=transposed, mutable_values=True)
    elif entry == "ex":
        p = flex_amd.Plan(a, k, order=flex_amd.FLEX_PLAN_STATS | flex_amd.FLEX_PLAN_XCD_INTERLEAVE, tuning={"chunk_records": 40},
                          transpose=transposed, mutable_values=True)
        assert p.stats()["records"] == p.info()["n_records"]
    else:
        sq, _ = scenario("zeros", k=k, m=300)
        vo, ap = flex_amd.perm_csr(sq, flex_amd.order_rcm(sq))
        p = flex_amd.Plan(ap, k, col_map=vo, rows=(10, 250), ldb=40, ldc=36, transpose=transposed, mutable_values=True)  # a shard of a reordered CSR
    p.self_check()
    assert p.tuning()["mfma"] == 2 and p.tuning()["blocks"] == 2


@pytest.mark.parametrize("order", [flex_amd.FLEX_ORDER_RCM, flex_amd.FLEX_ORDER_CLUSTER, flex_amd.FLEX_ORDER_GORDER])
def test_reordered_two_d_and_far_first_plans(sim, order):
    a, _ = scenario("tiny_vs_inf_B", k=64, m=700)
    flex_amd.Plan(a, 64, order=order, mutable_values=True).self_check()
    flex_amd.Plan(a, 64, order=order, tuning={"two_d": 1, "panel_kb": 1, "seg_min": 2}, mutable_values=True).self_check()
    flex_amd.Plan(a, 64, order=order, tuning={"far_first": 4, "bundle": 1}, transpose=True, mutable_values=True).self_check()


@pytest.mark.parametrize("shape", ["dups", "empty_rows_cols", "nnz0", "one_col", "long_row"])
def test_edge_shapes(sim, shape):
    if shape == "nnz0":
        a = binding.HostCsr(np.zeros(41, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=17)
    elif shape == "one_col":
        a = binding.HostCsr(np.arange(0, 61, dtype=np.uint32), np.zeros(60, np.uint32), np.full(60, 2.0 ** -148, np.float32), n=1)
    elif shape == "long_row":
        rng = np.random.default_rng(5)
        deg = rng.poisson(3, 400)
        deg[17] = 2600
        rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
        a = binding.HostCsr(rp, rng.integers(0, 3000, rp[-1]).astype(np.uint32), rng.uniform(-1, 1, rp[-1]).astype(np.float32), n=3000)
    else:
        a = {"dups": lambda: _directed(300, seed=6, dup=True), "empty_rows_cols": lambda: _directed(250, 260, seed=7)}[shape]()
    for k in (7, 16, 64, 256):
        for t in (False, True):
            flex_amd.Plan(a, k, transpose=t, mutable_values=True).self_check()


def test_the_image_does_not_depend_on_the_host_thread_count(sim):
    a, _ = scenario("nonfinite_A", k=32, m=3000)
    images = []
    for threads in (1, 8):
        sim.hostsim_upload_hash(1)
        flex_amd.Plan(a, 32, order=flex_amd.FLEX_ORDER_CLUSTER, tuning={"host_threads": threads}, transpose=True, mutable_values=True)
        images.append(sim.hostsim_upload_hash(1))
    assert images[0] == images[1]


def test_the_dense_tile_and_hot_block_routes_are_refused_with_the_flag(sim):
    a, _ = scenario("wide", k=64, pattern="block")
    for knob in ({"mfma": 1}, {"blocks": 1}, {"mfma": 1, "mfma_fill_pct": 50}):
        with pytest.raises(binding.FlexError, match="not supported"):
            flex_amd.Plan(a, 64, tuning=knob, mutable_values=True)
        flex_amd.Plan(a, 64, tuning=knob)  # the same without the flag still plans
    # the rule of either route may not take them either: the block pattern that the MFMA route would have routed stays flat
    p = flex_amd.Plan(a, 64, tuning={"mfma_fill_pct": 50}, mutable_values=True)
    assert p.info()["n_tiles"] == 0 and p.info()["n_blocks"] == 0
    p.self_check()


def test_the_bits_beside_the_flag_stay_refused(sim):
    a = _directed(60, seed=9)
    for bits in (0x400, 0x4000, 0x20000):
        for extra in (0, MUT, MUT | flex_amd.FLEX_PLAN_TRANSPOSE):
            with pytest.raises(binding.FlexError, match="invalid"):
                flex_amd.Plan(a, 32, order=bits | extra)

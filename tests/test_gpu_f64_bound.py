"""Every SpMM route against the float64 bound of tests/f64ref.py, over the fp32 value range: wide magnitudes, subnormal inputs with
normal products, products that underflow, sums near 2^120, cancelling rows with duplicate and unsorted columns, stored zeros, and
+-inf / NaN in A, in B and in both.  C must lie within gamma(nnz + P) |A||B| + (nnz + P) 2^-149 of the float64 result, and be
NaN / +inf / -inf exactly where that result is."""
import numpy as np
import pytest

import flex_amd
from f64ref import ROUTES, SCENARIOS, TINY, assert_within_f64_bound, plan_for_route, scenario

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def run_route(route, a, B):
    """C of `route` for (a, B), every plan of it self-checked."""
    spec = ROUTES[route]
    k = spec["k"]
    plans = plan_for_route(route, a)
    for p in plans:
        p.self_check()
    stream = torch.cuda.current_stream().cuda_stream
    if spec.get("shards"):
        outs = []
        for p in plans:
            C = p(torch.from_numpy(B).cuda())
            outs.append(C)
        torch.cuda.synchronize()
        return torch.cat(outs).cpu().numpy()
    p = plans[0]
    if spec.get("stamped"):
        Bd = torch.from_numpy(B).cuda()
        Cd = torch.full((a.m, k), -7.0, device="cuda")  # every row must be written
        p.measure_imbalance(Bd.data_ptr(), Cd.data_ptr(), stream)
        torch.cuda.synchronize()
        return Cd.cpu().numpy()
    if spec.get("unaligned"):
        bb = torch.zeros(a.n * k + 1, device="cuda")
        bb[1:] = torch.from_numpy(B).cuda().ravel()
        cc = torch.full((a.m * k + 1,), -7.0, device="cuda")
        p.spmm(bb[1:].data_ptr(), cc[1:].data_ptr(), stream)
        torch.cuda.synchronize()
        return cc[1:].reshape(a.m, k).cpu().numpy()
    if "ld" in spec:
        ldb, ldc = spec["ld"]
        Bs = torch.full((a.n, ldb), float("nan"), device="cuda")  # poison: columns >= k must never reach C
        Bs[:, :k] = torch.from_numpy(B).cuda()
        Cs = torch.full((a.m, ldc), -7.0, device="cuda")
        p.spmm(Bs.data_ptr(), Cs.data_ptr(), stream)
        torch.cuda.synchronize()
        Cs = Cs.cpu().numpy()
        assert np.all(Cs[:, k:] == -7.0)
        return np.ascontiguousarray(Cs[:, :k])
    C = p(torch.from_numpy(B).cuda())
    torch.cuda.synchronize()
    return C.cpu().numpy()


def _knobs_took_effect(route, plan):
    """The tuning knobs of `route` as the plan resolved them (flex_plan_get_tuning), and what they imply for the launch."""
    spec, tn, info = ROUTES[route], plan.tuning(), plan.info()
    for knob in ("lanes_per_nz", "tile_group", "unroll", "xcd_slices", "xcd_stretch", "rec_nt", "lds_extra", "split_rows", "block_rounds"):
        if knob in spec["tuning"]:
            assert tn[knob] == spec["tuning"][knob], (route, knob, tn[knob])
    if "order" in spec:
        assert info["order"] == spec["order"], info
    if route.startswith("tile_group"):
        assert (info["k"] + 4 * tn["lanes_per_nz"] - 1) // (4 * tn["lanes_per_nz"]) >= 2, info  # a multi-tile launch
        if route == "tile_group_rcm":
            assert tn["xcd_slices"] == 2, tn  # RCM: no XCD remap
    if route == "tile_group_split" or spec.get("stamped"):
        assert info["n_split_rows"] > 0, info


def _group_slice(plan):
    """Workgroups of one pass in an XCD's slice of the grouped grid (the whole pass without the XCD remap): 4 chunks per workgroup."""
    nwg = plan.info()["n_slots"] // 4
    return nwg // 8 if plan.tuning()["xcd_slices"] == 1 else nwg


@pytest.mark.parametrize("route", [r for r in ROUTES if r.startswith("tile_group")])
def test_the_grouped_routes_end_slices_in_a_short_group(route):
    """spmm_kernels.hip decodes the last group of a slice as short when the slice is not a multiple of tile_group: most scenarios of
    every grouped route meet that decode."""
    spec = ROUTES[route]
    slices = [_group_slice(plan_for_route(route, scenario(name, k=spec["k"], m=spec.get("m", 512))[0])[0]) for name in SCENARIOS]
    assert sum(s % spec["tuning"]["tile_group"] != 0 for s in slices) >= 9, slices


def _route_is_taken(route, plan_info):
    if route.startswith("mfma"):
        assert plan_info["n_tiles"] > 0, plan_info
    if route.startswith("blocks"):
        assert plan_info["n_blocks"] > 0, plan_info
    if route.startswith("bundles"):
        assert plan_info["n_bundles"] > 0, plan_info
    if route.startswith("split") or route == "order_rcm":
        assert plan_info["n_split_rows"] > 0, plan_info
    if route == "two_d":
        assert plan_info["two_d"] == 1, plan_info


@pytest.mark.parametrize("name", SCENARIOS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_route_within_the_float64_bound(route, name):
    spec = ROUTES[route]
    a, B = scenario(name, k=spec["k"], m=spec.get("m", 512), pattern=spec.get("pattern", "random"))
    plan = plan_for_route(route, a)[0]
    _route_is_taken(route, plan.info())
    _knobs_took_effect(route, plan)
    assert_within_f64_bound(a, B, run_route(route, a, B), route=f"{route}/{name}")


@pytest.mark.parametrize("route", ["flat_g8", "bundles_g8", "split_rows2", "mfma", "generic_odd_k"])
def test_subnormals_pass_through_every_kernel(route):
    """Subnormal A against B = 2^100 and A = 2^100 against subnormal B: the products are normal, so a kernel that flushed its
    inputs to zero would return 0 where the result is about 2^-40."""
    spec = ROUTES[route]
    for name in ("subnormal_A_large_B", "large_A_subnormal_B"):
        a, B = scenario(name, k=spec["k"], seed=5, pattern=spec.get("pattern", "random"))
        C = run_route(route, a, B)
        assert_within_f64_bound(a, B, C, route=f"{route}/{name}")
        nz = np.diff(a.rowPtr.astype(np.int64)) > 0
        assert np.all(np.abs(C[nz]).max(axis=1) > 0)


@pytest.mark.xfail(strict=True, reason="documented residual (include/flex_spmm.h): a task whose stored values are all nonzero subnormals "
                                       "of at most n_pad units of 2^-149 is padded with value 0, so 0 x inf = NaN where the result is inf")
def test_the_documented_padding_residual():
    """Row 0: the single value 2^-149 against a B row of +inf, on the narrow tile (S = 16 records per step: 15 padding records)."""
    rp = np.array([0, 1, 3], np.uint32)
    a = flex_amd.HostCsr(rp, np.array([1, 0, 2], np.uint32), np.array([TINY, 1.0, 1.0], np.float32), n=3)
    B = np.ones((3, 16), np.float32)
    B[1, :] = np.inf
    C = run_route("flat_g4", a, B)
    assert np.all(C[0] == np.inf)


def test_the_stamped_twin_refuses_row_blocks():
    """flex_plan_measure_imbalance exists for the vector kernel only: a plan with row blocks is refused with FLEX_ERR_UNSUPPORTED and C
    is left as it was."""
    a, B = scenario("wide", k=64, pattern="block")
    p = plan_for_route("blocks", a)[0]
    assert p.info()["n_blocks"] > 0
    Bd = torch.from_numpy(B).cuda()
    Cd = torch.full((a.m, 64), -7.0, device="cuda")
    with pytest.raises(flex_amd.FlexError, match=r"\(-4\)"):
        p.measure_imbalance(Bd.data_ptr(), Cd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((Cd == -7.0).all())

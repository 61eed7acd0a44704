"""The float64 checker of tests/f64ref.py, checked without a GPU: it accepts what is right (the fp32 oracle, and a float32 emulation of
the engine's sum order with its padding), it rejects what is subtly wrong (a dropped term or padding part, a scaled row, a changed
non-finite class, flushed subnormals), and the planner turns every scenario into a valid plan with no more records than uniform
values give (tests/hostsim)."""
import os

import numpy as np
import pytest

import flex_amd
import oracle
from f64ref import (ROUTES, SCENARIOS, TINY, check_f64_bound, f64_bound, plan_for_route, scenario, spmm_f64,
                    with_uniform_values)
from flex_amd import binding

hostsim = pytest.importorskip("hostsim")


def oracle_C(a, B):
    return oracle.spmm(a.rowPtr, a.col, a.vals, B)


# ---- a float32 emulation of the engine's order ----------------------------------------------------------------------------

def _split_parts(v, parts):
    """v (finite, nonzero) as `parts` exact same-sign values from its integer significand, or None when it has fewer units."""
    bits = int(np.float32(v).view(np.uint32))
    ex, man = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    sig = man | (1 << 23) if ex else man
    if sig < parts:
        return None
    d, r = divmod(sig, parts)
    scale = 2.0 ** (max(ex, 1) - 150)
    sign = -1.0 if bits >> 31 else 1.0
    return [np.float32(sign * (d + (i < r)) * scale) for i in range(parts)]


def pad_records(cols, vals, n_pad, fixed=True):
    """The records of one task (or bundle slot) after padding: plan_build.cpp, pad_row.  fixed=False: the zero-value fallback the
    planner had before (a value that cannot be halved n_pad times pads with (col, 0))."""
    cols, vals = list(cols), [np.float32(v) for v in vals]
    if n_pad == 0 or not cols:
        return cols, vals
    bits = int(vals[-1].view(np.uint32))
    ex = (bits >> 23) & 0xFF
    if n_pad + 1 < ex < 0xFF:  # halving: v/2 + v/4 + ... + v/2^p + v/2^p
        v = vals[-1]
        parts = [np.float32(v * np.float32(2.0 ** -(i + 1))) for i in range(n_pad)] + [np.float32(v * np.float32(2.0 ** -n_pad))]
        return cols + [cols[-1]] * n_pad, vals[:-1] + parts
    if fixed:
        for j in range(len(vals) - 1, -1, -1):
            v = vals[j]
            if not np.isfinite(v) or v == 0:  # copies: what the row already has
                return cols + [cols[j]] * n_pad, vals + [v] * n_pad
            parts = _split_parts(v, n_pad + 1)
            if parts is not None:
                vals[j] = parts[0]
                return cols + [cols[j]] * n_pad, vals + parts[1:]
    return cols + [cols[-1]] * n_pad, vals + [np.float32(0.0)] * n_pad


def _fma_chain(acc, v, brows):
    with np.errstate(invalid="ignore", over="ignore"):
        return (acc.astype(np.float64) + v.astype(np.float64)[:, None] * brows.astype(np.float64)).astype(np.float32)


def emulate(a, B, S=16, piece_len=32, long_row=48, bundle_len=12, fixed=True):
    """C in float32 the way the engine sums it: rows of at most bundle_len records alone in a bundle slot (one fma chain padded to
    bundle_len steps, the longest a bundle gets); longer rows in tasks of S slots (record j on slot j mod S, padded to whole steps),
    the slots meeting in a tree; rows longer than long_row cut into pieces of piece_len records whose partial sums are then added."""
    rp = a.rowPtr.astype(np.int64)
    k = B.shape[1]
    C = np.zeros((a.m, k), np.float32)

    def task(cols, vals, slots):
        steps = -(-len(cols) // slots)
        cols, vals = pad_records(cols, vals, steps * slots - len(cols), fixed)
        cols = np.array(cols, np.int64).reshape(steps, slots)
        vals = np.array(vals, np.float32).reshape(steps, slots)
        acc = np.zeros((slots, k), np.float32)
        for s in range(steps):
            acc = _fma_chain(acc, vals[s], B[cols[s]])
        while acc.shape[0] > 1:
            h = acc.shape[0] // 2
            with np.errstate(invalid="ignore", over="ignore"):
                acc = (acc[:h] + acc[h:2 * h]).astype(np.float32)
        return acc[0]

    for r in range(a.m):
        cols, vals = a.col[rp[r]:rp[r + 1]].astype(np.int64), a.vals[rp[r]:rp[r + 1]]
        n = len(cols)
        if n == 0:
            continue
        if n <= bundle_len:
            cols_p, vals_p = pad_records(cols, vals, bundle_len - n, fixed)
            acc = np.zeros((1, k), np.float32)
            for c, v in zip(cols_p, vals_p):
                acc = _fma_chain(acc, np.array([v], np.float32), B[[c]])
            C[r] = acc[0]
        elif n <= long_row:
            C[r] = task(cols, vals, S)
        else:
            acc = np.zeros(k, np.float32)
            for p0 in range(0, n, piece_len):
                with np.errstate(invalid="ignore", over="ignore"):
                    acc = (acc + task(cols[p0:p0 + piece_len], vals[p0:p0 + piece_len], S)).astype(np.float32)
            C[r] = acc
    return C


# ---- the bound is not too tight ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENARIOS)
def test_the_fp32_oracle_passes_the_bound(name):
    for k in (5, 32):
        a, B = scenario(name, k=k, m=300)
        msg = check_f64_bound(a, B, oracle_C(a, B), route="oracle")
        assert msg is None, msg


@pytest.mark.parametrize("S", [4, 16])
@pytest.mark.parametrize("name", SCENARIOS)
def test_an_emulation_of_the_padded_step_order_passes_the_bound(name, S):
    """Slot chains over padded steps, the cross-slot tree, pieces and their fix-up, bundle slots padded to the longest candidate --
    with the planner's padding, within the bound at the chosen P, and of the reference's class wherever that is not finite."""
    a, B = scenario(name, k=8, m=300)
    msg = check_f64_bound(a, B, emulate(a, B, S=S), route=f"emulated S={S}")
    assert msg is None, msg


@pytest.mark.parametrize("name", ["tiny_vs_inf_B", "inf_A_vs_inf_B"])
def test_the_zero_value_fallback_padding_is_rejected(name):
    """The padding the planner had before: a value that cannot be halved (tiny, subnormal, +-inf, NaN) padded with (col, 0), which
    adds 0 x inf = NaN to a row whose reference is +-inf.  The checker must see it on the CPU already."""
    a, B = scenario(name, k=8, m=300)
    msg = check_f64_bound(a, B, emulate(a, B, S=16, fixed=False), route="zero-value padding")
    assert msg is not None and "wrong class" in msg, msg
    assert check_f64_bound(a, B, emulate(a, B, S=16, fixed=True)) is None


def test_the_padding_parts_are_exact_and_keep_their_sign():
    for v in [1.0, -3.5, 2.0 ** -120, -(2.0 ** -126), 1000 * TINY, -17 * TINY, np.float32(1.2345e-40)]:
        v = np.float32(v)
        for n_pad in range(1, 16):
            _, vals = pad_records([7], [v], n_pad)
            if abs(float(v)) / TINY <= n_pad and abs(float(v)) < 2.0 ** -126:
                continue  # the documented residual: too few significand units (see the residual test)
            assert len(vals) == n_pad + 1 and sum(float(x) for x in vals) == float(v)
            assert all(x != 0 and np.sign(x) == np.sign(v) for x in vals), (v, n_pad, vals)
    for v in [np.inf, -np.inf, np.nan, 0.0, -0.0]:
        _, vals = pad_records([7], [np.float32(v)], 5)
        assert all(np.array_equal(np.float32(x), np.float32(v), equal_nan=True) for x in vals)


def test_the_residual_set_is_what_the_documentation_says():
    """The one set of inputs whose padding stays (col, 0): every stored value of a task (or bundle slot) a nonzero subnormal of at
    most n_pad units of 2^-149 -- too few to split, nothing to copy.  A row of one 2^-149 against an inf B row: NaN, not inf."""
    cols, vals = pad_records([3, 4], [np.float32(TINY), np.float32(-2 * TINY)], 3)
    assert [float(v) for v in vals[2:]] == [0.0, 0.0, 0.0]
    cols, vals = pad_records([3, 4], [np.float32(TINY), np.float32(4 * TINY)], 3)
    assert sum(float(v) for v in vals) == 5 * TINY and all(v != 0 for v in vals)


# ---- the bound has teeth --------------------------------------------------------------------------------------------------

def _ctx(name, k=16, m=300):
    a, B = scenario(name, k=k, m=m)
    return a, B, spmm_f64(a, B), f64_bound(a, B), oracle_C(a, B)


TEETH = ["wide", "subnormal_A_large_B", "large_A_subnormal_B", "huge", "cancel"]


@pytest.mark.parametrize("name", TEETH)
def test_one_dropped_term_fails(name):
    a, B, ref, bound, C = _ctx(name)
    rows = np.repeat(np.arange(a.m), np.diff(a.rowPtr.astype(np.int64)))
    terms = np.abs(a.vals.astype(np.float64)[:, None] * B.astype(np.float64)[a.col])
    e, j = np.unravel_index(int(np.argmax(terms / bound[rows])), terms.shape)
    r = rows[e]
    assert terms[e, j] > 2 * bound[r, j]
    bad = C.copy()
    bad[r, j] = np.float32(float(C[r, j]) - float(a.vals[e]) * float(B[a.col[e], j]))
    assert check_f64_bound(a, B, bad) is not None


@pytest.mark.parametrize("name", TEETH)
def test_a_dropped_last_padding_part_fails(name):
    """The last part v / 2^p of a task's halving padding lost (p <= 10), on rows of at most 8 records."""
    a, B, ref, bound, C = _ctx(name)
    rp = a.rowPtr.astype(np.int64)
    best = None
    for r in np.nonzero((np.diff(rp) > 0) & (np.diff(rp) <= 8))[0]:
        e = rp[r + 1] - 1
        t = np.abs(float(a.vals[e]) * B[a.col[e]].astype(np.float64)) * 2.0 ** -10 / bound[r]
        j = int(np.argmax(t))
        if best is None or t[j] > best[0]:
            best = (t[j], r, e, j)
    _, r, e, j = best
    for p in range(1, 11):
        bad = C.copy()
        bad[r, j] = np.float32(float(C[r, j]) - float(a.vals[e]) * 2.0 ** -p * float(B[a.col[e], j]))
        assert check_f64_bound(a, B, bad) is not None, p


@pytest.mark.parametrize("name", ["wide", "subnormal_A_large_B", "large_A_subnormal_B", "huge", "products_underflow"])
def test_a_row_scaled_by_one_plus_2_pow_minus_12_fails(name):
    a, B, ref, bound, C = _ctx(name)
    r = int(np.argmax((np.abs(ref) / bound).max(axis=1)))
    bad = C.copy()
    bad[r] = (C[r].astype(np.float64) * (1 + 2.0 ** -12)).astype(np.float32)
    assert check_f64_bound(a, B, bad) is not None


@pytest.mark.parametrize("name", ["nonfinite_A", "tiny_vs_inf_B", "inf_A_vs_inf_B", "nonfinite_B_wide_A"])
def test_a_changed_non_finite_class_fails(name):
    a, B, ref, bound, C = _ctx(name)
    assert check_f64_bound(a, B, C) is None
    inf = np.argwhere(np.isinf(ref))
    assert len(inf)
    r, j = inf[len(inf) // 2]
    for v in (np.nan, -C[r, j], np.float32(3.0e38)):
        bad = C.copy()
        bad[r, j] = v
        assert check_f64_bound(a, B, bad) is not None
    nan = np.argwhere(np.isnan(ref))
    if name != "tiny_vs_inf_B":
        assert len(nan)
    for r, j in nan[:3]:
        for v in (0.0, 1.0, np.inf):
            bad = C.copy()
            bad[r, j] = v
            assert check_f64_bound(a, B, bad) is not None


def test_flushed_subnormal_inputs_fail():
    a, B = scenario("subnormal_A_large_B", k=16, m=300)
    flushed = flex_amd.HostCsr(a.rowPtr, a.col, np.where(np.abs(a.vals) < 2.0 ** -126, 0, a.vals).astype(np.float32), n=a.n)
    assert check_f64_bound(a, B, oracle_C(flushed, B)) is not None
    a, B = scenario("large_A_subnormal_B", k=16, m=300)
    Bf = np.where(np.abs(B) < 2.0 ** -126, 0, B).astype(np.float32)
    assert check_f64_bound(a, B, oracle_C(a, Bf)) is not None


def test_the_bound_refuses_a_scenario_outside_the_checked_range():
    a, B = scenario("huge", k=8, m=100)
    with pytest.raises(AssertionError, match="2\\^120"):
        check_f64_bound(a, (B.astype(np.float64) * 4).astype(np.float32), oracle_C(a, B))


# ---- plans of the new values, host-simulated ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sim():
    so = os.environ.get("FLEX_HOSTSIM_LIB") or hostsim.build()
    old_so, old_lib = binding._SO, binding._lib
    binding._SO, binding._lib = so, None
    yield binding.lib()
    binding._SO, binding._lib = old_so, old_lib


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_plans_of_every_scenario_are_valid_and_add_no_records(sim, route):
    """Every scenario through every route's planner: flex_plan_self_check passes, and the plan streams as many records as the same
    pattern with uniform(-1, 1) values (the padding never adds any).  On the MFMA route non-finite A values stay with the vector
    kernel: the same tiles, each holding only the finite cells."""
    spec = ROUTES[route]
    for name in SCENARIOS:
        a, B = scenario(name, k=spec["k"], m=spec.get("m", 512), pattern=spec.get("pattern", "random"))
        plans = plan_for_route(route, a)
        uniform = plan_for_route(route, with_uniform_values(a))
        for p, q in zip(plans, uniform):
            p.self_check()
            i, u = p.info(), q.info()
            n_bad = int(np.sum(~np.isfinite(a.vals)))
            if n_bad and i["n_tiles"]:
                assert i["n_tiles"] == u["n_tiles"] and u["tile_nnz"] - n_bad <= i["tile_nnz"] <= u["tile_nnz"], (name, i, u)
                assert i["n_records"] >= u["n_records"]
            else:
                assert (i["n_records"], i["n_tiles"], i["tile_nnz"], i["n_tasks"]) == \
                    (u["n_records"], u["n_tiles"], u["tile_nnz"], u["n_tasks"]), (name, route)

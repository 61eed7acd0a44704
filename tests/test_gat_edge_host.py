"""Host checks of the per-edge score term of the fused GAT attention (include/flex_spmm.h: flex_edge_gat_attention and its backward):
the float64 reference (tests/gat_edge_ref.py) against an independent float64 torch autograd evaluation, an fp32 evaluation of the
kernel's arithmetic and a float64 result rounded to fp32 against both checkers, every planted fault against the checker it targets, the
public surface, and the census of the kernels in flex::gat_edge with the GPU case that runs each.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import attention_dropout_ref as ad
import flex_amd
import gat_attention_ref as gat
import gat_edge_ref as ge
from attention_forms import FORM_OF_K, FORMS
from conftest import ROOT
from flex_amd import binding
from test_gat_dropout_host import GPU_GRAPHS, PAIRS, SEED, _NoPlan, grad, graph

SLOPE = ge.SLOPE
DROPS = (0.0, 0.5)

# ---- the table of tests/test_gpu_gat_edge.py: the pairs and graphs of the sibling files (every (W, NS) form, idle lanes past k, d = 4
# and d = 256, H = 1; the wide pairs on the graph that holds every class of row and column), each at drop_p = 0 and 0.5
CASES = [(name, k, H, p) for k, H in PAIRS for name in (GPU_GRAPHS if k < 256 else ["thresholds_lifted"]) for p in DROPS]


def case_id(c):
    name, k, H, p = c
    return f"{name}-k{k}-h{H}-p{p}"


def kernels_of(c):
    """The two instantiations in flex::gat_edge that the forward and the backward of a case launch, as `nm -C` names them: written down
    from FORM_OF_K, not computed by the rule it checks.  (The column launch is the GAT family's.)"""
    W, NS = FORM_OF_K[c[1]]
    drop = "true" if c[3] else "false"
    return [f"gat_edge_rows<{W}, {NS}, {drop}>", f"gat_edge_rows_backward<{W}, {NS}, {drop}>"]


# kernel -> the id of the first case of test_every_output_against_float64 (tests/test_gpu_gat_edge.py) that launches it
RUN_BY = {}
for _c in CASES:
    for _kern in kernels_of(_c):
        RUN_BY.setdefault(_kern, case_id(_c))


def case_operands(name, k, H):
    """(a, el, er, ee, V, g): the inputs of a case.  Head h holds the el / er scenario (h + s) mod 6 and the ee scenario (h + 2 s + 1)
    mod 6, s the case's number, so that the pairings differ from case to case."""
    a = graph(name)
    shift = PAIRS.index((k, H)) + GPU_GRAPHS.index(name)
    el, er, ee, V = ge.operands(gat.scenarios_of(H, shift=shift), ge.edge_scenarios_of(H, shift=2 * shift + 1), a, k, seed=1)
    return a, el, er, ee, V, grad(a, k, 1)


# ---- the reference

@pytest.mark.parametrize("p", DROPS)
@pytest.mark.parametrize("name", ["thresholds", "directed_empty"])
@pytest.mark.parametrize("k,H", [(32, 4), (8, 1)])
def test_the_reference_agrees_with_an_independent_float64_torch_autograd_evaluation(name, k, H, p):
    """el, er and ee are multiples of 1 / 64 and the slope is 1 / 4, so that every score is exact in fp32: the reference's softmax
    starts from the score rounded to fp32, torch's from the float64 one, and the two are then the same number.  The mask enters torch
    as a constant tensor."""
    pytest.importorskip("torch")
    a, slope = graph(name), 0.25
    el, er, V = gat.operands(["uniform4"] * H, a, k, seed=1)
    ee = np.random.default_rng([k, H, 5]).uniform(-2, 2, (a.nnz, H))  # as wide as el and er: x spans +-6, both branches in most rows
    el, er, ee = (np.round(x * 64) / 64 + np.float32(0) for x in (el, er, ee))
    el, er, ee = (x.astype(np.float32) for x in (el, er, ee))
    g = grad(a, k, 2)
    ref = ge.reference(a, el, er, ee, V, slope, p, SEED)
    refb = ge.backward_reference(a, el, er, ee, V, ref["p"], g, slope, p, SEED)  # on the float64 alpha: torch keeps its own in float64 too
    kp = ad.kept_entries(a, H, p, SEED) if p else None
    want = ge.torch_float64(a, el, er, ee, V, slope, g, kp, ad.factor(p) if p else 1.0)
    for what, x, y in zip(("Out", "P", "gEl", "gEr", "gEe", "gV"), (ref["out"], ref["p"], refb["gel"], refb["ger"], refb["gee"], refb["gv"]), want):
        err = float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))
        assert err <= 1e-12, f"{name} k={k} H={H} p={p} {what}: {err:.3g}"


def _both_checkers(a, el, er, ee, V, g, p, res, what):
    each = {}
    ge.check(a, el, er, ee, V, SLOPE, p, SEED, res["out"], res["p"], what=what, ratios=each)
    ge.check_backward(a, el, er, ee, V, res["p"], g, SLOPE, p, SEED, res["gel"], res["ger"], res["gee"], res["gv"], what=what, ratios=each)
    return each


@pytest.mark.parametrize("p", DROPS)
@pytest.mark.parametrize("shift", range(6))
def test_an_fp32_evaluation_passes_both_checkers_on_every_scenario(shift, p):
    """Six heads: head h holds the el / er scenario h and the ee scenario h + shift, so the six runs layer every ee scenario on every
    el / er scenario.  The fp32 evaluation is the evidence that the bounds are not too tight: the worst err / bound is below 1."""
    a, k, H = graph("thresholds"), 24, 6
    el, er, ee, V = ge.operands(gat.scenarios_of(H), ge.edge_scenarios_of(H, shift=shift), a, k, seed=3)
    g = grad(a, k, 3)
    res = ge.fp32_evaluation(a, el, er, ee, V, SLOPE, p, SEED, g=g)
    each = _both_checkers(a, el, er, ee, V, g, p, res, f"shift {shift} p {p}")
    print(f"fp32 evaluation, ee scenarios shifted by {shift}, p = {p}: worst err / bound " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))
    assert max(each.values()) < 1.0


@pytest.mark.parametrize("edge", ["cancel", "near_cancel"])
def test_the_cancellation_reaches_a_visible_fraction_of_the_bound_on_p(edge):
    """Rows of TWO entries with el + er of magnitude about 2^6 on both: on the first ee cancels fl(el + er), so the computed x is +0
    (cancel) or a few ulps of el + er (near_cancel) while the float64 x keeps the rounding residue of the first addition, up to
    u |el + er|; on the second ee = -(el + er) rounded to a multiple of 2^-10, so its x is small and exact and the row's spread D stays
    near zero.  The score's term gamma(2) f |el + er| is then the larger part of dalpha's bracket (about 2 expm1(2 slope u 2^6) against
    gamma(n_r + 4 D + ...), some 40 u), and the error it allows is attained up to the residue's size: the worst err / bound on P must
    be above 1 / 100 -- two orders of magnitude are what `slack by orders of magnitude` means -- and, as everywhere, below 1."""
    m = 400
    rng = np.random.default_rng(17)
    rp = (2 * np.arange(m + 1)).astype(np.uint32)
    col = rng.permutation(2 * m).astype(np.uint32)
    a = binding.HostCsr(rp, col, np.ones(2 * m, np.float32), n=2 * m)
    el = rng.uniform(30, 60, (m, 1)).astype(np.float32)
    er = rng.uniform(30, 60, (2 * m, 1)).astype(np.float32)
    row = np.repeat(np.arange(m), 2)
    s = (el[row, 0] + er[col, 0]).astype(np.float32)
    ee = (-np.round(s.astype(np.float64) * 1024) / 1024).astype(np.float32)
    first = np.arange(0, 2 * m, 2)
    ee[first] = -s[first] if edge == "cancel" else (-s[first] * np.float32(1 + 2.0 ** -20)).astype(np.float32)
    ee = ee[:, None] + np.float32(0)
    V = rng.uniform(-1, 1, (2 * m, 4)).astype(np.float32)
    res = ge.fp32_evaluation(a, el, er, ee, V, SLOPE)
    each = {}
    ge.check(a, el, er, ee, V, SLOPE, 0.0, SEED, res["out"], res["p"], what=edge, ratios=each)
    print(f"{edge}: worst err / bound on P {each['p']:.3g}, on Out {each['out']:.3g}")
    assert 0.01 < each["p"] < 1.0


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_a_float64_result_rounded_to_fp32_passes_both_checkers_on_every_gpu_case(c):
    name, k, H, p = c
    a, el, er, ee, V, g = case_operands(name, k, H)
    res = ge.fp32_result(a, el, er, ee, V, SLOPE, p, SEED, g=g)
    assert max(_both_checkers(a, el, er, ee, V, g, p, res, case_id(c)).values()) <= 1.0


@pytest.mark.parametrize("p", DROPS)
def test_a_row_range_slice_reads_ee_at_the_whole_matrix_entries(p):
    a, k, H = graph("thresholds_lifted"), 32, 4
    el, er, ee, V = ge.operands(gat.scenarios_of(H, shift=1), ge.edge_scenarios_of(H, shift=1), a, k, seed=2)
    res = ge.fp32_result(a, el, er, ee, V, SLOPE, p, SEED)
    r0, r1 = 7, 60
    e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
    part = ge.fp32_result(a, el[r0:r1], er, ee, V, SLOPE, p, SEED, rows=(r0, r1))
    assert np.array_equal(part["out"], res["out"][r0:r1], equal_nan=True) and np.array_equal(part["p"], res["p"][e0:e1], equal_nan=True)
    assert ge.check(a, el[r0:r1], er, ee, V, SLOPE, p, SEED, part["out"], part["p"], rows=(r0, r1)) <= 1.0
    shifted = np.roll(ee, e0, axis=0)  # a shard that indexed ee from its own first entry
    bad = ge.fp32_result(a, el[r0:r1], er, shifted, V, SLOPE, p, SEED, rows=(r0, r1))
    with pytest.raises(AssertionError):
        ge.check(a, el[r0:r1], er, ee, V, SLOPE, p, SEED, bad["out"], bad["p"], rows=(r0, r1))


# ---- the planted faults

P_FAULT = 0.25


def _fault_case(fault):
    a, k, H = graph("thresholds_lifted"), 32, 4
    edge = {"mask_spreads": ["edge_masked", "spread", "zero_edge", "spread"], "branch_from_el_er": ["spread", "cancel", "spread", "near_cancel"]}
    el, er, ee, V = ge.operands(["uniform4", "spread80", "uniform4", "zero"], edge.get(fault, ["spread", "cancel", "zero_edge", "spread"]), a, k, seed=4)
    return a, k, H, el, er, ee, V, grad(a, k, 4)


# every fault without and with dropout; gee_unmasked with dropout only: without it there is no mask to leave out
@pytest.mark.parametrize("fault,p", [(f, p) for f in ge.FAULTS for p in (0.0, P_FAULT) if p or f != "gee_unmasked"])
def test_the_checker_a_fault_targets_rejects_it(fault, p):
    a, k, H, el, er, ee, V, g = _fault_case(fault)
    right = ge.fp32_result(a, el, er, ee, V, SLOPE, p, SEED, g=g)
    assert max(_both_checkers(a, el, er, ee, V, g, p, right, "right").values()) <= 1.0
    bad = ge.fp32_result(a, el, er, ee, V, SLOPE, p, SEED, g=g, probs=right["p"], fault=fault)
    if fault in ge.SCORE_FAULTS:
        with pytest.raises(AssertionError):  # Out gives it away
            ge.check(a, el, er, ee, V, SLOPE, p, SEED, bad["out"], what=fault)
        with pytest.raises(AssertionError, match=r"\bP\b"):  # and so does P beside the right Out
            ge.check(a, el, er, ee, V, SLOPE, p, SEED, right["out"], bad["p"], what=fault)
        if fault == "branch_from_el_er":  # the backward's branch as well, from the right P
            with pytest.raises(AssertionError, match="gee"):
                ge.check_backward(a, el, er, ee, V, right["p"], g, SLOPE, p, SEED, gEe=bad["gee"], what=fault)
        return
    with pytest.raises(AssertionError, match="gee"):
        ge.check_backward(a, el, er, ee, V, right["p"], g, SLOPE, p, SEED, gEe=bad["gee"], what=fault)
    assert all(np.array_equal(bad[key], right[key], equal_nan=True) for key in ("gel", "ger", "gv")), fault  # and nothing else moved


# ---- the public surface

NAMES_C = ("flex_edge_gat_attention", "flex_edge_gat_attention_backward")


def test_the_library_exports_the_two_calls_and_the_header_declares_them():
    hdr = open(os.path.join(ROOT, "include", "flex_spmm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+FLEX_ABI_VERSION\s+3\b", hdr)
    L = ctypes.CDLL(flex_amd.lib_path())
    for name in NAMES_C:
        assert re.search(r"^int\s+%s\s*\(" % name, code, re.M), f"{name} is not declared `int {name}(` in include/flex_spmm.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in binding.SYMBOLS
        assert not any(re.match(pat, name) for pat in (r"flex_(gat_)?attention\w*$", r"flex_gatv2_\w*$", r"flex_dropout_gatv2_\w*$")), name
    assert len(binding._values_fn(NAMES_C[0]).argtypes) == 12 and len(binding._values_fn(NAMES_C[1]).argtypes) == 17
    assert L.flex_abi_version() == 3
    for text in ("x_eh = fl(fl(el[r, h] + er[src(e), h]) + ee[e, h])", "|x^ - x| <= u (1 + u) |el + er| + u |x|",
                 "ds_e = gamma(2) f_e |el + er| + gamma(3) |s_e| + 2^-149"):  # the definition and the bound, verbatim in the header and the module
        assert text in hdr and text in ge.__doc__, text


def test_the_package_offers_the_methods_and_the_other_accessors_keep_their_entries():
    for f in ("gat_edge_attention", "gat_edge_attention_backward"):
        assert callable(getattr(flex_amd.Plan, f, None)), f
        assert callable(getattr(flex_amd.Plan, f + "_ptr", None)), f + "_ptr"
    pytest.importorskip("torch")
    from flex_amd import autograd
    assert len(autograd.functions()) == 10 and len(autograd.dropout_functions()) == 1 and len(autograd.gat_dropout_functions()) == 1
    assert len(autograd.gat_bf16_functions()) == 2
    assert [f.__name__ for f in autograd.gat_edge_functions()] == ["_FusedGatEdgeAttention"]


def test_the_operators_error_rules_with_edge():
    torch = pytest.importorskip("torch")
    import inspect
    assert list(inspect.signature(flex_amd.SparseOperator.gat_attention).parameters)[-1] == "edge"
    el, V, edge = torch.zeros((8, 4)), torch.zeros((8, 32)), torch.zeros((20, 4))
    for flags in (dict(), dict(fused_attention=True)):  # the NotImplementedError and ValueError rules are unchanged
        with pytest.raises(NotImplementedError, match="fused_backward=True"):
            _NoPlan(20, 32, **flags).gat_attention(el, el, V, edge=edge)
    op = _NoPlan(20, 32, fused_attention=True, fused_backward=True)
    for bad in (1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="probability"):
            op.gat_attention(el, el, V, dropout=bad, edge=edge)
    for bad in (edge.double(), edge.bfloat16(), torch.zeros((20,)), torch.zeros((4, 20)), torch.zeros((19, 4)), torch.zeros((20, 1)), edge.numpy(), 0.0):
        with pytest.raises(TypeError, match="edge"):
            op.gat_attention(el, el, V, edge=bad)
    with pytest.raises(TypeError, match="edge"):  # bf16 V has no edge form
        op.gat_attention(el, el, V.bfloat16(), edge=edge)
    with pytest.raises(TypeError, match="edge"):
        op.gat_attention(el.bfloat16(), el, V, edge=edge)


# ---- the census

def shipped_gat_edge_kernels(so):
    """The kernel handles (data symbols, not the launchers' code) of flex::gat_edge in a built library, as `nm -C` names them without the
    namespace and the parameters."""
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-C", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        _, kind, sym = line.split(" ", 2)
        head = sym.split("(", 1)[0]
        if kind in "tTwW" or "__device_stub__" in sym or "flex::gat_edge::" not in head:
            continue
        names.add(head.split("flex::gat_edge::", 1)[1])
    return names


def test_the_library_ships_exactly_the_twenty_eight_kernels_and_a_gpu_case_runs_each():
    so = os.path.join(os.path.dirname(binding.__file__), "lib", "libflex_spmm.so")
    assert os.path.exists(so), f"{so} is not built"
    shipped = shipped_gat_edge_kernels(so)
    assert len(shipped) == 28, sorted(shipped)
    wanted = {f"{kern}<{W}, {NS}, {drop}>" for W, NS in FORMS for kern in ("gat_edge_rows", "gat_edge_rows_backward") for drop in ("false", "true")}
    assert len(wanted) == 28 and shipped == wanted, (sorted(shipped - wanted), sorted(wanted - shipped))
    assert set(RUN_BY) == shipped, (f"kernels no GPU case launches: {sorted(shipped - set(RUN_BY))}", f"declared but not shipped: {sorted(set(RUN_BY) - shipped)}")
    ids = {case_id(c) for c in CASES}
    assert all(v in ids for v in RUN_BY.values())
    assert {FORM_OF_K[k] for k, _ in PAIRS} == set(FORMS)

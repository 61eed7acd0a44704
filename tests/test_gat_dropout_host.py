"""Host checks of the attention dropout in the fused GAT attention (include/flex_spmm.h: flex_gat_attention_dropout and its backward):
the float64 reference (tests/gat_dropout_ref.py) against an independent float64 torch autograd evaluation, a float64 result rounded to
fp32 against both checkers, every planted fault against the checker it targets, the public surface, and the census of the kernels in
flex::gat_dropout with the GPU case that runs each.  No GPU."""
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
import gat_dropout_ref as gd
from attention_forms import ALL_WANTED, COLUMN_KERNEL_ALONE, FORM_OF_K, FORMS, ROW_KERNEL_ALONE, fake_address
from backward_ref import _directed
from conftest import ROOT
from flex_amd import binding
from fused_attention_backward_ref import both_sides
from fused_attention_ref import threshold_graph
from softmax_ref import long_rows_graph

SLOPE = gat.SLOPE
SEED = 0x0123456789ABCDEF  # a non-zero high word

# ---- the table of tests/test_gpu_gat_dropout.py: every (W, NS) form, idle lanes past k (48), d = 4 and d = 256, H = 1; the wide pairs
# (k >= 256) run on the graph that holds every class of row and of column
PAIRS = [(4, 1), (8, 2), (32, 4), (48, 3), (64, 8), (128, 1), (256, 1), (512, 2), (1024, 64)]
GRAPHS = {
    "thresholds_lifted": lambda: both_sides(threshold_graph()),
    "directed_empty": lambda: _directed(250, 260, seed=7),
    "long_rows": long_rows_graph,
    "thresholds": threshold_graph,
}
GPU_GRAPHS = ["directed_empty", "long_rows", "thresholds_lifted"]
# (graph, k, H, p): p = 0.5 everywhere, and 0.1 and 0.9 at (32, 4)
CASES = [(name, k, H, p) for k, H in PAIRS for name in (GPU_GRAPHS if k < 256 else ["thresholds_lifted"])
         for p in ((0.5, 0.1, 0.9) if (k, H) == (32, 4) else (0.5,))]


def case_id(c):
    name, k, H, p = c
    return f"{name}-k{k}-h{H}-p{p}"


def kernels_of(c):
    """The three instantiations in flex::gat_dropout that the forward and the backward (every gradient wanted) of a case launch, as
    `nm -C` names them: written down from FORM_OF_K, not computed by the rule it checks."""
    W, NS = FORM_OF_K[c[1]]
    return [f"gat_dropout_rows<{W}, {NS}>", f"gat_dropout_rows_backward<{W}, {NS}>", f"gat_dropout_columns_backward<{W}, {NS}>"]


# kernel -> the id of the first case of test_every_output_against_float64 (tests/test_gpu_gat_dropout.py) that launches it
RUN_BY = {}
for _c in CASES:
    for _kern in kernels_of(_c):
        RUN_BY.setdefault(_kern, case_id(_c))

_graphs = {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = GRAPHS[name]()
    return _graphs[name]


def grad(a, k, seed):
    return np.random.default_rng([seed, k, 81]).uniform(-1, 1, (a.m, k)).astype(np.float32)


def case_operands(name, k, H):
    """(a, el, er, V, g): the inputs of a case, a score scenario per head (masks and poison come through el and er)."""
    a = graph(name)
    shift = PAIRS.index((k, H)) + GPU_GRAPHS.index(name)
    el, er, V = gat.operands(gat.scenarios_of(H, shift=shift), a, k, seed=1)
    return a, el, er, V, grad(a, k, 1)


# ---- the reference

@pytest.mark.parametrize("name", ["thresholds", "directed_empty"])
@pytest.mark.parametrize("k,H", [(32, 4), (8, 1)])
def test_the_reference_agrees_with_an_independent_float64_torch_autograd_evaluation(name, k, H):
    """el and er are multiples of 1 / 64 and the slope is 1 / 4, so that every score is exact in fp32: the reference's softmax starts
    from the score rounded to fp32, torch's from the float64 one, and the two are then the same number.  The mask enters torch as a
    constant tensor."""
    pytest.importorskip("torch")
    a, slope, p = graph(name), 0.25, 0.6
    el, er, V = gat.operands(gat.scenarios_of(H, shift=5)[:H] if H > 1 else ["uniform4"], a, k, seed=1)
    el, er = (np.where(np.isfinite(x), np.round(x * 64) / 64, x).astype(np.float32) for x in (el, er))
    el, er = np.nan_to_num(el, nan=0.5, neginf=-1.0), np.nan_to_num(er, nan=0.5, neginf=-1.0)  # every score finite: torch has no mask rules
    g = grad(a, k, 2)
    ref = gd.reference(a, el, er, V, slope, p, SEED)
    refb = gd.backward_reference(a, el, er, V, ref["p"], g, slope, p, SEED)  # on the float64 alpha: torch keeps its own in float64 too
    kp = ad.kept_entries(a, H, p, SEED)
    assert 0.3 < kp.mean() < 0.5
    want = gd.torch_float64(a, el, er, V, slope, g, kp, ad.factor(p))
    for what, x, y in zip(("Out", "gEl", "gEr", "gV"), (ref["out"], refb["gel"], refb["ger"], refb["gv"]), want):
        err = float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))
        assert err <= 1e-12, f"{name} k={k} H={H} {what}: {err:.3g}"


NAMES = {"finite": ["uniform4", "zero", "spread80", "uniform4"], "mixed": ["poisoned", "masked30", "rows_masked", "zero"]}


@pytest.mark.parametrize("name", ["thresholds_lifted", "directed_empty"])
@pytest.mark.parametrize("names", sorted(NAMES))
def test_a_float64_result_rounded_to_fp32_passes_both_checkers(name, names):
    a, k = graph(name), 32
    el, er, V = gat.operands(NAMES[names], a, k, seed=2)
    g = grad(a, k, 2)
    res = gd.fp32_result(a, el, er, V, SLOPE, 0.5, SEED, g=g)
    assert gd.check(a, el, er, V, SLOPE, 0.5, SEED, res["out"], res["p"], what="forward") <= 1.0
    assert gd.check_backward(a, el, er, V, res["p"], g, SLOPE, 0.5, SEED, res["gel"], res["ger"], res["gv"], res["dx"], what="backward") <= 1.0
    r0, r1 = 7, 60  # a row-range slice of the forward
    e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
    part = gd.fp32_result(a, el[r0:r1], er, V, SLOPE, 0.5, SEED, rows=(r0, r1))
    assert np.array_equal(part["out"], res["out"][r0:r1], equal_nan=True) and np.array_equal(part["p"], res["p"][e0:e1], equal_nan=True)
    assert gd.check(a, el[r0:r1], er, V, SLOPE, 0.5, SEED, part["out"], part["p"], rows=(r0, r1)) <= 1.0


# ---- the planted faults

P_FAULT = 0.25  # c = 4 / 3 and 1 / p = 4 differ (at p = 0.5 they are the same number)


def _fault_case(fault):
    a, k, H = graph("thresholds_lifted"), 32, 4
    el, er, V = gat.operands(["uniform4", "spread80", "uniform4", "masked30"], a, k, seed=4)
    if fault == "multiply_by_zero":  # an inf V row behind dropped entries (and behind kept ones, where it reaches Out in float64 too)
        kp = ad.kept_entries(a, H, P_FAULT, SEED)
        col = gat.coo(a)[1]
        V = V.copy()
        V[col[np.flatnonzero(~kp[:, 0])[:3]], :8] = np.inf
    return a, k, H, el, er, V, grad(a, k, 4)


@pytest.mark.parametrize("fault", gd.FAULTS)
def test_the_checker_a_fault_targets_rejects_it(fault):
    a, k, H, el, er, V, g = _fault_case(fault)
    rows = (17, 300) if fault == "shard_local" else None
    elr = el if rows is None else el[rows[0]:rows[1]]
    gg = None if rows or fault == "multiply_by_zero" else g
    right = gd.fp32_result(a, elr, er, V, SLOPE, P_FAULT, SEED, g=gg, rows=rows)
    assert gd.check(a, elr, er, V, SLOPE, P_FAULT, SEED, right["out"], right["p"], rows=rows) <= 1.0
    bad = gd.fp32_result(a, elr, er, V, SLOPE, P_FAULT, SEED, g=gg, probs=right["p"], rows=rows, fault=fault)
    if fault in gd.FORWARD_FAULTS:
        with pytest.raises(AssertionError):  # Out gives it away
            gd.check(a, elr, er, V, SLOPE, P_FAULT, SEED, bad["out"], rows=rows, what=fault)
        if fault == "mask_before_norm":
            with pytest.raises(AssertionError, match=r"\bP\b"):  # and so does P beside the right Out
                gd.check(a, elr, er, V, SLOPE, P_FAULT, SEED, right["out"], bad["p"], rows=rows, what=fault)
        return
    assert gd.check_backward(a, el, er, V, right["p"], g, SLOPE, P_FAULT, SEED, right["gel"], right["ger"], right["gv"], right["dx"]) <= 1.0
    targets = {"gv_unmasked": [("gv", "gV")], "ger_masked_twice": [("ger", "gEr")], "gel_masked_twice": [("gel", "gEl")],
               "da_unmasked": [("dx", "dx"), ("gel", "gEl"), ("ger", "gEr")]}[fault]  # da of a dropped entry is not +0, and dx, gEl and gEr follow
    for key, arg in targets:
        with pytest.raises(AssertionError, match=key):
            gd.check_backward(a, el, er, V, right["p"], g, SLOPE, P_FAULT, SEED, what=fault, **{arg: bad[key]})
    others = {"gel", "ger", "gv", "dx"} - {key for key, _ in targets}  # and nothing else moved
    assert all(np.array_equal(bad[key], right[key], equal_nan=True) for key in others), fault


def test_the_graphs_have_heads_of_non_empty_rows_with_every_entry_dropped():
    """What the GPU file's fourth test needs of its inputs, with the project's mask and that seed."""
    for name in GPU_GRAPHS:
        a = graph(name)
        row, _, rp = gat.coo(a)
        for H in (1, 4):
            for p in (0.5, 0.6, 0.9):
                kp = ad.kept_entries(a, H, p, SEED)
                dead = 0
                for h in range(H):
                    any_kept = np.zeros(a.m, bool)
                    any_kept[row[kp[:, h]]] = True
                    dead += int((~any_kept & (np.diff(rp) > 0)).sum())
                assert 18 <= dead <= 2236, (name, H, p, dead)


# ---- the public surface

NAMES_C = ("flex_gat_attention_dropout", "flex_gat_attention_dropout_backward")


def test_the_library_exports_the_two_calls_and_the_header_declares_them():
    hdr = open(os.path.join(ROOT, "include", "flex_spmm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+FLEX_ABI_VERSION\s+3\b", hdr)
    L = ctypes.CDLL(flex_amd.lib_path())
    for name in NAMES_C:
        assert re.search(r"^int\s+%s\s*\(" % name, code, re.M), f"{name} is not declared `int {name}(` in include/flex_spmm.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in binding.SYMBOLS
    assert len(binding._values_fn(NAMES_C[0]).argtypes) == 11 and len(binding._values_fn(NAMES_C[1]).argtypes) == 15
    assert L.flex_abi_version() == 3


def test_the_package_offers_the_methods_and_the_other_accessors_keep_their_entries():
    for f in ("gat_attention_dropout", "gat_attention_dropout_backward"):
        assert callable(getattr(flex_amd.Plan, f, None)), f
        assert callable(getattr(flex_amd.Plan, f + "_ptr", None)), f + "_ptr"
    pytest.importorskip("torch")
    from flex_amd import autograd
    assert len(autograd.functions()) == 10 and len(autograd.dropout_functions()) == 1
    assert [f.__name__ for f in autograd.gat_dropout_functions()] == ["_FusedGatAttentionDropout"]


class _NoPlan(flex_amd.SparseOperator):
    """The operator's argument checks without its plans (making a plan needs a GPU)."""

    def __init__(self, nnz, k, **flags):
        self.m = self.n = 8
        self.k, self.nnz = k, nnz
        self.learn_values = True
        self.fused_attention, self.fused_backward = flags.get("fused_attention", False), flags.get("fused_backward", False)


def test_gat_dropout_needs_both_fused_paths_and_a_probability():
    torch = pytest.importorskip("torch")
    el, V = torch.zeros((8, 4)), torch.zeros((8, 32))
    for flags in (dict(), dict(fused_attention=True)):
        for kw in (dict(), dict(dropout=0.5), dict(dropout=0.5, training=False)):
            with pytest.raises(NotImplementedError, match="fused_backward=True"):
                _NoPlan(20, 32, **flags).gat_attention(el, el, V, **kw)
    op = _NoPlan(20, 32, fused_attention=True, fused_backward=True)
    for bad in (1.0, -0.5, 2.0, float("nan")):
        for kw in (dict(), dict(training=False)):
            with pytest.raises(ValueError, match="probability"):
                op.gat_attention(el, el, V, dropout=bad, **kw)


# ---- the census

def shipped_gat_dropout_kernels(so):
    """The kernel handles (data symbols, not the launchers' code) of flex::gat_dropout in a built library, as `nm -C` names them without
    the namespace and the parameters."""
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-C", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        _, kind, sym = line.split(" ", 2)
        head = sym.split("(", 1)[0]
        if kind in "tTwW" or "__device_stub__" in sym or "flex::gat_dropout::" not in head:
            continue
        names.add(head.split("flex::gat_dropout::", 1)[1])
    return names


def test_the_library_ships_exactly_the_twenty_one_kernels_and_a_gpu_case_runs_each():
    so = os.path.join(os.path.dirname(binding.__file__), "lib", "libflex_spmm.so")
    assert os.path.exists(so), f"{so} is not built"
    shipped = shipped_gat_dropout_kernels(so)
    assert len(shipped) == 21, sorted(shipped)
    wanted = {f"{kern}<{W}, {NS}>" for W, NS in FORMS for kern in ("gat_dropout_rows", "gat_dropout_rows_backward", "gat_dropout_columns_backward")}
    assert len(wanted) == 21 and shipped == wanted, (sorted(shipped - wanted), sorted(wanted - shipped))
    assert set(RUN_BY) == shipped, (f"kernels no GPU case launches: {sorted(shipped - set(RUN_BY))}", f"declared but not shipped: {sorted(set(RUN_BY) - shipped)}")
    ids = {case_id(c) for c in CASES}
    assert all(v in ids for v in RUN_BY.values())
    assert {FORM_OF_K[k] for k, _ in PAIRS} == set(FORMS)


# ---- the census against the launches

@pytest.fixture
def sim():
    """(tests/hostsim, flex_amd.binding's library on the host simulator) for one test: the others here run on the library itself."""
    hostsim = pytest.importorskip("hostsim")
    for lib in hostsim.binding_on_simulator():
        yield hostsim, lib


def test_every_pair_launches_on_the_simulator_the_kernels_its_cases_declare(sim):
    """The forward and then the backward of every (k, H) on fake operands (nothing is read or written): the library's own entry points
    on the simulator's stand-in launchers must log kernels_of() of the case, and with one gradient wanted the forward and one backward
    kernel: gEl the row kernel, gV the column kernel."""
    hostsim, lib = sim
    a = graph("thresholds_lifted")
    el, er, v, out, g, pr, work, gel, ger, gv = (fake_address(i) for i in range(10))
    for k, H in PAIRS:
        plan = flex_amd.Plan(a, k, attention=True, attention_backward=True)

        def launch(want):
            plan.gat_attention_dropout_ptr(H, el, er, v, SLOPE, 0.5, SEED, out, pr)
            plan.gat_attention_dropout_backward_ptr(H, el, er, v, pr, g, SLOPE, 0.5, SEED, *(x if w else None for x, w in zip((gel, ger, gv), want)), work)
        names = ["gat_dropout::" + n for n in kernels_of(("thresholds_lifted", k, H, 0.5))]
        assert hostsim.launch_log(lib, lambda: launch(ALL_WANTED)) == names, (k, H)
        assert hostsim.launch_log(lib, lambda: launch(ROW_KERNEL_ALONE)) == names[:2], (k, H)
        assert hostsim.launch_log(lib, lambda: launch(COLUMN_KERNEL_ALONE)) == [names[0], names[2]], (k, H)
        plan.destroy()

"""Host checks of the fused GAT attention on bf16 V rows (include/flex_spmm.h: flex_gat_attention_bf16, its backward and the dropout
pair): the references tests/gat_bf16_ref.py composes against an independent float64 torch autograd evaluation on the bf16 operands, a
float64 result rounded ONCE to bf16 against both checkers on every case of the GPU table (the inputs are fair), every planted fault
against the checker it targets, the public surface, and the census of the kernels in flex::gat_bf16 with the GPU case that runs each.
No GPU."""
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
import gat_bf16_ref as gb
import gat_dropout_ref as gd
from attention_forms import ALL_WANTED, COLUMN_KERNEL_ALONE, FORM_OF_K, FORMS, ROW_KERNEL_ALONE, fake_address
from conftest import ROOT
from flex_amd import binding
from test_gat_dropout_host import CASES as DROP_CASES
from test_gat_dropout_host import GPU_GRAPHS, PAIRS, SEED, SLOPE, graph
from test_gat_dropout_host import case_operands as fp32_case_operands

# ---- the table of tests/test_gpu_gat_bf16.py: tests/test_gat_dropout_host.py's (graph, k, H, p) cases, and the same (graph, k, H)
# undropped (p = None)
CASES = [(name, k, H, None) for k, H in PAIRS for name in (GPU_GRAPHS if k < 256 else ["thresholds_lifted"])] + list(DROP_CASES)


def case_id(c):
    name, k, H, p = c
    return f"{name}-k{k}-h{H}-" + ("plain" if p is None else f"p{p}")


def drop_of(c):
    return None if c[3] is None else (c[3], SEED)


def kernels_of(c):
    """The three instantiations in flex::gat_bf16 that the forward and the backward (every gradient wanted) of a case launch, as `nm -C`
    names them: written down from FORM_OF_K, not computed by the rule it checks."""
    W, NS = FORM_OF_K[c[1]]
    drop = "false" if c[3] is None else "true"
    return [f"{kern}<{W}, {NS}, {drop}>" for kern in ("gat_bf16_rows", "gat_bf16_rows_backward", "gat_bf16_columns_backward")]


# kernel -> the id of the first case of test_every_output_against_float64 (tests/test_gpu_gat_bf16.py) that launches it
RUN_BY = {}
for _c in CASES:
    for _kern in kernels_of(_c):
        RUN_BY.setdefault(_kern, case_id(_c))

_operands = {}


def case_operands(name, k, H):
    """(a, el, er, V, g): the fp32 table's inputs with V and g rounded to bf16 and widened (fp32 arrays of bf16 numbers); el, er untouched."""
    key = (name, k, H)
    if key not in _operands:
        a, el, er, V, g = fp32_case_operands(name, k, H)
        _operands[key] = (a, el, er, gb.rounded(V), gb.rounded(g))
    return _operands[key]


# ---- the reference

@pytest.mark.parametrize("drop", [None, (0.6, SEED)], ids=["plain", "p0.6"])
@pytest.mark.parametrize("name", ["thresholds", "directed_empty"])
@pytest.mark.parametrize("k,H", [(32, 4), (8, 1)])
def test_the_reference_agrees_with_an_independent_float64_torch_autograd_evaluation(name, k, H, drop):
    """On bf16 V and g.  el and er are multiples of 1 / 64 and the slope is 1 / 4, so that every score is exact in fp32 (as in
    tests/test_gat_dropout_host.py); the mask enters torch as a constant tensor, all ones without dropout."""
    pytest.importorskip("torch")
    a, slope = graph(name), 0.25
    el, er, V = gb.operands(gat.scenarios_of(H, shift=5)[:H] if H > 1 else ["uniform4"], a, k, seed=1)
    el, er = (np.where(np.isfinite(x), np.round(x * 64) / 64, x).astype(np.float32) for x in (el, er))
    el, er = np.nan_to_num(el, nan=0.5, neginf=-1.0), np.nan_to_num(er, nan=0.5, neginf=-1.0)  # every score finite: torch has no mask rules
    g = gb.rounded(np.random.default_rng([2, k, 81]).uniform(-1, 1, (a.m, k)).astype(np.float32))
    assert np.array_equal(gb.rounded(V), V) and np.array_equal(gb.rounded(g), g)  # V and g hold bf16 numbers
    ref = gb.reference(a, el, er, V, slope, drop)
    refb = gb.backward_reference(a, el, er, V, ref["p"], g, slope, drop)  # on the float64 alpha: torch keeps its own in float64 too
    kp = np.ones((a.nnz, H), bool) if drop is None else ad.kept_entries(a, H, drop[0], drop[1])
    want = gd.torch_float64(a, el, er, V, slope, g, kp, 1.0 if drop is None else ad.factor(drop[0]))
    for what, x, y in zip(("Out", "gEl", "gEr", "gV"), (ref["out"], refb["gel"], refb["ger"], refb["gv"]), want):
        err = float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))
        assert err <= 1e-12, f"{name} k={k} H={H} {what}: {err:.3g}"


# ---- the inputs are fair: a float64 result rounded once passes both checkers on every case of the GPU table

@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_a_float64_result_rounded_once_passes_both_checkers(c):
    """Worst err / bound over the table, recorded from this test: Out 0.995 and gV 0.996 (a float64 value rounded once to bf16 spends
    the 2^-8 |x64| term of the bound alone, and comes as close to it as a value lies to the midpoint of two bf16 neighbours just above a
    power of two); rounded once to fp32, P stays below 0.018, gEl below 0.033, gEr below 0.062 and dx below 0.26."""
    name, k, H, _ = c
    a, el, er, V, g = case_operands(name, k, H)
    drop = drop_of(c)
    res = gb.result(a, el, er, V, SLOPE, drop, g=g)
    each = {}
    assert gb.check(a, el, er, V, SLOPE, res["out"], res["p"], drop=drop, what=case_id(c), ratios=each) <= 1.0
    assert gb.check_backward(a, el, er, V, res["p"], g, SLOPE, res["gel"], res["ger"], res["gv"], res["dx"], drop=drop, what=case_id(c), ratios=each) <= 1.0
    print(f"{case_id(c)}: worst err / bound " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))


def test_a_row_range_slice_of_the_forward_passes_the_checker():
    a, k = graph("thresholds_lifted"), 32
    el, er, V = gb.operands(["poisoned", "masked30", "rows_masked", "zero"], a, k, seed=2)
    r0, r1 = 7, 60
    e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
    for drop in (None, (0.5, SEED)):
        res = gb.result(a, el, er, V, SLOPE, drop)
        part = gb.result(a, el[r0:r1], er, V, SLOPE, drop, rows=(r0, r1))
        assert np.array_equal(part["out"], res["out"][r0:r1]) and np.array_equal(part["p"], res["p"][e0:e1], equal_nan=True)
        assert gb.check(a, el[r0:r1], er, V, SLOPE, part["out"], part["p"], rows=(r0, r1), drop=drop) <= 1.0


def test_an_operand_changed_in_place_is_evaluated_again():
    """gat_bf16_ref shares one float64 evaluation between result() and the checker that follows it; the same array object with other
    contents must not get the earlier evaluation."""
    a, k = graph("directed_empty"), 8
    el, er, V = gb.operands(["uniform4", "zero"], a, k, seed=3)
    g = gb.rounded(np.random.default_rng([3, k, 81]).uniform(-1, 1, (a.m, k)).astype(np.float32))
    first = gb.reference(a, el, er, V, SLOPE)
    assert gb.reference(a, el, er, V, SLOPE) is first
    firstb = gb.backward_reference(a, el, er, V, first["p"], g, SLOPE)
    V[:] = 2 * V  # still bf16 numbers
    g[:] = 2 * g
    again = gb.reference(a, el, er, V, SLOPE)
    assert again is not first and np.array_equal(again["out"], 2 * first["out"], equal_nan=True)
    assert np.array_equal(gb.backward_reference(a, el, er, V, first["p"], g, SLOPE)["gv"], 2 * firstb["gv"], equal_nan=True)


# ---- the planted faults

P_FAULT = 0.25  # c = 4 / 3


def _fault_case():
    a, k = graph("thresholds_lifted"), 32
    el, er, V = gb.operands(["uniform4", "spread80", "poisoned", "masked30"], a, k, seed=4)
    g = gb.rounded(np.random.default_rng([4, k, 81]).uniform(-1, 1, (a.m, k)).astype(np.float32))
    return a, el, er, V, g


# every fault without and with dropout; gV has a mask with dropout only
FAULT_CASES = [(fault, drop) for fault in gb.FAULTS for drop in (None, (P_FAULT, SEED)) if not (fault == "gv_unmasked" and drop is None)]


@pytest.mark.parametrize("fault,drop", FAULT_CASES, ids=[f"{f}-{'plain' if d is None else 'p0.25'}" for f, d in FAULT_CASES])
def test_the_checker_a_fault_targets_rejects_it(fault, drop):
    a, el, er, V, g = _fault_case()
    right = gb.result(a, el, er, V, SLOPE, drop, g=g)
    assert gb.check(a, el, er, V, SLOPE, right["out"], right["p"], drop=drop) <= 1.0
    assert gb.check_backward(a, el, er, V, right["p"], g, SLOPE, right["gel"], right["ger"], right["gv"], right["dx"], drop=drop) <= 1.0
    bad = gb.result(a, el, er, V, SLOPE, drop, g=g, p=right["p"], fault=fault)
    if fault in ("out_truncated", "out_rounded_twice", "poison_spreads"):
        assert np.array_equal(bad["p"], right["p"], equal_nan=True)
        with pytest.raises(AssertionError, match="Out"):
            gb.check(a, el, er, V, SLOPE, bad["out"], drop=drop, what=fault)
    elif fault in ("p_bf16", "el_er_bf16"):
        with pytest.raises(AssertionError, match=r"\bP\b"):
            gb.check(a, el, er, V, SLOPE, right["out"], bad["p"], drop=drop, what=fault)
    else:
        with pytest.raises(AssertionError, match="gv"):
            gb.check_backward(a, el, er, V, right["p"], g, SLOPE, gV=bad["gv"], drop=drop, what=fault)
        assert all(np.array_equal(bad[key], right[key], equal_nan=True) for key in ("gel", "ger", "dx")), fault


# ---- the public surface

NAMES_C = ("flex_gat_attention_bf16", "flex_gat_attention_bf16_backward", "flex_gat_attention_bf16_dropout", "flex_gat_attention_bf16_dropout_backward")


def test_the_library_exports_the_four_calls_and_the_header_declares_them():
    hdr = open(os.path.join(ROOT, "include", "flex_spmm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+FLEX_ABI_VERSION\s+3\b", hdr)
    L = ctypes.CDLL(flex_amd.lib_path())
    for name in NAMES_C:
        assert re.search(r"^int\s+%s\s*\(" % name, code, re.M), f"{name} is not declared `int {name}(` in include/flex_spmm.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in binding.SYMBOLS
    assert [len(binding._values_fn(n).argtypes) for n in NAMES_C] == [9, 13, 11, 15]
    assert L.flex_abi_version() == 3


def test_the_package_offers_the_methods_and_the_other_accessors_keep_their_entries():
    for f in ("gat_attention_bf16", "gat_attention_bf16_backward", "gat_attention_bf16_dropout", "gat_attention_bf16_dropout_backward"):
        assert callable(getattr(flex_amd.Plan, f, None)), f
        assert callable(getattr(flex_amd.Plan, f + "_ptr", None)), f + "_ptr"
    pytest.importorskip("torch")
    from flex_amd import autograd
    assert len(autograd.functions()) == 10 and len(autograd.dropout_functions()) == 1 and len(autograd.gat_dropout_functions()) == 1
    assert [f.__name__ for f in autograd.gat_bf16_functions()] == ["_FusedGatAttentionBf16", "_FusedGatAttentionBf16Dropout"]


class _NoPlan(flex_amd.SparseOperator):
    """The operator's argument checks without its plans (making a plan needs a GPU)."""

    def __init__(self, nnz, k, **flags):
        self.m = self.n = 8
        self.k, self.nnz = k, nnz
        self.learn_values = True
        self.fused_attention, self.fused_backward = flags.get("fused_attention", False), flags.get("fused_backward", False)


def test_the_operator_refuses_other_dtype_mixes_and_keeps_its_other_checks_on_bfloat16():
    torch = pytest.importorskip("torch")
    el, V = torch.zeros((8, 4)), torch.zeros((8, 32), dtype=torch.bfloat16)
    for flags in (dict(), dict(fused_attention=True)):
        for kw in (dict(), dict(dropout=0.5)):
            with pytest.raises(NotImplementedError, match="fused_backward=True"):
                _NoPlan(20, 32, **flags).gat_attention(el, el, V, **kw)
    op = _NoPlan(20, 32, fused_attention=True, fused_backward=True)
    for bad in (1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="probability"):
            op.gat_attention(el, el.bfloat16(), V, dropout=bad)
    for e, r, v in ((el.bfloat16(), el, V.float()), (el, el.bfloat16(), V.float()), (el.double(), el, V), (el, el.half(), V), (el, el, V.half()),
                    (el.double(), el.double(), V.double())):
        for kw in (dict(), dict(dropout=0.5, seed=1)):
            with pytest.raises(TypeError, match="bfloat16"):
                op.gat_attention(e, r, v, **kw)


# ---- the census

def shipped_gat_bf16_kernels(so):
    """The kernel handles (data symbols, not the launchers' code) of flex::gat_bf16 in a built library, as `nm -C` names them without
    the namespace and the parameters."""
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-C", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        _, kind, sym = line.split(" ", 2)
        head = sym.split("(", 1)[0]
        if kind in "tTwW" or "__device_stub__" in sym or "flex::gat_bf16::" not in head:
            continue
        names.add(head.split("flex::gat_bf16::", 1)[1])
    return names


def test_the_library_ships_exactly_the_forty_two_kernels_and_a_gpu_case_runs_each():
    so = os.path.join(os.path.dirname(binding.__file__), "lib", "libflex_spmm.so")
    assert os.path.exists(so), f"{so} is not built"
    shipped = shipped_gat_bf16_kernels(so)
    assert len(shipped) == 42, sorted(shipped)
    wanted = {f"{kern}<{W}, {NS}, {drop}>" for W, NS in FORMS for kern in ("gat_bf16_rows", "gat_bf16_rows_backward", "gat_bf16_columns_backward")
              for drop in ("false", "true")}
    assert len(wanted) == 42 and shipped == wanted, (sorted(shipped - wanted), sorted(wanted - shipped))
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
    """The forward and then the backward of every (k, H), undropped and dropped, on fake operands (nothing is read or written): the
    library's own entry points on the simulator's stand-in launchers must log kernels_of() of the case, and with one gradient wanted
    the forward and one backward kernel: gEl the row kernel, gV the column kernel."""
    hostsim, lib = sim
    a = graph("thresholds_lifted")
    el, er, v, out, g, pr, work, gel, ger, gv = (fake_address(i) for i in range(10))
    for k, H in PAIRS:
        plan = flex_amd.Plan(a, k, attention=True, attention_backward=True)
        for p in (None, 0.5):
            def launch(want):
                grads = [x if w else None for x, w in zip((gel, ger, gv), want)]
                if p is None:
                    plan.gat_attention_bf16_ptr(H, el, er, v, SLOPE, out, pr)
                    plan.gat_attention_bf16_backward_ptr(H, el, er, v, pr, g, SLOPE, *grads, work)
                else:
                    plan.gat_attention_bf16_dropout_ptr(H, el, er, v, SLOPE, p, SEED, out, pr)
                    plan.gat_attention_bf16_dropout_backward_ptr(H, el, er, v, pr, g, SLOPE, p, SEED, *grads, work)
            names = ["gat_bf16::" + n for n in kernels_of(("thresholds_lifted", k, H, p))]
            assert hostsim.launch_log(lib, lambda: launch(ALL_WANTED)) == names, (k, H, p)
            assert hostsim.launch_log(lib, lambda: launch(ROW_KERNEL_ALONE)) == names[:2], (k, H, p)
            assert hostsim.launch_log(lib, lambda: launch(COLUMN_KERNEL_ALONE)) == [names[0], names[2]], (k, H, p)
        plan.destroy()

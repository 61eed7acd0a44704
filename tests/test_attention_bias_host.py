"""Host checks of the biased fused attention's reference and checkers (tests/attention_bias_ref.py) and of its public surface: the float64
reference against an independent float64 torch autograd evaluation, a float64 result rounded once (to fp32, and to bf16) against both
checkers on every case of the GPU table, every planted fault against the checker it targets, and the exported symbols, the header's
declarations, the new methods and the autograd entry.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import attention_bf16_ref as bf
import attention_bias_ref as ab
from attention_forms import BIAS_PAIRS as PAIRS
import flex_amd
from backward_ref import _directed
from conftest import ROOT
from fused_attention_backward_ref import both_sides
from fused_attention_ref import threshold_graph
from softmax_ref import long_rows_graph

SCALE = 0.25

# the table of tests/test_gpu_attention_bias.py: the (k, H) pairs are tests/attention_forms.py's (every (W, NS) form, idle lanes past k
# (48), d = 4 and d = 256, H = 1); the wide pairs (k >= 256) run on the graph that holds every class of row and of column
GRAPHS = {
    "thresholds_lifted": lambda: both_sides(threshold_graph()),
    "directed_empty": lambda: _directed(250, 260, seed=7),
    "long_rows": long_rows_graph,
}
CASES = [(name, k, H) for k, H in PAIRS for name in (sorted(GRAPHS) if k < 256 else ["thresholds_lifted"])]
_graphs = {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = GRAPHS[name]()
    return _graphs[name]


def grad(a, k, seed, bf16=False):
    g = np.random.default_rng([seed, k, 78]).uniform(-1, 1, (a.m, k)).astype(np.float32)
    return bf.rounded(g) if bf16 else g


def case_operands(name, k, H, bf16=False):
    """(a, scenario names, Q, K, V, bias, g): the inputs of a case of the table, a different bias scenario in every head."""
    a = graph(name)
    names = ab.scenarios_of(H, shift=PAIRS.index((k, H)) + sorted(GRAPHS).index(name))
    Q, K, V, bias = ab.operands(names, a, k, seed=1, bf16=bf16)
    return a, names, Q, K, V, bias, grad(a, k, 1, bf16)


# ---- the reference

@pytest.mark.parametrize("name", ["thresholds_lifted", "directed_empty"])
@pytest.mark.parametrize("k,H", [(32, 4), (8, 1)])
def test_the_reference_agrees_with_an_independent_float64_torch_autograd_evaluation(name, k, H):
    """Q and K hold multiples of 1 / 8 within +-1, scale is 1 / 4 and the bias multiples of 1 / 64 within +-4, so every t is exact in
    fp32: the reference's softmax starts from t rounded to fp32, torch's from the float64 one, and the two are then the same number."""
    pytest.importorskip("torch")
    a = graph(name)
    rng = np.random.default_rng([k, H, 5])
    Q, K = (rng.integers(-8, 9, (r, k)).astype(np.float32) / 8 for r in (a.m, a.n))
    V = rng.uniform(-1, 1, (a.n, k)).astype(np.float32)
    bias = rng.integers(-256, 257, (a.nnz, H)).astype(np.float32) / 64
    g = grad(a, k, 2)
    ref = ab.reference(a, Q, K, V, bias, SCALE, H)
    t64 = np.stack([SCALE * (Q.astype(np.float64)[ab.coo(a)[0]][:, ab.head_columns(k, H, h)] * K.astype(np.float64)[ab.coo(a)[1]][:, ab.head_columns(k, H, h)]).sum(1)
                    for h in range(H)], axis=1) + bias
    assert np.array_equal(ref["s"].astype(np.float64), t64), "the scores of this test are exact in fp32"
    refb = ab.backward_reference(a, Q, K, V, ref["p"], g, SCALE, H)  # on the float64 p: torch keeps its own in float64 too
    want = ab.torch_float64(a, Q, K, V, bias, SCALE, H, g)
    for what, x, y in zip(("Out", "gQ", "gK", "gV", "gBias"), (ref["out"], refb["gq"], refb["gk"], refb["gv"], refb["gb"]), want):
        err = float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))
        assert err <= 1e-12, f"{name} k={k} H={H} {what}: {err:.3g}"
    # on the fp32 p a kernel is given, it is the reference the unbiased checkers hold gQ, gK, gV and ds to, and gBias is its ds at scale 1
    p32 = ref["p"].astype(np.float32)
    mine, theirs = ab.backward_reference(a, Q, K, V, p32, g, SCALE, H), ab.mh.backward_reference(a, Q, K, V, p32, g, SCALE, H)
    for key in ("gq", "gk", "gv", "ds"):
        assert np.array_equal(mine[key], theirs[key]), key
    ones = ab.mh.backward_reference(a, Q, K, V, p32, g, 1.0, H)
    assert np.array_equal(mine["gb"], ones["ds"]) and np.array_equal(mine["gb_bound"], ones["ds_bound"])


# ---- a right result passes

def _right(case, bf16):
    a, names, Q, K, V, bias, g = case
    H = len(names)
    res = ab.fp32_result(a, Q, K, V, bias, SCALE, H, g=g)
    if bf16:  # Out and the gradients rounded ONCE from float64, P, ds and gBias fp32
        ref = ab.reference(a, Q, K, V, bias, SCALE, H)
        refb = ab.backward_reference(a, Q, K, V, res["p"], g, SCALE, H)
        res.update(out=bf.f64_to_bf16(ref["out"]), **{key: bf.f64_to_bf16(refb[key]) for key in ("gq", "gk", "gv")})
    return res


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name,k,H", CASES)
def test_float64_rounded_once_stays_inside_the_bounds_on_every_case_of_the_gpu_table(name, k, H, bf16):
    case = case_operands(name, k, H, bf16)
    a, names, Q, K, V, bias, g = case
    res = _right(case, bf16)
    each = {}
    wf = ab.check(a, Q, K, V, bias, SCALE, H, res["out"], res["p"], what=f"{name} k={k} H={H}", ratios=each, bf16=bf16)
    wb = ab.check_backward(a, Q, K, V, res["p"], g, SCALE, H, res["gq"], res["gk"], res["gv"], res["gb"], res["ds"], what=f"{name} k={k} H={H}",
                           ratios=each, bf16=bf16)
    print(f"{name} k={k} H={H} {'/'.join(names[:7])}: float64 rounded once, worst err / bound " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))
    assert max(wf, wb) <= 1.0


def test_every_scenario_does_what_its_name_says():
    a, k, H = graph("thresholds_lifted"), 28, 7
    Q, K, V, bias = ab.operands(ab.BIAS_SCENARIOS, a, k, seed=3)
    ref = ab.reference(a, Q, K, V, bias, SCALE, H)
    row, col, rp = ab.coo(a)
    by = {name: h for h, name in enumerate(ab.BIAS_SCENARIOS)}
    assert np.isfinite(Q).all() and np.isfinite(np.delete(K, by["opposed"] * 4, axis=1)).all()  # what masks and poisons is the bias
    for name in ("zero", "uniform4", "spread80"):
        assert np.isfinite(ref["p"][:, by[name]]).all() and np.isfinite(ref["out"][:, ab.head_columns(k, H, by[name])]).all()
    top = np.zeros(a.m)
    np.maximum.at(top, row, ref["p"][:, by["spread80"]])
    assert np.median(top[np.diff(rp) > 4]) > 0.9  # the bias decides the row: one entry takes nearly all of it
    masked = ref["s"][:, by["masked30"]] == -np.inf
    assert 0.25 < masked.mean() < 0.35 and np.all(ref["p"][masked, by["masked30"]] == 0)
    with np.errstate(over="ignore", invalid="ignore"):  # every p > 0 of a finite row is a normal fp32 number (the note in operands)
        p32 = np.nan_to_num(ref["p"]).astype(np.float32)
    assert not ((p32 > 0) & (p32 < 2.0 ** -126)).any()
    dead = np.ones(a.m, bool)
    dead[row[ref["s"][:, by["rows_masked"]] != -np.inf]] = False
    assert (dead & (np.diff(rp) > 0)).sum() >= 3  # whole rows masked through the bias alone
    for name in ("poisoned", "opposed"):
        nan_rows = np.unique(row[np.isnan(ref["p"][:, by[name]])])
        assert len(nan_rows) >= 2, name
        assert np.isnan(ref["out"][nan_rows][:, ab.head_columns(k, H, by[name])]).all()
    h = by["opposed"]
    nan_t = np.isnan(ref["s"][:, h])
    assert nan_t.any() and np.all(bias[nan_t, h] == -np.inf)  # +inf against -inf: the mask does not win


# ---- the planted faults

FAULT_NAMES = {"max_before_bias": ["rows_masked", "uniform4", "poisoned", "zero"]}


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fault", ab.FAULTS)
def test_the_checker_a_fault_targets_rejects_it(fault, bf16):
    a, k, H = graph("thresholds_lifted"), 32, 4
    names = FAULT_NAMES.get(fault, ["uniform4", "spread80", "uniform4", "masked30"])
    Q, K, V, bias = ab.operands(names, a, k, seed=4, bf16=bf16)
    g = grad(a, k, 4, bf16)
    rows = (17, 300) if fault == "shard_local" else None
    Qr = Q if rows is None else Q[rows[0]:rows[1]]
    narrow = (lambda x: bf.to_bf16(x)) if bf16 else (lambda x: x)
    right = ab.fp32_result(a, Qr, K, V, bias, SCALE, H, g=None if rows else g, rows=rows)
    assert ab.check(a, Qr, K, V, bias, SCALE, H, narrow(right["out"]), right["p"], rows=rows, bf16=bf16) <= 1.0
    bad = ab.fp32_result(a, Qr, K, V, bias, SCALE, H, g=None if rows else g, p=right["p"], rows=rows, fault=fault)
    if fault in ab.FORWARD_FAULTS:
        with pytest.raises(AssertionError):  # Out alone gives it away
            ab.check(a, Qr, K, V, bias, SCALE, H, narrow(bad["out"]), rows=rows, what=fault, bf16=bf16)
        with pytest.raises(AssertionError):  # and so does P beside the right Out
            ab.check(a, Qr, K, V, bias, SCALE, H, narrow(right["out"]), bad["p"], rows=rows, what=fault, bf16=bf16)
        return
    grads = lambda r: tuple(narrow(r[key]) for key in ("gq", "gk", "gv"))
    assert ab.check_backward(a, Q, K, V, right["p"], g, SCALE, H, *grads(right), right["gb"], right["ds"], bf16=bf16) <= 1.0
    key = "ds" if fault == "work_holds_gb" else "gB"
    with pytest.raises(AssertionError, match="ds" if key == "ds" else "gBias"):
        ab.check_backward(a, Q, K, V, right["p"], g, SCALE, H, **{key: bad["ds" if key == "ds" else "gb"]}, what=fault, bf16=bf16)
    with pytest.raises(AssertionError):
        ab.check_backward(a, Q, K, V, right["p"], g, SCALE, H, *grads(bad), bad["gb"], bad["ds"], what=fault, bf16=bf16)


def test_the_checkers_hold_p_and_gbias_to_fp32_and_the_layout_of_the_edge_arrays():
    a, k, H = graph("directed_empty"), 32, 4
    Q, K, V, bias = ab.operands(["uniform4", "spread80", "uniform4", "masked30"], a, k, seed=6, bf16=True)
    g = grad(a, k, 6, True)
    res = _right((a, [None] * H, Q, K, V, bias, g), True)
    ab.check(a, Q, K, V, bias, SCALE, H, res["out"], res["p"], bf16=True)
    with pytest.raises(AssertionError, match="entries of P beyond the bound"):
        ab.check(a, Q, K, V, bias, SCALE, H, res["out"], bf.rounded(res["p"]), what="P in bf16", bf16=True)
    with pytest.raises(AssertionError, match="gBias beyond the bound"):
        ab.check_backward(a, Q, K, V, res["p"], g, SCALE, H, gB=bf.rounded(res["gb"]), what="gBias in bf16", bf16=True)
    with pytest.raises(AssertionError):  # head-major edge arrays in the same memory
        ab.check(a, Q, K, V, bias, SCALE, H, res["out"], np.ascontiguousarray(res["p"].T).reshape(res["p"].shape), bf16=True)
    with pytest.raises(AssertionError):
        ab.check_backward(a, Q, K, V, res["p"], g, SCALE, H, gB=np.ascontiguousarray(res["gb"].T).reshape(res["gb"].shape), bf16=True)
    with pytest.raises(AssertionError):  # fp32 Out handed over in place of bf16 bits
        ab.check(a, Q, K, V, bias, SCALE, H, bf.from_bf16(res["out"]), bf16=True)


# ---- the public surface

NAMES = ("flex_attention_bias", "flex_attention_bias_backward", "flex_attention_bf16_bias", "flex_attention_bf16_bias_backward")


def test_the_library_exports_the_four_calls_and_the_header_declares_them():
    hdr = open(os.path.join(ROOT, "include", "flex_spmm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+FLEX_ABI_VERSION\s+3\b", hdr)
    L = ctypes.CDLL(flex_amd.lib_path())
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/flex_spmm.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in flex_amd.binding.SYMBOLS
        assert len(flex_amd.binding._values_fn(name).argtypes) == (14 if name.endswith("backward") else 10)
    assert L.flex_abi_version() == 3


def test_the_package_offers_the_methods_and_functions_keeps_its_first_nine_entries():
    for f in ("attention_bias", "attention_bias_backward", "attention_bf16_bias", "attention_bf16_bias_backward"):
        assert callable(getattr(flex_amd.Plan, f, None)), f
        assert callable(getattr(flex_amd.Plan, f + "_ptr", None)), f + "_ptr"
    pytest.importorskip("torch")
    from flex_amd import autograd
    fs = autograd.functions()
    assert [f.__name__ for f in fs[:9]] == ["_SpMM", "_AxwLayer", "_SpMMValues", "_Sddmm", "_EdgeSoftmax", "_FusedAttention", "_FusedAttentionHeads",
                                           "_FusedGatAttention", "_FusedAttentionBf16"]
    assert len(fs) == 10 and fs[9].__name__ == "_FusedAttentionBias"


class _NoPlan(flex_amd.SparseOperator):
    """The operator's argument checks without its plans (making a plan needs a GPU)."""

    def __init__(self, nnz, k, **flags):
        self.m = self.n = 8
        self.k, self.nnz = k, nnz
        self.learn_values = True
        self.fused_attention, self.fused_backward = flags.get("fused_attention", False), flags.get("fused_backward", False)


def test_a_bias_needs_both_fused_paths_one_dtype_and_its_shape():
    torch = pytest.importorskip("torch")
    Q = torch.zeros((8, 32))
    b = torch.zeros((20, 4))
    for flags in (dict(), dict(fused_attention=True)):
        for H, bias in ((4, b), (1, b[:, 0])):
            with pytest.raises(NotImplementedError, match="fused_backward=True"):
                _NoPlan(20, 32, **flags).attention(Q, Q, Q, heads=H, bias=bias)
    op = _NoPlan(20, 32, fused_attention=True, fused_backward=True)
    for mixed in ((Q.bfloat16(), Q, Q), (Q, Q.bfloat16(), Q), (Q, Q, Q.double())):
        with pytest.raises(TypeError, match="one dtype"):
            op.attention(*mixed, heads=4, bias=b)
    for bad in (b.double(), b.bfloat16(), b[:, :2], b[:19], b.T, b[:, 0]):  # [nnz] stands for [nnz, 1] with one head only
        with pytest.raises(TypeError, match="bias of shape"):
            op.attention(Q, Q, Q, heads=4, bias=bad)

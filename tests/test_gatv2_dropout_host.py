"""Host checks of the attention dropout in the fused GATv2 attention (include/flex_spmm.h: flex_dropout_gatv2_attention and its
backward): the float64 reference (tests/gatv2_dropout_ref.py) against an independent float64 torch autograd evaluation, the fp32
evaluation against both checkers on every scenario and element, every planted fault against the checker it targets, the input
conditions of tests/test_gpu_gatv2_dropout.py, the public surface, and the census of the kernels in flex::gatv2_dropout with the GPU
case that runs each.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import attention_dropout_ref as ad
import flex_amd
import gatv2_attention_ref as v2
import gatv2_dropout_ref as vd
from attention_forms import FORM_OF_K, FORMS
from backward_ref import _directed
from conftest import ROOT
from flex_amd import binding
from fused_attention_backward_ref import both_sides
from fused_attention_ref import threshold_graph
from softmax_ref import long_rows_graph

SLOPE = v2.SLOPE
SEED = 0x0123456789ABCDEF  # a non-zero high word

# ---- the table of tests/test_gpu_gatv2_dropout.py: every (W, NS) form, idle lanes past k (48), d = 4 and d = 256, H = 1; the wide
# pairs (k >= 256) run on the graph that holds every class of row and of column
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
    """The three instantiations in flex::gatv2_dropout that the forward and the backward (every gradient wanted) of a case launch, as
    `nm -C` names them: written down from FORM_OF_K, not computed by the rule it checks."""
    W, NS = FORM_OF_K[c[1]]
    return [f"rows<{W}, {NS}>", f"rows_backward<{W}, {NS}>", f"columns_backward<{W}, {NS}>"]


# kernel -> the id of the first case of test_every_output_against_float64 (tests/test_gpu_gatv2_dropout.py) that launches it
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
    return np.random.default_rng([seed, k, 83]).uniform(-1, 1, (a.m, k)).astype(np.float32)


def case_operands(name, k, H):
    """(a, xt, xs, att, g): the inputs of a case, a scenario per head."""
    a = graph(name)
    shift = PAIRS.index((k, H)) + GPU_GRAPHS.index(name)
    xt, xs, att = v2.operands(v2.scenarios_of(H, shift=shift), a, k, seed=1)
    return a, xt, xs, att, grad(a, k, 1)


# ---- the reference

@pytest.mark.parametrize("name", ["thresholds", "directed_empty"])
@pytest.mark.parametrize("k,H", [(32, 4), (8, 1)])
def test_the_reference_agrees_with_an_independent_float64_torch_autograd_evaluation(name, k, H):
    """Xt and Xs are multiples of 1 / 64, att of 1 / 16 and the slope is 1 / 4, so that every score (d = 8 terms) is exact in fp32: the
    reference's softmax starts from the score rounded to fp32, torch's from the float64 one, and the two are then the same number.  The
    mask enters torch as a constant tensor."""
    pytest.importorskip("torch")
    a, slope, p = graph(name), 0.25, 0.6
    xt, xs, att = v2.operands(["uniform4", "att_signs", "spread80", "x_zero"][:H], a, k, seed=1)
    xt, xs = (np.nan_to_num(np.round(x * 64) / 64, nan=0.5).astype(np.float32) for x in (xt, xs))
    att = (np.round(att * 16) / 16).astype(np.float32)
    g = grad(a, k, 2)
    ref = vd.reference(a, xt, xs, att, slope, p, SEED)
    refb = vd.backward_reference(a, xt, xs, att, ref["p"], g, slope, p, SEED)  # on the float64 alpha: torch keeps its own in float64 too
    kp = ad.kept_entries(a, H, p, SEED)
    assert 0.3 < kp.mean() < 0.5
    want = vd.torch_float64(a, xt, xs, att, slope, g, kp, ad.factor(p))
    for what, x, y in zip(("Out", "P", "gXt", "gXs", "gAtt"), (ref["out"], ref["p"], refb["gxt"], refb["gxs"], refb["gatt"]), want):
        err = float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))
        assert err <= 1e-12, f"{name} k={k} H={H} {what}: {err:.3g}"


def _run_checkers(a, xt, xs, att, g, p, res, pin, ratios=None, what=""):
    wf = vd.check(a, xt, xs, att, SLOPE, p, SEED, res["out"], res["p"], what=what + " forward", ratios=ratios)
    wb = vd.check_backward(a, xt, xs, att, pin, g, SLOPE, p, SEED, res["gxt"], res["gxs"], res["gatt"], res["dz"], what=what + " backward", ratios=ratios)
    return wf, wb


@pytest.mark.parametrize("name", ["thresholds", "directed_empty"])
@pytest.mark.parametrize("k,H,p", [(48, 6, 0.5), (64, 1, 0.9), (16, 4, 0.1)])
def test_the_fp32_evaluation_stays_within_the_bound_on_every_scenario_and_element(name, k, H, p):
    a = graph(name)
    names = v2.scenarios_of(H, shift=k)
    xt, xs, att = v2.operands(names, a, k, seed=2)
    g = grad(a, k, 2)
    res = vd.fp32_result(a, xt, xs, att, SLOPE, p, SEED, g=g)
    each = {}
    wf, wb = _run_checkers(a, xt, xs, att, g, p, res, res["p"], each)
    print(f"{name} k={k} H={H} p={p} {'/'.join(names)}: worst err / bound forward {wf:.3g}, backward {wb:.3g} (" + " ".join(f"{key} {v:.3g}" for key, v in each.items()) + ")")
    assert wf <= 1.0 and wb <= 1.0, (wf, wb)
    r0, r1 = 7, 60  # a row-range slice of the forward
    e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
    part = vd.fp32_result(a, xt[r0:r1], xs, att, SLOPE, p, SEED, rows=(r0, r1))
    assert np.array_equal(part["out"], res["out"][r0:r1], equal_nan=True) and np.array_equal(part["p"], res["p"][e0:e1], equal_nan=True)
    assert vd.check(a, xt[r0:r1], xs, att, SLOPE, p, SEED, part["out"], part["p"], rows=(r0, r1)) <= 1.0


# ---- the planted faults

P_FAULT = 0.25  # c = 4 / 3 and 1 / p = 4 differ (at p = 0.5 they are the same number)


def _fault_case(fault):
    a, k, H = graph("thresholds_lifted"), 32, 4
    xt, xs, att = v2.operands(["uniform4", "spread80", "x_zero", "att_signs"], a, k, seed=4)
    if fault == "multiply_by_zero":  # In GATv2 the Xs row is score operand too: an inf there poisons the head.  A -inf under att > 0
        # gives s = -inf and alpha = +0 instead, and 0 x -inf reaches Out only if the dropped entry is multiplied.
        kp = ad.kept_entries(a, H, P_FAULT, SEED)
        _, col, _ = v2.coo(a)
        xs, att = xs.copy(), np.full_like(att, 0.5)
        only_dropped = np.setdiff1d(col[~kp[:, 0]], col[kp[:, 0]])  # columns all of whose entries head 0 drops
        assert len(only_dropped) >= 3
        xs[only_dropped[:3], 0] = -np.inf
    return a, k, H, xt, xs, att, grad(a, k, 4)


@pytest.mark.parametrize("fault", vd.FAULTS)
def test_the_checker_a_fault_targets_rejects_it(fault):
    a, k, H, xt, xs, att, g = _fault_case(fault)
    rows = (17, 300) if fault == "shard_local" else None
    xtr = xt if rows is None else xt[rows[0]:rows[1]]
    gg = None if rows or fault == "multiply_by_zero" else g
    right = vd.fp32_result(a, xtr, xs, att, SLOPE, P_FAULT, SEED, g=gg, rows=rows)
    assert vd.check(a, xtr, xs, att, SLOPE, P_FAULT, SEED, right["out"], right["p"], rows=rows) <= 1.0
    bad = vd.fp32_result(a, xtr, xs, att, SLOPE, P_FAULT, SEED, g=gg, probs=right["p"], rows=rows, fault=fault)
    if fault in vd.FORWARD_FAULTS:
        with pytest.raises(AssertionError):  # Out gives it away
            vd.check(a, xtr, xs, att, SLOPE, P_FAULT, SEED, bad["out"], rows=rows, what=fault)
        if fault in ("mask_before_norm", "gather_skipped"):
            with pytest.raises(AssertionError, match=r"\bP\b"):  # and so does P beside the right Out
                vd.check(a, xtr, xs, att, SLOPE, P_FAULT, SEED, right["out"], bad["p"], rows=rows, what=fault)
        return
    assert vd.check_backward(a, xt, xs, att, right["p"], g, SLOPE, P_FAULT, SEED, right["gxt"], right["gxs"], right["gatt"], right["dz"]) <= 1.0
    targets = {"gxs_score_masked": [("gxs", "gXs")], "gxt_masked_twice": [("gxt", "gXt")], "gatt_masked_twice": [("gatt", "gAtt")],
               "gxs_value_unmasked": [("gxs", "gXs")],
               "da_unmasked": [("dz", "dz"), ("gxt", "gXt"), ("gxs", "gXs"), ("gatt", "gAtt")]}[fault]  # da of a dropped entry is not +0, and all follows
    for key, arg in targets:
        with pytest.raises(AssertionError, match=key):
            vd.check_backward(a, xt, xs, att, right["p"], g, SLOPE, P_FAULT, SEED, what=fault, **{arg: bad[key]})
    others = {"gxt", "gxs", "gatt", "dz"} - {key for key, _ in targets}  # and nothing else moved
    assert all(np.array_equal(bad[key], right[key], equal_nan=True) for key in others), fault


# ---- the input conditions of the GPU tests

SELECTION_GRAPHS = ["directed_empty", "long_rows", "thresholds_lifted", "thresholds"]


def dead_row_heads(a, H, p):
    """per head, the non-empty rows whose entries are all dropped under SEED"""
    row, _, rp = v2.coo(a)
    kp = ad.kept_entries(a, H, p, SEED)
    dead = []
    for h in range(H):
        any_kept = np.zeros(a.m, bool)
        any_kept[row[kp[:, h]]] = True
        dead.append(np.flatnonzero(~any_kept & (np.diff(rp) > 0)))
    return dead


def test_the_graphs_have_heads_of_non_empty_rows_with_every_entry_dropped():
    """What the GPU file's test 4 (a) needs of its inputs, with the project's mask and that seed."""
    for p, lo, hi in ((0.5, 11, 657), (0.9, 48, 4434)):
        counts = [sum(len(r) for r in dead_row_heads(graph(name), H, p)) for name in SELECTION_GRAPHS for H in (1, 2, 4, 8)]
        assert lo <= min(counts) and max(counts) <= hi, (p, counts)


def masked_source_case(name, k=32, H=4):
    """(a, xt, xs, att) of the GPU file's test 4 (b): att = 0.5, and Xs[c, first column of head 1] = -inf on every 7th column c, so the
    score of head 1 of an entry from such a column is -inf and its alpha +0: a KEPT one adds 0 x -inf = NaN to Out, a dropped one
    nothing."""
    a = graph(name)
    rng = np.random.default_rng([k, H, 91])
    xt, xs = (rng.uniform(-2, 2, (r, k)).astype(np.float32) for r in (a.m, a.n))
    xs[::7, k // H] = -np.inf
    return a, xt, xs, np.full((H, k // H), 0.5, np.float32)


def masked_source_rows(a, xs, k, H, p):
    """(rows with a kept entry from a -inf column in head 1, rows with such entries and all of them dropped)"""
    row, col, _ = v2.coo(a)
    hit = np.isinf(xs[col, k // H])
    kp = ad.kept_entries(a, H, p, SEED)[:, 1]
    with_kept, with_any = np.zeros(a.m, bool), np.zeros(a.m, bool)
    with_kept[row[hit & kp]] = True
    with_any[row[hit]] = True
    return np.flatnonzero(with_kept), np.flatnonzero(with_any & ~with_kept)


@pytest.mark.parametrize("name,kept,dropped", [("directed_empty", 51, 48), ("thresholds_lifted", 419, 230), ("long_rows", 94, 57)])
def test_the_masked_source_case_has_rows_of_both_kinds_and_the_reference_is_nan_exactly_on_the_first(name, kept, dropped):
    """What the GPU file's test 4 (b) needs of its inputs."""
    k, H, p = 32, 4, 0.5
    a, xt, xs, att = masked_source_case(name, k, H)
    with_kept, only_dropped = masked_source_rows(a, xs, k, H, p)
    assert (len(with_kept), len(only_dropped)) == (kept, dropped)
    ref = vd.reference(a, xt, xs, att, SLOPE, p, SEED)
    nan_rows = np.flatnonzero(np.isnan(ref["out"]).any(1))
    assert np.array_equal(nan_rows, with_kept)
    assert np.array_equal(np.flatnonzero(np.isnan(ref["out"]).any(0)), [k // H])  # that column alone
    plain = v2.reference(a, xt, xs, att, SLOPE)
    assert np.isnan(plain["out"][np.concatenate([with_kept, only_dropped])]).any(1).all()  # the undropped reference is NaN on all of them
    res = vd.fp32_result(a, xt, xs, att, SLOPE, p, SEED)
    assert np.array_equal(np.isnan(res["out"]), np.isnan(ref["out"]))
    assert vd.check(a, xt, xs, att, SLOPE, p, SEED, res["out"], res["p"]) <= 1.0


def one_mask_case():
    """(a, lens, row, j) of the GPU file's test 3: col(e) = e, row r has r + 1 entries, r < 256; entry e is the j-th of its row."""
    lens = np.arange(1, 257)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    nnz = int(rp[-1])
    a = binding.HostCsr(rp, np.arange(nnz, dtype=np.uint32), np.ones(nnz, np.float32), n=nnz)
    row = np.repeat(np.arange(256), lens)
    return a, lens, row, np.arange(nnz) - rp[:-1].astype(np.int64)[row]


def test_the_one_mask_case_has_131584_bits_and_a_zero_score_term():
    a, lens, row, j = one_mask_case()
    assert a.nnz * 4 == 131584 and a.n == a.nnz and j.max() == 255 and np.array_equal(np.bincount(row), lens)
    k, H = 16, 4  # the same construction at a small k: att = 0 makes alpha uniform and the score term of gXs exactly 0
    d = k // H
    xs = np.zeros((a.n, k), np.float32)
    for h in range(H):
        xs[np.arange(a.n), h * d + np.arange(a.n) % d] = 1
    xt, att, g = np.zeros((a.m, k), np.float32), np.zeros((H, d), np.float32), np.ones((a.m, k), np.float32)
    ref = vd.reference(a, xt, xs, att, SLOPE, 0.5, SEED)
    assert np.allclose(ref["p"], (1.0 / lens)[row][:, None], rtol=1e-15)
    refb = vd.backward_reference(a, xt, xs, att, ref["p"], g, SLOPE, 0.5, SEED)
    kp = ad.kept_entries(a, H, 0.5, SEED)
    nz = (refb["gxs"] != 0).reshape(a.n, H, d)
    assert np.array_equal(nz.all(2), kp) and np.array_equal(nz.any(2), kp)  # gXs[e, head h] = p w g: non-zero exactly where kept


# ---- the public surface

NAMES_C = ("flex_dropout_gatv2_attention", "flex_dropout_gatv2_attention_backward")


def test_the_library_exports_the_two_calls_and_the_header_declares_them():
    hdr = open(os.path.join(ROOT, "include", "flex_spmm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+FLEX_ABI_VERSION\s+3\b", hdr)
    L = ctypes.CDLL(flex_amd.lib_path())
    for name in NAMES_C:
        assert re.search(r"^int\s+%s\s*\(" % name, code, re.M), f"{name} is not declared `int {name}(` in include/flex_spmm.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in binding.SYMBOLS
    assert len(binding._values_fn(NAMES_C[0]).argtypes) == 11 and len(binding._values_fn(NAMES_C[1]).argtypes) == 16
    assert L.flex_abi_version() == 3


def test_the_package_offers_the_methods_and_the_other_accessors_keep_their_entries():
    for f in ("gatv2_attention_dropout", "gatv2_attention_dropout_backward"):
        assert callable(getattr(flex_amd.Plan, f, None)), f
        assert callable(getattr(flex_amd.Plan, f + "_ptr", None)), f + "_ptr"
    pytest.importorskip("torch")
    from flex_amd import autograd
    assert len(autograd.functions()) == 10 and len(autograd.dropout_functions()) == 1 and len(autograd.gat_dropout_functions()) == 1
    assert [f.__name__ for f in autograd.gatv2_functions()] == ["_FusedGatv2Attention"]
    assert [f.__name__ for f in autograd.gatv2_dropout_functions()] == ["_FusedGatv2AttentionDropout"]


class _NoPlan(flex_amd.SparseOperator):
    """The operator's argument checks without its plans (making a plan needs a GPU)."""

    def __init__(self, nnz, k, **flags):
        self.m = self.n = 8
        self.k, self.nnz = k, nnz
        self.learn_values = True
        self.fused_attention, self.fused_backward = flags.get("fused_attention", False), flags.get("fused_backward", False)


def test_gatv2_dropout_needs_both_fused_paths_a_probability_and_float32():
    """The checks and their order are gat_attention's: the probability first, then the fused paths, then the dtypes."""
    torch = pytest.importorskip("torch")
    x, att = torch.zeros((8, 32)), torch.zeros((4, 8))
    for flags in (dict(), dict(fused_attention=True)):
        for kw in (dict(), dict(dropout=0.5), dict(dropout=0.5, training=False)):
            with pytest.raises(NotImplementedError, match="fused_backward=True"):
                _NoPlan(20, 32, **flags).gatv2_attention(x, x, att, **kw)
        with pytest.raises(ValueError, match="probability"):  # the probability comes first
            _NoPlan(20, 32, **flags).gatv2_attention(x, x, att, dropout=1.0)
    op = _NoPlan(20, 32, fused_attention=True, fused_backward=True)
    for bad in (1.0, -0.5, 2.0, float("nan")):
        for kw in (dict(), dict(training=False)):
            with pytest.raises(ValueError, match="probability"):
                op.gatv2_attention(x, x, att, dropout=bad, **kw)
    for kw in (dict(), dict(dropout=0.5)):
        with pytest.raises(TypeError, match="float32"):
            op.gatv2_attention(x.double(), x, att, **kw)


# ---- the census

def shipped_kernels(so, space):
    """The kernel handles (data symbols, not the launchers' code) of namespace flex::<space> in a built library, as `nm -C` names them
    without the namespace and the parameters."""
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-C", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        _, kind, sym = line.split(" ", 2)
        head = sym.split("(", 1)[0]
        if kind in "tTwW" or "__device_stub__" in sym or f"flex::{space}::" not in head:
            continue
        names.add(head.split(f"flex::{space}::", 1)[1])
    return names


def test_the_library_ships_exactly_the_twenty_one_kernels_and_a_gpu_case_runs_each():
    so = os.path.join(os.path.dirname(binding.__file__), "lib", "libflex_spmm.so")
    assert os.path.exists(so), f"{so} is not built"
    shipped = shipped_kernels(so, "gatv2_dropout")
    assert len(shipped) == 21, sorted(shipped)
    wanted = {f"{kern}<{W}, {NS}>" for W, NS in FORMS for kern in ("rows", "rows_backward", "columns_backward")}
    assert len(wanted) == 21 and shipped == wanted, (sorted(shipped - wanted), sorted(wanted - shipped))
    assert set(RUN_BY) == shipped, (f"kernels no GPU case launches: {sorted(shipped - set(RUN_BY))}", f"declared but not shipped: {sorted(set(RUN_BY) - shipped)}")
    ids = {case_id(c) for c in CASES}
    assert all(v in ids for v in RUN_BY.values())
    assert {FORM_OF_K[k] for k, _ in PAIRS} == set(FORMS)
    plain = shipped_kernels(so, "gatv2")  # the undropped namespace keeps its 22: 21 and gatt_reduce, which both families launch
    assert len(plain) == 22 and plain == wanted | {"gatt_reduce"}, sorted(plain)

"""Host checks of the fused GAT attention's reference and checkers (tests/gat_attention_ref.py) and of its public surface: the float64
reference against an independent float64 torch autograd evaluation of the same layer, a float64 result rounded to fp32 against both
checkers, the faults the checkers must reject, and the exported symbols and methods.  No GPU."""
import ctypes

import numpy as np
import pytest

import flex_amd
import gat_attention_ref as gat
from backward_ref import _directed

GRAPHS = {"thresholds": gat.threshold_graph, "directed_empty": lambda: _directed(250, 260, seed=7)}
_graphs = {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = GRAPHS[name]()
    return _graphs[name]


def _grad(a, k, seed):
    return np.random.default_rng([seed, k, 78]).uniform(-1, 1, (a.m, k)).astype(np.float32)


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("k,H", [(32, 4), (8, 1)])
def test_the_reference_agrees_with_an_independent_float64_torch_autograd_evaluation(name, k, H):
    """el and er are multiples of 1 / 64 and the slope is 1 / 4, so that every score is exact in fp32: the reference's softmax starts
    from the score rounded to fp32, torch's from the float64 one, and the two are then the same number."""
    torch = pytest.importorskip("torch")
    a, slope = graph(name), 0.25
    el, er, V = gat.operands(gat.scenarios_of(H, shift=5)[:H] if H > 1 else ["uniform4"], a, k, seed=1)
    el, er = (np.where(np.isfinite(x), np.round(x * 64) / 64, x).astype(np.float32) for x in (el, er))
    el, er = np.nan_to_num(el, nan=0.5, neginf=-1.0), np.nan_to_num(er, nan=0.5, neginf=-1.0)  # every score finite: torch has no mask rules
    g = _grad(a, k, 1)
    ref = gat.reference(a, el, er, V, slope)
    refb = gat.backward_reference(a, el, er, V, ref["p"], g, slope)
    row, col, _ = gat.coo(a)
    d = k // H
    row_t, col_t = torch.from_numpy(row), torch.from_numpy(col)
    el_t, er_t, V_t = (torch.from_numpy(x).double().requires_grad_() for x in (el, er, V))
    s = torch.nn.functional.leaky_relu(el_t[row_t] + er_t[col_t], slope)
    M = torch.full((a.m, H), -np.inf, dtype=torch.float64).scatter_reduce(0, row_t[:, None].expand(-1, H), s.detach(), "amax")
    t = torch.exp(s - M[row_t])
    p = t / torch.zeros((a.m, H), dtype=torch.float64).index_add_(0, row_t, t)[row_t]
    out = torch.zeros((a.m, H, d), dtype=torch.float64).index_add_(0, row_t, p[:, :, None] * V_t.view(a.n, H, d)[col_t]).reshape(a.m, k)
    out.backward(torch.from_numpy(g).double())
    for what, x, y in (("Out", ref["out"], out.detach().numpy()), ("gEl", refb["gel"], el_t.grad.numpy()), ("gEr", refb["ger"], er_t.grad.numpy()),
                       ("gV", refb["gv"], V_t.grad.numpy())):
        err = float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))
        assert err <= 1e-12, f"{name} k={k} H={H} {what}: {err:.3g}"


NAMES = {"finite": ["uniform4", "zero", "spread80", "uniform4"], "mixed": ["poisoned", "masked30", "rows_masked", "zero"]}


def _run_checkers(a, el, er, V, g, res, pin):
    wf = gat.check(a, el, er, V, gat.SLOPE, res["out"], res["p"], what="forward")
    wb = gat.check_backward(a, el, er, V, pin, g, gat.SLOPE, res["gel"], res["ger"], res["gv"], res["dx"], what="backward")
    return wf, wb


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("names", sorted(NAMES))
def test_a_float64_result_rounded_to_fp32_passes_both_checkers(name, names):
    a, k = graph(name), 32
    el, er, V = gat.operands(NAMES[names], a, k, seed=2)
    g = _grad(a, k, 2)
    res = gat.fp32_result(a, el, er, V, gat.SLOPE, g=g)
    wf, wb = _run_checkers(a, el, er, V, g, res, res["p"])
    assert wf < 1.0 and wb < 1.0, (wf, wb)
    # a row-range slice of the forward
    r0, r1 = 7, 60
    e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
    assert gat.check(a, el[r0:r1], er, V, gat.SLOPE, res["out"][r0:r1], res["p"][e0:e1], rows=(r0, r1)) < 1.0


@pytest.mark.parametrize("fault", gat.FAULTS)
def test_the_checkers_reject_each_fault(fault):
    a, k = graph("thresholds"), 32
    names = NAMES["mixed" if fault == "poison_spreads" else "finite"]
    el, er, V = gat.operands(names, a, k, seed=3)
    g = _grad(a, k, 3)
    right = gat.fp32_result(a, el, er, V, gat.SLOPE, g=g)
    res = gat.fp32_result(a, el, er, V, gat.SLOPE, g=g, p=right["p"], fault=fault)
    with pytest.raises(AssertionError):
        _run_checkers(a, el, er, V, g, res, right["p"])


def test_the_library_and_the_package_offer_the_calls():
    L = ctypes.CDLL(flex_amd.lib_path())
    for s in ("flex_gat_attention", "flex_gat_attention_backward"):
        assert hasattr(L, s), s
    for f in ("gat_attention_ptr", "gat_attention", "gat_attention_backward_ptr", "gat_attention_backward"):
        assert callable(getattr(flex_amd.Plan, f, None)), f
    assert callable(getattr(flex_amd.SparseOperator, "gat_attention", None))

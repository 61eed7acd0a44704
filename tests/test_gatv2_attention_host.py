"""Host checks of the fused GATv2 attention's reference, bounds and checkers (tests/gatv2_attention_ref.py) and of its public surface:
the float64 reference against an independent float64 torch autograd evaluation of the same layer, the fp32 evaluation against both
checkers on every scenario and element (the bound is not too tight), the faults the checkers must reject, and the exported symbols
and methods.  No GPU."""
import ctypes

import numpy as np
import pytest

import flex_amd
import gatv2_attention_ref as v2
from backward_ref import _directed

GRAPHS = {"thresholds": v2.threshold_graph, "directed_empty": lambda: _directed(250, 260, seed=7)}
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
    """Xt and Xs are multiples of 1 / 64, att of 1 / 16 and the slope is 1 / 4, so that every score (d = 8 terms) is exact in fp32: the
    reference's softmax starts from the score rounded to fp32, torch's from the float64 one, and the two are then the same number."""
    torch = pytest.importorskip("torch")
    a, slope, d = graph(name), 0.25, k // H
    xt, xs, att = v2.operands(["uniform4", "att_signs", "spread80", "x_zero"][:H], a, k, seed=1)
    xt, xs = (np.nan_to_num(np.round(x * 64) / 64, nan=0.5).astype(np.float32) for x in (xt, xs))
    att = (np.round(att * 16) / 16).astype(np.float32)
    g = _grad(a, k, 1)
    ref = v2.reference(a, xt, xs, att, slope)
    refb = v2.backward_reference(a, xt, xs, att, ref["p"], g, slope)
    row, col, _ = v2.coo(a)
    row_t, col_t = torch.from_numpy(row.astype(np.int64)), torch.from_numpy(col.astype(np.int64))
    xt_t, xs_t, att_t = (torch.from_numpy(x).double().requires_grad_() for x in (xt, xs, att))
    x = (xt_t[row_t] + xs_t[col_t]).view(-1, H, d)
    s = (torch.nn.functional.leaky_relu(x, slope) * att_t).sum(-1)
    p = torch.cat([torch.softmax(s[int(a.rowPtr[r]):int(a.rowPtr[r + 1])], 0) for r in range(a.m)], 0)  # a plain softmax per row
    out = torch.zeros((a.m, H, d), dtype=torch.float64).index_add_(0, row_t, p[:, :, None] * xs_t.view(a.n, H, d)[col_t]).reshape(a.m, k)
    out.backward(torch.from_numpy(g).double())
    for what, mine, theirs in (("Out", ref["out"], out.detach().numpy()), ("P", ref["p"], p.detach().numpy()), ("gXt", refb["gxt"], xt_t.grad.numpy()),
                               ("gXs", refb["gxs"], xs_t.grad.numpy()), ("gAtt", refb["gatt"], att_t.grad.numpy())):
        err = float(np.abs(mine - theirs).max() / max(np.abs(theirs).max(), 1e-300))
        assert err <= 1e-12, f"{name} k={k} H={H} {what}: {err:.3g}"


NAMES = {"all": list(v2.SCENARIOS), "finite": ["uniform4", "x_zero", "spread80", "att_signs"]}


def _run_checkers(a, xt, xs, att, g, res, pin, ratios=None):
    wf = v2.check(a, xt, xs, att, v2.SLOPE, res["out"], res["p"], what="forward")
    wb = v2.check_backward(a, xt, xs, att, pin, g, v2.SLOPE, res["gxt"], res["gxs"], res["gatt"], res["dz"], what="backward", ratios=ratios)
    return wf, wb


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("k,H", [(48, 6), (64, 1), (16, 4)])
def test_the_fp32_evaluation_stays_within_the_bound_on_every_scenario_and_element(name, k, H):
    a = graph(name)
    names = v2.scenarios_of(H, shift=k)
    xt, xs, att = v2.operands(names, a, k, seed=2)
    g = _grad(a, k, 2)
    res = v2.fp32_result(a, xt, xs, att, v2.SLOPE, g=g)
    each = {}
    wf, wb = _run_checkers(a, xt, xs, att, g, res, res["p"], each)
    print(f"{name} k={k} H={H} {'/'.join(names)}: worst err / bound forward {wf:.3g}, backward {wb:.3g} (" + " ".join(f"{key} {v:.3g}" for key, v in each.items()) + ")")
    assert wf <= 1.0 and wb <= 1.0, (wf, wb)
    # a row-range slice of the forward
    r0, r1 = 7, 60
    e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
    assert v2.check(a, xt[r0:r1], xs, att, v2.SLOPE, res["out"][r0:r1], res["p"][e0:e1], rows=(r0, r1)) <= 1.0


def test_every_scenario_is_what_its_name_says():
    a, k, H = graph("thresholds"), 48, 6
    xt, xs, att = v2.operands(v2.SCENARIOS, a, k, seed=2)
    ref = v2.reference(a, xt, xs, att, v2.SLOPE)
    row, col, _ = v2.coo(a)
    by = {name: h for h, name in enumerate(v2.SCENARIOS)}
    c = v2.head_columns(k, H, by["x_zero"])
    x = xt[row][:, c] + xs[col][:, c]
    assert (x == 0).all(1).any() and not (x == 0).all(), "x_zero: x = 0 in every column of some entries, not of all"
    c = v2.head_columns(k, H, by["zero"])
    assert not xt[:, c].any() and not xs[:, c].any() and att[by["zero"]].any() and not ref["out"][:, c].any()
    assert np.isnan(ref["p"][:, by["poisoned"]]).any() and not np.isnan(np.delete(ref["p"], by["poisoned"], axis=1)).any()
    assert (att[by["att_signs"]] == 0).any() and (att[by["att_signs"]] > 0).any() and (att[by["att_signs"]] < 0).any()
    s = ref["s"]
    assert np.ptp(s[:, by["spread80"]]) > 40 > np.ptp(s[:, by["uniform4"]])


@pytest.mark.parametrize("fault", v2.FAULTS)
def test_the_checkers_reject_each_fault(fault):
    a, k = graph("thresholds"), 32
    names = ["uniform4", "poisoned", "x_zero", "att_signs"] if fault == "poison_spreads" else NAMES["finite"]
    xt, xs, att = v2.operands(names, a, k, seed=3)
    g = _grad(a, k, 3)
    right = v2.fp32_result(a, xt, xs, att, v2.SLOPE, g=g)
    _run_checkers(a, xt, xs, att, g, right, right["p"])
    res = v2.fp32_result(a, xt, xs, att, v2.SLOPE, g=g, p=right["p"], fault=fault)
    with pytest.raises(AssertionError):
        _run_checkers(a, xt, xs, att, g, res, right["p"])


def test_the_library_and_the_package_offer_the_calls():
    L = ctypes.CDLL(flex_amd.lib_path())
    for s in ("flex_gatv2_attention", "flex_gatv2_attention_backward", "flex_gatv2_attention_work_size"):
        assert hasattr(L, s), s
    for f in ("gatv2_attention_ptr", "gatv2_attention", "gatv2_attention_backward_ptr", "gatv2_attention_backward", "gatv2_attention_work_size"):
        assert callable(getattr(flex_amd.Plan, f, None)), f
    assert callable(getattr(flex_amd.SparseOperator, "gatv2_attention", None))

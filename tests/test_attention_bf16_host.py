"""The bf16 attention reference on the host (tests/attention_bf16_ref.py): to_bf16 is torch's rounding bit for bit; the library exports
the two bf16 calls and the header declares them; the checkers reject the faults a bf16 kernel can have that an fp32 one cannot -- Out
truncated, Out rounded twice, P rounded, a poisoned head's NaN spread over the row, a gradient rounded before its last merge -- and the
reference itself, float64 rounded ONCE to bf16, stays inside the bound on every case of the GPU table.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import attention_bf16_ref as bf
from attention_forms import BF16_PAIRS as PAIRS
import flex_amd
import multihead_attention_ref as mh
from backward_ref import _directed
from conftest import ROOT
from fused_attention_backward_ref import both_sides
from fused_attention_ref import coo, threshold_graph
from softmax_ref import long_rows_graph

torch = pytest.importorskip("torch")

K, HEADS, SCALE = 32, 4, 0.25

# the table of tests/test_gpu_attention_bf16.py: the (k, H) pairs are tests/attention_forms.py's (every (W, NS) form, idle lanes past k,
# d = 4 and d = 256, H = 1)
GRAPHS = {
    "thresholds": threshold_graph,
    "thresholds_lifted": lambda: both_sides(threshold_graph()),
    "directed_empty": lambda: _directed(250, 260, seed=7),
    "long_rows": long_rows_graph,
}
CASES = [(name, k, H) for k, H in PAIRS for name in (sorted(GRAPHS) if k < 256 else ["thresholds", "thresholds_lifted"])]
_graphs = {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = GRAPHS[name]()
    return _graphs[name]


def case_operands(name, k, H):
    """(a, scenario names, Q, K, V, g): the inputs of a case of the table, bf16 numbers held as fp32."""
    a = graph(name)
    names = mh.scenarios_of(H, shift=PAIRS.index((k, H)) + sorted(GRAPHS).index(name))
    Q, Kk, V = bf.operands(names, a, k, seed=1)
    g = bf.rounded(np.random.default_rng([1, k, 78]).uniform(-1, 1, (a.m, k)).astype(np.float32))
    return a, names, Q, Kk, V, g


@pytest.fixture(scope="module")
def a():
    return threshold_graph()


# ---- the conversion

def _patterns():
    rng = np.random.default_rng(3)
    u = rng.integers(0, 2 ** 32, 2 ** 16, dtype=np.uint64).astype(np.uint32)
    hi = rng.integers(0, 2 ** 16, 4096, dtype=np.uint64).astype(np.uint32) << 16
    ties = np.concatenate([hi | 0x8000, hi | 0x7FFF, hi | 0x8001])               # exactly half way, one below, one above
    sub = np.concatenate([np.arange(0, 0x00800000, 0x3FFF, dtype=np.uint32), np.uint32(0x80000000) | np.arange(0, 0x00800000, 0x3FFF, dtype=np.uint32)])
    special = np.array([0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x00000001, 0x00008000, 0x00018000],
                       np.uint32)
    return np.concatenate([u, ties, sub, special]).view(np.float32)


def test_to_bf16_is_the_rounding_of_torch_bit_for_bit_and_keeps_nan():
    x = _patterns()
    nan = np.isnan(x)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = bf.to_bf16(x)
    assert got.dtype == np.uint16 and np.array_equal(got[~nan], want[~nan])
    assert nan.sum() > 100 and np.all(np.isnan(bf.from_bf16(got[nan])))
    assert bf.to_bf16(np.float32(3.4028235e38)) == 0x7F80 and bf.to_bf16(np.float32(-3.4028235e38)) == 0xFF80  # the largest float rounds to inf
    assert np.array_equal(bf.to_bf16(bf.from_bf16(got[~nan])), got[~nan])                                          # exact on bf16 numbers
    assert np.array_equal(bf.from_bf16(want).view(np.uint32), want.astype(np.uint32) << 16)
    # rounded once from float64: where the float64 lies between an fp32 tie and the fp32 above it, the way through fp32 rounds twice
    x64 = np.array([1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 2.0 ** -8 - 2.0 ** -30, -(1.0 + 3 * 2.0 ** -8) + 2.0 ** -30, 2.0 ** -140, np.inf, 3.0])
    assert bf.f64_to_bf16(x64).tolist() == [0x3F81, 0x3F80, 0xBF81, 0x0000, 0x7F80, 0x4040]
    assert bf.to_bf16(x64[:1].astype(np.float32)).tolist() == [0x3F80]


# ---- the ABI

def test_the_library_exports_the_two_bf16_calls_and_the_header_declares_them():
    hdr = open(os.path.join(ROOT, "include", "flex_spmm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"typedef\s+uint16_t\s+flex_bf16\s*;", code)
    L = ctypes.CDLL(flex_amd.lib_path())
    for name in ("flex_attention_bf16", "flex_attention_bf16_backward"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/flex_spmm.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in flex_amd.binding.SYMBOLS


# ---- a right result passes, planted faults do not

def _right(a, names, seed):
    """What a right kernel returns up to roundings: float64, Out and the gradients rounded once to bf16, P and ds to fp32."""
    Q, Kk, V = bf.operands(names, a, K, seed=seed)
    g = bf.rounded(np.random.default_rng(seed).uniform(-1, 1, (a.m, K)).astype(np.float32))
    ref = mh.reference(a, Q, Kk, V, SCALE, HEADS)
    with np.errstate(invalid="ignore", over="ignore"):
        p = ref["p"].astype(np.float32)
    refb = mh.backward_reference(a, Q, Kk, V, p, g, SCALE, HEADS)
    return Q, Kk, V, g, ref, p, refb


def test_a_right_result_passes_and_out_truncated_or_rounded_twice_does_not(a):
    names = ["uniform4", "spread80", "masked30", "rows_masked"]
    Q, Kk, V, g, ref, p, refb = _right(a, names, 1)
    assert bf.check(a, Q, Kk, V, SCALE, HEADS, bf.f64_to_bf16(ref["out"]), p, what="right") <= 1.0
    out32 = ref["out"].astype(np.float32)
    assert bf.check(a, Q, Kk, V, SCALE, HEADS, bf.to_bf16(out32), p, what="through fp32") <= 1.0
    truncated = (out32.view(np.uint32) >> 16).astype(np.uint16)
    with pytest.raises(AssertionError, match="beyond the bf16 bound"):
        bf.check(a, Q, Kk, V, SCALE, HEADS, truncated, what="truncated")
    u = out32.view(np.uint32).astype(np.uint64)
    eleven = (((u + 0xFFF + ((u >> 13) & 1)) >> 13) << 13).astype(np.uint32).view(np.float32)  # an fp16-like step: 11 significant bits
    with pytest.raises(AssertionError, match="beyond the bf16 bound"):
        bf.check(a, Q, Kk, V, SCALE, HEADS, bf.to_bf16(eleven), what="rounded twice")
    with pytest.raises(AssertionError):  # fp32 Out handed over in place of bf16 bits
        bf.check(a, Q, Kk, V, SCALE, HEADS, out32, what="fp32")


def test_the_checker_rejects_p_rounded_to_bf16(a):
    Q, Kk, V, g, ref, p, refb = _right(a, ["uniform4", "spread80", "uniform4", "masked30"], 2)
    out = bf.f64_to_bf16(ref["out"])
    bf.check(a, Q, Kk, V, SCALE, HEADS, out, p)
    with pytest.raises(AssertionError, match="entries of P beyond the fp32 bound"):
        bf.check(a, Q, Kk, V, SCALE, HEADS, out, bf.rounded(p), what="P in bf16")


def test_the_checker_rejects_a_poisoned_head_that_spreads_over_the_row(a):
    Q, Kk, V, g, ref, p, refb = _right(a, ["uniform4", "poisoned", "uniform4", "masked30"], 4)
    out = bf.f64_to_bf16(ref["out"])
    c1 = mh.head_columns(K, HEADS, 1)
    bad = np.isnan(bf.from_bf16(out)[:, c1]).all(1)
    assert bad.sum() == 3 and not np.isnan(np.delete(bf.from_bf16(out), np.r_[c1], axis=1)).any()  # three poisoned rows, in head 1 only
    bf.check(a, Q, Kk, V, SCALE, HEADS, out, p)
    spread = out.copy()
    spread[bad] = 0x7FC0
    with pytest.raises(AssertionError, match="head [023]"):
        bf.check(a, Q, Kk, V, SCALE, HEADS, spread, p)


def test_the_backward_checker_rejects_a_gradient_rounded_before_its_last_merge(a):
    Q, Kk, V, g, ref, p, refb = _right(a, ["uniform4", "spread80", "uniform4", "spread80"], 5)
    good = tuple(bf.f64_to_bf16(refb[key]) for key in ("gq", "gk", "gv"))
    ds = refb["ds"].astype(np.float32)
    assert bf.check_backward(a, Q, Kk, V, p, g, SCALE, HEADS, *good, ds, what="right") <= 1.0
    row, col, _ = coo(a)
    Q64, K64, g64 = (np.asarray(x, np.float64) for x in (Q, Kk, g))
    early = {}
    for key, w, x, seg, n in (("gq", refb["ds"], K64[col], row, a.m), ("gk", refb["ds"], Q64[row], col, a.n), ("gv", p.astype(np.float64), g64[row], col, a.n)):
        terms = np.concatenate([bf.from_bf16(bf.f64_to_bf16(w[:, h, None] * x[:, mh.head_columns(K, HEADS, h)])).astype(np.float64) for h in range(HEADS)], axis=1)
        tot = np.zeros((n, K))
        np.add.at(tot, seg, terms)  # every entry's term is already a bf16 number: what a partial sum rounded before the merge loses
        early[key] = bf.f64_to_bf16(tot)
    for i, key in enumerate(("gq", "gk", "gv")):
        with pytest.raises(AssertionError, match=f"elements of {key} beyond the bf16 bound"):
            bf.check_backward(a, Q, Kk, V, p, g, SCALE, HEADS, **{("gQ", "gK", "gV")[i]: early[key]}, what="rounded early")
    with pytest.raises(AssertionError):  # ds rounded to bf16
        bf.check_backward(a, Q, Kk, V, p, g, SCALE, HEADS, ds=bf.rounded(ds), what="ds in bf16")


# ---- the bound is one the reference itself keeps

@pytest.mark.parametrize("name,k,H", CASES)
def test_float64_rounded_once_to_bf16_stays_inside_the_bound_on_every_case_of_the_gpu_table(name, k, H):
    a, names, Q, Kk, V, g = case_operands(name, k, H)
    ref = mh.reference(a, Q, Kk, V, SCALE, H)
    with np.errstate(invalid="ignore", over="ignore"):
        p = ref["p"].astype(np.float32)
    each = {}
    wf = bf.check(a, Q, Kk, V, SCALE, H, bf.f64_to_bf16(ref["out"]), p, what=f"{name} k={k} H={H}", ratios=each)
    refb = mh.backward_reference(a, Q, Kk, V, p, g, SCALE, H)
    with np.errstate(invalid="ignore", over="ignore"):
        ds = refb["ds"].astype(np.float32)
    wb = bf.check_backward(a, Q, Kk, V, p, g, SCALE, H, *(bf.f64_to_bf16(refb[key]) for key in ("gq", "gk", "gv")), ds, what=f"{name} k={k} H={H}", ratios=each)
    print(f"{name} k={k} H={H}: float64 rounded once, worst err / bound " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))
    assert max(wf, wb) <= 1.0

"""The multi-head attention reference on the host (tests/multihead_attention_ref.py): the stacked per-head checker accepts a float64
evaluation rounded to fp32 and rejects the faults a multi-head kernel can have that a single-head one cannot -- one softmax over all
heads jointly, P delivered head-major, one head's poisoned row turning the whole Out row NaN, a head normalised by its neighbour's
sum -- and with heads = 1 it is the existing single-head reference exactly.  No GPU."""
import numpy as np
import pytest

import fused_attention_backward_ref as backward
import fused_attention_ref as forward
import multihead_attention_ref as mh
from backward_ref import _directed
from fused_attention_ref import threshold_graph

K, HEADS, SCALE = 32, 4, 0.25


@pytest.fixture(scope="module")
def a():
    return threshold_graph()


def test_a_right_result_passes_with_different_scenarios_in_the_heads(a):
    for shift in (0, 2):
        names = mh.scenarios_of(HEADS, shift)
        Q, Kk, V = mh.operands(names, a, K, seed=1)
        out, p = mh.fp32_result(a, Q, Kk, V, SCALE, HEADS)
        assert p.shape == (a.nnz, HEADS)
        assert mh.check(a, Q, Kk, V, SCALE, HEADS, out, p, what=str(names)) < 1.0
    Q, Kk, V = mh.operands(["uniform4", "spread80", "uniform4", "spread80"], a, K, seed=2)
    out, p = mh.fp32_result(a, Q, Kk, V, SCALE, HEADS, joint_softmax=False, next_heads_sum=False)
    mh.check(a, Q, Kk, V, SCALE, HEADS, out, p)


@pytest.mark.parametrize("fault", ["joint_softmax", "head_major", "next_heads_sum"])
def test_the_checker_rejects_what_mixes_the_heads(a, fault):
    Q, Kk, V = mh.operands(["uniform4", "spread80", "uniform4", "spread80"], a, K, seed=3)
    out, p = mh.fp32_result(a, Q, Kk, V, SCALE, HEADS, **{fault: True})
    if fault == "head_major":  # Out is right, only P's layout is wrong
        mh.check(a, Q, Kk, V, SCALE, HEADS, out)
    with pytest.raises(AssertionError):
        mh.check(a, Q, Kk, V, SCALE, HEADS, out, p, what=fault)
    if fault != "head_major":  # and Out alone gives the fault away
        with pytest.raises(AssertionError):
            mh.check(a, Q, Kk, V, SCALE, HEADS, out, what=fault)


def test_the_checker_rejects_a_poisoned_head_that_spreads_over_the_row(a):
    names = ["uniform4", "poisoned", "uniform4", "masked30"]
    Q, Kk, V = mh.operands(names, a, K, seed=4)
    out, p = mh.fp32_result(a, Q, Kk, V, SCALE, HEADS)
    c1 = mh.head_columns(K, HEADS, 1)
    bad = np.isnan(out[:, c1]).all(1)
    assert bad.sum() == 3 and not np.isnan(np.delete(out, np.r_[c1], axis=1)).any()  # three poisoned rows, in head 1 only
    mh.check(a, Q, Kk, V, SCALE, HEADS, out, p)
    spread, _ = mh.fp32_result(a, Q, Kk, V, SCALE, HEADS, poison_spreads=True)
    assert np.isnan(spread[bad]).all()
    with pytest.raises(AssertionError, match="head [023]"):
        mh.check(a, Q, Kk, V, SCALE, HEADS, spread, p)


def test_one_head_is_the_existing_reference_exactly():
    g = _directed(250, 260, seed=7)
    k = 24
    Q, Kk, V = forward.operands("masked30", g, k, seed=5)
    one, ref = mh.reference(g, Q, Kk, V, SCALE, 1), forward.reference(g, Q, Kk, V, SCALE)
    for key in ("out", "out_bound"):
        assert np.array_equal(one[key], ref[key], equal_nan=True)
    for key in ("p", "p_bound", "s"):
        assert one[key].shape == (g.nnz, 1) and np.array_equal(one[key][:, 0], ref[key], equal_nan=True)
    p = ref["p"].astype(np.float32)
    grad = np.random.default_rng(6).uniform(-1, 1, (g.m, k)).astype(np.float32)
    oneb, refb = mh.backward_reference(g, Q, Kk, V, p[:, None], grad, SCALE, 1), backward.reference(g, Q, Kk, V, p, grad, SCALE)
    for key in ("gq", "gk", "gv", "gq_bound", "gk_bound", "gv_bound"):
        assert np.array_equal(oneb[key], refb[key], equal_nan=True)
    for key in ("ds", "ds_bound"):
        assert np.array_equal(oneb[key][:, 0], refb[key], equal_nan=True)


def test_the_backward_checker_takes_entry_major_edge_arrays_and_rejects_a_swap_of_two_heads(a):
    Q, Kk, V = mh.operands(["uniform4", "spread80", "uniform4", "spread80"], a, K, seed=7)
    grad = np.random.default_rng(8).uniform(-1, 1, (a.m, K)).astype(np.float32)
    p = mh.reference(a, Q, Kk, V, SCALE, HEADS)["p"].astype(np.float32)
    ref = mh.backward_reference(a, Q, Kk, V, p, grad, SCALE, HEADS)
    good = tuple(ref[key].astype(np.float32) for key in ("gq", "gk", "gv", "ds"))
    assert mh.check_backward(a, Q, Kk, V, p, grad, SCALE, HEADS, *good) <= 1.0
    with pytest.raises(AssertionError):  # ds of heads 0 and 1 exchanged
        mh.check_backward(a, Q, Kk, V, p, grad, SCALE, HEADS, ds=good[3][:, [1, 0, 2, 3]])
    with pytest.raises(AssertionError):  # gK computed with another head's ds
        d = K // HEADS
        mh.check_backward(a, Q, Kk, V, p, grad, SCALE, HEADS, gK=np.roll(good[1], d, axis=1))
    with pytest.raises(AssertionError):
        mh.check_backward(a, Q, Kk, V, p, grad, SCALE, HEADS, ds=np.ascontiguousarray(good[3].T).reshape(good[3].shape))

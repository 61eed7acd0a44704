"""Harness tests: the backward checkers of tests/backward_ref.py on the CPU.  Every case the GPU suite runs stays in the checked
range, a float32 emulation of the stated association order passes, and the mutant that multiplies by A instead of A^T fails.  They
check the checker, not the library, so they pass with or without the backward pass (tests/test_gpu_backward.py tests that)."""
import numpy as np
import pytest

from backward_ref import backward_case, check_dw, check_dx, dw_chain, dw_range_guard, transpose
from f64ref import AX_W, AXW_SCENARIOS, axw_range_guard, spmm64


def _emulate(a, X, W, D):
    """float32 G = A^T D (float64 sums rounded once), then G W^T and X^T G in float32 matmuls: well inside both bounds."""
    G = spmm64(transpose(a), D).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return G @ W.T, X.T @ G


@pytest.mark.parametrize("name", AXW_SCENARIOS)
def test_every_scenario_stays_in_the_checked_range(name):
    for shape in ((600, 128, 100), (300, 64, 32)):
        a, X, W, D = backward_case(name, *shape)
        at = transpose(a)
        assert dw_range_guard(at, X, D) is None
        assert axw_range_guard(at, D, np.ascontiguousarray(W.T), AX_W) is None


@pytest.mark.parametrize("n,dim,c", [(n, dim, c) for n in (32, 33, 517) for dim in (4, 32, 100, 128, 256) for c in (1, 100, 128, 256)])
def test_every_edge_shape_stays_in_the_checked_range(n, dim, c):
    a, X, W, D = backward_case("uniform", n, dim, c)
    assert dw_range_guard(transpose(a), X, D) is None


@pytest.mark.parametrize("name", ["uniform", "wide", "cancel"])
def test_an_emulation_passes_and_the_a_for_a_transpose_mutant_fails(name):
    a, X, W, D = backward_case(name, 517, 32, 100)
    gx, gw = _emulate(a, X, W, D)
    at = transpose(a)
    assert check_dx(at, D, W, gx) is None
    assert check_dw(at, X, D, gw, dw_chain(a.n, 256)) is None
    mx, mw = _emulate(transpose(a), X, W, D)  # uses A where A^T belongs
    assert check_dx(at, D, W, mx) is not None
    assert check_dw(at, X, D, mw, dw_chain(a.n, 256)) is not None


def test_a_dropped_slice_fails_the_dw_bound():
    a, X, W, D = backward_case("uniform", 4096, 32, 32)
    at = transpose(a)
    _, gw = _emulate(a, X, W, D)
    G = spmm64(at, D).astype(np.float32)
    short = X[256:].T @ G[256:]  # the first 256-row slice missing
    assert check_dw(at, X, D, gw, dw_chain(a.n, 256)) is None
    assert check_dw(at, X, D, short, dw_chain(a.n, 256)) is not None


def test_the_chain_length():
    assert dw_chain(232965, 256) == -(-232965 // 256) + 256
    assert dw_chain(33, 256) == 34

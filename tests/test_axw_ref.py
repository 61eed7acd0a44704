"""Checks the checkers of the A*X*W tests on the CPU: oracle_axw_gemm_chain (the MFMA GEMM's fmaf chain) against exact rational
arithmetic, its k order, and the composed float64 bound of tests/f64ref.py -- fp32 emulations of both association orders pass every
scenario, and mutants (a dropped k term, a flushed subnormal, a shifted column, NaN in a padding column, a changed class) fail it."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import oracle
from f64ref import (AX_W, AXW_SCENARIOS, A_XW, axw_range_guard, axw_scenario, check_axw, check_gemm_bound)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_MAX_EXP = 128


# ---- exact fp32 fma -----------------------------------------------------------------------------------------------------------

def round_f32(q: Fraction) -> float:
    """q rounded to fp32, round-half-even, subnormals and overflow included (q != 0)."""
    s = -1.0 if q < 0 else 1.0
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()  # 2^e <= q < 2^(e+2)
    if Fraction(2) ** e > q:
        e -= 1
    if Fraction(2) ** (e + 1) <= q:
        e += 1
    e = max(e, -126)  # below 2^-126 the quantum stays 2^-149
    quantum = Fraction(2) ** (e - 23)
    m = q / quantum
    f = m.numerator // m.denominator
    rem = m - f
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and f % 2 == 1):
        f += 1
    v = Fraction(f) * quantum
    if v >= Fraction(2) ** F32_MAX_EXP:
        return s * float("inf")
    return s * float(v)


def exact_fma(a, b, c) -> np.float32:
    a, b, c = (np.float32(x) for x in (a, b, c))
    q = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if q == 0:  # exact zero: -0 only when the product and c are both -0 (round-to-nearest)
        prod_neg = (np.signbit(a) != np.signbit(b))
        return np.float32(-0.0) if (float(a) * float(b) == 0 and prod_neg and np.signbit(c) and c == 0) else np.float32(0.0)
    return np.float32(round_f32(q))


def _fma_cases(rng):
    """(a, b, c) fp32 triples: double-rounding traps, subnormal results, cancellation, random scales."""
    a, b, c = [], [], []
    for _ in range(600):  # c + ab just below c's half ulp, with c's last bit odd: fl32(fl64(c + ab)) rounds to even, fma does not
        t = int(rng.integers(15, 24))
        e = int(rng.integers(-100, 100))
        sig = (int(rng.integers(0, 1 << 22)) << 1) | 1 | (1 << 23)  # odd 24-bit significand
        cc = sig * 2.0 ** (e - 23)
        sgn = float(rng.choice([-1.0, 1.0]))
        a.append(1 - 2.0 ** -t)
        b.append(sgn * 2.0 ** (e - 24) * (1 + 2.0 ** -t))
        c.append(sgn * cc)
    for _ in range(600):  # subnormal results
        a.append(float(rng.uniform(-1, 1)) * 2.0 ** int(rng.integers(-80, -60)))
        b.append(float(rng.uniform(-1, 1)) * 2.0 ** int(rng.integers(-80, -60)))
        c.append(float(rng.integers(-(1 << 23), 1 << 23)) * 2.0 ** -149)
    for _ in range(600):  # near-cancellation: c = -fl(ab) and its neighbours
        x, y = np.float32(rng.uniform(-2, 2)), np.float32(rng.uniform(-2, 2))
        p = np.float32(x * y)
        a.append(float(x)), b.append(float(y)), c.append(float(-np.nextafter(p, np.float32(rng.choice([-3, 3])))))
    for _ in range(2000):  # random scales, zeros of both signs
        ex = rng.integers(-140, 120, size=3)
        v = rng.uniform(-1, 1, size=3) * np.exp2(ex.astype(np.float64))
        v[rng.random(3) < 0.05] = rng.choice([0.0, -0.0])
        a.append(v[0]), b.append(v[1]), c.append(v[2])
    f = lambda x: np.array(x, np.float32)  # noqa: E731
    c = f(c)
    c[c == 0] = 0.0  # the chain starts from +0, so the c it passes on is never -0 (fma(c, 1, +0) = +0 for c = -0)
    return f(a), f(b), c


def _emulator_fma(a, b, c):
    """fma(a_i, b_i, c_i) through oracle_axw_gemm_chain: row i of L = [c_i, -0, a_i, -0], column i of Wp = [1, 0, b_i, 0]: the chain
    (k = 0, 2, 1, 3) is fma(-0, 0, fma(a, b, fma(c, 1, +0))), and fma(-0, 0, x) = x for every x."""
    n = len(a)
    L = np.zeros((n, 4), np.float32)
    L[:, 0], L[:, 1], L[:, 2], L[:, 3] = c, -0.0, a, -0.0
    Wp = np.zeros((4, n), np.float32)
    Wp[0], Wp[2] = 1.0, b
    return np.diagonal(oracle.axw_gemm_chain(L, Wp, nthreads=4)).copy()


def _same_bits(x, y):
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    return (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))


def test_the_emulator_is_an_exact_fma():
    a, b, c = _fma_cases(np.random.default_rng(11))
    got = _emulator_fma(a, b, c)
    want = np.array([exact_fma(*t) for t in zip(a, b, c)], np.float32)
    ok = _same_bits(got, want)
    assert ok.all(), [(a[i], b[i], c[i], got[i], want[i]) for i in np.nonzero(~ok)[0][:5]]
    # the traps are live: rounding the float64 sum to fp32 misses them, and some results are subnormal
    with np.errstate(over="ignore"):
        twice = (a[:600].astype(np.float64) * b[:600] + c[:600]).astype(np.float32)
    assert (~_same_bits(twice, want[:600])).sum() >= 500
    assert ((np.abs(want) < 2.0 ** -126) & (want != 0)).sum() >= 300


def test_the_emulator_follows_the_kernel_k_order():
    """Each entry is fma over k = 0, 2, 1, 3, 4, 6, 5, 7 from +0; plain k order gives other bits on this data."""
    rng = np.random.default_rng(2)
    L = (rng.uniform(-1, 1, (6, 8)) * np.exp2(rng.integers(-12, 12, (6, 8)))).astype(np.float32)
    Wp = (rng.uniform(-1, 1, (8, 5)) * np.exp2(rng.integers(-12, 12, (8, 5)))).astype(np.float32)
    got = oracle.axw_gemm_chain(L, Wp)

    def chain(order):
        out = np.zeros((6, 5), np.float32)
        for r in range(6):
            for j in range(5):
                acc = np.float32(0.0)
                for k in order:
                    acc = exact_fma(L[r, k], Wp[k, j], acc)
                out[r, j] = acc
        return out

    assert _same_bits(got, chain([0, 2, 1, 3, 4, 6, 5, 7])).all()
    assert not _same_bits(got, chain(range(8))).all()
    with pytest.raises(ValueError):
        oracle.axw_gemm_chain(L[:, :6], Wp[:6])


# ---- fp32 emulations of the library, both orders --------------------------------------------------------------------------------

def gemm_fp32(L, W, cp):
    """L W in fp32 with Out's padding +0: the kernel's chain when dim % 4 == 0, else a k-ordered mul + add (rocBLAS's shapes)."""
    n, dim = L.shape
    c = W.shape[1]
    Wp = np.zeros((dim, cp), np.float32)
    Wp[:, :c] = W
    if dim % 4 == 0:
        out = oracle.axw_gemm_chain(L, Wp, nthreads=4)
    else:
        out = np.zeros((n, cp), np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(dim):
                out = out + L[:, k, None] * Wp[None, k, :]
    out[:, c:] = 0.0
    return out


def emulate_axw(a, X, W, order, cp):
    if order == A_XW:
        Y = gemm_fp32(X, W, cp)
        with np.errstate(invalid="ignore", over="ignore"):
            out = oracle.spmm(a.rowPtr, a.col, a.vals, Y)
        out[:, W.shape[1]:] = 0.0  # the library zeroes the padding after the SpMM when A holds an inf or NaN
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        Z = oracle.spmm(a.rowPtr, a.col, a.vals, X)
    return gemm_fp32(Z, W, cp)


SHAPES = [(150, 4, 33), (97, 7, 31), (64, 12, 1), (40, 1, 32)]


@pytest.mark.parametrize("name", AXW_SCENARIOS)
def test_fp32_emulations_of_both_orders_pass(name):
    for n, dim, c in SHAPES:
        a, X, W = axw_scenario(name, n, dim, c, seed=3)
        cp = -(-c // 32) * 32
        for order in (A_XW, AX_W):
            msg = check_axw(a, X, W, emulate_axw(a, X, W, order, cp), order, route=f"{name}/{n}x{dim}x{c}/order{order}")
            assert msg is None, msg


@pytest.mark.parametrize("name", AXW_SCENARIOS)
def test_the_gemm_emulator_passes_the_gemm_bound(name):
    _, X, W = axw_scenario(name, 96, 12, 40, seed=4)
    assert check_gemm_bound(X, W, gemm_fp32(X, W, 64)[:, :40]) is None


def test_the_orders_differ_in_class_where_the_issue_says():
    """X[s,k] = 0 against W[k,j] = inf: NaN in A (X W); +inf in (A X) W when another neighbour of the row has a nonzero in column k."""
    import flex_amd
    a = flex_amd.HostCsr(np.array([0, 2, 2], np.uint32), np.array([0, 1], np.uint32), np.array([1.0, 1.0], np.float32), n=2)
    X = np.array([[0.0], [1.0]], np.float32)
    W = np.array([[np.inf]], np.float32)
    from f64ref import axw_f64
    assert np.isnan(axw_f64(a, X, W, A_XW)[0, 0]) and axw_f64(a, X, W, AX_W)[0, 0] == np.inf
    for order in (A_XW, AX_W):
        assert check_axw(a, X, W, emulate_axw(a, X, W, order, 32), order) is None


# ---- mutants --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [A_XW, AX_W])
def test_a_dropped_k_term_fails(order):
    a, X, W = axw_scenario("uniform", 120, 8, 33, seed=5)
    X2 = X.copy()
    X2[:, 5] = 0.0
    assert check_axw(a, X, W, emulate_axw(a, X2, W, order, 64), order) is not None


@pytest.mark.parametrize("order", [A_XW, AX_W])
def test_a_flushed_subnormal_input_fails(order):
    a, X, W = axw_scenario("subnormal_X_large_W", 120, 4, 33, seed=5)
    X2 = X.copy()
    X2[np.abs(X2) < 2.0 ** -126] = 0.0
    assert check_axw(a, X, W, emulate_axw(a, X, W, order, 64), order) is None
    assert check_axw(a, X, W, emulate_axw(a, X2, W, order, 64), order) is not None


@pytest.mark.parametrize("name", ["uniform", "wide", "cancel"])
def test_a_column_shifted_by_one_fails(name):
    a, X, W = axw_scenario(name, 120, 12, 33, seed=6)
    out = emulate_axw(a, X, W, A_XW, 64)
    out[:, 1:33] = out[:, 0:32].copy()
    assert check_axw(a, X, W, out, A_XW) is not None


@pytest.mark.parametrize("bad", [np.nan, -0.0, 2.0 ** -149])
def test_anything_but_plus_zero_in_a_padding_column_fails(bad):
    a, X, W = axw_scenario("uniform", 120, 12, 33, seed=7)
    out = emulate_axw(a, X, W, AX_W, 64)
    assert check_axw(a, X, W, out, AX_W) is None
    out[17, 50] = bad
    assert "padding" in check_axw(a, X, W, out, AX_W)


@pytest.mark.parametrize("name", ["nonfinite_X", "nonfinite_W", "nonfinite_A", "zeros"])
def test_a_changed_class_fails(name):
    for order in (A_XW, AX_W):
        a, X, W = axw_scenario(name, 150, 8, 33, seed=8)
        out = emulate_axw(a, X, W, order, 64)
        nf = np.argwhere(~np.isfinite(out[:, :33]))
        assert len(nf), "the scenario produces non-finite entries"
        r, j = nf[0]
        v = out[r, j]
        for repl in ([np.inf, -np.inf, 1.0] if np.isnan(v) else [np.nan, -v, 1.0]):
            o = out.copy()
            o[r, j] = repl
            assert "class" in check_axw(a, X, W, o, order)


def test_the_range_guards_reject_what_they_must():
    import flex_amd
    # A X cancels to a value fp32 may round to zero, and meets an inf of W
    a = flex_amd.HostCsr(np.array([0, 2, 2], np.uint32), np.array([0, 1], np.uint32), np.array([1.0, -1.0], np.float32), n=2)
    X = np.array([[1.0], [1.0 - 2.0 ** -24]], np.float32)
    W = np.array([[np.inf]], np.float32)
    assert axw_range_guard(a, X, W, AX_W) is not None
    assert axw_range_guard(a, X, W, A_XW) is None
    # a stage sum at 2^120
    W = np.array([[2.0 ** 120]], np.float32)
    assert "2^120" in axw_range_guard(a, X, W, A_XW)


def test_the_gemm_launcher_is_exported():
    so = os.path.join(ROOT, "flex_amd", "lib", "libflex_axw.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert any(ln.split()[-1] == "flex_axw_gemm_launch" and ln.split()[-2] == "T" for ln in out.splitlines() if ln.strip())
    with open(os.path.join(ROOT, "include", "flex_axw.h")) as f:
        assert "flex_axw_gemm_launch" not in f.read()  # private: reached through flex_amd.axw._gemm_launch only

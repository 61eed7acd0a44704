"""The float64 reference of flex_sddmm and its bound, shared by tests/test_gpu_values.py, tests/test_gpu_values_address_limits.py and the
CPU checks of tests/test_kernel_routes.py:  out[e] = <G[row e], B[col e]>, |out - out64| <= gamma(k) T + k 2^-149 with T = sum |G B| over the
finite terms (include/flex_spmm.h), classes exact where the reference is not finite."""
import numpy as np

from f64ref import TINY, gamma


def _gb(kind, mg, nb, k, seed):
    """(G [mg, k], B [nb, k]) float32 of a value kind."""
    rng = np.random.default_rng([seed, k, mg, nb])
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)  # noqa: E731
    logu = lambda lo, hi, *s: (rng.choice([-1.0, 1.0], s) * np.exp2(rng.uniform(lo, hi, s))).astype(np.float32)  # noqa: E731
    if kind == "uniform":
        return u(mg, k), u(nb, k)
    if kind == "wide":
        return logu(-30, 30, mg, k), logu(-30, 30, nb, k)
    if kind == "underflow":
        return logu(-80, -60, mg, k), logu(-90, -68, nb, k)
    if kind == "subnormal":
        return (rng.choice([-1.0, 1.0], (mg, k)) * rng.integers(1, 1 << 23, (mg, k)) * TINY).astype(np.float32), logu(90, 110, nb, k)
    if kind == "nonfinite":
        G, B = u(mg, k), u(nb, k)
        for X, n in ((G, mg), (B, nb)):
            rows = rng.choice(n, size=max(2, n // 15), replace=False)
            for i, r in enumerate(rows):
                if i % 3 == 0:
                    X[r, rng.integers(0, k)] = np.inf
                elif i % 3 == 1:
                    X[r, rng.integers(0, k)] = -np.inf
                else:
                    X[r, rng.integers(0, k)] = np.nan
        return G, B
    raise ValueError(kind)


def sddmm64(rows, cols, G, B):
    """The float64 dot <G[rows[e]], B[cols[e]]> of the fp32 inputs, and T = sum |G B| over the finite terms."""
    G64, B64 = G.astype(np.float64), B.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = np.einsum("ek,ek->e", G64[rows], B64[cols])
        Ga, Ba = np.abs(G64), np.abs(B64)
        Ga[~np.isfinite(Ga)] = 0
        Ba[~np.isfinite(Ba)] = 0
        T = np.einsum("ek,ek->e", Ga[rows], Ba[cols])
    return ref, T


def assert_sddmm_within_bound(got, ref, T, k, what=""):
    got = np.asarray(got, np.float32).astype(np.float64)
    assert np.all(T < 2.0 ** 120), what
    fin = np.isfinite(ref)
    bad = (np.isnan(ref) & ~np.isnan(got)) | ((ref == np.inf) & (got != np.inf)) | ((ref == -np.inf) & (got != -np.inf)) | (fin & ~np.isfinite(got))
    assert not bad.any(), f"[{what}] {int(bad.sum())} entries of the wrong class; first {np.argmax(bad)}: got {got[np.argmax(bad)]!r}, want {ref[np.argmax(bad)]!r}"
    bound = gamma(k) * T + k * TINY
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(got - ref), 0.0)
    worst = int(np.argmax(err - bound)) if err.size else 0
    assert np.all(err <= bound), f"[{what}] {int((err > bound).sum())} entries beyond the bound; worst {worst}: got {got[worst]!r}, want {ref[worst]!r}, bound {bound[worst]:.3g}"
    return float((err / bound).max()) if err.size else 0.0  # the worst err / bound, for reports

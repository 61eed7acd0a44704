"""float64 reference, bounds, graphs and score scenarios of the edge softmax (include/flex_spmm.h: flex_edge_softmax,
flex_edge_softmax_backward), shared by tests/test_softmax_host.py and tests/test_gpu_attention.py.

The reference is float64 numpy on the fp32 inputs with the header's definitions: a -inf score is a masked edge (p = +0), a row whose
scores are all -inf is +0 everywhere, a row that holds a +inf or a NaN is NaN everywhere.  Bounds (u = 2^-24, gamma(n) = n u / (1 - n u),
n_r = entries of the row, D_r = min(104, scale x the spread of the row's finite scores)):
    forward    |p - p64| <= gamma(n_r + 4 D_r + 2 E + 4) p64 + 2^-126
    backward   |gs - gs64| <= gamma(n_r + 4) scale p_e (|g_e| + sum_j |p_j g_j|) + n_r 2^-149       (float64 on the same fp32 p)"""
import numpy as np

from flex_amd.binding import HostCsr

U = 2.0 ** -24
# The error of the exponential in ulp that the forward bound grants: twice the measured maximum of the function the kernels use, rounded
# up.  Measured on gfx950 over every fp32 argument in [-104, 0] against float64 (tools/probe_attention.py, profiles/attention_probe.txt):
# expf 1.000 ulp (the kernels' choice), exp2f on the prescaled argument 63.7 ulp, __expf 8.4e6 (subnormal results flushed; results below
# 2^-126 are measured in units of 2^-149).
E_ULP = 2
SCALES = (1.0, 0.125, 96 ** -0.5)


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def _segments(rp):
    """(starts of the nonempty rows, row of every entry, entries of every entry's row), rp relative to the first entry."""
    rp = np.asarray(rp, np.int64) - int(rp[0])
    deg = np.diff(rp)
    return rp[:-1][deg > 0], np.repeat(np.arange(len(deg)), deg), np.repeat(deg, deg)


def _per_row(ufunc, x, starts, row):
    """ufunc-reduce x over each row, handed back to every entry of the row."""
    if x.size == 0:
        return x.copy()
    mark = np.zeros(len(x), np.int64)
    mark[starts] = 1
    return ufunc.reduceat(x, starts)[np.cumsum(mark) - 1]


def forward_ref(rp, s, scale):
    """(p64, bound) for the scores s (fp32, the entries of the rows of rp) in float64."""
    s64 = np.asarray(s, np.float32).astype(np.float64)
    starts, row, n_r = _segments(rp)
    if s64.size == 0:
        return s64, s64
    poisoned = _per_row(np.logical_or, np.isnan(s64) | (s64 == np.inf), starts, row)
    clean = np.where(np.isnan(s64) | (s64 == np.inf), -np.inf, s64)
    M = _per_row(np.maximum, clean, starts, row)
    dead = M == -np.inf  # every score of the row is -inf
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.where(dead | (clean == -np.inf), 0.0, np.exp(np.float64(np.float32(scale)) * (clean - np.where(dead, 0.0, M))))
    L = _per_row(np.add, t, starts, row)
    p = np.where(dead, 0.0, t / np.where(dead, 1.0, L))
    p = np.where(poisoned, np.nan, p)
    lo = _per_row(np.minimum, np.where(clean == -np.inf, np.inf, clean), starts, row)
    with np.errstate(invalid="ignore"):
        D = np.where(dead, 0.0, np.minimum(104.0, np.float64(np.float32(scale)) * (M - lo)))
    bound = gamma(n_r + 4 * D + 2 * E_ULP + 4) * np.where(np.isnan(p), 0.0, p) + 2.0 ** -126
    return p, bound


def backward_ref(rp, p, g, scale):
    """(gs64, bound) of scale p (g - sum_j p_j g_j) in float64 on the fp32 p and g."""
    p64, g64 = np.asarray(p, np.float32).astype(np.float64), np.asarray(g, np.float32).astype(np.float64)
    starts, row, n_r = _segments(rp)
    if p64.size == 0:
        return p64, p64
    sc = np.float64(np.float32(scale))
    with np.errstate(invalid="ignore", over="ignore"):
        pg = p64 * g64
        gs = sc * p64 * (g64 - _per_row(np.add, pg, starts, row))
        bound = gamma(n_r + 4) * sc * np.abs(p64) * (np.abs(g64) + _per_row(np.add, np.abs(pg), starts, row)) + n_r * 2.0 ** -149
    return gs, bound


def forward_fp32(rp, s, scale):
    """The same formulas evaluated in fp32 by numpy (difference, product by scale, exp, a sequential sum, one division)."""
    s = np.asarray(s, np.float32)
    starts, row, _ = _segments(rp)
    if s.size == 0:
        return s.copy()
    bad = np.isnan(s) | (s == np.inf)
    poisoned = _per_row(np.logical_or, bad, starts, row)
    clean = np.where(bad, np.float32(-np.inf), s)
    M = _per_row(np.maximum, clean, starts, row)
    dead = M == -np.inf
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        d = (clean - np.where(dead, np.float32(0), M)).astype(np.float32)
        t = np.where(dead | (clean == -np.inf), np.float32(0), np.exp((np.float32(scale) * d).astype(np.float32)).astype(np.float32)).astype(np.float32)
        L = np.empty_like(t)
        ends = np.append(starts[1:], len(t))
        for a, b in zip(starts, ends):
            acc = np.float32(0)
            for x in t[a:b]:
                acc = np.float32(acc + x)
            L[a:b] = acc
        p = np.where(dead, np.float32(0), (t / np.where(dead, np.float32(1), L)).astype(np.float32))
    return np.where(poisoned, np.float32(np.nan), p).astype(np.float32)


def check_forward(rp, s, scale, got, what=""):
    """Asserts the classes exactly and the bound on every entry, and that each live row sums to 1 within its bound; the worst err / bound."""
    got = np.asarray(got, np.float32)
    s = np.asarray(s, np.float32)
    p, bound = forward_ref(rp, s, scale)
    assert got.shape == p.shape, (what, got.shape, p.shape)
    if p.size == 0:
        return 0.0
    starts, row, _ = _segments(rp)
    nan_ref = np.isnan(p)
    assert np.array_equal(np.isnan(got), nan_ref), f"{what}: NaN exactly on the rows that hold a +inf or a NaN ({int((np.isnan(got) != nan_ref).sum())} entries differ)"
    masked = ~nan_ref & (s == -np.inf)
    assert np.all(got[masked].view(np.uint32) == 0), f"{what}: a masked entry is not +0 bit for bit"
    ok = ~nan_ref
    err = np.abs(got[ok].astype(np.float64) - p[ok])
    ratio = err / bound[ok]
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} entries beyond the forward bound, worst err / bound {worst:.3g}"
    rs = _per_row(np.add, np.where(ok, got.astype(np.float64), 0.0), starts, row)
    rb = _per_row(np.add, np.where(ok, bound, 0.0), starts, row)
    live = ok & (_per_row(np.add, np.where(ok, p, 0.0), starts, row) > 0.5)
    assert np.all(np.abs(rs[live] - 1.0) <= rb[live]), f"{what}: a row does not sum to 1 within its bound"
    dead = ok & ~live
    assert np.all(got[dead].view(np.uint32) == 0), f"{what}: a fully masked row is not +0 everywhere"
    return worst


def check_backward(rp, p, g, scale, got, what=""):
    """Asserts the bound where the float64 result is finite and NaN / inf classes as float64 gives them; the worst err / bound."""
    got = np.asarray(got, np.float32)
    gs, bound = backward_ref(rp, p, g, scale)
    assert got.shape == gs.shape, (what, got.shape, gs.shape)
    fin = np.isfinite(gs)
    assert np.array_equal(np.isnan(got), np.isnan(gs)), f"{what}: NaN where float64 gives NaN, and nowhere else"
    assert np.array_equal(got[~fin & ~np.isnan(gs)].astype(np.float64), gs[~fin & ~np.isnan(gs)]), f"{what}: infinities as float64 gives them"
    ratio = np.abs(got[fin].astype(np.float64) - gs[fin]) / bound[fin]
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} entries beyond the backward bound, worst err / bound {worst:.3g}"
    return worst


# ---- graphs

def csr_from_degrees(deg, n, seed=0):
    rng = np.random.default_rng(seed)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    nnz = int(rp[-1])
    return HostCsr(rp, rng.integers(0, n, nnz).astype(np.uint32), rng.uniform(-1, 1, nnz).astype(np.float32), n=n)


def long_rows_graph():
    """Short rows around a 600-entry row (a wave of its own), a 2 600-entry row (a workgroup, kept in registers) and a 9 000-entry row
    (a workgroup that reads its row twice); empty rows in between."""
    deg = np.random.default_rng(5).poisson(3, 400)
    deg[17], deg[100], deg[101], deg[250], deg[399] = 2600, 600, 0, 9000, 1030
    return csr_from_degrees(deg, 3000, seed=5)


def boundary_graph():
    """Every row exactly 256 or 257 entries long: first entries at every alignment, so 256-entry rows of both classes."""
    deg = np.where(np.random.default_rng(6).random(40) < 0.5, 256, 257)
    return csr_from_degrees(deg, 700, seed=6)


def expected_classes(rp):
    """(empty, packed, wave, block) rows by the rule of internal.h (softmax_row_class): the span counts from the 4-entry mark below the row's first entry."""
    rp = np.asarray(rp, np.int64)
    deg = np.diff(rp)
    span = rp[:-1] % 4 + deg
    ne = deg > 0
    return (int((~ne).sum()), int((ne & (span <= 256)).sum()), int((ne & (span > 256) & (span <= 1024)).sum()), int((ne & (span > 1024)).sum()))


# ---- scores

SCORE_SCENARIOS = ["uniform4", "spread80", "equal", "equal_3e38", "subnormal", "masked30", "rows_masked", "poisoned"]


def chosen_rows(rp):
    """A short row, the row nearest to 256 entries and the longest row (nonempty ones)."""
    deg = np.diff(np.asarray(rp, np.int64))
    ne = np.flatnonzero(deg > 0)
    if ne.size == 0:
        return []
    return sorted({int(ne[np.argmin(deg[ne])]), int(ne[np.argmin(np.abs(deg[ne] - 256))]), int(ne[np.argmax(deg[ne])])})


def scores(name, rp, seed=0):
    rp = np.asarray(rp, np.int64)
    nnz = int(rp[-1] - rp[0])
    rng = np.random.default_rng([seed, SCORE_SCENARIOS.index(name)])
    if name == "uniform4":
        s = rng.uniform(-4, 4, nnz)
    elif name == "spread80":
        s = rng.uniform(-80, 80, nnz)
    elif name == "equal":
        s = np.full(nnz, 1.25)
    elif name == "equal_3e38":
        s = np.full(nnz, 3e38)
    elif name == "subnormal":
        s = rng.integers(-(1 << 22), 1 << 22, nnz) * 2.0 ** -149
    else:
        s = rng.uniform(-4, 4, nnz)
    s = s.astype(np.float32)
    off = rp - rp[0]
    if name == "masked30":
        s[rng.random(nnz) < 0.3] = -np.inf
    elif name == "rows_masked":
        s[rng.random(nnz) < 0.1] = -np.inf
        rows = set(chosen_rows(rp)) | set(rng.integers(0, len(rp) - 1, max(1, (len(rp) - 1) // 10)).tolist())
        for r in rows:
            s[off[r]:off[r + 1]] = -np.inf
    elif name == "poisoned":
        s[rng.random(nnz) < 0.1] = -np.inf
        for i, r in enumerate(chosen_rows(rp)):
            a, b = int(off[r]), int(off[r + 1])
            s[a + (b - a) // 2] = np.inf if i % 2 == 0 else np.nan
            if b - a > 2:
                s[b - 1] = np.nan if i % 2 == 0 else np.inf
    return s

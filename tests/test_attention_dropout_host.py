"""Host checks of the attention dropout (include/flex_spmm.h: flex_attention_dropout and its backward, bf16 and bias forms, and
flex_dropout_mask): the mask's test vectors and flex_dropout_mask against the numpy restatement, the statistics of the mask, the float64
reference (tests/attention_dropout_ref.py) against an independent float64 torch autograd evaluation, every planted fault against the
checker it targets, the public surface, and the census of the kernels in flex::dropout with the GPU case that runs each and the launches
of every pair on the host simulator.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import attention_bf16_ref as bf
import attention_bias_ref as ab
import attention_dropout_ref as ad
import flex_amd
import multihead_attention_ref as mh
from attention_forms import ALL_WANTED, COLUMN_KERNEL_ALONE, FORM_OF_K, FORMS, ROW_KERNEL_ALONE, fake_address
from backward_ref import _directed
from conftest import ROOT
from flex_amd import binding
from fused_attention_backward_ref import both_sides
from fused_attention_ref import threshold_graph
from softmax_ref import long_rows_graph

SCALE = 0.25
SEED = 0x0123456789ABCDEF  # a non-zero high word

# ---- the table of tests/test_gpu_attention_dropout.py: every (W, NS) form, idle lanes past k (48), d = 4 and d = 256, H = 1; the wide
# pairs (k >= 256) run on the graph that holds every class of row and of column
PAIRS = [(4, 1), (64, 1), (8, 2), (32, 4), (48, 3), (128, 8), (256, 4), (512, 4), (1024, 64)]
GRAPHS = {
    "thresholds_lifted": lambda: both_sides(threshold_graph()),
    "directed_empty": lambda: _directed(250, 260, seed=7),
    "long_rows": long_rows_graph,
}
KINDS = ["fp32", "bf16"]
# (graph, k, H, kind, bias, p): p = 0.5 everywhere, and 0.1 and 0.9 at (32, 4)
CASES = [(name, k, H, kind, bias, p) for k, H in PAIRS for name in (sorted(GRAPHS) if k < 256 else ["thresholds_lifted"])
         for kind in KINDS for bias in (False, True) for p in ((0.5, 0.1, 0.9) if (k, H) == (32, 4) else (0.5,))]


def case_id(c):
    name, k, H, kind, bias, p = c
    return f"{name}-k{k}-h{H}-{kind}-{'bias' if bias else 'nobias'}-p{p}"


def kernels_of(c):
    """The three instantiations in flex::dropout that the forward and the backward (every gradient wanted) of a case launch, as `nm -C`
    names them: written down from FORM_OF_K, not computed by the rule it checks."""
    name, k, H, kind, bias, p = c
    W, NS = FORM_OF_K[k]
    e, b = "float" if kind == "fp32" else "unsigned short", "true" if bias else "false"
    return [f"attention_dropout_rows<{W}, {NS}, {b}, {e}>", f"attention_dropout_rows_backward<{W}, {NS}, {b}, {e}>",
            f"attention_dropout_columns_backward<{W}, {NS}, {e}>"]


# kernel -> the id of the first case of test_every_output_against_float64 (tests/test_gpu_attention_dropout.py) that launches it
RUN_BY = {}
for _c in CASES:
    for _kern in kernels_of(_c):
        RUN_BY.setdefault(_kern, case_id(_c))

_graphs = {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = GRAPHS[name]()
    return _graphs[name]


def grad(a, k, seed, bf16=False):
    g = np.random.default_rng([seed, k, 79]).uniform(-1, 1, (a.m, k)).astype(np.float32)
    return bf.rounded(g) if bf16 else g


def case_operands(name, k, H, bf16=False, bias=False):
    """(a, Q, K, V, bias or None, g): the inputs of a case.  With a bias: attention_bias_ref's, a bias scenario per head; without:
    multihead_attention_ref's, a score scenario per head (masks and poison come through Q and K)."""
    a = graph(name)
    shift = PAIRS.index((k, H)) + sorted(GRAPHS).index(name)
    if bias:
        Q, K, V, b = ab.operands(ab.scenarios_of(H, shift=shift), a, k, seed=1, bf16=bf16)
    else:
        Q, K, V = mh.operands(mh.scenarios_of(H, shift=shift), a, k, seed=1)
        if bf16:
            Q, K, V = (bf.rounded(x) for x in (Q, K, V))
        b = None
    return a, Q, K, V, b, grad(a, k, 1, bf16)


# ---- the mask

def test_the_five_test_vectors():
    assert int(ad.bits(0, [0])[0]) == 0xAE6F80F1
    for i, r in ((0, 0x477CB3F3), (1, 0x7A8A410E), (2 ** 32 + 5, 0xEB2C8D08), (2 ** 40 + 123, 0x5CBB10BA)):
        assert int(ad.bits(SEED, np.array([i], np.uint64))[0]) == r, hex(i)
    # and through the library: p = 0.5 keeps exactly the indices with r < 2^31
    for i, r in ((0, 0x477CB3F3), (1, 0x7A8A410E), (2 ** 32 + 5, 0xEB2C8D08), (2 ** 40 + 123, 0x5CBB10BA)):
        assert int(binding.dropout_mask(SEED, 0.5, i, 1)[0]) == int(r < 2 ** 31), hex(i)
    assert int(binding.dropout_mask(0, 0.5, 0, 1)[0]) == 0


@pytest.mark.parametrize("seed", [0, 1, SEED, 2 ** 64 - 1, 2 ** 32])
@pytest.mark.parametrize("first", [0, 2 ** 32 - 1000, 2 ** 32 + 7, 2 ** 40 + 100, 2 ** 63])
def test_flex_dropout_mask_is_the_numpy_mask(seed, first):
    n = 4096
    i = np.uint64(first) + np.arange(n, dtype=np.uint64)
    for p in (0.1, 0.5, 0.6, 0.9):
        got = binding.dropout_mask(seed, p, first, n)
        assert got.dtype == np.uint8 and np.array_equal(got.astype(bool), ad.keep(seed, p, i)), (seed, first, p)


def test_the_threshold_at_the_ends_of_the_range_of_p():
    below_one = float(np.nextafter(np.float32(1), np.float32(0)))
    assert ad.threshold(1e-30) == 2 ** 32 - 1  # 1 - 1e-30 is 1 in double: floor gives 2^32, the minimum caps it
    assert ad.threshold(0.5) == 2 ** 31
    assert ad.threshold(below_one) == 256      # 2^-24 x 2^32
    assert ad.threshold(0.0) == 2 ** 32 - 1
    r = ad.bits(3, np.arange(1 << 20, dtype=np.uint64))
    for p in (1e-30, 0.5, below_one):
        got = binding.dropout_mask(3, p, 0, 1 << 20).astype(bool)
        assert np.array_equal(got, r < np.uint64(ad.threshold(p))), p
    assert binding.dropout_mask(3, 1e-30, 0, 1 << 20).sum() >= (1 << 20) - 1 and binding.dropout_mask(3, below_one, 0, 1 << 20).sum() <= 4
    for bad in (1.0, -0.1, 1.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(binding.FlexError, match="invalid"):
            binding.dropout_mask(3, bad, 0, 4)
    assert binding.dropout_mask(3, 0.5, 0, 0).shape == (0,)


N_STAT = 1 << 22
STAT_SEEDS = [0, 1, 2, SEED, 2 ** 64 - 1, 2 ** 32, 2 ** 32 + 1]
STAT_PS = [0.1, 0.5, 0.6, 0.9]
LAGS = [1, 2, 3, 4, 8, 64, 4096]
SEED_PAIRS = [(0, 1), (1, 2), (5, 5 + 2 ** 32)]
_bits = {}


def _r(seed):
    if seed not in _bits:
        _bits[seed] = ad.bits(seed, np.arange(N_STAT, dtype=np.uint64))
    return _bits[seed]


def test_the_statistics_of_the_mask_stay_within_five_standard_deviations():
    """The keep rate against thr / 2^32 (sigma = sqrt(q (1 - q) / N)), the correlation of the keep bits at the lags (sigma =
    1 / sqrt(N - lag)) and between seed pairs (sigma = 1 / sqrt(N)), over 2^22 consecutive indices.  The cap is a condition on the
    hash, not a measurement of it; the worst of the set is printed."""
    worst = 0.0
    for p in STAT_PS:
        thr = np.uint64(ad.threshold(p))
        q = float(thr) / 2.0 ** 32
        x = {}
        for seed in STAT_SEEDS + [5, 5 + 2 ** 32]:
            kp = (_r(seed) < thr).astype(np.float64)
            z = abs(kp.mean() - q) / np.sqrt(q * (1 - q) / N_STAT)
            worst = max(worst, z)
            assert z <= 5, f"seed {seed:#x} p {p}: the keep rate is {z:.2f} sigma off"
            x[seed] = (kp - q) / np.sqrt(q * (1 - q))
        for seed in STAT_SEEDS:
            for lag in LAGS:
                z = abs(float(np.dot(x[seed][:-lag], x[seed][lag:]))) / np.sqrt(N_STAT - lag)
                worst = max(worst, z)
                assert z <= 5, f"seed {seed:#x} p {p}: lag {lag} correlation is {z:.2f} sigma"
        for s0, s1 in SEED_PAIRS:
            z = abs(float(np.dot(x[s0], x[s1]))) / np.sqrt(N_STAT)
            worst = max(worst, z)
            assert z <= 5, f"seeds {s0:#x}, {s1:#x} p {p}: correlation is {z:.2f} sigma"
    print(f"the mask over 2^22 indices: worst deviation {worst:.2f} sigma")
    _bits.clear()


# ---- the reference

@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("name", ["thresholds_lifted", "directed_empty"])
@pytest.mark.parametrize("k,H", [(32, 4), (8, 1)])
def test_the_reference_agrees_with_an_independent_float64_torch_autograd_evaluation(name, k, H, with_bias):
    """Q and K hold multiples of 1 / 8 within +-1, scale is 1 / 4 and the bias multiples of 1 / 64 within +-4, so every score is exact in
    fp32 and the reference's softmax (from the fp32 score) and torch's (from the float64 one) start from the same numbers.  The mask
    enters torch as a constant tensor."""
    pytest.importorskip("torch")
    a = graph(name)
    rng = np.random.default_rng([k, H, 6])
    Q, K = (rng.integers(-8, 9, (r, k)).astype(np.float32) / 8 for r in (a.m, a.n))
    V = rng.uniform(-1, 1, (a.n, k)).astype(np.float32)
    bias = rng.integers(-256, 257, (a.nnz, H)).astype(np.float32) / 64 if with_bias else None
    g = grad(a, k, 2)
    p = 0.6
    ref = ad.reference(a, Q, K, V, bias, SCALE, H, p, SEED)
    refb = ad.backward_reference(a, Q, K, V, ref["p"], g, SCALE, H, p, SEED)  # on the float64 alpha: torch keeps its own in float64 too
    kp = ad.kept_entries(a, H, p, SEED)
    assert 0.3 < kp.mean() < 0.5
    want = ad.torch_float64(a, Q, K, V, bias, SCALE, H, g, kp, ad.factor(p))
    for what, x, y in zip(("Out", "gQ", "gK", "gV", "gBias"), (ref["out"], refb["gq"], refb["gk"], refb["gv"], refb["gb"]), want):
        if y is None:
            continue
        err = float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))
        assert err <= 1e-12, f"{name} k={k} H={H} {what}: {err:.3g}"


# ---- the planted faults

P_FAULT = 0.25  # c = 4 / 3 and 1 / p = 4 differ (at p = 0.5 they are the same number)


def _fault_case(fault, bf16, with_bias):
    a, k, H = graph("thresholds_lifted"), 32, 4
    if with_bias:
        Q, K, V, bias = ab.operands(["uniform4", "spread80", "uniform4", "masked30"], a, k, seed=4, bf16=bf16)
    else:
        Q, K, V = mh.operands(["uniform4", "spread80", "uniform4", "masked30"], a, k, seed=4)
        if bf16:
            Q, K, V = (bf.rounded(x) for x in (Q, K, V))
        bias = None
    if fault == "multiply_by_zero":  # an inf V row behind dropped entries (and behind kept ones, where it reaches Out in float64 too)
        kp = ad.kept_entries(a, H, P_FAULT, SEED)
        col = ab.coo(a)[1]
        V = V.copy()
        V[col[np.flatnonzero(~kp[:, 0])[:3]], :8] = np.inf
    return a, k, H, Q, K, V, bias, grad(a, k, 4, bf16)


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fault", ad.FAULTS)
def test_the_checker_a_fault_targets_rejects_it(fault, bf16, with_bias):
    a, k, H, Q, K, V, bias, g = _fault_case(fault, bf16, with_bias)
    rows = (17, 300) if fault == "shard_local" else None
    Qr = Q if rows is None else Q[rows[0]:rows[1]]
    narrow = (lambda x: bf.to_bf16(x)) if bf16 else (lambda x: x)
    gg = None if rows or fault == "multiply_by_zero" else g
    right = ad.fp32_result(a, Qr, K, V, bias, SCALE, H, P_FAULT, SEED, g=gg, rows=rows)
    assert ad.check(a, Qr, K, V, bias, SCALE, H, P_FAULT, SEED, narrow(right["out"]), right["p"], rows=rows, bf16=bf16) <= 1.0
    bad = ad.fp32_result(a, Qr, K, V, bias, SCALE, H, P_FAULT, SEED, g=gg, probs=right["p"], rows=rows, fault=fault)
    if fault in ad.FORWARD_FAULTS:
        with pytest.raises(AssertionError):  # Out gives it away
            ad.check(a, Qr, K, V, bias, SCALE, H, P_FAULT, SEED, narrow(bad["out"]), rows=rows, what=fault, bf16=bf16)
        if fault == "mask_before_norm":
            with pytest.raises(AssertionError, match=r"\bP\b"):  # and so does P beside the right Out
                ad.check(a, Qr, K, V, bias, SCALE, H, P_FAULT, SEED, narrow(right["out"]), bad["p"], rows=rows, what=fault, bf16=bf16)
        return
    grads = lambda r: tuple(narrow(r[key]) for key in ("gq", "gk", "gv"))
    assert ad.check_backward(a, Q, K, V, right["p"], g, SCALE, H, P_FAULT, SEED, *grads(right), right["gb"], right["ds"], bf16=bf16) <= 1.0
    if fault == "gv_unmasked":
        with pytest.raises(AssertionError, match="gv"):
            ad.check_backward(a, Q, K, V, right["p"], g, SCALE, H, P_FAULT, SEED, gV=narrow(bad["gv"]), what=fault, bf16=bf16)
    else:  # da_unmasked: da of a dropped entry is not +0, and ds, gBias, gQ and gK follow
        for key, kw in (("ds", dict(ds=bad["ds"])), ("gBias", dict(gB=bad["gb"])), ("gq", dict(gQ=narrow(bad["gq"]))), ("gk", dict(gK=narrow(bad["gk"])))):
            with pytest.raises(AssertionError, match=key):
                ad.check_backward(a, Q, K, V, right["p"], g, SCALE, H, P_FAULT, SEED, what=fault, bf16=bf16, **kw)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_float64_rounded_once_stays_inside_the_bounds(bf16):
    for with_bias in (False, True):
        a, Q, K, V, bias, g = case_operands("thresholds_lifted", 48, 3, bf16, with_bias)
        res = ad.fp32_result(a, Q, K, V, bias, SCALE, 3, 0.5, SEED, g=g)
        if bf16:
            ref = ad.reference(a, Q, K, V, bias, SCALE, 3, 0.5, SEED)
            refb = ad.backward_reference(a, Q, K, V, res["p"], g, SCALE, 3, 0.5, SEED)
            res.update(out=bf.f64_to_bf16(ref["out"]), **{key: bf.f64_to_bf16(refb[key]) for key in ("gq", "gk", "gv")})
        assert ad.check(a, Q, K, V, bias, SCALE, 3, 0.5, SEED, res["out"], res["p"], bf16=bf16) <= 1.0
        assert ad.check_backward(a, Q, K, V, res["p"], g, SCALE, 3, 0.5, SEED, res["gq"], res["gk"], res["gv"], res["gb"], res["ds"], bf16=bf16) <= 1.0


# ---- the public surface

NAMES = ("flex_attention_dropout", "flex_attention_dropout_backward", "flex_attention_bf16_dropout", "flex_attention_bf16_dropout_backward")


def test_the_library_exports_the_five_calls_and_the_header_declares_them():
    hdr = open(os.path.join(ROOT, "include", "flex_spmm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+FLEX_ABI_VERSION\s+3\b", hdr)
    L = ctypes.CDLL(flex_amd.lib_path())
    for name in NAMES + ("flex_dropout_mask",):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/flex_spmm.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in binding.SYMBOLS
    for name in NAMES:
        assert len(binding._values_fn(name).argtypes) == (16 if name.endswith("backward") else 12)
    assert L.flex_abi_version() == 3


def test_the_package_offers_the_methods_and_functions_keeps_its_ten_entries():
    for f in ("attention_dropout", "attention_dropout_backward", "attention_bf16_dropout", "attention_bf16_dropout_backward"):
        assert callable(getattr(flex_amd.Plan, f, None)), f
        assert callable(getattr(flex_amd.Plan, f + "_ptr", None)), f + "_ptr"
    assert callable(binding.dropout_mask)
    pytest.importorskip("torch")
    from flex_amd import autograd
    fs = autograd.functions()
    assert len(fs) == 10 and fs[9].__name__ == "_FusedAttentionBias"
    assert [f.__name__ for f in autograd.dropout_functions()] == ["_FusedAttentionDropout"]


class _NoPlan(flex_amd.SparseOperator):
    """The operator's argument checks without its plans (making a plan needs a GPU)."""

    def __init__(self, nnz, k, **flags):
        self.m = self.n = 8
        self.k, self.nnz = k, nnz
        self.learn_values = True
        self.fused_attention, self.fused_backward = flags.get("fused_attention", False), flags.get("fused_backward", False)


def test_dropout_needs_both_fused_paths_one_dtype_a_probability_and_a_bias_of_its_shape():
    torch = pytest.importorskip("torch")
    Q = torch.zeros((8, 32))
    b = torch.zeros((20, 4))
    for flags in (dict(), dict(fused_attention=True)):
        for kw in (dict(), dict(bias=b)):
            with pytest.raises(NotImplementedError, match="fused_backward=True"):
                _NoPlan(20, 32, **flags).attention(Q, Q, Q, heads=4, dropout=0.5, **kw)
    op = _NoPlan(20, 32, fused_attention=True, fused_backward=True)
    for mixed in ((Q.bfloat16(), Q, Q), (Q, Q.bfloat16(), Q), (Q, Q, Q.double())):
        with pytest.raises(TypeError, match="one dtype"):
            op.attention(*mixed, heads=4, dropout=0.5)
    for bad in (b.double(), b[:, :2], b[:19], b[:, 0]):
        with pytest.raises(TypeError, match="bias of shape"):
            op.attention(Q, Q, Q, heads=4, bias=bad, dropout=0.5)
    for bad in (1.0, -0.5, 2.0, float("nan")):
        with pytest.raises(ValueError, match="probability"):
            op.attention(Q, Q, Q, heads=4, dropout=bad)


# ---- the census

def shipped_dropout_kernels(so):
    """The kernel handles (data symbols, not the launchers' code) of flex::dropout in a built library, as `nm -C` names them without
    the namespace and the parameters."""
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-C", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        _, kind, sym = line.split(" ", 2)
        head = sym.split("(", 1)[0]
        if kind in "tTwW" or "__device_stub__" in sym or "flex::dropout::" not in head:
            continue
        names.add(head.split("flex::dropout::", 1)[1])
    return names


def test_the_library_ships_exactly_the_seventy_kernels_and_a_gpu_case_runs_each():
    so = os.path.join(os.path.dirname(binding.__file__), "lib", "libflex_spmm.so")
    assert os.path.exists(so), f"{so} is not built"
    shipped = shipped_dropout_kernels(so)
    assert len(shipped) == 70, sorted(shipped)
    wanted = set()
    for W, NS in FORMS:
        for e in ("float", "unsigned short"):
            for b in ("false", "true"):
                wanted |= {f"attention_dropout_rows<{W}, {NS}, {b}, {e}>", f"attention_dropout_rows_backward<{W}, {NS}, {b}, {e}>"}
            wanted.add(f"attention_dropout_columns_backward<{W}, {NS}, {e}>")
    assert len(wanted) == 70 and shipped == wanted, (sorted(shipped - wanted), sorted(wanted - shipped))
    assert set(RUN_BY) == shipped, (f"kernels no GPU case launches: {sorted(shipped - set(RUN_BY))}", f"declared but not shipped: {sorted(set(RUN_BY) - shipped)}")
    ids = {case_id(c) for c in CASES}
    assert all(v in ids for v in RUN_BY.values())
    assert {FORM_OF_K[k] for k, _ in PAIRS} == set(FORMS)


# ---- the census against the launches

@pytest.fixture
def sim():
    """(tests/hostsim, flex_amd.binding's library on the host simulator) for one test: the others here run on the library itself."""
    hostsim = pytest.importorskip("hostsim")
    for lib in hostsim.binding_on_simulator():
        yield hostsim, lib


def test_every_pair_launches_on_the_simulator_the_kernels_its_cases_declare(sim):
    """The forward and then the backward of every (k, H), element type and bias setting, on fake operands (nothing is read or written):
    the library's own entry points on the simulator's stand-in launchers must log kernels_of() of the case, and with one gradient
    wanted the forward and one backward kernel: gQ (with a bias: and gBias) the row kernel, gV the column kernel."""
    hostsim, lib = sim
    a = graph("thresholds_lifted")
    q, kk, v, out, g, pr, work, bias, gb, gq, gk, gv = (fake_address(i) for i in range(12))
    for k, H in PAIRS:
        plan = flex_amd.Plan(a, k, attention=True, attention_backward=True)
        for kind in KINDS:
            fwd, bwd = ((plan.attention_dropout_ptr, plan.attention_dropout_backward_ptr) if kind == "fp32" else
                        (plan.attention_bf16_dropout_ptr, plan.attention_bf16_dropout_backward_ptr))
            for with_bias in (False, True):
                def launch(want, want_bias):
                    fwd(q, kk, v, bias if with_bias else None, SCALE, 0.5, SEED, out, pr, heads=H)
                    bwd(q, kk, v, pr, g, SCALE, 0.5, SEED, *(x if w else None for x, w in zip((gq, gk, gv), want)), gb if want_bias else None, work,
                        heads=H)
                names = ["dropout::" + n for n in kernels_of(("thresholds_lifted", k, H, kind, with_bias, 0.5))]
                assert hostsim.launch_log(lib, lambda: launch(ALL_WANTED, with_bias)) == names, (k, H, kind, with_bias)
                assert hostsim.launch_log(lib, lambda: launch(ROW_KERNEL_ALONE, with_bias)) == names[:2], (k, H, kind, with_bias)
                # gBias is the row kernel's: the column kernel runs alone where it is not wanted either
                assert hostsim.launch_log(lib, lambda: launch(COLUMN_KERNEL_ALONE, False)) == [names[0], names[2]], (k, H, kind, with_bias)
        plan.destroy()

"""The multi-head fused attention on bf16 row operands on the GPU (flex_attention_bf16, flex_attention_bf16_backward): Out, P, gQ, gK, gV
and ds against the stacked float64 reference on every element -- the gradients and Out under the bf16 bound of
tests/attention_bf16_ref.py, P and ds under the fp32 bounds unchanged -- with a different score scenario in every head, over every
(k, H) of the table of tests/test_attention_bf16_host.py (every (W, NS) form, idle lanes past k, d = 4 and d = 256, H = 1); the same
bits as the fp32 walk (flex_attention_heads / _backward on the widened operands: P and dWork bit for bit, the rest their bf16 rounding);
head isolation; the output invariants (dP = NULL, subsets of the gradients, run to run, a captured graph); refusals; a row-range shard;
and SparseOperator.attention on bfloat16 leaves with its gradients against a float64 torch evaluation.

Graphs: those of tests/test_gpu_multihead_attention.py (thresholds, its lift, directed_empty, long_rows); the wide pairs (k >= 256) run
on the two threshold graphs alone."""
import numpy as np
import pytest

import attention_bf16_ref as bf
import flex_amd
import multihead_attention_ref as mh
import test_gpu_attention as composition
from backward_ref import _directed
from flex_amd import binding
from test_attention_bf16_host import CASES, case_operands, graph

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FILL = 0x5A5A  # bf16 bits no test computes; an edge array starts at SENTINEL
SENTINEL = -12345.5
SCALE = 0.25
_plans, _runs = {}, {}


def plan(name, k, **kw):
    key = (name, k, tuple(sorted(kw.items())))
    if key not in _plans:
        kw.setdefault("attention_backward", True)
        _plans[key] = flex_amd.Plan(graph(name), k, attention=True, **kw)
        _plans[key].self_check()
    return _plans[key]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _dev_bf16(x):
    """an fp32 array of bf16 numbers (or any fp32 array: it is rounded) as a torch.bfloat16 cuda tensor"""
    return torch.from_numpy(bf.to_bf16(x).view(np.int16)).cuda().view(torch.bfloat16)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(t):
    """the bf16 bits (uint16) of a torch.bfloat16 tensor"""
    torch.cuda.synchronize()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _filled(shape):
    return torch.full(shape, FILL, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and bool(np.array_equal(x.view(np.uint8), y.view(np.uint8)))


def _grad(a, k, seed):
    return bf.rounded(np.random.default_rng([seed, k, 78]).uniform(-1, 1, (a.m, k)).astype(np.float32))


def _forward(p, a, Q, K, V, H, scale=SCALE, with_p=True):
    """(Out bits, P [nnz, H] fp32) on the host; Out starts at FILL and P at the sentinel."""
    pd = torch.full((a.nnz, H), SENTINEL, device="cuda") if with_p else None
    out = p.attention_bf16(_dev_bf16(Q), _dev_bf16(K), _dev_bf16(V), scale, heads=H, out=_filled((a.m, p.info()["k"])), p=pd)
    return _bits(out), (_host(pd) if with_p else None)


def _backward(p, a, Q, K, V, pr, g, H, scale=SCALE, want=(True, True, True)):
    """(gQ, gK, gV bits, ds [nnz, H] fp32) on the host; an output that is not wanted is None, ds is what dWork holds afterwards."""
    work = torch.full((a.nnz, H), SENTINEL, device="cuda")
    outs = p.attention_bf16_backward(_dev_bf16(Q), _dev_bf16(K), _dev_bf16(V), _dev(pr), _dev_bf16(g), scale, heads=H, work=work, want=want)
    return tuple(None if t is None else _bits(t) for t in outs) + (_host(work),)


def _run(name, k, H):
    """The bf16 forward and backward of a case of the table, run once and shared by the tests below; nothing changes it."""
    if (name, k, H) not in _runs:
        a, names, Q, K, V, g = case_operands(name, k, H)
        p = plan(name, k)
        out, pr = _forward(p, a, Q, K, V, H)
        _runs[(name, k, H)] = (out, pr) + _backward(p, a, Q, K, V, pr, g, H)
    return _runs[(name, k, H)]


# ---- 1. against float64

@pytest.mark.parametrize("name,k,H", CASES)
def test_every_output_against_float64_with_a_scenario_per_head(name, k, H):
    a, names, Q, K, V, g = case_operands(name, k, H)
    out, pr, gq, gk, gv, ds = _run(name, k, H)
    each = {}
    bf.check(a, Q, K, V, SCALE, H, out, pr, what=f"{name} k={k} H={H}", ratios=each)
    bf.check_backward(a, Q, K, V, pr, g, SCALE, H, gq, gk, gv, ds, what=f"{name} k={k} H={H}", ratios=each)
    print(f"{name} k={k} H={H} {'/'.join(names[:5])}: worst err / bound " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))


# ---- 2. the same bits as the fp32 walk

@pytest.mark.parametrize("name,k,H", [c for c in CASES if c[2] >= 2])
def test_the_same_bits_as_the_fp32_walk_on_the_widened_operands(name, k, H):
    a, names, Q, K, V, g = case_operands(name, k, H)
    out, pr, gq, gk, gv, ds = _run(name, k, H)
    p = plan(name, k)
    Qd, Kd, Vd, gd = (_dev(x) for x in (Q, K, V, g))
    p32 = torch.full((a.nnz, H), SENTINEL, device="cuda")
    out32 = _host(p.attention(Qd, Kd, Vd, SCALE, p=p32, heads=H))
    assert _same_bits(_host(p32), pr), f"{name} k={k} H={H}: P differs from the fp32 call's in {int((_host(p32).view(np.uint32) != pr.view(np.uint32)).sum())} entries"
    work32 = torch.full((a.nnz, H), SENTINEL, device="cuda")
    grads32 = p.attention_backward(Qd, Kd, Vd, p32, gd, SCALE, work=work32, heads=H)
    assert _same_bits(_host(work32), ds), f"{name} k={k} H={H}: dWork differs from the fp32 call's"
    for key, got, x32 in zip(("out", "gq", "gk", "gv"), (out, gq, gk, gv), (out32,) + tuple(_host(t) for t in grads32)):
        nan = np.isnan(x32)
        assert np.array_equal(np.isnan(bf.from_bf16(got)), nan), f"{name} k={k} H={H} {key}: NaN exactly where the fp32 call has it"
        differ = (got != bf.to_bf16(x32)) & ~nan
        assert not differ.any(), f"{name} k={k} H={H} {key}: {int(differ.sum())} elements are not the bf16 rounding of the fp32 call's"


# ---- 3. head isolation

@pytest.mark.parametrize("k,H", [(32, 4), (512, 4)])
def test_what_one_head_holds_reaches_no_other_head(k, H):
    name = "thresholds_lifted"
    a, p, d = graph(name), plan(name, k), k // H
    Q, K, V = bf.operands(mh.scenarios_of(H, shift=2), a, k, seed=4)
    g = _grad(a, k, 4)

    def run(Q, K, V, g):
        out, pr = _forward(p, a, Q, K, V, H)
        return (out, pr) + _backward(p, a, Q, K, V, pr, g, H)

    base = run(Q, K, V, g)
    rng = np.random.default_rng(5)
    for j in sorted({0, H // 2, H - 1}):
        c = mh.head_columns(k, H, j)
        Q2, K2, V2, g2 = (x.copy() for x in (Q, K, V, g))
        for x in (Q2, K2, V2, g2):
            x[:, c] = bf.rounded(rng.uniform(-3, 3, (x.shape[0], d)).astype(np.float32))
            x[rng.integers(0, x.shape[0], 9), c.start + rng.integers(0, d, 9)] = [np.nan, np.inf, -np.inf] * 3
        other = run(Q2, K2, V2, g2)
        keep_cols = np.ones(k, bool)
        keep_cols[c] = False
        keep_heads = np.arange(H) != j
        for key, x, y in zip(("out", "p", "gq", "gk", "gv", "ds"), base, other):
            sel = keep_heads if key in ("p", "ds") else keep_cols
            assert _same_bits(x[:, sel], y[:, sel]), f"k={k} H={H}: changing head {j} changed {key} of another head"
        assert not _same_bits(base[0][:, c], other[0][:, c])


# ---- 4. and 5. output invariants

def test_without_p_the_same_out_and_every_gradient_has_the_same_bits_whichever_others_are_asked_for():
    name, k, H = "thresholds_lifted", 48, 3
    a, names, Q, K, V, g = case_operands(name, k, H)
    p = plan(name, k)
    out, pr, *full = _run(name, k, H)
    assert _same_bits(_forward(p, a, Q, K, V, H, with_p=False)[0], out)
    for mask in range(7):
        want = tuple(bool(mask >> i & 1) for i in range(3))
        got = _backward(p, a, Q, K, V, pr, g, H, want=want)
        for i in range(3):
            assert (got[i] is None) if not want[i] else _same_bits(got[i], full[i]), (want, i)
        if want[0] or want[1]:
            assert _same_bits(got[3], full[3]), want
        else:
            assert np.all(got[3] == SENTINEL), want  # neither gQ nor gK: the row launch is skipped and dWork is not written


def test_two_runs_and_a_captured_graph_give_the_same_bits():
    name, k, H = "long_rows", 128, 8
    a, names, Q, K, V, g = case_operands(name, k, H)
    p = plan(name, k)
    first = _run(name, k, H)
    out2, pr2 = _forward(p, a, Q, K, V, H)
    again = (out2, pr2) + _backward(p, a, Q, K, V, pr2, g, H)
    for x, y in zip(first, again):
        assert _same_bits(x, y)
    Qd, Kd, Vd, gd = (_dev_bf16(x) for x in (Q, K, V, g))
    o, pd, work = _filled((a.m, k)), torch.empty((a.nnz, H), device="cuda"), torch.empty((a.nnz, H), device="cuda")
    gq, gk, gv = _filled((a.m, k)), _filled((a.n, k)), _filled((a.n, k))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=side):  # one stream: the three launches are a chain
        p.attention_bf16(Qd, Kd, Vd, SCALE, heads=H, out=o, p=pd)
        p.attention_bf16_backward(Qd, Kd, Vd, pd, gd, SCALE, heads=H, grad_q=gq, grad_k=gk, grad_v=gv, work=work)
    for t in (pd, work):
        t.fill_(SENTINEL)
    for t in (o, gq, gk, gv):
        t.view(torch.int16).fill_(FILL)
    graph_.replay()
    for x, t in zip(first, (o, pd, gq, gk, gv, work)):
        assert _same_bits(x, _bits(t) if t.dtype == torch.bfloat16 else _host(t))


# ---- 6. refusals

def test_refused_calls():
    name, k = "directed_empty", 32
    a, p = graph(name), plan(name, k)
    Q, K, V = (_dev_bf16(x) for x in bf.operands(["uniform4"], a, k))
    g = _dev_bf16(_grad(a, k, 8))
    s = torch.cuda.current_stream().cuda_stream

    def calls(pl, H, kk, shift=0, same_work=False, grad_shift=0):
        """(forward, backward) through the pointer forms; nothing may be launched, so every output is checked to keep its fill."""
        Qd = torch.zeros((a.m * kk + 8,), dtype=torch.bfloat16, device="cuda")
        Kd, Vd, gd = (torch.zeros((r, kk), dtype=torch.bfloat16, device="cuda") for r in (a.n, a.n, a.m))
        outs = [_filled((r * kk + 8,)) for r in (a.m, a.m, a.n, a.n)]
        edge = [torch.full((a.nnz * max(H, 1),), SENTINEL, device="cuda") for _ in range(2)]
        fwd = lambda: pl.attention_bf16_ptr(Qd.data_ptr() + shift, Kd.data_ptr(), Vd.data_ptr(), SCALE, outs[0].data_ptr(), edge[0].data_ptr(), s, heads=H)
        bwd = lambda: pl.attention_bf16_backward_ptr(Qd.data_ptr() + shift, Kd.data_ptr(), Vd.data_ptr(), edge[0].data_ptr(), gd.data_ptr(), SCALE,
                                                     outs[1].data_ptr(), outs[2].data_ptr() + grad_shift, outs[3].data_ptr(),
                                                     edge[0 if same_work else 1].data_ptr(), s, heads=H)
        untouched = lambda: all(bool((_bits(t) == FILL).all()) for t in outs) and all(bool((_host(t) == SENTINEL).all()) for t in edge)
        return fwd, bwd, untouched

    def refused(pl, H, kk, match, **kw):
        fwd, bwd, untouched = calls(pl, H, kk, **kw)
        for f in (fwd, bwd):
            with pytest.raises(binding.FlexError, match=match):
                f()
        assert untouched()

    refused(p, 0, k, "invalid")
    refused(p, -2, k, "invalid")
    refused(p, 3, k, "not supported")                                             # 3 does not divide 32
    refused(plan(name, 24), 2, 24, "not supported")                               # d = 12
    refused(plan(name, 1024), 2, 1024, "not supported")                           # d = 512
    refused(plan(name, 48), 1, 48, "not supported")                               # one head is served here: d = 48 is no power of two
    refused(plan(name, 300), 1, 300, "not supported")                             # d = 300
    refused(plan(name, k, ldb=34, ldc=36), 4, 36, "not supported")                # ldb % 4 != 0
    refused(p, 4, k, "not supported", shift=4)                                    # Q 4-byte but not 8-byte aligned
    refused(p, 4, k, "not supported", shift=2)                                    # Q aligned as a bf16 only
    fwd, bwd, untouched = calls(p, 4, k, grad_shift=4)                            # an output of the backward 4-byte aligned
    with pytest.raises(binding.FlexError, match="not supported"):
        bwd()
    assert untouched()
    refused(flex_amd.Plan(a, k), 4, k, "invalid")                                 # no FLEX_PLAN_ATTENTION
    fwd, bwd, untouched = calls(plan(name, k, attention_backward=False), 4, k)    # the forward's flag alone
    fwd()
    with pytest.raises(binding.FlexError, match="invalid"):
        bwd()
    fwd, bwd, untouched = calls(p, 4, k, same_work=True)                          # dWork == dP
    with pytest.raises(binding.FlexError, match="invalid"):
        bwd()
    assert untouched()
    pd = torch.zeros((a.nnz, 4), device="cuda")
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(binding.FlexError, match="invalid"):
            p.attention_bf16(Q, K, V, scale, heads=4)
        with pytest.raises(binding.FlexError, match="invalid"):
            p.attention_bf16_backward(Q, K, V, pd, g, scale, heads=4)
    with pytest.raises(binding.FlexError, match="invalid"):
        p.attention_bf16_ptr(None, K.data_ptr(), V.data_ptr(), SCALE, g.data_ptr(), None, s, heads=4)
    work = torch.full((a.nnz, 4), SENTINEL, device="cuda")
    with pytest.raises(binding.FlexError, match="invalid"):                       # no dWork
        p.attention_bf16_backward_ptr(Q.data_ptr(), K.data_ptr(), V.data_ptr(), pd.data_ptr(), g.data_ptr(), SCALE, None, None, None, None, s, heads=4)
    p.attention_bf16_backward_ptr(Q.data_ptr(), K.data_ptr(), V.data_ptr(), pd.data_ptr(), g.data_ptr(), SCALE, None, None, None, work.data_ptr(), s, heads=4)
    assert np.all(_host(work) == SENTINEL)                                        # no output asked for: nothing is launched
    empty = binding.HostCsr(np.zeros(41, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=17)
    pe = flex_amd.Plan(empty, k, attention=True, attention_backward=True)
    pe.attention_bf16_ptr(None, None, None, 1.0, None, heads=4)  # no entries: no launch, nothing read
    pe.attention_bf16_backward_ptr(None, None, None, None, None, 1.0, None, None, None, None, heads=4)
    with pytest.raises(AssertionError):                                           # the tensor forms take bfloat16 rows only
        p.attention_bf16(Q.float(), K, V, SCALE, heads=4)
    with pytest.raises(AssertionError):                                           # and the existing ones float32 only
        p.attention(Q, K, V, SCALE, heads=4)


def test_rows_8_bytes_off_a_16_byte_mark_are_served_and_give_the_bits_of_the_aligned_run():
    """What the refusals above stop short of: a row operand four elements (8 bytes) into its buffer is aligned as the 8-byte form needs.
    Q and gK alone, then every row operand (Q, K, V, g, Out, gQ, gK, gV): nothing is refused, every output has the aligned run's bits,
    and the elements before and after the moved rows keep their fill."""
    name, k, H = "directed_empty", 32, 4
    a, names, Q, K, V, g = case_operands(name, k, H)
    p = plan(name, k)
    aligned = dict(zip(("out", "p", "gq", "gk", "gv", "ds"), _run(name, k, H)))
    s = torch.cuda.current_stream().cuda_stream
    rows = {"Q": a.m, "K": a.n, "V": a.n, "g": a.m, "out": a.m, "gq": a.m, "gk": a.n, "gv": a.n}
    for moved in (("Q", "gk"), tuple(rows)):
        t = {key: _filled((r * k + 8,)) for key, r in rows.items()}
        at = {key: 4 if key in moved else 0 for key in t}
        for key, x in (("Q", Q), ("K", K), ("V", V), ("g", g)):
            t[key][at[key]:at[key] + rows[key] * k] = _dev_bf16(x).view(-1)
        ptr = {key: t[key].data_ptr() + 2 * at[key] for key in t}
        assert all((ptr[key] % 16 == 8) == (key in moved) for key in t)
        pd, work = (torch.full((a.nnz, H), SENTINEL, device="cuda") for _ in range(2))
        p.attention_bf16_ptr(ptr["Q"], ptr["K"], ptr["V"], SCALE, ptr["out"], pd.data_ptr(), s, heads=H)
        p.attention_bf16_backward_ptr(ptr["Q"], ptr["K"], ptr["V"], pd.data_ptr(), ptr["g"], SCALE, ptr["gq"], ptr["gk"], ptr["gv"], work.data_ptr(), s, heads=H)
        for key in ("out", "gq", "gk", "gv"):
            x, lo, hi = _bits(t[key]), at[key], at[key] + rows[key] * k
            assert bool((x[:lo] == FILL).all()) and bool((x[hi:] == FILL).all()), (moved, key)
            assert _same_bits(x[lo:hi].reshape(rows[key], k), aligned[key]), (moved, key)
        assert _same_bits(_host(pd), aligned["p"]) and _same_bits(_host(work), aligned["ds"]), moved


# ---- 7. a row-range shard, forward

def test_a_shard_writes_its_own_rows_and_entries_only_and_has_no_backward():
    name, k, H = "long_rows", 32, 4
    a = graph(name)
    Q, K, V = bf.operands(mh.scenarios_of(H, shift=3), a, k, seed=9)
    whole, whole_p = _forward(plan(name, k), a, Q, K, V, H)
    Qd, Kd, Vd = _dev_bf16(Q), _dev_bf16(K), _dev_bf16(V)
    s = torch.cuda.current_stream().cuda_stream
    cuts = [0, 17, 18, 18, 101, 260, a.m]
    union, union_p = np.full((a.m, k), np.uint16(FILL)), np.full((a.nnz, H), np.float32(SENTINEL))
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        shard = flex_amd.Plan(a, k, rows=(r0, r1), attention=True)
        shard.self_check()
        e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
        out, pd = _filled((a.m, k)), torch.full((a.nnz, H), SENTINEL, device="cuda")
        shard.attention_bf16_ptr(Qd.data_ptr() + 2 * k * r0, Kd.data_ptr(), Vd.data_ptr(), SCALE, out.data_ptr() + 2 * k * r0, pd.data_ptr(), s, heads=H)
        with pytest.raises(binding.FlexError, match="invalid"):  # the backward is not defined on a shard
            shard.attention_bf16_backward_ptr(Qd.data_ptr() + 2 * k * r0, Kd.data_ptr(), Vd.data_ptr(), pd.data_ptr(), Qd.data_ptr(), SCALE,
                                              None, None, out.data_ptr(), pd.data_ptr() + 4, s, heads=H)
        out, pd = _bits(out), _host(pd)
        assert np.all(out[:r0] == FILL) and np.all(out[r1:] == FILL), (r0, r1)
        assert np.all(pd[:e0] == SENTINEL) and np.all(pd[e1:] == SENTINEL), (r0, r1)
        if r1 > r0:
            bf.check(a, Q[r0:r1], K, V, SCALE, H, out[r0:r1], pd[e0:e1], rows=(r0, r1), what=f"rows [{r0}, {r1})")
        union[r0:r1], union_p[e0:e1] = out[r0:r1], pd[e0:e1]
    assert _same_bits(union, whole) and _same_bits(union_p, whole_p)


# ---- 8. autograd

@pytest.mark.parametrize("k,H", [(32, 4), (128, 8)])
def test_the_operator_on_bfloat16_leaves_and_its_gradients_against_float64(k, H):
    from test_gpu_fused_attention_backward import _fused_backward_tolerances
    a = _directed(300, seed=6, dup=True)
    d = k // H
    rng = np.random.default_rng([k, H, 23])
    Q, K, V = (bf.rounded(rng.uniform(-1, 1, (r, k)).astype(np.float32)) for r in (a.m, a.n, a.n))
    gOut = bf.rounded(rng.uniform(-1, 1, (a.m, k)).astype(np.float32))
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    Qd, Kd, Vd = (_dev_bf16(x).requires_grad_() for x in (Q, K, V))
    out = op.attention(Qd, Kd, Vd, heads=H)  # the default scale: d ** -0.5
    out.backward(_dev_bf16(gOut))
    assert all(t.dtype == torch.bfloat16 for t in (out, Qd.grad, Kd.grad, Vd.grad))
    got = tuple(bf.from_bf16(_bits(t)) for t in (out.detach(), Qd.grad, Kd.grad, Vd.grad))
    scale = d ** -0.5
    worst = 0.0
    for h in range(H):
        c = mh.head_columns(k, H, h)
        want = composition._attention_f64(a, Q[:, c], K[:, c], V[:, c], scale, gOut[:, c])
        tols = _fused_backward_tolerances(a, Q[:, c], K[:, c], V[:, c], scale, gOut[:, c], want[5])
        for what, x, ref, tol in zip(("Out", "grad_Q", "grad_K", "grad_V"), got, want[:4], tols):
            err, tol = np.abs(x[:, c].astype(np.float64) - ref), bf.bound_bf16(ref, tol)  # the propagated bound, then the one rounding to bf16
            worst = max(worst, float((err / tol).max()))
            assert np.all(err <= tol), f"{what} k={k} H={H} head {h}: worst err / tolerance {float((err / tol).max()):.3g}"
    print(f"k={k} H={H}: worst err / tolerance {worst:.3g}")
    with torch.no_grad():  # no gradient wanted: nothing nnz-sized is written, the same Out
        assert _same_bits(_bits(op.attention(Qd, Kd, Vd, heads=H)), _bits(out.detach()))
    want = op.plan.attention_bf16(Qd.detach(), Kd.detach(), Vd.detach(), scale, heads=H)
    assert _same_bits(_bits(want), _bits(out.detach()))


def test_bfloat16_needs_both_fused_paths_and_one_dtype():
    a, k = _directed(120, seed=9), 32
    Q, K, V = (_dev_bf16(x) for x in bf.operands(["uniform4"], a, k, seed=10))
    for kw in (dict(), dict(fused_attention=True)):
        op = flex_amd.SparseOperator(a, k, learn_values=True, **kw)
        for H in (1, 4):
            with pytest.raises(NotImplementedError, match="fused_backward=True"):
                op.attention(Q, K, V, heads=H)
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    for mixed in ((Q.float(), K, V), (Q, K.float(), V), (Q, K, V.float())):
        with pytest.raises(TypeError, match="one dtype"):
            op.attention(*mixed, heads=4)
    one = op.attention(Q, K, V)  # one head runs on bf16 as well: flex_attention_bf16 with heads = 1, scale k ** -0.5
    assert one.dtype == torch.bfloat16 and _same_bits(_bits(one), _bits(op.plan.attention_bf16(Q, K, V, k ** -0.5, heads=1)))
    f32 = op.attention(Q.float(), K.float(), V.float(), heads=4)  # the float32 path is the one it was
    assert f32.dtype == torch.float32 and _same_bits(_host(f32), _host(op.plan.attention(Q.float(), K.float(), V.float(), 8 ** -0.5, heads=4)))

"""The fused attention with a per-edge bias on the GPU (flex_attention_bias, flex_attention_bias_backward and their bf16 forms): Out, P,
gQ, gK, gV, gBias and dWork against float64 on every element under the header's bounds (tests/attention_bias_ref.py), a different bias
scenario in every head, over every (k, H) of the table of tests/test_attention_bias_host.py (every (W, NS) form, idle lanes past k, d = 4
and d = 256, H = 1), for fp32 rows and for bf16 rows; the bf16 walk against the fp32 walk bit for bit; a zero bias, and one head against
the composition sddmm -> torch add -> edge_softmax -> SpMM with its autograd; head isolation; the output invariants (dP = NULL, the 15
subsets of the four gradients, run to run, a captured graph); the refusals; a row-range shard; and SparseOperator.attention(..., bias=b)
with its gradients against a float64 torch evaluation.

Classes are exact everywhere: NaN where float64 has it and nowhere else, +0 rows as +0 bits, masked p as the +0 bit pattern."""
import numpy as np
import pytest

import attention_bf16_ref as bf
import attention_bias_ref as ab
import flex_amd
import multihead_attention_ref as mh
from backward_ref import _directed
from flex_amd import binding
from test_attention_bias_host import CASES, case_operands, grad, graph

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FILL = 0x5A5A  # bf16 bits no test computes; fp32 rows and edge arrays start at SENTINEL
SENTINEL = -12345.5
SCALE = 0.25
KINDS = ["fp32", "bf16"]
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
    return torch.from_numpy(bf.to_bf16(x).view(np.int16)).cuda().view(torch.bfloat16)


def _rows(x, kind):
    """a row operand on the device: float32, or bfloat16 (x then holds bf16 numbers)"""
    return _dev_bf16(x) if kind == "bf16" else _dev(x)


def _host(t):
    """float32 tensors as they are, bfloat16 ones as their bits (uint16)"""
    torch.cuda.synchronize()
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.cpu().numpy()


def _filled(shape, kind):
    if kind == "bf16":
        return torch.full(shape, FILL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return torch.full(shape, SENTINEL, device="cuda")


def _is_fill(x):
    return bool(np.all(x == (FILL if x.dtype == np.uint16 else np.float32(SENTINEL))))


def _same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and bool(np.array_equal(x.view(np.uint8), y.view(np.uint8)))


def _forward(p, a, Q, K, V, bias, H, kind, scale=SCALE, with_p=True):
    """(Out, P [nnz, H] fp32) on the host; Out starts at its fill and P at the sentinel."""
    pd = torch.full((a.nnz, H), SENTINEL, device="cuda") if with_p else None
    run = p.attention_bf16_bias if kind == "bf16" else p.attention_bias
    out = run(_rows(Q, kind), _rows(K, kind), _rows(V, kind), _dev(bias), scale, heads=H, out=_filled((a.m, p.info()["k"]), kind), p=pd)
    return _host(out), (_host(pd) if with_p else None)


def _backward(p, a, Q, K, V, pr, g, H, kind, scale=SCALE, want=(True, True, True, True)):
    """(gQ, gK, gV, gBias, ds) on the host; an output that is not wanted is None, ds is what dWork holds afterwards."""
    work = torch.full((a.nnz, H), SENTINEL, device="cuda")
    run = p.attention_bf16_bias_backward if kind == "bf16" else p.attention_bias_backward
    outs = run(_rows(Q, kind), _rows(K, kind), _rows(V, kind), _dev(pr), _rows(g, kind), scale, heads=H, work=work, want=want)
    return tuple(None if t is None else _host(t) for t in outs) + (_host(work),)


def _run(name, k, H, kind):
    """The forward and backward of a case of the table, run once and shared by the tests below; nothing changes it.
    (Out, P, gQ, gK, gV, gBias, ds)."""
    if (name, k, H, kind) not in _runs:
        a, names, Q, K, V, bias, g = case_operands(name, k, H, kind == "bf16")
        p = plan(name, k)
        out, pr = _forward(p, a, Q, K, V, bias, H, kind)
        _runs[(name, k, H, kind)] = (out, pr) + _backward(p, a, Q, K, V, pr, g, H, kind)
    return _runs[(name, k, H, kind)]


# ---- 1. against float64

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,k,H", CASES)
def test_every_output_against_float64_with_a_bias_scenario_per_head(name, k, H, kind):
    a, names, Q, K, V, bias, g = case_operands(name, k, H, kind == "bf16")
    out, pr, gq, gk, gv, gb, ds = _run(name, k, H, kind)
    each = {}
    ab.check(a, Q, K, V, bias, SCALE, H, out, pr, what=f"{name} k={k} H={H} {kind}", ratios=each, bf16=kind == "bf16")
    ab.check_backward(a, Q, K, V, pr, g, SCALE, H, gq, gk, gv, gb, ds, what=f"{name} k={k} H={H} {kind}", ratios=each, bf16=kind == "bf16")
    print(f"{name} k={k} H={H} {kind} {'/'.join(names[:7])}: worst err / bound " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))


# ---- 2. the bf16 walk has the bits of the fp32 walk

@pytest.mark.parametrize("name,k,H", [c for c in CASES if c[2] >= 2])
def test_bf16_rows_give_the_bits_of_the_fp32_call_on_the_widened_operands(name, k, H):
    a, names, Q, K, V, bias, g = case_operands(name, k, H, True)
    out, pr, gq, gk, gv, gb, ds = _run(name, k, H, "bf16")
    p = plan(name, k)
    out32, p32 = _forward(p, a, Q, K, V, bias, H, "fp32")
    what = f"{name} k={k} H={H}"
    assert _same_bits(p32, pr), f"{what}: P differs from the fp32 call's in {int((p32.view(np.uint32) != pr.view(np.uint32)).sum())} entries"
    gq32, gk32, gv32, gb32, ds32 = _backward(p, a, Q, K, V, p32, g, H, "fp32")
    assert _same_bits(ds32, ds), f"{what}: dWork differs from the fp32 call's"
    assert _same_bits(gb32, gb), f"{what}: gBias differs from the fp32 call's"
    for key, got, x32 in zip(("out", "gq", "gk", "gv"), (out, gq, gk, gv), (out32, gq32, gk32, gv32)):
        nan = np.isnan(x32)
        assert np.array_equal(np.isnan(bf.from_bf16(got)), nan), f"{what} {key}: NaN exactly where the fp32 call has it"
        differ = (got != bf.to_bf16(x32)) & ~nan
        assert not differ.any(), f"{what} {key}: {int(differ.sum())} elements are not the bf16 rounding of the fp32 call's"


# ---- 3. a zero bias, and one head against the composition

@pytest.mark.parametrize("kind", KINDS)
def test_a_zero_bias_stays_within_the_bounds(kind):
    name, k, H = "thresholds_lifted", 48, 3
    a, p = graph(name), plan(name, k)
    Q, K, V, bias = ab.operands(["zero"] * H, a, k, seed=11, bf16=kind == "bf16")
    g = grad(a, k, 11, kind == "bf16")
    assert not bias.any()
    out, pr = _forward(p, a, Q, K, V, bias, H, kind)
    gq, gk, gv, gb, ds = _backward(p, a, Q, K, V, pr, g, H, kind)
    each = {}
    ab.check(a, Q, K, V, bias, SCALE, H, out, pr, what="zero bias", ratios=each, bf16=kind == "bf16")
    ab.check_backward(a, Q, K, V, pr, g, SCALE, H, gq, gk, gv, gb, ds, what="zero bias", ratios=each, bf16=kind == "bf16")
    # and, the score being scale s exactly, within the unbiased reference's own bounds as well
    (bf if kind == "bf16" else mh).check(a, Q, K, V, SCALE, H, out, pr, what="zero bias, unbiased reference")
    print(f"zero bias {kind}: worst err / bound " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))


@pytest.mark.parametrize("name,k", [("directed_dups", 32), ("thresholds_lifted", 64)])
def test_one_head_against_the_composition_of_the_existing_calls(name, k):
    """sddmm, a torch add, edge_softmax at scale 1 and the SpMM with the result as values, with their autograd: what a user needed
    before.  Both paths lie within their own propagated bound of float64, so within the sum of the two of each other."""
    a = _directed(300, seed=6, dup=True) if name == "directed_dups" else graph(name)
    rng = np.random.default_rng([k, 31])
    Q, K, V = (rng.uniform(-1, 1, (r, k)).astype(np.float32) for r in (a.m, a.n, a.n))
    bias = rng.uniform(-4, 4, (a.nnz, 1)).astype(np.float32)
    gOut = rng.uniform(-1, 1, (a.m, k)).astype(np.float32)
    scale = k ** -0.5
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    results = []
    for fused in (True, False):
        Qd, Kd, Vd, bd = (_dev(x).requires_grad_() for x in (Q, K, V, bias[:, 0]))
        if fused:
            out = op.attention(Qd, Kd, Vd, bias=bd)
        else:
            out = op(Vd, values=op.edge_softmax(float(np.float32(scale)) * op.sddmm(Qd, Kd) + bd, 1.0))
        out.backward(_dev(gOut))
        results.append(tuple(_host(t) for t in (out.detach(), Qd.grad, Kd.grad, Vd.grad, bd.grad[:, None])))
    want = ab.torch_float64(a, Q, K, V, bias, scale, 1, gOut)
    tol_f = ab.propagated_bounds(a, Q, K, V, bias, scale, 1, gOut)
    tol_c = ab.propagated_bounds(a, Q, K, V, bias, scale, 1, gOut, composition=True)
    for what, f, c, ref, tf, tc in zip(("Out", "grad_Q", "grad_K", "grad_V", "grad_bias"), *results, want, tol_f, tol_c):
        ef, ec, between = np.abs(f.astype(np.float64) - ref), np.abs(c.astype(np.float64) - ref), np.abs(f.astype(np.float64) - c)
        print(f"{name} k={k} {what}: worst err / tolerance fused {float((ef / tf).max()):.3g}, composition {float((ec / tc).max()):.3g}, "
              f"between them {float((between / (tf + tc)).max()):.3g}")
        assert np.all(ef <= tf), f"{what}: the fused call, worst err / tolerance {float((ef / tf).max()):.3g}"
        assert np.all(ec <= tc), f"{what}: the composition, worst err / tolerance {float((ec / tc).max()):.3g}"
        assert np.all(ef <= tf + tc) and np.all(between <= tf + tc), what


# ---- 4. head isolation

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,H", [(32, 4), (512, 4)])
def test_what_the_bias_of_one_head_holds_reaches_no_other_head(k, H, kind):
    name = "thresholds_lifted"
    a, p = graph(name), plan(name, k)
    Q, K, V, bias = ab.operands(ab.scenarios_of(H, shift=1), a, k, seed=4, bf16=kind == "bf16")
    g = grad(a, k, 4, kind == "bf16")
    row, col, rp = ab.coo(a)

    def run(b):
        out, pr = _forward(p, a, Q, K, V, b, H, kind)
        return (out, pr) + _backward(p, a, Q, K, V, pr, g, H, kind)

    base = run(bias)
    rng = np.random.default_rng(5)
    for j in sorted({0, H // 2, H - 1}):
        c = mh.head_columns(k, H, j)
        keep_cols, keep_heads = np.ones(k, bool), np.arange(H) != j
        keep_cols[c] = False
        hit = rng.integers(0, a.nnz, 6)
        poisoned = bias.copy()
        poisoned[:, j] = rng.uniform(-4, 4, a.nnz)
        poisoned[hit, j] = [np.nan, np.inf] * 3
        masked = bias.copy()
        masked[:, j] = -np.inf
        for what, b in (("NaN and +inf", poisoned), ("a -inf column", masked)):
            other = run(b)
            for key, x, y in zip(("out", "p", "gq", "gk", "gv", "gb", "ds"), base, other):
                sel = keep_heads if key in ("p", "gb", "ds") else keep_cols
                assert _same_bits(x[:, sel], y[:, sel]), f"k={k} H={H} {kind}: {what} in the bias of head {j} changed {key} of another head"
        out, pr = other[0], other[1]  # the -inf column: head j is masked everywhere: +0 bits in its columns of Out and its entries of P
        assert not np.ascontiguousarray(out[:, c]).view(np.uint8).any() and not np.ascontiguousarray(pr[:, j]).view(np.uint8).any()
        out, pr = run(poisoned)[:2]
        val = bf.from_bf16(out) if kind == "bf16" else out
        bad = np.zeros(a.m, bool)
        bad[row[hit]] = True
        assert np.isnan(val[bad][:, c]).all() and not np.isnan(val[~bad][:, c]).any()
        assert np.array_equal(np.isnan(pr[:, j]), bad[row])


# ---- 5. output invariants

@pytest.mark.parametrize("kind", KINDS)
def test_without_p_the_same_out_and_every_gradient_has_the_same_bits_whichever_others_are_asked_for(kind):
    name, k, H = "thresholds_lifted", 48, 3
    a, names, Q, K, V, bias, g = case_operands(name, k, H, kind == "bf16")
    p = plan(name, k)
    out, pr, *full = _run(name, k, H, kind)
    assert _same_bits(_forward(p, a, Q, K, V, bias, H, kind, with_p=False)[0], out)
    for mask in range(1, 16):
        want = tuple(bool(mask >> i & 1) for i in range(4))
        got = _backward(p, a, Q, K, V, pr, g, H, kind, want=want)
        for i in range(4):
            assert (got[i] is None) if not want[i] else _same_bits(got[i], full[i]), (want, i)
        if want[0] or want[1] or want[3]:
            assert _same_bits(got[4], full[4]), want
        else:
            assert np.all(got[4] == SENTINEL), want  # gV alone: the rows' launch is skipped and dWork is not written
    # gBias alone writes nothing else but dWork
    gbd, work = torch.full((a.nnz, H), SENTINEL, device="cuda"), torch.full((a.nnz, H), SENTINEL, device="cuda")
    ptr = p.attention_bf16_bias_backward_ptr if kind == "bf16" else p.attention_bias_backward_ptr
    Qd, Kd, Vd, gd, pd = _rows(Q, kind), _rows(K, kind), _rows(V, kind), _rows(g, kind), _dev(pr)
    ptr(Qd.data_ptr(), Kd.data_ptr(), Vd.data_ptr(), pd.data_ptr(), gd.data_ptr(), SCALE, None, None, None, gbd.data_ptr(), work.data_ptr(),
        torch.cuda.current_stream().cuda_stream, heads=H)
    assert _same_bits(_host(gbd), full[3]) and _same_bits(_host(work), full[4]) and _same_bits(_host(pd), pr)


@pytest.mark.parametrize("kind", KINDS)
def test_two_runs_and_a_captured_graph_give_the_same_bits(kind):
    name, k, H = "long_rows", 128, 8
    a, names, Q, K, V, bias, g = case_operands(name, k, H, kind == "bf16")
    p = plan(name, k)
    first = _run(name, k, H, kind)
    out2, pr2 = _forward(p, a, Q, K, V, bias, H, kind)
    again = (out2, pr2) + _backward(p, a, Q, K, V, pr2, g, H, kind)
    for x, y in zip(first, again):
        assert _same_bits(x, y)
    Qd, Kd, Vd, gd, bd = _rows(Q, kind), _rows(K, kind), _rows(V, kind), _rows(g, kind), _dev(bias)
    o, pd, work, gb = _filled((a.m, k), kind), *(torch.empty((a.nnz, H), device="cuda") for _ in range(3))
    gq, gk, gv = _filled((a.m, k), kind), _filled((a.n, k), kind), _filled((a.n, k), kind)
    fwd, bwd = (p.attention_bf16_bias, p.attention_bf16_bias_backward) if kind == "bf16" else (p.attention_bias, p.attention_bias_backward)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=side):  # one stream: the three launches are a chain
        fwd(Qd, Kd, Vd, bd, SCALE, heads=H, out=o, p=pd)
        bwd(Qd, Kd, Vd, pd, gd, SCALE, heads=H, grad_q=gq, grad_k=gk, grad_v=gv, grad_bias=gb, work=work)
    for t in (pd, work, gb):
        t.fill_(SENTINEL)
    for t in (o, gq, gk, gv):
        t.copy_(_filled(tuple(t.shape), kind))
    graph_.replay()
    for x, t in zip(first, (o, pd, gq, gk, gv, gb, work)):
        assert _same_bits(x, _host(t))


# ---- 6. refusals

@pytest.mark.parametrize("kind", KINDS)
def test_refused_calls(kind):
    name, k = "directed_empty", 32
    a, p = graph(name), plan(name, k)
    es = 2 if kind == "bf16" else 4  # bytes of a row element
    dt = torch.bfloat16 if kind == "bf16" else torch.float32
    s = torch.cuda.current_stream().cuda_stream
    names = ("attention_bf16_bias_ptr", "attention_bf16_bias_backward_ptr") if kind == "bf16" else ("attention_bias_ptr", "attention_bias_backward_ptr")

    def calls(pl, H, kk, shift=0, work=1, gbias=2, grad_shift=0, no_bias=False):
        """(forward, backward, untouched) through the pointer forms; edge arrays: 0 = P, 1 = Work, 2 = gBias."""
        f_ptr, b_ptr = getattr(pl, names[0]), getattr(pl, names[1])
        Qd = torch.zeros((a.m * kk + 8,), dtype=dt, device="cuda")
        Kd, Vd, gd = (torch.zeros((r, kk), dtype=dt, device="cuda") for r in (a.n, a.n, a.m))
        outs = [_filled((r * kk + 8,), kind) for r in (a.m, a.m, a.n, a.n)]
        edge = [torch.full((a.nnz * max(H, 1) + 2,), SENTINEL, device="cuda") for _ in range(3)]
        bd = torch.zeros((a.nnz * max(H, 1) + 2,), device="cuda")
        fwd = lambda: f_ptr(Qd.data_ptr() + shift, Kd.data_ptr(), Vd.data_ptr(), None if no_bias else bd.data_ptr(), SCALE,
                            outs[0].data_ptr(), edge[0].data_ptr(), s, heads=H)
        bwd = lambda: b_ptr(Qd.data_ptr() + shift, Kd.data_ptr(), Vd.data_ptr(), edge[0].data_ptr(), gd.data_ptr(), SCALE, outs[1].data_ptr(),
                            outs[2].data_ptr() + grad_shift, outs[3].data_ptr(), edge[gbias].data_ptr(), edge[work].data_ptr(), s, heads=H)
        untouched = lambda: all(_is_fill(_host(t)) for t in outs) and all(_is_fill(_host(t)) for t in edge)
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
    refused(plan(name, k, ldb=34, ldc=36), 4, 36, "not supported")                # an odd stride: ldb % 4 != 0
    refused(p, 4, k, "not supported", shift=es)                                   # Q aligned as one element only
    refused(p, 4, k, "not supported", shift=2 * es)                               # Q aligned to two elements: half the vector
    fwd, bwd, untouched = calls(p, 4, k, grad_shift=2 * es)                       # an output of the backward misaligned
    with pytest.raises(binding.FlexError, match="not supported"):
        bwd()
    assert untouched()
    refused(flex_amd.Plan(a, k), 4, k, "invalid")                                 # the wrong kind of plan: no FLEX_PLAN_ATTENTION
    fwd, bwd, untouched = calls(plan(name, k, attention_backward=False), 4, k)    # the forward's flag alone
    fwd()
    with pytest.raises(binding.FlexError, match="invalid"):
        bwd()
    fwd, bwd, untouched = calls(p, 4, k, no_bias=True)                            # a NULL bias
    with pytest.raises(binding.FlexError, match="invalid"):
        fwd()
    assert untouched()
    for kw in (dict(work=0), dict(gbias=0), dict(gbias=1)):                       # dWork == dP, gBias == dP, gBias == dWork
        fwd, bwd, untouched = calls(p, 4, k, **kw)
        with pytest.raises(binding.FlexError, match="invalid"):
            bwd()
        assert untouched()
    Q, K, V = (_rows(x, kind) for x in ab.operands(["uniform4"] * 4, a, k, bf16=kind == "bf16")[:3])
    g, bd, pd = _rows(grad(a, k, 8, kind == "bf16"), kind), torch.zeros((a.nnz, 4), device="cuda"), torch.zeros((a.nnz, 4), device="cuda")
    fwd_t, bwd_t = (p.attention_bf16_bias, p.attention_bf16_bias_backward) if kind == "bf16" else (p.attention_bias, p.attention_bias_backward)
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(binding.FlexError, match="invalid"):
            fwd_t(Q, K, V, bd, scale, heads=4)
        with pytest.raises(binding.FlexError, match="invalid"):
            bwd_t(Q, K, V, pd, g, scale, heads=4)
    f_ptr, b_ptr = getattr(p, names[0]), getattr(p, names[1])
    with pytest.raises(binding.FlexError, match="invalid"):                       # no Q
        f_ptr(None, K.data_ptr(), V.data_ptr(), bd.data_ptr(), SCALE, g.data_ptr(), None, s, heads=4)
    work = torch.full((a.nnz, 4), SENTINEL, device="cuda")
    with pytest.raises(binding.FlexError, match="invalid"):                       # no dWork
        b_ptr(Q.data_ptr(), K.data_ptr(), V.data_ptr(), pd.data_ptr(), g.data_ptr(), SCALE, None, None, None, None, None, s, heads=4)
    b_ptr(Q.data_ptr(), K.data_ptr(), V.data_ptr(), pd.data_ptr(), g.data_ptr(), SCALE, None, None, None, None, work.data_ptr(), s, heads=4)
    assert np.all(_host(work) == SENTINEL)                                        # no output asked for: nothing is launched
    empty = binding.HostCsr(np.zeros(41, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=17)
    pe = flex_amd.Plan(empty, k, attention=True, attention_backward=True)
    getattr(pe, names[0])(None, None, None, None, 1.0, None, heads=4)             # no entries: no launch, nothing read
    getattr(pe, names[1])(None, None, None, None, None, 1.0, None, None, None, None, None, heads=4)
    with pytest.raises(AssertionError):                                           # the tensor forms take rows of their own dtype only
        fwd_t(Q.double(), K, V, bd, SCALE, heads=4)
    with pytest.raises(AssertionError):                                           # a bias of another shape or dtype
        fwd_t(Q, K, V, bd[:, :2].contiguous(), SCALE, heads=4)
    with pytest.raises(AssertionError):
        fwd_t(Q, K, V, bd.double(), SCALE, heads=4)
    with pytest.raises(AssertionError):                                           # [nnz] stands for [nnz, 1] with one head only
        fwd_t(Q, K, V, bd[:, 0].contiguous(), SCALE, heads=4)


@pytest.mark.parametrize("kind", KINDS)
def test_a_bias_and_a_gbias_at_an_odd_float_offset_are_served(kind):
    name, k, H = "directed_empty", 32, 4
    a, names, Q, K, V, bias, g = case_operands(name, k, H, kind == "bf16")
    p = plan(name, k)
    out, pr, gq, gk, gv, gb, ds = _run(name, k, H, kind)
    s = torch.cuda.current_stream().cuda_stream
    Qd, Kd, Vd, gd, pd = _rows(Q, kind), _rows(K, kind), _rows(V, kind), _rows(g, kind), _dev(pr)
    odd = torch.zeros((a.nnz * H + 1,), device="cuda")
    assert odd.data_ptr() % 16 == 0
    odd[1:] = _dev(bias).reshape(-1)
    o, pd2 = _filled((a.m, k), kind), torch.full((a.nnz, H), SENTINEL, device="cuda")
    f_ptr, b_ptr = ((p.attention_bf16_bias_ptr, p.attention_bf16_bias_backward_ptr) if kind == "bf16"
                    else (p.attention_bias_ptr, p.attention_bias_backward_ptr))
    f_ptr(Qd.data_ptr(), Kd.data_ptr(), Vd.data_ptr(), odd.data_ptr() + 4, SCALE, o.data_ptr(), pd2.data_ptr(), s, heads=H)
    assert _same_bits(_host(o), out) and _same_bits(_host(pd2), pr)
    gb_odd, work = torch.full((a.nnz * H + 1,), SENTINEL, device="cuda"), torch.full((a.nnz, H), SENTINEL, device="cuda")
    b_ptr(Qd.data_ptr(), Kd.data_ptr(), Vd.data_ptr(), pd.data_ptr(), gd.data_ptr(), SCALE, None, None, None, gb_odd.data_ptr() + 4, work.data_ptr(), s,
          heads=H)
    got = _host(gb_odd)
    assert got[0] == np.float32(SENTINEL) and _same_bits(got[1:].reshape(a.nnz, H), gb) and _same_bits(_host(work), ds)


# ---- 7. a row-range shard, forward

@pytest.mark.parametrize("kind", KINDS)
def test_a_shard_reads_the_bias_of_its_own_entries_and_writes_its_own_rows_and_entries_only(kind):
    name, k, H = "long_rows", 32, 4
    a = graph(name)
    Q, K, V, bias = ab.operands(ab.scenarios_of(H, shift=3), a, k, seed=9, bf16=kind == "bf16")
    whole, whole_p = _forward(plan(name, k), a, Q, K, V, bias, H, kind)
    Qd, Kd, Vd = _rows(Q, kind), _rows(K, kind), _rows(V, kind)
    es = Qd.element_size()
    s = torch.cuda.current_stream().cuda_stream
    cuts = [0, 17, 18, 18, 101, 260, a.m]
    union = np.full((a.m, k), np.uint16(FILL) if kind == "bf16" else np.float32(SENTINEL))
    union_p = np.full((a.nnz, H), np.float32(SENTINEL))
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        shard = flex_amd.Plan(a, k, rows=(r0, r1), attention=True)
        shard.self_check()
        e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
        # what lies outside the shard's entries is NaN: a shard that read another's bias would be poisoned
        own = np.full((a.nnz, H), np.nan, np.float32)
        own[e0:e1] = bias[e0:e1]
        out, pd = _filled((a.m, k), kind), torch.full((a.nnz, H), SENTINEL, device="cuda")
        f_ptr, b_ptr = ((shard.attention_bf16_bias_ptr, shard.attention_bf16_bias_backward_ptr) if kind == "bf16"
                        else (shard.attention_bias_ptr, shard.attention_bias_backward_ptr))
        ownd = _dev(own)
        f_ptr(Qd.data_ptr() + es * k * r0, Kd.data_ptr(), Vd.data_ptr(), ownd.data_ptr(), SCALE, out.data_ptr() + es * k * r0, pd.data_ptr(), s, heads=H)
        with pytest.raises(binding.FlexError, match="invalid"):  # the backward is not defined on a shard
            b_ptr(Qd.data_ptr() + es * k * r0, Kd.data_ptr(), Vd.data_ptr(), pd.data_ptr(), Qd.data_ptr(), SCALE, None, None, out.data_ptr(), None,
                  pd.data_ptr() + 4, s, heads=H)
        out, pd = _host(out), _host(pd)
        assert _is_fill(out[:r0]) and _is_fill(out[r1:]), (r0, r1)
        assert np.all(pd[:e0] == SENTINEL) and np.all(pd[e1:] == SENTINEL), (r0, r1)
        if r1 > r0:
            ab.check(a, Q[r0:r1], K, V, bias, SCALE, H, out[r0:r1], pd[e0:e1], rows=(r0, r1), what=f"rows [{r0}, {r1})", bf16=kind == "bf16")
        union[r0:r1], union_p[e0:e1] = out[r0:r1], pd[e0:e1]
    assert _same_bits(union, whole) and _same_bits(union_p, whole_p)


# ---- 8. autograd

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,H", [(32, 4), (128, 8)])
def test_the_operator_with_a_bias_and_its_gradients_against_float64(k, H, kind):
    a = _directed(300, seed=6, dup=True)
    d = k // H
    rng = np.random.default_rng([k, H, 23])
    Q, K, V, gOut = (rng.uniform(-1, 1, (r, k)).astype(np.float32) for r in (a.m, a.n, a.n, a.m))
    if kind == "bf16":
        Q, K, V, gOut = (bf.rounded(x) for x in (Q, K, V, gOut))
    bias = rng.uniform(-4, 4, (a.nnz, H)).astype(np.float32)
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    Qd, Kd, Vd = (_rows(x, kind).requires_grad_() for x in (Q, K, V))
    bd = _dev(bias).requires_grad_()
    before = _host(op.attention(Qd.detach(), Kd.detach(), Vd.detach(), heads=H))
    out = op.attention(Qd, Kd, Vd, heads=H, bias=bd)  # the default scale: d ** -0.5
    out.backward(_rows(gOut, kind))
    dt = torch.bfloat16 if kind == "bf16" else torch.float32
    assert all(t.dtype == dt for t in (out, Qd.grad, Kd.grad, Vd.grad)) and bd.grad.dtype == torch.float32 and bd.grad.shape == bd.shape
    got = tuple(_host(t) for t in (out.detach(), Qd.grad, Kd.grad, Vd.grad, bd.grad))
    scale = d ** -0.5
    want = ab.torch_float64(a, Q, K, V, bias, scale, H, gOut)
    tols = ab.propagated_bounds(a, Q, K, V, bias, scale, H, gOut)
    worst = 0.0
    for what, x, ref, tol in zip(("Out", "grad_Q", "grad_K", "grad_V", "grad_bias"), got, want, tols):
        if x.dtype == np.uint16:  # the propagated bound, then the one rounding to bf16
            x, tol = bf.from_bf16(x), bf.bound_bf16(ref, tol)
        err = np.abs(x.astype(np.float64) - ref)
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), f"{what} k={k} H={H} {kind}: worst err / tolerance {float((err / tol).max()):.3g}"
    print(f"k={k} H={H} {kind}: worst err / tolerance {worst:.3g}")
    with torch.no_grad():  # no gradient wanted: nothing nnz-sized is written, the same Out
        assert _same_bits(_host(op.attention(Qd, Kd, Vd, heads=H, bias=bd)), got[0])
    run = op.plan.attention_bf16_bias if kind == "bf16" else op.plan.attention_bias
    assert _same_bits(_host(run(Qd.detach(), Kd.detach(), Vd.detach(), bd.detach(), scale, heads=H)), got[0])
    # only the bias wants a gradient: the others stay None
    b2 = _dev(bias).requires_grad_()
    op.attention(Qd.detach(), Kd.detach(), Vd.detach(), heads=H, bias=b2).backward(_rows(gOut, kind))
    assert _same_bits(_host(b2.grad), got[4])
    # bias=None on the same operator gives the bits it gave before, and the bits of the unbiased call
    after = _host(op.attention(Qd.detach(), Kd.detach(), Vd.detach(), heads=H, bias=None))
    assert _same_bits(after, before)
    plain = op.plan.attention_bf16(Qd.detach(), Kd.detach(), Vd.detach(), scale, heads=H) if kind == "bf16" else \
        op.plan.attention(Qd.detach(), Kd.detach(), Vd.detach(), scale, heads=H)
    assert _same_bits(_host(plain), before)


def test_one_head_takes_a_bias_of_nnz_elements():
    a, k = _directed(120, seed=9), 32
    Q, K, V, bias = ab.operands(["uniform4"], a, k, seed=10)
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    Qd, Kd, Vd = (_dev(x) for x in (Q, K, V))
    flat = _dev(bias[:, 0]).requires_grad_()
    one = op.attention(Qd, Kd, Vd, bias=flat)
    one.sum().backward()
    assert flat.grad.shape == flat.shape
    two = op.plan.attention_bias(Qd, Kd, Vd, _dev(bias), k ** -0.5, heads=1)
    assert _same_bits(_host(one.detach()), _host(two))
    ab.check(a, Q, K, V, bias, k ** -0.5, 1, _host(two), what="one head")

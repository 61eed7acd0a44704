"""The attention dropout of the fused multi-head attention on the GPU (flex_attention_dropout, flex_attention_dropout_backward and their
bf16 forms, with and without the per-edge bias): Out, P, gQ, gK, gV, gBias and dWork against float64 on every element under the bounds of
tests/attention_dropout_ref.py over the table of tests/test_attention_dropout_host.py (every (W, NS) form in every kernel family); P
and p = 0 against the undropped calls bit for bit; one mask in all three launches, equal to flex_dropout_mask; non-finite V rows behind
dropped entries; the output invariants (no P, the subsets of the gradients, run to run, a captured graph, another seed); the refusals;
a row-range shard; and SparseOperator.attention(..., dropout=p) with its gradients against a float64 torch evaluation."""
import numpy as np
import pytest

import attention_bf16_ref as bf
import attention_bias_ref as ab
import attention_dropout_ref as ad
import flex_amd
from backward_ref import _directed
from flex_amd import binding
from test_attention_dropout_host import CASES, SEED, case_id, case_operands, grad, graph

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


def _rows(x, kind):
    """a row operand on the device: float32, or bfloat16 (x then holds bf16 numbers)"""
    return torch.from_numpy(bf.to_bf16(x).view(np.int16)).cuda().view(torch.bfloat16) if kind == "bf16" else _dev(x)


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


def _forward(p, a, Q, K, V, bias, H, kind, drop, seed=SEED, scale=SCALE, with_p=True):
    """(Out, P [nnz, H] fp32) on the host; Out starts at its fill and P at the sentinel."""
    pd = torch.full((a.nnz, H), SENTINEL, device="cuda") if with_p else None
    run = p.attention_bf16_dropout if kind == "bf16" else p.attention_dropout
    out = run(_rows(Q, kind), _rows(K, kind), _rows(V, kind), scale, drop, seed, heads=H, bias=None if bias is None else _dev(bias),
              out=_filled((a.m, p.info()["k"]), kind), probs=pd)
    return _host(out), (_host(pd) if with_p else None)


def _backward(p, a, Q, K, V, pr, g, H, kind, drop, seed=SEED, scale=SCALE, want=(True, True, True, True)):
    """(gQ, gK, gV, gBias, ds) on the host; an output that is not wanted is None, ds is what dWork holds afterwards."""
    work = torch.full((a.nnz, H), SENTINEL, device="cuda")
    run = p.attention_bf16_dropout_backward if kind == "bf16" else p.attention_dropout_backward
    outs = run(_rows(Q, kind), _rows(K, kind), _rows(V, kind), _dev(pr), _rows(g, kind), scale, drop, seed, heads=H, work=work, want=want)
    return tuple(None if t is None else _host(t) for t in outs) + (_host(work),)


def _run(c):
    """The forward and backward of a case of the table, run once and shared by the tests below; nothing changes it.
    (Out, P, gQ, gK, gV, gBias or None, ds)."""
    if c not in _runs:
        name, k, H, kind, bias, drop = c
        a, Q, K, V, b, g = case_operands(name, k, H, kind == "bf16", bias)
        p = plan(name, k)
        out, pr = _forward(p, a, Q, K, V, b, H, kind, drop)
        _runs[c] = (out, pr) + _backward(p, a, Q, K, V, pr, g, H, kind, drop, want=(True, True, True, bias))
    return _runs[c]


# ---- 1. against float64

@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_every_output_against_float64(c):
    name, k, H, kind, bias, drop = c
    a, Q, K, V, b, g = case_operands(name, k, H, kind == "bf16", bias)
    out, pr, gq, gk, gv, gb, ds = _run(c)
    each, what = {}, case_id(c)
    ad.check(a, Q, K, V, b, SCALE, H, drop, SEED, out, pr, what=what, ratios=each, bf16=kind == "bf16")
    ad.check_backward(a, Q, K, V, pr, g, SCALE, H, drop, SEED, gq, gk, gv, gb, ds, what=what, ratios=each, bf16=kind == "bf16")
    print(f"{what}: worst err / bound " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))


# ---- 2. P is the undropped call's, and p = 0 is the undropped call

def _undropped(p, a, Q, K, V, b, g, H, kind):
    """(Out, P, gQ, gK, gV, gBias or None, ds) of the undropped entry points on the same operands."""
    Qd, Kd, Vd, gd = (_rows(x, kind) for x in (Q, K, V, g))
    pd, work = (torch.full((a.nnz, H), SENTINEL, device="cuda") for _ in range(2))
    o = _filled((a.m, Q.shape[1]), kind)
    if b is None:
        if kind == "bf16":
            p.attention_bf16(Qd, Kd, Vd, SCALE, heads=H, out=o, p=pd)
            grads = p.attention_bf16_backward(Qd, Kd, Vd, pd, gd, SCALE, heads=H, work=work) + (None,)
        else:
            p.attention(Qd, Kd, Vd, SCALE, out=o, p=pd if H > 1 else pd.view(-1), heads=H)
            grads = p.attention_backward(Qd, Kd, Vd, pd if H > 1 else pd.view(-1), gd, SCALE, work=work if H > 1 else work.view(-1), heads=H) + (None,)
    else:
        fwd, bwd = (p.attention_bf16_bias, p.attention_bf16_bias_backward) if kind == "bf16" else (p.attention_bias, p.attention_bias_backward)
        fwd(Qd, Kd, Vd, _dev(b), SCALE, heads=H, out=o, p=pd)
        grads = bwd(Qd, Kd, Vd, pd, gd, SCALE, heads=H, work=work)
    return (_host(o), _host(pd)) + tuple(None if t is None else _host(t) for t in grads) + (_host(work),)


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,k,H", [("thresholds_lifted", 48, 3), ("long_rows", 128, 8), ("directed_empty", 64, 1), ("thresholds_lifted", 1024, 64)])
def test_p_is_the_undropped_calls_and_p_zero_is_the_undropped_call(name, k, H, kind, bias):
    a, Q, K, V, b, g = case_operands(name, k, H, kind == "bf16", bias)
    p = plan(name, k)
    plain = _undropped(p, a, Q, K, V, b, g, H, kind)
    pr = _run((name, k, H, kind, bias, 0.5))[1]
    # one head, fp32, no bias: the undropped entry point forwards to the single-head kernels, whose reduction tree is another one; the
    # dropout call runs the per-head kernels there (as the bf16 and bias calls do), so only p = 0, which forwards too, has those bits
    assert (H == 1 and kind == "fp32" and not bias) or _same_bits(pr, plain[1]), f"P differs from the undropped call's in {int((pr.view(np.uint32) != plain[1].view(np.uint32)).sum())} entries"
    out0, p0 = _forward(p, a, Q, K, V, b, H, kind, 0.0)
    zero = (out0, p0) + _backward(p, a, Q, K, V, p0, g, H, kind, 0.0, want=(True, True, True, bias))
    for key, x, y in zip(("out", "p", "gq", "gk", "gv", "gb", "ds"), zero, plain):
        assert (x is None and y is None) or _same_bits(x, y), f"p = 0: {key} differs from the undropped entry point's"


# ---- 3. one mask in all three launches, and it is flex_dropout_mask

@pytest.mark.parametrize("kind", KINDS)
def test_the_three_launches_and_flex_dropout_mask_agree_on_every_bit(kind):
    """Every column has exactly one entry (col(e) = e) and row r has r + 1 entries, r < d: slot rows and wave rows.  Q = K = 0, so alpha
    is 1 / len; V is one-hot: entry e, the j-th of its row, holds 1 at column j of every head, so Out[r, h d + j] is alpha w of that entry
    and head alone; g = 1, so gV[e, head h] is alpha w in every column of the head."""
    k, H = 1024, 4
    d = k // H
    lens = np.arange(1, d + 1)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    nnz = int(rp[-1])
    a = binding.HostCsr(rp, np.arange(nnz, dtype=np.uint32), np.ones(nnz, np.float32), n=nnz)
    p = flex_amd.Plan(a, k, attention=True, attention_backward=True)
    row = np.repeat(np.arange(d), lens)
    j = np.arange(nnz) - rp[:-1].astype(np.int64)[row]
    dt = torch.bfloat16 if kind == "bf16" else torch.float32
    Vd = torch.zeros((nnz, k), dtype=dt, device="cuda")
    e_t, j_t = torch.arange(nnz, device="cuda"), torch.from_numpy(j).cuda()
    for h in range(H):
        Vd[e_t, h * d + j_t] = 1
    Qd, Kd, gd = torch.zeros((d, k), dtype=dt, device="cuda"), torch.zeros((nnz, k), dtype=dt, device="cuda"), torch.ones((d, k), dtype=dt, device="cuda")
    pd = torch.empty((nnz, H), device="cuda")
    fwd, bwd = (p.attention_bf16_dropout, p.attention_bf16_dropout_backward) if kind == "bf16" else (p.attention_dropout, p.attention_dropout_backward)
    for drop in (0.5, 0.9):
        out = fwd(Qd, Kd, Vd, SCALE, drop, SEED, heads=H, probs=pd)
        _, _, gv, _ = bwd(Qd, Kd, Vd, pd, gd, SCALE, drop, SEED, heads=H, want=(False, False, True, False))
        torch.cuda.synchronize()
        want = binding.dropout_mask(SEED, drop, 0, nnz * H).astype(bool).reshape(nnz, H)
        assert np.array_equal(want, ad.keep(SEED, drop, np.arange(nnz * H, dtype=np.uint64)).reshape(nnz, H))
        out_nz = (out.float() != 0).cpu().numpy().reshape(d, H, d)
        gv_nz = (gv.float() != 0).view(nnz, H, d)
        assert bool((gv_nz.all(2) == gv_nz.any(2)).all()), "gV: a head of an entry is zero in all of its columns or in none"
        gv_keep = gv_nz.any(2).cpu().numpy()
        fwd_keep = out_nz[row, :, j]
        tail = np.arange(d)[None, :] >= lens[:, None]  # columns past the row's entries stay 0
        assert not out_nz.transpose(0, 2, 1)[tail].any()
        assert np.array_equal(fwd_keep, want), f"p={drop}: the forward's mask differs from flex_dropout_mask in {int((fwd_keep != want).sum())} bits"
        assert np.array_equal(gv_keep, want), f"p={drop}: the column launch's mask differs from flex_dropout_mask in {int((gv_keep != want).sum())} bits"
        # the row backward: ds = scale p (da - delta) with da = w d (g = 1, V one-hot summed over the head: <g, V> = 1)
        work = torch.empty((nnz, H), device="cuda")
        bwd(Qd, Kd, Vd, pd, gd, SCALE, drop, SEED, heads=H, work=work, want=(True, False, False, False))
        ds = _host(work).astype(np.float64)
        al, c = 1.0 / lens[row], ad.factor(drop)
        da = want * c
        delta = np.zeros((d, H))
        np.add.at(delta, row, al[:, None] * da)
        ref = SCALE * al[:, None] * (da - delta[row])
        assert np.all(np.abs(ds - ref) <= 1e-5 * c), f"p={drop}: the row backward's mask differs"
    p.destroy()


# ---- 4. non-finite V behind dropped entries

@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_non_finite_v_row_behind_dropped_entries_reaches_nothing(kind, bias):
    name, k, H, drop = "thresholds_lifted", 32, 4, 0.5
    a = graph(name)
    d = k // H
    Q, K, V, b = ab.operands(["uniform4"] * H, a, k, seed=12, bf16=kind == "bf16")
    b = b if bias else None
    g = grad(a, k, 12, kind == "bf16")
    p = plan(name, k)
    row, col, rp = ab.coo(a)
    kp = ad.kept_entries(a, H, drop, SEED)
    Vbad, hit = V.copy(), 0
    for h in range(H):
        any_kept = np.zeros(a.n, bool)
        any_kept[col[kp[:, h]]] = True
        cols = np.flatnonzero(~any_kept & (np.bincount(col, minlength=a.n) > 0))  # columns with entries, all of them dropped in head h
        Vbad[cols[0::2], h * d:(h + 1) * d] = np.inf
        Vbad[cols[1::2], h * d:(h + 1) * d] = np.nan
        hit += len(cols)
    assert hit >= 8 * H

    def run(Vx):
        out, pr = _forward(p, a, Q, K, Vx, b, H, kind, drop)
        return (out, pr) + _backward(p, a, Q, K, Vx, pr, g, H, kind, drop, want=(True, True, True, bias))

    clean, dirty = run(V), run(Vbad)
    for key, x, y in zip(("out", "p", "gq", "gk", "gv", "gb", "ds"), clean, dirty):
        if x is None:
            continue
        val = bf.from_bf16(y) if y.dtype == np.uint16 else y
        assert np.isfinite(val).all(), f"{key} is not finite"
        assert _same_bits(x, y), f"{key} changed with the V rows behind dropped entries"
    # a head of a row whose entries are all dropped is +0 bits in Out; the other heads hold what the checker holds them to
    out = clean[0]
    dead = 0
    for h in range(H):
        any_kept = np.zeros(a.m, bool)
        any_kept[row[kp[:, h]]] = True
        rows = np.flatnonzero(~any_kept & (np.diff(rp) > 0))
        dead += len(rows)
        assert not np.ascontiguousarray(out[rows, h * d:(h + 1) * d]).view(np.uint8).any()
    assert dead >= H
    ad.check(a, Q, K, Vbad, b, SCALE, H, drop, SEED, dirty[0], dirty[1], what="non-finite V", bf16=kind == "bf16")


# ---- 5. output invariants

@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("kind", KINDS)
def test_without_p_the_same_out_and_every_gradient_has_the_same_bits_whichever_others_are_asked_for(kind, bias):
    c = ("thresholds_lifted", 48, 3, kind, bias, 0.5)
    name, k, H = c[:3]
    a, Q, K, V, b, g = case_operands(name, k, H, kind == "bf16", bias)
    p = plan(name, k)
    out, pr, *full = _run(c)
    assert _same_bits(_forward(p, a, Q, K, V, b, H, kind, 0.5, with_p=False)[0], out)
    for mask in range(1, 16 if bias else 8):
        want = tuple(bool(mask >> i & 1) for i in range(4))
        got = _backward(p, a, Q, K, V, pr, g, H, kind, 0.5, want=want)
        for i in range(4):
            assert (got[i] is None) if not want[i] else _same_bits(got[i], full[i]), (want, i)
        if want[0] or want[1] or want[3]:
            assert _same_bits(got[4], full[4]), want
        else:
            assert np.all(got[4] == SENTINEL), want  # gV alone: the rows' launch is skipped and dWork is not written
    other = _forward(p, a, Q, K, V, b, H, kind, 0.5, seed=SEED + 1)
    assert not _same_bits(other[0], out) and _same_bits(other[1], pr)  # another seed: another Out, the same P


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("kind", KINDS)
def test_two_runs_and_a_captured_graph_give_the_same_bits(kind, bias):
    c = ("long_rows", 128, 8, kind, bias, 0.5)
    name, k, H = c[:3]
    a, Q, K, V, b, g = case_operands(name, k, H, kind == "bf16", bias)
    p = plan(name, k)
    first = _run(c)
    out2, pr2 = _forward(p, a, Q, K, V, b, H, kind, 0.5)
    again = (out2, pr2) + _backward(p, a, Q, K, V, pr2, g, H, kind, 0.5, want=(True, True, True, bias))
    for x, y in zip(first, again):
        assert (x is None and y is None) or _same_bits(x, y)
    Qd, Kd, Vd, gd = _rows(Q, kind), _rows(K, kind), _rows(V, kind), _rows(g, kind)
    bd = None if b is None else _dev(b)
    o, pd, work, gb = _filled((a.m, k), kind), *(torch.empty((a.nnz, H), device="cuda") for _ in range(3))
    gq, gk, gv = _filled((a.m, k), kind), _filled((a.n, k), kind), _filled((a.n, k), kind)
    fwd, bwd = (p.attention_bf16_dropout, p.attention_bf16_dropout_backward) if kind == "bf16" else (p.attention_dropout, p.attention_dropout_backward)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=side):  # one stream: the three launches are a chain
        fwd(Qd, Kd, Vd, SCALE, 0.5, SEED, heads=H, bias=bd, out=o, probs=pd)
        bwd(Qd, Kd, Vd, pd, gd, SCALE, 0.5, SEED, heads=H, grad_q=gq, grad_k=gk, grad_v=gv, grad_bias=gb if bias else None, work=work,
            want=(True, True, True, bias))
    for t in (pd, work, gb):
        t.fill_(SENTINEL)
    for t in (o, gq, gk, gv):
        t.copy_(_filled(tuple(t.shape), kind))
    graph_.replay()
    for x, t in zip(first, (o, pd, gq, gk, gv, gb, work)):
        assert x is None or _same_bits(x, _host(t))


# ---- 6. refusals

@pytest.mark.parametrize("kind", KINDS)
def test_refused_calls_leave_the_outputs_untouched(kind):
    name, k = "directed_empty", 32
    a, p = graph(name), plan(name, k)
    es = 2 if kind == "bf16" else 4  # bytes of a row element
    dt = torch.bfloat16 if kind == "bf16" else torch.float32
    s = torch.cuda.current_stream().cuda_stream
    names = ("attention_bf16_dropout_ptr", "attention_bf16_dropout_backward_ptr") if kind == "bf16" else ("attention_dropout_ptr", "attention_dropout_backward_ptr")

    def calls(pl, H, kk, drop=0.5, shift=0, work=1, gbias=2, grad_shift=0, scale=SCALE):
        """(forward, backward, untouched) through the pointer forms; edge arrays: 0 = P, 1 = Work, 2 = gBias."""
        f_ptr, b_ptr = getattr(pl, names[0]), getattr(pl, names[1])
        Qd = torch.zeros((a.m * kk + 8,), dtype=dt, device="cuda")
        Kd, Vd, gd = (torch.zeros((r, kk), dtype=dt, device="cuda") for r in (a.n, a.n, a.m))
        outs = [_filled((r * kk + 8,), kind) for r in (a.m, a.m, a.n, a.n)]
        edge = [torch.full((a.nnz * max(H, 1) + 2,), SENTINEL, device="cuda") for _ in range(3)]
        bd = torch.zeros((a.nnz * max(H, 1) + 2,), device="cuda")
        fwd = lambda: f_ptr(Qd.data_ptr() + shift, Kd.data_ptr(), Vd.data_ptr(), bd.data_ptr(), scale, drop, SEED, outs[0].data_ptr(),
                            edge[0].data_ptr(), s, heads=H)
        bwd = lambda: b_ptr(Qd.data_ptr() + shift, Kd.data_ptr(), Vd.data_ptr(), edge[0].data_ptr(), gd.data_ptr(), scale, drop, SEED,
                            outs[1].data_ptr(), outs[2].data_ptr() + grad_shift, outs[3].data_ptr(), edge[gbias].data_ptr(), edge[work].data_ptr(), s,
                            heads=H)
        untouched = lambda: all(_is_fill(_host(t)) for t in outs) and all(_is_fill(_host(t)) for t in edge)
        return fwd, bwd, untouched

    def refused(pl, H, kk, match, **kw):
        fwd, bwd, untouched = calls(pl, H, kk, **kw)
        for f in (fwd, bwd):
            with pytest.raises(binding.FlexError, match=match):
                f()
        assert untouched()

    for bad in (1.0, -0.25, 1.5, float("nan"), float("inf"), -float("inf")):     # p outside [0, 1)
        refused(p, 4, k, "invalid", drop=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):                          # the scale check beside it
        refused(p, 4, k, "invalid", scale=bad)
    refused(p, 0, k, "invalid")
    refused(p, 3, k, "not supported")                                             # 3 does not divide 32
    refused(plan(name, 24), 2, 24, "not supported")                               # d = 12
    refused(plan(name, 1024), 2, 1024, "not supported")                           # d = 512
    refused(plan(name, 48), 1, 48, "not supported")                               # one head is served here: d = 48 is no power of two
    refused(plan(name, 48), 1, 48, "not supported", drop=0.0)                     # and p = 0 refuses what p > 0 refuses
    refused(plan(name, k, ldb=34, ldc=36), 4, 36, "not supported")                # an odd stride: ldb % 4 != 0
    refused(p, 4, k, "not supported", shift=es)                                   # Q aligned as one element only
    refused(p, 4, k, "not supported", shift=2 * es, drop=0.0)                     # half the vector, at p = 0 as well
    fwd, bwd, untouched = calls(p, 4, k, grad_shift=2 * es)                       # an output of the backward misaligned
    with pytest.raises(binding.FlexError, match="not supported"):
        bwd()
    assert untouched()
    refused(flex_amd.Plan(a, k), 4, k, "invalid")                                 # the wrong kind of plan: no FLEX_PLAN_ATTENTION
    fwd, bwd, untouched = calls(plan(name, k, attention_backward=False), 4, k)    # the forward's flag alone
    fwd()
    with pytest.raises(binding.FlexError, match="invalid"):
        bwd()
    for kw in (dict(work=0), dict(gbias=0), dict(gbias=1)):                       # dWork == dP, gBias == dP, gBias == dWork
        fwd, bwd, untouched = calls(p, 4, k, **kw)
        with pytest.raises(binding.FlexError, match="invalid"):
            bwd()
        assert untouched()
    empty = binding.HostCsr(np.zeros(41, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=17)
    pe = flex_amd.Plan(empty, k, attention=True, attention_backward=True)
    getattr(pe, names[0])(None, None, None, None, 1.0, 0.5, SEED, None, heads=4)  # no entries: no launch, nothing read
    getattr(pe, names[1])(None, None, None, None, None, 1.0, 0.5, SEED, None, None, None, None, None, heads=4)


# ---- 7. a row-range shard, forward

@pytest.mark.parametrize("kind", KINDS)
def test_a_shard_takes_the_bias_and_the_mask_at_the_entries_of_the_whole_matrix(kind):
    name, k, H, drop = "long_rows", 32, 4, 0.5
    a = graph(name)
    Q, K, V, bias = ab.operands(ab.scenarios_of(H, shift=3), a, k, seed=9, bf16=kind == "bf16")
    whole, whole_p = _forward(plan(name, k), a, Q, K, V, bias, H, kind, drop)
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
        own = np.full((a.nnz, H), np.nan, np.float32)  # NaN outside the shard: a shard that read another's bias would be poisoned
        own[e0:e1] = bias[e0:e1]
        out, pd = _filled((a.m, k), kind), torch.full((a.nnz, H), SENTINEL, device="cuda")
        f_ptr = shard.attention_bf16_dropout_ptr if kind == "bf16" else shard.attention_dropout_ptr
        ownd = _dev(own)
        f_ptr(Qd.data_ptr() + es * k * r0, Kd.data_ptr(), Vd.data_ptr(), ownd.data_ptr(), SCALE, drop, SEED, out.data_ptr() + es * k * r0, pd.data_ptr(), s,
              heads=H)
        out, pd = _host(out), _host(pd)
        assert _is_fill(out[:r0]) and _is_fill(out[r1:]), (r0, r1)
        assert np.all(pd[:e0] == SENTINEL) and np.all(pd[e1:] == SENTINEL), (r0, r1)
        if r1 > r0:
            ad.check(a, Q[r0:r1], K, V, bias, SCALE, H, drop, SEED, out[r0:r1], pd[e0:e1], rows=(r0, r1), what=f"rows [{r0}, {r1})", bf16=kind == "bf16")
        union[r0:r1], union_p[e0:e1] = out[r0:r1], pd[e0:e1]
        shard.destroy()
    assert _same_bits(union, whole) and _same_bits(union_p, whole_p)


# ---- 8. autograd

@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,H", [(32, 4), (128, 8)])
def test_the_operator_with_dropout_and_its_gradients_against_float64(k, H, kind, bias):
    """Against float64 torch autograd with the numpy mask as a constant.  Tolerance: attention_bias_ref.propagated_bounds of the
    undropped step (the backward starts from the forward's fp32 alpha) times 2 c: every term of those bounds is linear in |V|, |da| or
    dda of an entry, which dropout multiplies by w <= c, and the one more rounding per count (gamma(n + 1) for gamma(n), n >= 1) at most
    doubles a term.  The operator's outputs are also held to the plan's own calls bit for bit, which test 1 holds to the tight bounds."""
    a = _directed(300, seed=6, dup=True)
    d, drop, seed = k // H, 0.6, SEED ^ 0x55
    rng = np.random.default_rng([k, H, 24])
    Q, K, V, gOut = (rng.uniform(-1, 1, (r, k)).astype(np.float32) for r in (a.m, a.n, a.n, a.m))
    if kind == "bf16":
        Q, K, V, gOut = (bf.rounded(x) for x in (Q, K, V, gOut))
    b = rng.uniform(-4, 4, (a.nnz, H)).astype(np.float32) if bias else None
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    Qd, Kd, Vd = (_rows(x, kind).requires_grad_() for x in (Q, K, V))
    bd = _dev(b).requires_grad_() if bias else None
    plain_before = _host(op.attention(Qd.detach(), Kd.detach(), Vd.detach(), heads=H, bias=None if bd is None else bd.detach()))
    out = op.attention(Qd, Kd, Vd, heads=H, bias=bd, dropout=drop, seed=seed)  # the default scale: d ** -0.5
    out.backward(_rows(gOut, kind))
    dt = torch.bfloat16 if kind == "bf16" else torch.float32
    assert all(t.dtype == dt for t in (out, Qd.grad, Kd.grad, Vd.grad))
    got = tuple(_host(t) for t in (out.detach(), Qd.grad, Kd.grad, Vd.grad)) + ((_host(bd.grad),) if bias else (None,))
    scale = d ** -0.5
    kp, c = ad.kept_entries(a, H, drop, seed), ad.factor(drop)
    want = ad.torch_float64(a, Q, K, V, b, scale, H, gOut, kp, c)
    tols = ab.propagated_bounds(a, Q, K, V, b if bias else np.zeros((a.nnz, H), np.float32), scale, H, gOut)
    worst = 0.0
    for what, x, ref, tol in zip(("Out", "grad_Q", "grad_K", "grad_V", "grad_bias"), got, want, tols):
        if x is None:
            continue
        tol = 2 * c * tol
        if x.dtype == np.uint16:  # the propagated bound, then the one rounding to bf16
            x, tol = bf.from_bf16(x), bf.bound_bf16(ref, tol)
        err = np.abs(x.astype(np.float64) - ref)
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), f"{what} k={k} H={H} {kind}: worst err / tolerance {float((err / tol).max()):.3g}"
    print(f"k={k} H={H} {kind} {'bias' if bias else 'nobias'}: worst err / tolerance {worst:.3g}")
    # the plan's own calls give the same bits
    pd = torch.zeros((a.nnz, H), device="cuda")
    fwd, bwd = (op.plan.attention_bf16_dropout, op.plan.attention_bf16_dropout_backward) if kind == "bf16" else (op.plan.attention_dropout, op.plan.attention_dropout_backward)
    o2 = fwd(Qd.detach(), Kd.detach(), Vd.detach(), scale, drop, seed, heads=H, bias=None if bd is None else bd.detach(), probs=pd)
    g2 = bwd(Qd.detach(), Kd.detach(), Vd.detach(), pd, _rows(gOut, kind), scale, drop, seed, heads=H, want=(True, True, True, bias))
    for x, t in zip(got, (o2,) + tuple(g2)):
        assert (x is None and t is None) or _same_bits(x, _host(t))
    # dropout=0 and training=False take the paths they took before: the same bits
    for kw in (dict(dropout=0.0), dict(dropout=drop, training=False), dict(dropout=0.0, seed=3)):
        assert _same_bits(_host(op.attention(Qd.detach(), Kd.detach(), Vd.detach(), heads=H, bias=None if bd is None else bd.detach(), **kw)), plain_before)
    # seed=None draws from torch's default generator: torch.manual_seed reproduces a run, and the next draw differs
    torch.manual_seed(11)
    x1 = _host(op.attention(Qd.detach(), Kd.detach(), Vd.detach(), heads=H, dropout=drop))
    x2 = _host(op.attention(Qd.detach(), Kd.detach(), Vd.detach(), heads=H, dropout=drop))
    torch.manual_seed(11)
    assert _same_bits(_host(op.attention(Qd.detach(), Kd.detach(), Vd.detach(), heads=H, dropout=drop)), x1) and not _same_bits(x1, x2)

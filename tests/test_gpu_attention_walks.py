"""The fused-attention kernels on walks whose group budget is above the floor of 64 (internal.h: attention_group_budget), where a wave runs
several items of its group one after the other, and on unsorted rows with repeated (row, column) pairs.  Every family: the single head
(16-byte and generic form), heads, GAT, bf16, the bias in fp32 and bf16, and dropout in fp32 and bf16 with and without the bias; forward,
row backward and column backward.

  (a) budget 128: walk_graph(1) (tests/attention_walk_graphs.py: 70 000 rows and columns, 213 658 entries, every class of row and of
      column) against float64 on every element of Out, P, gQ, gK, gV, ds and gBias (GAT: gEl, gEr, dx), with the family's own reference,
      bounds and checker and a scenario per head.
  (b) budgets 512 and 2048: 7 and 30 copies of that graph on the diagonal with the operands repeated.  A slot row is owned by one slot,
      a wave or block line by one wave or workgroup, a column's sum takes its entries in CSR order, and the items do not depend on the
      budget, only their packing into groups does: every copy's block of every output has the bits of the one-copy run, which (a) holds
      to float64.  Outputs start at a sentinel; lines without entries are +0.  No output was found that is not bit-stable.
  (c) dropout at budget 512: the mask is a hash of the entry's index in the whole graph, so the copies differ; P (undropped) copy by
      copy, everything else against float64 over the 1 495 606 entries.
  (d) thresholds_lifted with shuffled rows and a tenth of its entries repeated: every family against float64 on every element, the bias
      of a repeated entry differing between its copies, and SparseOperator.attention with a bias against float64 torch autograd.
  (e) the forward and backward of the heads at budget 512 in a captured graph, and without P.

Left out: the two- and four-slab forms (k > 256): slabs do not change the walk, and their float64 reference at 213 658 entries is what
would make a test slow.  For the same reason (a) runs W = 4 and W = 8 in every family (k = 8 and k = 32, the generic form at k = 30) and
W = 16 in the heads alone ((64, 4): 7.5 items per group); the other pairs that were meant for it -- k = 64 elsewhere, k = 128 and 256
everywhere, dropout's (128, 8) -- are cut, widest first, to keep the file within twice the time of tests/test_gpu_attention_dropout.py
(profiles/attention_walks_gpu_tests.txt).  W = 16 and W = 64 of every family run in (b), where the one-copy run they
are compared with is not held to float64 in this file.  There is no dropout case at 30 copies (the clamp).

The table of the cases, their declared budgets and items per group, and the models of the faults these checks must catch are in
tests/test_attention_walks_host.py."""
import zlib

import numpy as np
import pytest

import attention_bf16_ref as bf
import attention_bias_ref as ab
import attention_dropout_ref as ad
import flex_amd
import fused_attention_backward_ref as fb
import fused_attention_ref as fa
import gat_attention_ref as gat
import multihead_attention_ref as mh
from attention_walk_graphs import BUDGETS, multi_edge_graph, tile_rows, walk_graph
from test_attention_walks_host import (A_PAIRS, B_PAIRS, DROP, DROPOUT_FAMILIES, FAMILIES, MULTI_EDGE_PAIRS, SCALE, SEED, check_copies, is_bf16, leading,
                                       operands, shift_of)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FILL = 0x5A5A  # bf16 bits no test computes; fp32 rows and edge arrays start at SENTINEL
SENTINEL = -12345.5
SLOPE = gat.SLOPE
_plans, _digests = {}, {}


def graph_of(which):
    return multi_edge_graph()[0] if which == "multi" else walk_graph(which)


def plan(which, k, ldb=None, ldc=None):
    """The plan of walk_graph(which) (which = "multi": the multi-edge graph), held to the budget its cases declare."""
    key = (which, k, ldb, ldc)
    if key not in _plans:
        p = flex_amd.Plan(graph_of(which), k, attention=True, attention_backward=True, ldb=ldb or k, ldc=ldc or k)
        p.self_check()
        want = 64 if which == "multi" else BUDGETS[which]
        assert p.attention_info()["group_budget"] == p.attention_backward_info()["group_budget"] == want, (key, p.attention_info())
        _plans[key] = p
    return _plans[key]


def _dev(x, b16=False):
    if b16:
        return torch.from_numpy(bf.to_bf16(x).view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def to_dev(family, o):
    """The host operands on the device: the row operands of a bf16 family as bfloat16, everything else float32."""
    return {key: _dev(x, is_bf16(family) and key in ("Q", "K", "V", "g")) for key, x in o.items()}


def _host(t):
    """float32 tensors as they are, bfloat16 ones as their bits (uint16)"""
    torch.cuda.synchronize()
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.cpu().numpy()


def to_host(got):
    return {key: None if t is None else _host(t) for key, t in got.items()}


def _filled(shape, b16=False):
    if b16:
        return torch.full(shape, FILL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return torch.full(shape, SENTINEL, device="cuda")


def _single_generic(p, a, d, k, ldb, ldc):
    """flex_attention and flex_attention_backward on rows that lie ldb (K, V, gK, gV) or ldc (Q, Out, g, gQ) floats apart in NaN-filled
    buffers: the dense [rows, k] outputs, after the cells past k were seen to be NaN still."""
    def embed(x, ld):
        t = torch.full((x.shape[0], ld), float("nan"), device="cuda")
        t[:, :k] = x
        return t
    Q, K, V, g = embed(d["Q"], ldc), embed(d["K"], ldb), embed(d["V"], ldb), embed(d["g"], ldc)
    out, gq, gk, gv = (torch.full((rows, ld), float("nan"), device="cuda") for rows, ld in ((a.m, ldc), (a.m, ldc), (a.n, ldb), (a.n, ldb)))
    pd, work = torch.full((a.nnz,), SENTINEL, device="cuda"), torch.full((a.nnz,), SENTINEL, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    p.attention_ptr(Q.data_ptr(), K.data_ptr(), V.data_ptr(), SCALE, out.data_ptr(), pd.data_ptr(), s)
    p.attention_backward_ptr(Q.data_ptr(), K.data_ptr(), V.data_ptr(), pd.data_ptr(), g.data_ptr(), SCALE, gq.data_ptr(), gk.data_ptr(), gv.data_ptr(),
                             work.data_ptr(), s)
    for t in (out, gq, gk, gv):
        assert bool(torch.isnan(t[:, k:]).all()), "a cell past k was written"
    return dict(out=out[:, :k].contiguous(), p=pd, gq=gq[:, :k].contiguous(), gk=gk[:, :k].contiguous(), gv=gv[:, :k].contiguous(), ds=work)


def run(family, p, a, d, k, H, with_p=True):
    """The forward and the backward (every gradient) of a family on plan p and the device operands d: a dict of device tensors.  Every
    output starts at its fill.  with_p=False: the forward alone, without P."""
    b16 = is_bf16(family)
    if family == "single_generic":
        return _single_generic(p, a, d, k, *leading(family, k))
    edge = (lambda: torch.full((a.nnz,), SENTINEL, device="cuda")) if family == "single" else (lambda: torch.full((a.nnz, H), SENTINEL, device="cuda"))
    out, pd = _filled((a.m, k), b16), (edge() if with_p else None)
    if family == "gat":
        p.gat_attention(d["el"], d["er"], d["V"], SLOPE, out=out, p=pd)
    elif family in ("single", "heads"):
        p.attention(d["Q"], d["K"], d["V"], SCALE, out=out, p=pd, heads=H)
    elif family == "bf16":
        p.attention_bf16(d["Q"], d["K"], d["V"], SCALE, heads=H, out=out, p=pd)
    elif family.startswith("bias"):
        (p.attention_bf16_bias if b16 else p.attention_bias)(d["Q"], d["K"], d["V"], d["bias"], SCALE, heads=H, out=out, p=pd)
    else:
        (p.attention_bf16_dropout if b16 else p.attention_dropout)(d["Q"], d["K"], d["V"], SCALE, DROP, SEED, heads=H, bias=d.get("bias"), out=out, probs=pd)
    if not with_p:
        return dict(out=out)
    work, gv = edge(), _filled((a.n, k), b16)
    if family == "gat":
        gel, ger = _filled((a.m, H)), _filled((a.n, H))
        p.gat_attention_backward(d["el"], d["er"], d["V"], pd, d["g"], SLOPE, grad_el=gel, grad_er=ger, grad_v=gv, work=work)
        return dict(out=out, p=pd, gel=gel, ger=ger, gv=gv, ds=work)
    gq, gk = _filled((a.m, k), b16), _filled((a.n, k), b16)
    grads = dict(grad_q=gq, grad_k=gk, grad_v=gv, work=work)
    got = dict(out=out, p=pd, gq=gq, gk=gk, gv=gv, ds=work)
    if family in ("single", "heads"):
        p.attention_backward(d["Q"], d["K"], d["V"], pd, d["g"], SCALE, heads=H, **grads)
    elif family == "bf16":
        p.attention_bf16_backward(d["Q"], d["K"], d["V"], pd, d["g"], SCALE, heads=H, **grads)
    elif family.startswith("bias"):
        got["gb"] = edge()
        (p.attention_bf16_bias_backward if b16 else p.attention_bias_backward)(d["Q"], d["K"], d["V"], pd, d["g"], SCALE, heads=H, grad_bias=got["gb"], **grads)
    else:
        got["gb"] = edge() if "bias" in d else None
        (p.attention_bf16_dropout_backward if b16 else p.attention_dropout_backward)(
            d["Q"], d["K"], d["V"], pd, d["g"], SCALE, DROP, SEED, heads=H, grad_bias=got["gb"], want=(True, True, True, "bias" in d), **grads)
    return got


def check64(family, a, o, H, got, what):
    """Every output of a run (on the host) against the float64 reference, the bounds and the checker of the family's own GPU file;
    the worst err / bound of each output."""
    each = {}
    b16 = is_bf16(family)
    if family.startswith("single"):
        each["out/p"] = fa.check(a, o["Q"], o["K"], o["V"], SCALE, got["out"], got["p"], what=what)
        fb.check(a, o["Q"], o["K"], o["V"], got["p"], o["g"], SCALE, got["gq"], got["gk"], got["gv"], got["ds"], what=what, ratios=each)
    elif family == "heads":
        each["out/p"] = mh.check(a, o["Q"], o["K"], o["V"], SCALE, H, got["out"], got["p"], what=what)
        mh.check_backward(a, o["Q"], o["K"], o["V"], got["p"], o["g"], SCALE, H, got["gq"], got["gk"], got["gv"], got["ds"], what=what, ratios=each)
    elif family == "gat":
        each["out/p"] = gat.check(a, o["el"], o["er"], o["V"], SLOPE, got["out"], got["p"], what=what)
        gat.check_backward(a, o["el"], o["er"], o["V"], got["p"], o["g"], SLOPE, got["gel"], got["ger"], got["gv"], got["ds"], what=what, ratios=each)
    elif family == "bf16":
        bf.check(a, o["Q"], o["K"], o["V"], SCALE, H, got["out"], got["p"], what=what, ratios=each)
        bf.check_backward(a, o["Q"], o["K"], o["V"], got["p"], o["g"], SCALE, H, got["gq"], got["gk"], got["gv"], got["ds"], what=what, ratios=each)
    elif family.startswith("bias"):
        ab.check(a, o["Q"], o["K"], o["V"], o["bias"], SCALE, H, got["out"], got["p"], what=what, ratios=each, bf16=b16)
        ab.check_backward(a, o["Q"], o["K"], o["V"], got["p"], o["g"], SCALE, H, got["gq"], got["gk"], got["gv"], got["gb"], got["ds"], what=what, ratios=each,
                          bf16=b16)
    else:
        ad.check(a, o["Q"], o["K"], o["V"], o.get("bias"), SCALE, H, DROP, SEED, got["out"], got["p"], what=what, ratios=each, bf16=b16)
        ad.check_backward(a, o["Q"], o["K"], o["V"], got["p"], o["g"], SCALE, H, DROP, SEED, got["gq"], got["gk"], got["gv"], got["gb"], got["ds"], what=what,
                          ratios=each, bf16=b16)
    print(f"{what}: worst err / bound " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))
    return each


def _digest(got):
    return {key: zlib.crc32(np.ascontiguousarray(x).tobytes()) for key, x in got.items() if x is not None}


def _ids(cases):
    return [f"{c[0]}-k{c[1]}-h{c[2]}" + (f"-T{c[3]}" if len(c) > 3 else "") for c in cases]


# ---- (a) budget 128 against float64, every element

A_CASES = [(f, k, H) for f, pairs in A_PAIRS.items() for k, H in pairs]


@pytest.mark.parametrize("family,k,H", A_CASES, ids=_ids(A_CASES))
def test_budget_128_every_output_against_float64(family, k, H):
    a = walk_graph(1)
    o = operands(family, k, H, a, shift_of(family, k, H))
    got = to_host(run(family, plan(1, k, *leading(family, k)) if family == "single_generic" else plan(1, k), a, to_dev(family, o), k, H))
    _digests[(family, k, H)] = _digest(got)
    check64(family, a, o, H, got, f"budget 128 {family} k={k} H={H}")


# ---- (b) budgets 512 and 2048 by copies, bit for bit

B_CASES = [(f, k, H, 7) for f in FAMILIES for k, H in B_PAIRS[f]] + [(f, *B_PAIRS[f][0], 30) for f in FAMILIES]


def _tiled(d, T):
    return {key: t.repeat((T,) + (1,) * (t.dim() - 1)) for key, t in d.items()}


@pytest.mark.parametrize("family,k,H,T", B_CASES, ids=_ids(B_CASES))
def test_every_copy_has_the_bits_of_the_one_copy_run(family, k, H, T):
    """No output is exempt: Out, P, gQ, ds and gBias (gEl) are owned by the slot, wave or workgroup of their row, gK, gV (gEr) by that of
    their column, summed in CSR order, and a copy's rows, columns and entries keep their order."""
    a = walk_graph(1)
    o = operands(family, k, H, a, shift_of(family, k, H))
    d = to_dev(family, o)
    base = run(family, plan(1, k), a, d, k, H)
    if (family, k, H) in _digests:  # the run that (a) held to float64
        assert _digest(to_host(base)) == _digests[(family, k, H)], "the one-copy run differs from run to run"
    got = run(family, plan(T, k), walk_graph(T), _tiled(d, T), k, H)
    torch.cuda.synchronize()
    check_copies(f"budget {BUDGETS[T]} {family} k={k} H={H}", a, got, base, T)


# ---- (c) dropout at budget 512

@pytest.mark.parametrize("family", DROPOUT_FAMILIES)
def test_dropout_at_budget_512_p_by_copies_and_the_rest_against_float64(family):
    """The mask is taken at the entry's index in the 7-copy graph, so Out and the gradients differ from copy to copy and are held to
    float64 over the whole graph (attention_dropout_ref, the mask restated from flex_dropout_mask's definition and held to it on the
    host); P is undropped and has the bits of the one-copy run.  No case at 30 copies."""
    T, k, H = 7, 8, 2
    a1, a = walk_graph(1), walk_graph(T)
    o1 = operands(family, k, H, a1, shift_of(family, k, H))
    d1 = to_dev(family, o1)
    base = run(family, plan(1, k), a1, d1, k, H)
    got = run(family, plan(T, k), a, _tiled(d1, T), k, H)
    check_copies(f"budget 512 {family}", a1, dict(p=got["p"]), dict(p=base["p"]), T)
    assert not torch.equal(got["out"][:a1.m], got["out"][a1.m:2 * a1.m])  # another mask in every copy
    kp = flex_amd.binding.dropout_mask(SEED, DROP, 0, a.nnz * H).astype(bool).reshape(a.nnz, H)
    assert np.array_equal(kp, ad.kept_entries(a, H, DROP, SEED))
    check64(family, a, {key: tile_rows(x, T) for key, x in o1.items()}, H, to_host(got), f"budget 512 {family} k={k} H={H}")


# ---- (d) unsorted rows and repeated (row, column) pairs

D_CASES = [(f, k, H) for f, pairs in MULTI_EDGE_PAIRS.items() for k, H in pairs]


@pytest.mark.parametrize("family,k,H", D_CASES, ids=_ids(D_CASES))
def test_unsorted_rows_and_repeated_entries_against_float64(family, k, H):
    """P, ds, gBias and the bias are per entry in the order given: the two copies of a repeated entry hold different biases, and the
    float64 check is per entry.  The references were held to independent torch evaluations on this graph on the host."""
    a, first = multi_edge_graph()
    o = operands(family, k, H, a, shift_of(family, k, H))
    got = to_host(run(family, plan("multi", k), a, to_dev(family, o), k, H))
    check64(family, a, o, H, got, f"multi-edge {family} k={k} H={H}")
    if "bias" in family:
        rep = np.flatnonzero(first != np.arange(a.nnz))
        b, other = o["bias"][rep], o["bias"][first[rep]]
        differ = np.isfinite(b) & np.isfinite(other) & (b != other)
        assert differ.mean() > 0.5
        p, p_other = got["p"][rep][differ], got["p"][first[rep]][differ]
        live = (p > 0) & (p_other > 0)
        assert live.sum() > 100 and (p[live] != p_other[live]).mean() > 0.99  # each copy of a repeated entry has the P of its own bias


def test_the_operator_with_a_bias_on_unsorted_rows_and_repeated_entries_against_float64_autograd():
    """SparseOperator.attention(..., heads=4, bias=b): tolerance attention_bias_ref.propagated_bounds, as tests/test_gpu_attention_bias.py
    has it on its sorted graph."""
    a, _ = multi_edge_graph()
    k, H = 32, 4
    d = k // H
    rng = np.random.default_rng([k, H, 25])
    Q, K, V, gOut = (rng.uniform(-1, 1, (r, k)).astype(np.float32) for r in (a.m, a.n, a.n, a.m))
    bias = rng.uniform(-4, 4, (a.nnz, H)).astype(np.float32)
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    Qd, Kd, Vd, bd = (_dev(x).requires_grad_() for x in (Q, K, V, bias))
    out = op.attention(Qd, Kd, Vd, heads=H, bias=bd)  # the default scale: d ** -0.5
    out.backward(_dev(gOut))
    got = tuple(_host(t) for t in (out.detach(), Qd.grad, Kd.grad, Vd.grad, bd.grad))
    scale = d ** -0.5
    want = ab.torch_float64(a, Q, K, V, bias, scale, H, gOut)
    tols = ab.propagated_bounds(a, Q, K, V, bias, scale, H, gOut)
    worst = 0.0
    for what, x, ref, tol in zip(("Out", "grad_Q", "grad_K", "grad_V", "grad_bias"), got, want, tols):
        err = np.abs(x.astype(np.float64) - ref)
        worst = max(worst, float((err / tol).max()))
        assert x.shape == ref.shape and np.all(err <= tol), f"{what}: worst err / tolerance {float((err / tol).max()):.3g}"
    print(f"multi-edge operator k={k} H={H}: worst err / tolerance {worst:.3g}")


# ---- (e) the captured graph and dP = NULL

def test_at_budget_512_a_captured_graph_and_a_forward_without_p_give_the_bits_of_the_eager_run():
    family, k, H, T = "heads", 8, 2, 7
    a1, a, p = walk_graph(1), walk_graph(T), plan(T, k)
    d = _tiled(to_dev(family, operands(family, k, H, a1, shift_of(family, k, H))), T)
    eager = run(family, p, a, d, k, H)
    assert torch.equal(run(family, p, a, d, k, H, with_p=False)["out"].view(torch.int32), eager["out"].view(torch.int32))
    out, gq, gk, gv = _filled((a.m, k)), _filled((a.m, k)), _filled((a.n, k)), _filled((a.n, k))
    pd, work = _filled((a.nnz, H)), _filled((a.nnz, H))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=side):  # one stream: the three launches are a chain
        p.attention(d["Q"], d["K"], d["V"], SCALE, out=out, p=pd, heads=H)
        p.attention_backward(d["Q"], d["K"], d["V"], pd, d["g"], SCALE, grad_q=gq, grad_k=gk, grad_v=gv, work=work, heads=H)
    for t in (out, gq, gk, gv, pd, work):
        t.fill_(SENTINEL)
    graph_.replay()
    torch.cuda.synchronize()
    for key, t in (("out", out), ("p", pd), ("gq", gq), ("gk", gk), ("gv", gv), ("ds", work)):
        assert torch.equal(t.view(torch.int32), eager[key].view(torch.int32)), f"{key}: the replay differs from the eager run"

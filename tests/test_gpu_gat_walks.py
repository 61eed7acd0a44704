"""The dropout and bf16 kernels of the fused GAT attention (flex::gat_dropout, flex::gat_bf16) on walks whose group budget is above the
floor of 64 (internal.h: attention_group_budget), where a wave runs several items of its group one after the other, and on unsorted
rows with repeated (row, column) pairs.  Each of these kernels holds a copy of its own of the loop over a group's items, which
tests/test_gpu_attention_walks.py (the undropped fp32 GAT calls) does not run.  Three families -- gat_dropout, gat_bf16 and
gat_bf16_dropout -- each with its forward, row backward and column backward; p = 0.5.

  (a) budget 128: walk_graph(1) (tests/attention_walk_graphs.py) against float64 on every element of Out, P, gEl, gEr, gV and dx with
      the family's own reference, bounds and checker and a scenario per head: W = 4 and W = 8 in every family, W = 16 in
      gat_bf16_dropout.
  (b) budgets 512 and 2048: 7 and 30 copies of that graph on the diagonal with the operands repeated.  gat_bf16: every copy's block of
      every output has the bits of the one-copy run, lines without entries +0; a slot row is owned by one slot, a wave or block line by
      one wave or workgroup, and a column's sum takes its entries in CSR order, so no output is exempt, and none was found that is not
      bit-stable.  The dropout families: the mask is a hash of the entry's index in the whole graph, so only P (undropped) has the bits
      of the one-copy run, and Out must differ between the copies; the forward alone is run.
  (c) dropout at budget 512: at (8, 2) P copy by copy, the mask against flex_dropout_mask, and every other output against float64 over
      the 1 495 606 entries; at (64, 8) the forward on the 7 copies with Out and P of the rows of copy 3 against float64, the mask taken
      at the entries of the whole matrix (the checkers' rows argument): the only independent check of the mask index at W = 16 on later
      items of a group.  The backward at that width under dropout is not held to float64 above budget 128.
  (d) thresholds_lifted with shuffled rows and a tenth of its entries repeated: every family against float64 per entry; under dropout
      the two copies of a repeated entry hold the same P and differ in the mask in about half of them; and
      SparseOperator.gat_attention on bfloat16 leaves with dropout against float64 torch autograd.
  (e) the forward and backward of gat_bf16_dropout at budget 512 in one captured graph, and a forward without P.

The table of the cases, their declared budgets and items per group, and the models of the faults these checks must catch are in
tests/test_gat_walks_host.py."""
import zlib

import numpy as np
import pytest

import attention_dropout_ref as ad
import flex_amd
import gat_attention_ref as gat
import gat_bf16_ref as gb
import gat_dropout_ref as gd
from attention_bf16_ref import bound_bf16
from attention_walk_graphs import BUDGETS, multi_edge_graph, walk_graph
from test_attention_walks_host import check_copies
from test_gat_walks_host import (A_PAIRS, B_PAIRS, C_PAIRS, C_RANGE_PAIRS, DROP, DROPOUT_FAMILIES, E_CASE, FAMILIES, KEYS, MULTI_EDGE_PAIRS, RANGE_COPY, SEED, SLOPE,
                                 check64, is_bf16, operands, repeats_that_differ_in_the_mask, shift_of, tiled_operands)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FILL = 0x5A5A  # bf16 bits no test computes; fp32 rows and edge arrays start at SENTINEL
SENTINEL = -12345.5
_plans, _digests = {}, {}


def plan(which, k):
    """The plan of walk_graph(which) (which = "multi": the multi-edge graph), held to the budget its cases declare."""
    if (which, k) not in _plans:
        p = flex_amd.Plan(multi_edge_graph()[0] if which == "multi" else walk_graph(which), k, attention=True, attention_backward=True)
        p.self_check()
        want = 64 if which == "multi" else BUDGETS[which]
        assert p.attention_info()["group_budget"] == p.attention_backward_info()["group_budget"] == want, ((which, k), p.attention_info())
        _plans[(which, k)] = p
    return _plans[(which, k)]


def _dev(x, b16=False):
    if b16:
        bits = gb.to_bf16(x)
        assert np.array_equal(gb.from_bf16(bits), np.asarray(x, np.float32), equal_nan=True)  # bf16 numbers already
        return torch.from_numpy(bits.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def to_dev(family, o):
    """The host operands on the device: V and g of a bf16 family as bfloat16, el and er float32 always."""
    return {key: _dev(x, is_bf16(family) and key in ("V", "g")) for key, x in o.items()}


def _host(t):
    """float32 tensors as they are, bfloat16 ones as their bits (uint16)"""
    torch.cuda.synchronize()
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.cpu().numpy()


def to_host(got):
    return {key: _host(t) for key, t in got.items()}


def _filled(shape, b16=False):
    if b16:
        return torch.full(shape, FILL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return torch.full(shape, SENTINEL, device="cuda")


def _refill(t):
    (t.view(torch.int16).fill_(FILL)) if t.dtype == torch.bfloat16 else t.fill_(SENTINEL)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _calls(family, p):
    """(forward(el, er, V, out, probs), backward(el, er, V, probs, g, gel, ger, gv, work)) of a family on plan p."""
    if family == "gat_bf16":
        return (lambda el, er, V, out, pd: p.gat_attention_bf16(el, er, V, SLOPE, out=out, p=pd),
                lambda el, er, V, pd, g, gel, ger, gv, work: p.gat_attention_bf16_backward(el, er, V, pd, g, SLOPE, grad_el=gel, grad_er=ger, grad_v=gv, work=work))
    f, b = ((p.gat_attention_bf16_dropout, p.gat_attention_bf16_dropout_backward) if family == "gat_bf16_dropout" else
            (p.gat_attention_dropout, p.gat_attention_dropout_backward))
    return (lambda el, er, V, out, pd: f(el, er, V, SLOPE, DROP, SEED, out=out, probs=pd),
            lambda el, er, V, pd, g, gel, ger, gv, work: b(el, er, V, pd, g, SLOPE, DROP, SEED, grad_el=gel, grad_er=ger, grad_v=gv, work=work))


def _outputs(family, a, k, H, with_p=True, backward=True):
    """dict of the outputs of a run, every one at its fill."""
    b16 = is_bf16(family)
    outs = dict(out=_filled((a.m, k), b16))
    if with_p:
        outs["p"] = _filled((a.nnz, H))
    if with_p and backward:
        outs.update(gel=_filled((a.m, H)), ger=_filled((a.n, H)), gv=_filled((a.n, k), b16), dx=_filled((a.nnz, H)))
    return outs


def _launch(family, p, d, outs):
    """The forward, and the backward where outs holds its outputs, into outs."""
    fwd, bwd = _calls(family, p)
    fwd(d["el"], d["er"], d["V"], outs["out"], outs.get("p"))
    if "gv" in outs:
        bwd(d["el"], d["er"], d["V"], outs["p"], d["g"], outs["gel"], outs["ger"], outs["gv"], outs["dx"])
    return outs


def run(family, p, a, d, k, H, with_p=True, backward=True):
    """The forward and the backward (every gradient) of a family on plan p and the device operands d: a dict of device tensors keyed
    out, p, gel, ger, gv, dx (dx: what dWork holds afterwards).  Every output starts at its fill.  with_p=False: the forward alone,
    without P; backward=False: the forward alone, with P."""
    return _launch(family, p, d, _outputs(family, a, k, H, with_p, backward))


def _digest(got):
    return {key: zlib.crc32(np.ascontiguousarray(x).tobytes()) for key, x in got.items()}


def _ids(cases):
    return [f"{c[0]}-k{c[1]}-h{c[2]}" + (f"-T{c[3]}" if len(c) > 3 else "") for c in cases]


def _tiled(d, T):
    return {key: t.repeat((T,) + (1,) * (t.dim() - 1)) for key, t in d.items()}


# ---- (a) budget 128 against float64, every element

A_CASES = [(f, k, H) for f in FAMILIES for k, H in A_PAIRS[f]]


@pytest.mark.parametrize("family,k,H", A_CASES, ids=_ids(A_CASES))
def test_budget_128_every_output_against_float64(family, k, H):
    a = walk_graph(1)
    o = operands(family, k, H, a, shift_of(family, k, H))
    got = to_host(run(family, plan(1, k), a, to_dev(family, o), k, H))
    _digests[(family, k, H)] = _digest(got)
    assert set(check64(family, a, o, got, f"budget 128 {family} k={k} H={H}")) == set(KEYS)


# ---- (b) budgets 512 and 2048 by copies, bit for bit

B_CASES = [(f, k, H, 7) for f in FAMILIES for k, H in B_PAIRS[f]] + [(f, *B_PAIRS[f][0], 30) for f in FAMILIES]
B_BF16 = [c for c in B_CASES if c[0] not in DROPOUT_FAMILIES]
B_DROPOUT = [c for c in B_CASES if c[0] in DROPOUT_FAMILIES]


@pytest.mark.parametrize("family,k,H,T", B_BF16, ids=_ids(B_BF16))
def test_every_copy_has_the_bits_of_the_one_copy_run(family, k, H, T):
    """No output is exempt: Out, P, gEl and dx are owned by the slot, wave or workgroup of their row, gEr and gV by that of their
    column, summed in CSR order, and a copy's rows, columns and entries keep their order."""
    a = walk_graph(1)
    d = to_dev(family, operands(family, k, H, a, shift_of(family, k, H)))
    base = run(family, plan(1, k), a, d, k, H)
    if (family, k, H) in _digests:  # the run that (a) held to float64
        assert _digest(to_host(base)) == _digests[(family, k, H)], "the one-copy run differs from run to run"
    got = run(family, plan(T, k), walk_graph(T), _tiled(d, T), k, H)
    torch.cuda.synchronize()
    assert set(got) == set(base) == set(KEYS)
    check_copies(f"budget {BUDGETS[T]} {family} k={k} H={H}", a, got, base, T)


@pytest.mark.parametrize("family,k,H,T", B_DROPOUT, ids=_ids(B_DROPOUT))
def test_under_dropout_p_of_every_copy_has_the_bits_of_the_one_copy_run_and_out_differs(family, k, H, T):
    a = walk_graph(1)
    d = to_dev(family, operands(family, k, H, a, shift_of(family, k, H)))
    base = run(family, plan(1, k), a, d, k, H, backward=False)
    if (family, k, H) in _digests:
        assert _digest(to_host(base)) == {key: _digests[(family, k, H)][key] for key in ("out", "p")}, "the one-copy run differs from run to run"
    got = run(family, plan(T, k), walk_graph(T), _tiled(d, T), k, H, backward=False)
    torch.cuda.synchronize()
    check_copies(f"budget {BUDGETS[T]} {family} k={k} H={H}", a, dict(p=got["p"]), dict(p=base["p"]), T)
    assert not torch.equal(_bits(got["out"][:a.m]), _bits(got["out"][a.m:2 * a.m]))  # another mask in every copy
    assert not bool((_bits(got["out"]) == _bits(_filled((1,), is_bf16(family)))).all(1).any())  # and no row of Out was left out


# ---- (c) dropout at budget 512

C_CASES = [(f, k, H) for f in DROPOUT_FAMILIES for k, H in C_PAIRS[f]]
C_RANGE_CASES = [(f, k, H) for f in DROPOUT_FAMILIES for k, H in C_RANGE_PAIRS[f]]


@pytest.mark.parametrize("family,k,H", C_CASES, ids=_ids(C_CASES))
def test_dropout_at_budget_512_p_by_copies_and_the_rest_against_float64(family, k, H):
    """The mask is taken at the entry's index in the 7-copy graph, so Out and the gradients differ from copy to copy and are held to
    float64 over the whole graph (the mask restated from flex_dropout_mask's definition and held to it here); P is undropped and has the
    bits of the one-copy run.  No case at 30 copies."""
    T = 7
    a1, a = walk_graph(1), walk_graph(T)
    o1 = operands(family, k, H, a1, shift_of(family, k, H))
    d1 = to_dev(family, o1)
    base = run(family, plan(1, k), a1, d1, k, H, backward=False)
    got = run(family, plan(T, k), a, _tiled(d1, T), k, H)
    check_copies(f"budget 512 {family}", a1, dict(p=got["p"]), dict(p=base["p"]), T)
    assert not torch.equal(_bits(got["out"][:a1.m]), _bits(got["out"][a1.m:2 * a1.m]))
    kp = flex_amd.binding.dropout_mask(SEED, DROP, 0, a.nnz * H).astype(bool).reshape(a.nnz, H)
    assert np.array_equal(kp, ad.kept_entries(a, H, DROP, SEED))
    assert set(check64(family, a, tiled_operands(o1, T), to_host(got), f"budget 512 {family} k={k} H={H}")) == set(KEYS)


@pytest.mark.parametrize("family,k,H", C_RANGE_CASES, ids=_ids(C_RANGE_CASES))
def test_dropout_at_budget_512_the_forward_of_one_copy_against_float64_with_the_mask_of_the_whole_graph(family, k, H):
    """W = 16 at 31 items per group: the forward runs on the 7 copies, and Out and P of the rows of copy 3 are held to float64 with the
    mask taken at their entries' indices in the whole graph.  The backward at this width under dropout is not held to float64 above
    budget 128."""
    T = 7
    a1, a = walk_graph(1), walk_graph(T)
    o1 = operands(family, k, H, a1, shift_of(family, k, H))
    got = to_host(run(family, plan(T, k), a, _tiled(to_dev(family, o1), T), k, H, backward=False))
    r0, r1 = RANGE_COPY * a1.m, (RANGE_COPY + 1) * a1.m
    e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
    assert (e0, e1) == (RANGE_COPY * a1.nnz, (RANGE_COPY + 1) * a1.nnz)
    o = tiled_operands(o1, T)
    each = check64(family, a, dict(o, el=o["el"][r0:r1]), dict(out=got["out"][r0:r1], p=got["p"][e0:e1]), f"budget 512 {family} k={k} H={H} rows [{r0}, {r1})",
                   rows=(r0, r1), backward=False)
    assert set(each) == {"out", "p"}


# ---- (d) unsorted rows and repeated (row, column) pairs

D_CASES = [(f, k, H) for f in FAMILIES for k, H in MULTI_EDGE_PAIRS[f]]


@pytest.mark.parametrize("family,k,H", D_CASES, ids=_ids(D_CASES))
def test_unsorted_rows_and_repeated_entries_against_float64(family, k, H):
    """P and dx are per entry in the order given, and the column launch takes the mask at the entry's own index: the float64 check is
    per entry.  The scores of the two copies of a repeated entry are equal, so their P is; the mask is taken per entry, so about half
    of them differ in it (held on the host).  The references were held to an independent torch evaluation on this graph on the host."""
    a, first = multi_edge_graph()
    o = operands(family, k, H, a, shift_of(family, k, H))
    got = to_host(run(family, plan("multi", k), a, to_dev(family, o), k, H))
    assert set(check64(family, a, o, got, f"multi-edge {family} k={k} H={H}")) == set(KEYS)
    if family in DROPOUT_FAMILIES:
        rep = np.flatnonzero(first != np.arange(a.nnz))
        live = got["p"] > 0
        both = live[rep] & live[first[rep]]
        assert np.array_equal(got["p"][rep][both].view(np.uint32), got["p"][first[rep]][both].view(np.uint32))
        share, count = repeats_that_differ_in_the_mask(a, first, H, live=live)
        assert count == int(both.sum()) > 100 and 0.3 < share < 0.7, (share, count)


def test_the_operator_on_bfloat16_leaves_with_dropout_on_unsorted_rows_and_repeated_entries_against_float64_autograd():
    """SparseOperator.gat_attention(el, er, V, dropout=0.5) on float32 el, er and bfloat16 V.  Tolerance, as tests/test_gpu_gat_bf16.py
    has it on its graph: gat_attention_ref.propagated_bounds times 2 c, as bound32 of the bf16 bound for Out and grad V."""
    a, _ = multi_edge_graph()
    k, H = 32, 4
    seed = SEED ^ 0x55
    rng = np.random.default_rng([k, H, 25])
    el, er = (rng.uniform(-2, 2, (r, H)).astype(np.float32) for r in (a.m, a.n))
    V, gOut = (gb.rounded(rng.uniform(-1, 1, (r, k)).astype(np.float32)) for r in (a.n, a.m))
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    eld, erd = (_dev(x).requires_grad_() for x in (el, er))
    Vd = _dev(V, True).requires_grad_()
    out = op.gat_attention(eld, erd, Vd, dropout=DROP, seed=seed)
    assert out.dtype == torch.bfloat16
    out.backward(_dev(gOut, True))
    assert Vd.grad.dtype == torch.bfloat16 and eld.grad.dtype == erd.grad.dtype == torch.float32
    got = tuple(_host(t) for t in (out.detach(), eld.grad, erd.grad, Vd.grad))
    kp, c = ad.kept_entries(a, H, DROP, seed), ad.factor(DROP)
    want = gd.torch_float64(a, el, er, V, SLOPE, gOut, kp, c)
    tols = gat.propagated_bounds(a, el, er, V, SLOPE, gOut)
    worst = 0.0
    for what, x, ref, tol in zip(("Out", "grad_el", "grad_er", "grad_V"), got, want, tols):
        tol = 2 * c * tol
        if x.dtype == np.uint16:
            x, tol = gb.from_bf16(x), bound_bf16(ref, tol)
        err = np.abs(x.astype(np.float64) - ref)
        worst = max(worst, float((err / tol).max()))
        assert x.shape == ref.shape and np.all(err <= tol), f"{what}: worst err / tolerance {float((err / tol).max()):.3g}"
    print(f"multi-edge operator k={k} H={H} dropout={DROP}: worst err / tolerance {worst:.3g}")


# ---- (e) the captured graph and dP = NULL

def test_at_budget_512_a_captured_graph_and_a_forward_without_p_give_the_bits_of_the_eager_run():
    family, k, H, T = E_CASE
    a1, a, p = walk_graph(1), walk_graph(T), plan(T, k)
    d = _tiled(to_dev(family, operands(family, k, H, a1, shift_of(family, k, H))), T)
    eager = run(family, p, a, d, k, H)
    assert torch.equal(_bits(run(family, p, a, d, k, H, with_p=False)["out"]), _bits(eager["out"]))
    outs = _outputs(family, a, k, H)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=side):  # one stream: the three launches are a chain
        _launch(family, p, d, outs)
    for t in outs.values():
        _refill(t)
    graph_.replay()
    torch.cuda.synchronize()
    for key in KEYS:
        assert torch.equal(_bits(outs[key]), _bits(eager[key])), f"{key}: the replay differs from the eager run"

"""The kernels of the per-edge score term of the fused GAT attention (flex::gat_edge: gat_edge_rows, gat_edge_rows_backward, DROP off
and on) on walks whose group budget is above the floor of 64 (internal.h: attention_group_budget), where a wave runs several items of
its group one after the other, on unsorted rows with repeated (row, column) pairs, and on the branch without the XCD remap.  Both
kernels hold a copy of their own of the loop over a group's items, of the class pick and of the remap, and ee is read at the entry's
index in the whole matrix; tests/test_gpu_gat_edge.py plans every graph at the floor.  Two families: gat_edge (drop_p = 0) and
gat_edge_dropout (p = 0.5); the keys are out, p, gel, ger, gee, gv, gee being what the work array holds afterwards.

Every output starts at the sentinel, and every plan is held to the budget its cases declare.

  (a) budget 128: walk_graph(1) (tests/attention_walk_graphs.py) against float64 on every element of all six outputs with
      gat_edge_ref's bounds and checkers and a scenario pair per head, W = 4, 8 and 16 in both families; dWork keeps the sentinel
      when dGradEe is given.
  (b) budgets 512 and 2048: 7 and 30 copies on the diagonal with el, er, ee, V and g repeated.  gat_edge: every copy's block of every
      output has the bits of the one-copy run, which has the digest of the run that (a) held to float64; lines without entries are +0.
      gat_edge_dropout: the mask is a hash of the entry's index in the whole graph, so only P has the bits of the one-copy run, Out
      must differ between the copies and no row may keep the sentinel; the forward alone is run.
  (b') ee = +0 at budget 512, W = 16 and 64, both families: every output has the bits of gat_attention / gat_attention_dropout and of
      their backward calls on the same plan (tests/test_gpu_attention_walks.py and tests/test_gpu_gat_walks.py hold those above the
      floor); gee is their dWork.
  (c) budget 512 against float64 with the operands DRAWN ON THE WHOLE 7-copy graph: on tiled ee an index that is wrong by the entries
      of a copy reads the same numbers, and (b) accepts it (tests/test_gat_edge_walks_host.py runs that model).  At (8, 2) all six
      outputs of both families over the 1 495 606 entries; at (64, 8) the forward alone, Out and P of the rows of copy 3 through the
      checkers' rows argument, ee and the mask taken at the entries of the whole graph.  Under dropout the mask is held to
      flex_dropout_mask.
  (d) thresholds_lifted with shuffled rows and a tenth of its entries repeated: both families against float64 per entry.  The two
      copies of a repeated pair hold other ee, so their P differs: the first family where the CSR order shows in P itself.  And
      SparseOperator.gat_attention(..., dropout=0.5, edge=e) against float64 torch autograd.
  (e) the branch without the remap (tuning xcd_slices = 2) at T = 1, (8, 2): every output has the bits of the default plan's run.
  (f) gat_edge_dropout at budget 512, (8, 2): a forward without P, a backward with grad_ee = None whose work array is dWork (it then
      holds gEe, and gEl, gEr and gV keep their bits), and the forward with both of these backward calls in one captured graph on one
      side stream, against the eager bits.

The table of the cases, their declared budgets and items per group, and the models of the faults these checks must catch are in
tests/test_gat_edge_walks_host.py."""
import zlib

import numpy as np
import pytest

import attention_dropout_ref as ad
import flex_amd
import gat_edge_ref as ge
from attention_walk_graphs import BUDGETS, multi_edge_graph, walk_graph
from test_attention_walks_host import check_copies
from test_gat_edge_walks_host import (A_PAIRS, B_PAIRS, C_PAIRS, C_RANGE_PAIRS, DROP, DROPOUT_FAMILIES, E_CASES, F_CASE, FAMILIES, KEYS, MULTI_EDGE_PAIRS, NO_REMAP,
                                      RANGE_COPY, SEED, SLOPE, ZERO_PAIRS, check64, drop_of, operands, repeats_that_differ_in_p, repeats_that_differ_in_the_mask)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = -12345.5
_plans, _digests = {}, {}


def plan(which, k, remap=True):
    """The plan of walk_graph(which) (which = "multi": the multi-edge graph), held to the budget its cases declare; remap=False: the
    same under tuning xcd_slices = 2."""
    if (which, k, remap) not in _plans:
        p = flex_amd.Plan(multi_edge_graph()[0] if which == "multi" else walk_graph(which), k, attention=True, attention_backward=True,
                          tuning=None if remap else NO_REMAP)
        p.self_check()
        want = 64 if which == "multi" else BUDGETS[which]
        assert p.attention_info()["group_budget"] == p.attention_backward_info()["group_budget"] == want, ((which, k), p.attention_info())
        assert p.tuning()["xcd_slices"] == (1 if remap else 2)
        _plans[(which, k, remap)] = p
    return _plans[(which, k, remap)]


def to_dev(o):
    return {key: torch.from_numpy(np.ascontiguousarray(x)).cuda() for key, x in o.items()}


def to_host(got):
    torch.cuda.synchronize()
    return {key: t.cpu().numpy() for key, t in got.items()}


def _filled(shape):
    return torch.full(shape, SENTINEL, device="cuda")


def _bits(t):
    return t.view(torch.int32)


def _outputs(a, k, H, with_p=True, backward=True):
    """dict of the outputs of a run, every one at the sentinel; work is dWork beside a given dGradEe."""
    outs = dict(out=_filled((a.m, k)))
    if with_p:
        outs["p"] = _filled((a.nnz, H))
    if with_p and backward:
        outs.update(gel=_filled((a.m, H)), ger=_filled((a.n, H)), gee=_filled((a.nnz, H)), gv=_filled((a.n, k)), work=_filled((a.nnz, H)))
    return outs


def _launch(family, p, d, outs):
    """The forward, and the backward where outs holds its outputs, into outs: dGradEe is the work array, dWork is passed beside it."""
    p.gat_edge_attention(d["el"], d["er"], d["ee"], d["V"], SLOPE, drop_of(family), SEED, out=outs["out"], probs=outs.get("p"))
    if "gv" in outs:
        p.gat_edge_attention_backward(d["el"], d["er"], d["ee"], d["V"], outs["p"], d["g"], SLOPE, drop_of(family), SEED, grad_el=outs["gel"], grad_er=outs["ger"],
                                      grad_ee=outs["gee"], grad_v=outs["gv"], work=outs["work"])
    return outs


def run(family, p, a, d, k, H, with_p=True, backward=True):
    """The forward and the backward (every gradient) of a family on plan p and the device operands d: a dict of device tensors keyed
    out, p, gel, ger, gee, gv.  Every output starts at the sentinel, and dWork, which is not the work array when dGradEe is given, must
    keep it.  with_p=False: the forward alone, without P; backward=False: the forward alone, with P."""
    outs = _launch(family, p, d, _outputs(a, k, H, with_p, backward))
    work = outs.pop("work", None)
    if work is not None:
        assert bool((work == SENTINEL).all()), "dWork was written although dGradEe was given"
    return outs


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
    o = operands(family, k, H, a)
    got = to_host(run(family, plan(1, k), a, to_dev(o), k, H))
    _digests[(family, k, H)] = _digest(got)
    assert set(check64(family, a, o, got, f"budget 128 {family} k={k} H={H}")) == set(KEYS)


# ---- (b) budgets 512 and 2048 by copies, bit for bit

B_CASES = [(f, k, H, 7) for f in FAMILIES for k, H in B_PAIRS[f]] + [(f, *B_PAIRS[f][0], 30) for f in FAMILIES]
B_PLAIN = [c for c in B_CASES if c[0] not in DROPOUT_FAMILIES]
B_DROPOUT = [c for c in B_CASES if c[0] in DROPOUT_FAMILIES]


@pytest.mark.parametrize("family,k,H,T", B_PLAIN, ids=_ids(B_PLAIN))
def test_every_copy_has_the_bits_of_the_one_copy_run(family, k, H, T):
    """No output is exempt: Out, P, gEl and gEe are owned by the slot, wave or workgroup of their row, gEr and gV by that of their
    column, summed in CSR order, and a copy's rows, columns and entries keep their order."""
    a = walk_graph(1)
    d = to_dev(operands(family, k, H, a))
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
    d = to_dev(operands(family, k, H, a))
    base = run(family, plan(1, k), a, d, k, H, backward=False)
    if (family, k, H) in _digests:
        assert _digest(to_host(base)) == {key: _digests[(family, k, H)][key] for key in ("out", "p")}, "the one-copy run differs from run to run"
    got = run(family, plan(T, k), walk_graph(T), _tiled(d, T), k, H, backward=False)
    torch.cuda.synchronize()
    check_copies(f"budget {BUDGETS[T]} {family} k={k} H={H}", a, dict(p=got["p"]), dict(p=base["p"]), T)
    assert not torch.equal(_bits(got["out"][:a.m]), _bits(got["out"][a.m:2 * a.m]))  # another mask in every copy
    assert not bool((got["out"] == SENTINEL).all(1).any())  # and no row of Out was left out


# ---- (b') ee = +0 is the GAT call, bit for bit, above the floor

ZERO_CASES = [(f, k, H) for f in FAMILIES for k, H in ZERO_PAIRS[f]]


@pytest.mark.parametrize("family,k,H", ZERO_CASES, ids=_ids(ZERO_CASES))
def test_at_budget_512_a_zero_edge_term_gives_the_bits_of_the_gat_calls(family, k, H):
    """No operand is -0 (gat_edge_ref.operands), so x + (+0) has the bits of x: a sweep of the edge kernels that diverged from the GAT
    family's on a later item of a group shows here.  gee is the dWork of the GAT backward."""
    T = 7
    a, p = walk_graph(T), plan(T, k)
    d = _tiled(to_dev(operands(family, k, H, walk_graph(1))), T)
    got = run(family, p, a, dict(d, ee=torch.zeros_like(d["ee"])), k, H)
    theirs = {key: _filled(tuple(t.shape)) for key, t in got.items()}
    if family in DROPOUT_FAMILIES:
        p.gat_attention_dropout(d["el"], d["er"], d["V"], SLOPE, DROP, SEED, out=theirs["out"], probs=theirs["p"])
        p.gat_attention_dropout_backward(d["el"], d["er"], d["V"], theirs["p"], d["g"], SLOPE, DROP, SEED, grad_el=theirs["gel"], grad_er=theirs["ger"],
                                         grad_v=theirs["gv"], work=theirs["gee"])
    else:
        p.gat_attention(d["el"], d["er"], d["V"], SLOPE, out=theirs["out"], p=theirs["p"])
        p.gat_attention_backward(d["el"], d["er"], d["V"], theirs["p"], d["g"], SLOPE, grad_el=theirs["gel"], grad_er=theirs["ger"], grad_v=theirs["gv"], work=theirs["gee"])
    torch.cuda.synchronize()
    for key in KEYS:
        assert not bool((theirs[key] == SENTINEL).all()), key
        assert torch.equal(_bits(got[key]), _bits(theirs[key])), f"{key} differs from the GAT call's in {int((_bits(got[key]) != _bits(theirs[key])).sum())} elements"


# ---- (c) budget 512 against float64, the operands drawn on the whole graph

C_CASES = [(f, k, H) for f in FAMILIES for k, H in C_PAIRS[f]]
C_RANGE_CASES = [(f, k, H) for f in FAMILIES for k, H in C_RANGE_PAIRS[f]]


def _mask_is_the_librarys(a, H):
    kp = flex_amd.binding.dropout_mask(SEED, DROP, 0, a.nnz * H).astype(bool).reshape(a.nnz, H)
    assert np.array_equal(kp, ad.kept_entries(a, H, DROP, SEED))


@pytest.mark.parametrize("family,k,H", C_CASES, ids=_ids(C_CASES))
def test_at_budget_512_every_output_against_float64_on_operands_of_the_whole_graph(family, k, H):
    """ee, el, er, V and g differ from copy to copy, so an index that is off by a whole copy, or by a block of entries, reads other
    numbers: all six outputs over the 1 495 606 entries of the 7-copy graph."""
    T = 7
    a = walk_graph(T)
    assert a.nnz == 1_495_606
    o = operands(family, k, H, a)
    assert not np.array_equal(o["ee"][:a.nnz // T], o["ee"][a.nnz // T:2 * (a.nnz // T)])
    got = to_host(run(family, plan(T, k), a, to_dev(o), k, H))
    if family in DROPOUT_FAMILIES:
        _mask_is_the_librarys(a, H)
    assert set(check64(family, a, o, got, f"budget 512 {family} k={k} H={H}")) == set(KEYS)


@pytest.mark.parametrize("family,k,H", C_RANGE_CASES, ids=_ids(C_RANGE_CASES))
def test_at_budget_512_the_forward_of_one_copy_against_float64_with_ee_and_the_mask_of_the_whole_graph(family, k, H):
    """W = 16 at 31 items per group: the forward runs on the 7 copies with operands drawn on the whole graph, and Out and P of the rows
    of copy 3 are held to float64 with ee and the mask taken at their entries' indices in the whole graph."""
    T = 7
    a1, a = walk_graph(1), walk_graph(T)
    o = operands(family, k, H, a)
    got = to_host(run(family, plan(T, k), a, to_dev(o), k, H, backward=False))
    r0, r1 = RANGE_COPY * a1.m, (RANGE_COPY + 1) * a1.m
    e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
    assert (e0, e1) == (RANGE_COPY * a1.nnz, (RANGE_COPY + 1) * a1.nnz)
    if family in DROPOUT_FAMILIES:
        _mask_is_the_librarys(a, H)
    each = check64(family, a, dict(o, el=o["el"][r0:r1]), dict(out=got["out"][r0:r1], p=got["p"][e0:e1]), f"budget 512 {family} k={k} H={H} rows [{r0}, {r1})",
                   rows=(r0, r1), backward=False)
    assert set(each) == {"out", "p"}


# ---- (d) unsorted rows and repeated (row, column) pairs

D_CASES = [(f, k, H) for f in FAMILIES for k, H in MULTI_EDGE_PAIRS[f]]


@pytest.mark.parametrize("family,k,H", D_CASES, ids=_ids(D_CASES))
def test_unsorted_rows_and_repeated_entries_against_float64(family, k, H):
    """P and gEe are per entry in the order given, ee is read at the entry's own index, and the column launch takes the mask there
    too: the float64 check is per entry.  The two copies of a repeated pair hold other ee, so among the pairs live in both P differs
    in more than 100; under dropout about half of them differ in the mask.  The references were held to an independent torch
    evaluation on this graph on the host."""
    a, first = multi_edge_graph()
    o = operands(family, k, H, a)
    got = to_host(run(family, plan("multi", k), a, to_dev(o), k, H))
    assert set(check64(family, a, o, got, f"multi-edge {family} k={k} H={H}")) == set(KEYS)
    differ, live = repeats_that_differ_in_p(got["p"], first)
    print(f"multi-edge {family} k={k} H={H}: P differs in {differ} of the {live} repeat pairs live in both copies")
    assert differ > 100, (differ, live)
    if family in DROPOUT_FAMILIES:
        share, count = repeats_that_differ_in_the_mask(a, first, H, live=got["p"] > 0)
        print(f"multi-edge {family} k={k} H={H}: {share:.3f} of them differ in the mask")
        assert count == live and 0.3 < share < 0.7, (share, count)


def test_the_operator_with_edge_and_dropout_on_unsorted_rows_and_repeated_entries_against_float64_autograd():
    """SparseOperator.gat_attention(el, er, V, dropout=0.5, edge=e) against float64 torch autograd with the numpy mask as a constant.
    Tolerance, as tests/test_gpu_gat_edge.py section 9 derives it: gat_edge_ref.propagated_bounds of the undropped step times 2 c."""
    a, _ = multi_edge_graph()
    k, H = 32, 4
    seed = SEED ^ 0x55
    rng = np.random.default_rng([k, H, 27])
    el, er = (rng.uniform(-2, 2, (r, H)).astype(np.float32) for r in (a.m, a.n))
    ee = rng.uniform(-2, 2, (a.nnz, H)).astype(np.float32)
    V, gOut = (rng.uniform(-1, 1, (r, k)).astype(np.float32) for r in (a.n, a.m))
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    eld, erd, eed, Vd = (t.requires_grad_() for t in to_dev(dict(el=el, er=er, ee=ee, V=V)).values())
    out = op.gat_attention(eld, erd, Vd, dropout=DROP, seed=seed, edge=eed)
    out.backward(torch.from_numpy(gOut).cuda())
    got = tuple(to_host(dict(out=out.detach(), gel=eld.grad, ger=erd.grad, gee=eed.grad, gv=Vd.grad)).values())
    kp, c = ad.kept_entries(a, H, DROP, seed), ad.factor(DROP)
    want = ge.torch_float64(a, el, er, ee, V, SLOPE, gOut, kp, c)
    want = (want[0],) + want[2:]
    tols = ge.propagated_bounds(a, el, er, ee, V, SLOPE, gOut)
    each = {}
    for what, x, ref, tol in zip(("Out", "grad_el", "grad_er", "grad_edge", "grad_V"), got, want, tols):
        err = np.abs(x.astype(np.float64) - ref)
        each[what] = float((err / (2 * c * tol)).max())
        assert x.shape == ref.shape and np.all(err <= 2 * c * tol), f"{what}: worst err / tolerance {each[what]:.3g}"
    print(f"multi-edge operator k={k} H={H} dropout={DROP}: worst err / tolerance " + " ".join(f"{key} {v:.3g}" for key, v in each.items()))


# ---- (e) the branch without the remap

@pytest.mark.parametrize("family,k,H,T", E_CASES, ids=_ids(E_CASES))
def test_without_the_remap_every_output_has_the_bits_of_the_default_plans_run(family, k, H, T):
    """Which workgroup runs a group does not decide what it computes.  The grid of the default plan is rounded up to a multiple of 8
    workgroups (737 -> 744 at this shape); without the remap it is not, and wg is blockIdx.x itself."""
    a = walk_graph(T)
    d = to_dev(operands(family, k, H, a))
    base = run(family, plan(T, k), a, d, k, H)
    got = run(family, plan(T, k, remap=False), a, d, k, H)
    torch.cuda.synchronize()
    if (family, k, H) in _digests:
        assert _digest(to_host(base)) == _digests[(family, k, H)], "the one-copy run differs from run to run"
    for key in KEYS:
        assert torch.equal(_bits(got[key]), _bits(base[key])), f"{key}: the plan without the remap gives other bits"


# ---- (f) the captured graph, dP = NULL and dWork as the work array

def test_at_budget_512_a_captured_graph_a_forward_without_p_and_a_backward_into_dwork_give_the_eager_bits():
    family, k, H, T = F_CASE
    a1, a, p = walk_graph(1), walk_graph(T), plan(F_CASE[3], F_CASE[1])
    d = _tiled(to_dev(operands(family, k, H, a1)), T)
    eager = run(family, p, a, d, k, H)
    assert torch.equal(_bits(run(family, p, a, d, k, H, with_p=False)["out"]), _bits(eager["out"]))
    # grad_ee = None: dWork is the work array and holds gEe afterwards; the other gradients keep their bits
    part = _outputs(a, k, H)
    gel, ger, gee, gv = p.gat_edge_attention_backward(d["el"], d["er"], d["ee"], d["V"], eager["p"], d["g"], SLOPE, DROP, SEED, want=(True, True, False, True),
                                                      grad_el=part["gel"], grad_er=part["ger"], grad_ee=None, grad_v=part["gv"], work=part["work"])
    torch.cuda.synchronize()
    assert gee is None and bool((part["gee"] == SENTINEL).all())
    assert torch.equal(_bits(part["work"]), _bits(eager["gee"])), "dWork as the work array does not hold the bits of gEe"
    for key in ("gel", "ger", "gv"):
        assert torch.equal(_bits(part[key]), _bits(eager[key])), f"{key}: with dWork as the work array the bits differ"
    # one captured graph: the forward, the backward with dGradEe as the work array, and a second backward into dWork with gradients of its own
    outs, second = _outputs(a, k, H), _outputs(a, k, H)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=side):  # one stream: the five launches are a chain
        _launch(family, p, d, outs)
        p.gat_edge_attention_backward(d["el"], d["er"], d["ee"], d["V"], outs["p"], d["g"], SLOPE, DROP, SEED, want=(True, True, False, True),
                                      grad_el=second["gel"], grad_er=second["ger"], grad_ee=None, grad_v=second["gv"], work=second["work"])
    for t in list(outs.values()) + list(second.values()):
        t.fill_(SENTINEL)
    graph_.replay()
    torch.cuda.synchronize()
    assert bool((outs["work"] == SENTINEL).all()) and bool((second["gee"] == SENTINEL).all())
    for key in KEYS:
        assert torch.equal(_bits(outs[key]), _bits(eager[key])), f"{key}: the replay differs from the eager run"
    assert torch.equal(_bits(second["work"]), _bits(eager["gee"])), "the replay's dWork as the work array does not hold the bits of gEe"
    for key in ("gel", "ger", "gv"):
        assert torch.equal(_bits(second[key]), _bits(eager[key])), f"{key}: the replay with dWork as the work array differs from the eager run"

"""The kernels of the fused GATv2 attention and of its dropout twin (flex::gatv2, flex::gatv2_dropout) on walks whose group budget is
above the floor of 64 (internal.h: attention_group_budget), where a wave runs several items of its group one after the other, on
unsorted rows with repeated (row, column) pairs, and on the branch without the XCD remap; gAtt by its partials.  Each of the six
kernels holds a copy of its own of the loop over a group's items, and rows_backward keeps a lane's gAtt partial across all of them;
tests/test_gpu_gatv2_attention.py and tests/test_gpu_gatv2_dropout.py plan every graph at the floor.  p = 0.5.

Every output starts at a sentinel, dAttWork among them: it is always passed explicitly.  gAtt is held in the two stages of the kernels
(tests/gatv2_attention_ref.py, check_att): every row of dAttWork, the partial of one workgroup, to float64 over that workgroup's own
entries under gamma(n_w + 3), rows without entries +0; then the bits of gAtt to att_reduce32 of the rows the kernel wrote.

  (a) budget 128: walk_graph(1) (tests/attention_walk_graphs.py) against float64 on every element of Out, P, gXt, gXs and dz with the
      family's checker and a scenario per head, gAtt by check_att: W = 4 and W = 8 in both families, W = 16 under dropout.
  (b) budgets 512 and 2048: 7 and 30 copies on the diagonal with the operands repeated.  gatv2: every copy's block of Out, P, gXt, gXs
      and dz has the bits of the one-copy run, lines without entries +0; gAtt has the bits of att_reduce32 of the rows of dAttWork,
      whose rows without entries are +0 and none of which keeps the sentinel; at (8, 2) the rows are held to float64 as well, at both
      T, by regrouping: the per-line float64 sums of the one-copy graph are computed once and added up by the T-copy layout, a
      workgroup's entries being whole lines of known copies and P and dz bit-equal across the copies by the check before (under half
      a second of numpy at T = 30: every row of all 30 copies is held, not those of two copies alone).  At T = 7 the rows of the
      same run are also held to float64 over the entries of the 7-copy graph, and the two references must give the same worst ratio.
      gatv2_dropout: the mask is a hash of the entry's index in the whole graph, so only P has the bits of the one-copy run, Out must
      differ between the copies and no row may keep the sentinel; the forward alone is run.
  (c) dropout at budget 512: at (8, 2) P copy by copy, the mask against flex_dropout_mask, and every other output against float64
      over the 1 495 606 entries, gAtt by check_att; at (64, 8) the forward with Out and P of the rows of copy 3 against float64, the
      mask taken at the entries of the whole graph (the checkers' rows argument).
  (d) thresholds_lifted with shuffled rows and a tenth of its entries repeated: both families against float64 per entry, gAtt by
      check_att; under dropout the two copies of a repeated entry hold the same P and differ in the mask in about half of them; and
      SparseOperator.gatv2_attention(..., dropout=0.5) against float64 torch autograd.
  (e) the branch without the remap (tuning xcd_slices = 2) at T = 1, (8, 2): Out, P, gXt, gXs and dz have the bits of the default
      plan's run, dAttWork has the other row count and passes check_att under the other layout.
  (f) at budget 512: the forward and backward of gatv2_dropout in one captured graph against the eager bits, a forward without P, and
      a backward without gAtt, which leaves dAttWork at its sentinel.

The table of the cases, their declared budgets and items per group, and the models of the faults these checks must catch are in
tests/test_gatv2_walks_host.py."""
import time
import zlib

import numpy as np
import pytest

import attention_dropout_ref as ad
import flex_amd
import gatv2_attention_ref as v2
import gatv2_dropout_ref as vd
from attention_walk_graphs import BUDGETS, multi_edge_graph, walk_graph
from test_gatv2_walks_host import (A_PAIRS, B_PAIRS, C_PAIRS, C_RANGE_PAIRS, DROP, DROPOUT_FAMILIES, E_CASES, F_CASE, FAMILIES, KEYS, MULTI_EDGE_PAIRS, NO_REMAP,
                                   RANGE_COPY, SEED, SLOPE, check64, check_copies, drop_of, layout_of, operands, repeats_that_differ_in_the_mask, shift_of,
                                   tiled_operands)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = -12345.5
ALL = KEYS + ("gatt", "att_work")
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


def layout(which, k, remap=True):
    a = multi_edge_graph()[0] if which == "multi" else walk_graph(which)
    return layout_of(a, k, 64 if which == "multi" else BUDGETS[which], remap)


def to_dev(o):
    return {key: torch.from_numpy(np.ascontiguousarray(x)).cuda() for key, x in o.items()}


def to_host(got):
    torch.cuda.synchronize()
    return {key: t.cpu().numpy() for key, t in got.items()}


def _filled(shape):
    return torch.full(shape, SENTINEL, device="cuda")


def _bits(t):
    return t.view(torch.int32)


def _outputs(p, a, k, H, with_p=True, backward=True):
    """dict of the outputs of a run, every one at the sentinel; att_work holds the plan's gatv2_attention_work_size() floats."""
    outs = dict(out=_filled((a.m, k)))
    if with_p:
        outs["p"] = _filled((a.nnz, H))
    if with_p and backward:
        outs.update(gxt=_filled((a.m, k)), gxs=_filled((a.n, k)), gatt=_filled((H, k // H)), dz=_filled((a.nnz, H)), att_work=_filled((p.gatv2_attention_work_size(),)))
    return outs


def _launch(family, p, d, outs, want=(True, True, True)):
    """The forward, and the backward where outs holds its outputs, into outs."""
    xt, xs, att = d["xt"], d["xs"], d["att"]
    grads = dict(grad_xt=outs.get("gxt"), grad_xs=outs.get("gxs"), grad_att=outs.get("gatt"), work=outs.get("dz"), want=want, att_work=outs.get("att_work"))
    if family == "gatv2":
        p.gatv2_attention(xt, xs, att, SLOPE, out=outs["out"], p=outs.get("p"))
        if "gxt" in outs:
            p.gatv2_attention_backward(xt, xs, att, outs["p"], d["g"], SLOPE, **grads)
    else:
        p.gatv2_attention_dropout(xt, xs, att, SLOPE, DROP, SEED, out=outs["out"], probs=outs.get("p"))
        if "gxt" in outs:
            p.gatv2_attention_dropout_backward(xt, xs, att, outs["p"], d["g"], SLOPE, DROP, SEED, **grads)
    return outs


def run(family, p, a, d, k, H, with_p=True, backward=True):
    """The forward and the backward (every gradient) of a family on plan p and the device operands d: a dict of device tensors keyed
    out, p, gxt, gxs, gatt, dz (what dWork holds afterwards) and att_work (dAttWork).  with_p=False: the forward alone, without P;
    backward=False: the forward alone, with P."""
    return _launch(family, p, d, _outputs(p, a, k, H, with_p, backward))


def _digest(got):
    return {key: zlib.crc32(np.ascontiguousarray(x).tobytes()) for key, x in got.items()}


def _ids(cases):
    return [f"{c[0]}-k{c[1]}-h{c[2]}" + (f"-T{c[3]}" if len(c) > 3 else "") for c in cases]


def _tiled(d, T):
    return {key: t if key == "att" else t.repeat((T,) + (1,) * (t.dim() - 1)) for key, t in d.items()}


def rows_written(att_work, lay, k, what):
    """dAttWork on the host as [rows, k]: it has the layout's row count, no element keeps the sentinel and a row without entries is +0."""
    rows = att_work.reshape(-1, k)
    assert rows.shape[0] == lay[1], f"{what}: dAttWork has {rows.shape[0]} rows, the layout {lay[1]}"
    assert not (rows == np.float32(SENTINEL)).any(), f"{what}: {int((rows == np.float32(SENTINEL)).any(1).sum())} rows of dAttWork keep the sentinel"
    idle = np.bincount(lay[0], minlength=lay[1]) == 0
    assert not rows[idle].view(np.uint32).any(), f"{what}: a row of dAttWork without entries is not +0"
    return rows


# ---- (a) budget 128 against float64, every element, gAtt by its partials

A_CASES = [(f, k, H) for f in FAMILIES for k, H in A_PAIRS[f]]


@pytest.mark.parametrize("family,k,H", A_CASES, ids=_ids(A_CASES))
def test_budget_128_every_output_against_float64_and_gatt_by_its_partials(family, k, H):
    a = walk_graph(1)
    o = operands(family, k, H, a, shift_of(family, k, H))
    got = to_host(run(family, plan(1, k), a, to_dev(o), k, H))
    _digests[(family, k, H)] = _digest(got)
    lay = layout(1, k)
    rows_written(got["att_work"], lay, k, f"budget 128 {family} k={k} H={H}")
    each = check64(family, a, o, got, f"budget 128 {family} k={k} H={H}", layout=lay)
    assert {"gxt", "gxs", "gatt", "dz", "att_work"} <= set(each)


# ---- (b) budgets 512 and 2048 by copies, bit for bit

B_CASES = [(f, k, H, 7) for f in FAMILIES for k, H in B_PAIRS[f]] + [(f, *B_PAIRS[f][0], 30) for f in FAMILIES]
B_PLAIN = [c for c in B_CASES if c[0] not in DROPOUT_FAMILIES]
B_DROPOUT = [c for c in B_CASES if c[0] in DROPOUT_FAMILIES]


@pytest.mark.parametrize("family,k,H,T", B_PLAIN, ids=_ids(B_PLAIN))
def test_every_copy_has_the_bits_of_the_one_copy_run_and_gatt_those_of_the_reduction_of_its_rows(family, k, H, T):
    """Out, P, gXt and dz are owned by the slot, wave or workgroup of their row, gXs by that of its column, summed in CSR order, and a
    copy's rows, columns and entries keep their order: no output is exempt.  gAtt sums over all copies; it is held by the rows of
    dAttWork and the bits of their reduction, and at (8, 2) the rows are held to float64 (the module's docstring, (b))."""
    a = walk_graph(1)
    o = operands(family, k, H, a, shift_of(family, k, H))
    d = to_dev(o)
    what = f"budget {BUDGETS[T]} {family} k={k} H={H}"
    base = run(family, plan(1, k), a, d, k, H)
    if (family, k, H) in _digests:  # the run that (a) held to float64
        assert _digest(to_host(base)) == _digests[(family, k, H)], "the one-copy run differs from run to run"
    got = run(family, plan(T, k), walk_graph(T), _tiled(d, T), k, H)
    torch.cuda.synchronize()
    assert set(got) == set(base) == set(ALL)
    check_copies(what, a, {key: got[key] for key in KEYS}, {key: base[key] for key in KEYS}, T)
    lay = layout(T, k)
    rows, gatt = rows_written(got["att_work"].cpu().numpy(), lay, k, what), got["gatt"].cpu().numpy()
    v2.check_att_reduce(rows, gatt, what)
    if (k, H) == B_PAIRS[family][0]:
        t0 = time.perf_counter()
        worst = v2.check_att(a, o["xt"], o["xs"], o["att"], base["p"].cpu().numpy(), o["g"], SLOPE, rows, gatt, lay, what=what, copies=T)
        print(f"{what}: worst err / bound att_work {worst:.3g} ({lay[1]} rows regrouped from the one-copy lines in {time.perf_counter() - t0:.2f} s)")


def test_at_seven_copies_the_regrouped_reference_of_the_rows_is_that_of_the_whole_graph():
    """The two ways to the float64 rows of dAttWork, on the run of (b) at T = 7, (8, 2): over the entries of the 7-copy graph with its
    own P, and regrouped from the lines of the one-copy graph.  Both must accept the rows; T = 30 has the second alone."""
    family, (k, H), T = "gatv2", B_PAIRS["gatv2"][0], 7
    a1, a = walk_graph(1), walk_graph(T)
    o = operands(family, k, H, a1, shift_of(family, k, H))
    got = to_host(run(family, plan(T, k), a, _tiled(to_dev(o), T), k, H))
    lay = layout(T, k)
    whole = v2.check_att(a, *(tiled_operands(o, T)[x] for x in ("xt", "xs", "att")), got["p"], tiled_operands(o, T)["g"], SLOPE, got["att_work"], got["gatt"], lay,
                         what="whole graph")
    lines = v2.check_att(a1, o["xt"], o["xs"], o["att"], got["p"][:a1.nnz], o["g"], SLOPE, got["att_work"], got["gatt"], lay, what="regrouped", copies=T)
    print(f"budget 512 gatv2 k={k} H={H}: worst err / bound att_work {whole:.3g} over the whole graph, {lines:.3g} regrouped")
    assert abs(whole - lines) <= 1e-6 * max(whole, lines)


@pytest.mark.parametrize("family,k,H,T", B_DROPOUT, ids=_ids(B_DROPOUT))
def test_under_dropout_p_of_every_copy_has_the_bits_of_the_one_copy_run_and_out_differs(family, k, H, T):
    a = walk_graph(1)
    d = to_dev(operands(family, k, H, a, shift_of(family, k, H)))
    base = run(family, plan(1, k), a, d, k, H, backward=False)
    if (family, k, H) in _digests:
        assert _digest(to_host(base)) == {key: _digests[(family, k, H)][key] for key in ("out", "p")}, "the one-copy run differs from run to run"
    got = run(family, plan(T, k), walk_graph(T), _tiled(d, T), k, H, backward=False)
    torch.cuda.synchronize()
    check_copies(f"budget {BUDGETS[T]} {family} k={k} H={H}", a, dict(p=got["p"]), dict(p=base["p"]), T)
    assert not torch.equal(_bits(got["out"][:a.m]), _bits(got["out"][a.m:2 * a.m]))  # another mask in every copy
    assert not bool((got["out"] == SENTINEL).all(1).any())  # and no row of Out was left out


# ---- (c) dropout at budget 512

C_CASES = [(f, k, H) for f in DROPOUT_FAMILIES for k, H in C_PAIRS[f]]
C_RANGE_CASES = [(f, k, H) for f in DROPOUT_FAMILIES for k, H in C_RANGE_PAIRS[f]]


@pytest.mark.parametrize("family,k,H", C_CASES, ids=_ids(C_CASES))
def test_dropout_at_budget_512_p_by_copies_and_the_rest_against_float64(family, k, H):
    """The mask is taken at the entry's index in the 7-copy graph, so Out and the gradients differ from copy to copy and are held to
    float64 over the whole graph (the mask restated from flex_dropout_mask's definition and held to it here), gAtt by check_att over
    the whole graph; P is undropped and has the bits of the one-copy run."""
    T = 7
    a1, a = walk_graph(1), walk_graph(T)
    o1 = operands(family, k, H, a1, shift_of(family, k, H))
    d1 = to_dev(o1)
    base = run(family, plan(1, k), a1, d1, k, H, backward=False)
    got = run(family, plan(T, k), a, _tiled(d1, T), k, H)
    check_copies(f"budget 512 {family}", a1, dict(p=got["p"]), dict(p=base["p"]), T)
    assert not torch.equal(_bits(got["out"][:a1.m]), _bits(got["out"][a1.m:2 * a1.m]))
    kp = flex_amd.binding.dropout_mask(SEED, DROP, 0, a.nnz * H).astype(bool).reshape(a.nnz, H)
    assert np.array_equal(kp, ad.kept_entries(a, H, DROP, SEED))
    got, lay = to_host(got), layout(T, k)
    rows_written(got["att_work"], lay, k, f"budget 512 {family}")
    each = check64(family, a, tiled_operands(o1, T), got, f"budget 512 {family} k={k} H={H}", layout=lay)
    assert {"out", "p", "gxt", "gxs", "gatt", "dz", "att_work"} == set(each)


@pytest.mark.parametrize("family,k,H", C_RANGE_CASES, ids=_ids(C_RANGE_CASES))
def test_dropout_at_budget_512_the_forward_of_one_copy_against_float64_with_the_mask_of_the_whole_graph(family, k, H):
    """W = 16 at 31 items per group: the forward runs on the 7 copies, and Out and P of the rows of copy 3 are held to float64 with the
    mask taken at their entries' indices in the whole graph."""
    T = 7
    a1, a = walk_graph(1), walk_graph(T)
    o1 = operands(family, k, H, a1, shift_of(family, k, H))
    got = to_host(run(family, plan(T, k), a, _tiled(to_dev(o1), T), k, H, backward=False))
    r0, r1 = RANGE_COPY * a1.m, (RANGE_COPY + 1) * a1.m
    e0, e1 = int(a.rowPtr[r0]), int(a.rowPtr[r1])
    assert (e0, e1) == (RANGE_COPY * a1.nnz, (RANGE_COPY + 1) * a1.nnz)
    o = tiled_operands(o1, T)
    each = check64(family, a, dict(o, xt=o["xt"][r0:r1]), dict(out=got["out"][r0:r1], p=got["p"][e0:e1]), f"budget 512 {family} k={k} H={H} rows [{r0}, {r1})",
                   rows=(r0, r1), backward=False)
    assert set(each) == {"out", "p"}


# ---- (d) unsorted rows and repeated (row, column) pairs

D_CASES = [(f, k, H) for f in FAMILIES for k, H in MULTI_EDGE_PAIRS[f]]


@pytest.mark.parametrize("family,k,H", D_CASES, ids=_ids(D_CASES))
def test_unsorted_rows_and_repeated_entries_against_float64(family, k, H):
    """P and dz are per entry in the order given, and the column launch takes its (row, entry) stream, and under dropout the mask, at
    the entry's own index: the float64 check is per entry.  The scores of the two copies of a repeated entry are equal, so their P is;
    the mask is taken per entry, so about half of them differ in it.  The references were held to an independent torch evaluation on
    this graph on the host."""
    a, first = multi_edge_graph()
    o = operands(family, k, H, a, shift_of(family, k, H))
    got = to_host(run(family, plan("multi", k), a, to_dev(o), k, H))
    lay = layout("multi", k)
    rows_written(got["att_work"], lay, k, f"multi-edge {family} k={k} H={H}")
    each = check64(family, a, o, got, f"multi-edge {family} k={k} H={H}", layout=lay)
    assert {"gxt", "gxs", "gatt", "dz", "att_work"} <= set(each)
    rep = np.flatnonzero(first != np.arange(a.nnz))
    live = got["p"] > 0
    both = live[rep] & live[first[rep]]
    assert both.sum() > 100 and np.array_equal(got["p"][rep][both].view(np.uint32), got["p"][first[rep]][both].view(np.uint32))
    if family in DROPOUT_FAMILIES:
        share, count = repeats_that_differ_in_the_mask(a, first, H, live=live)
        assert count == int(both.sum()) and 0.3 < share < 0.7, (share, count)


def test_the_operator_with_dropout_on_unsorted_rows_and_repeated_entries_against_float64_autograd():
    """SparseOperator.gatv2_attention(xt, xs, att, dropout=0.5) against float64 torch autograd with the numpy mask as a constant,
    within gatv2_dropout_ref.propagated_bounds (finite scores)."""
    a, _ = multi_edge_graph()
    k, H = 32, 4
    seed = SEED ^ 0x55
    xt, xs, att = v2.operands(["uniform4", "x_zero", "spread80", "att_signs"], a, k, seed=25)
    gOut = np.random.default_rng([k, H, 25]).uniform(-1, 1, (a.m, k)).astype(np.float32)
    op = flex_amd.SparseOperator(a, k, learn_values=True, fused_attention=True, fused_backward=True)
    xtd, xsd, attd = (t.requires_grad_() for t in to_dev(dict(xt=xt, xs=xs, att=att)).values())
    out = op.gatv2_attention(xtd, xsd, attd, dropout=DROP, seed=seed)
    out.backward(torch.from_numpy(gOut).cuda())
    got = tuple(to_host(dict(out=out.detach(), gxt=xtd.grad, gxs=xsd.grad, gatt=attd.grad)).values())
    kp, c = ad.kept_entries(a, H, DROP, seed), ad.factor(DROP)
    ref_out, _, ref_gxt, ref_gxs, ref_gatt = vd.torch_float64(a, xt, xs, att, SLOPE, gOut, kp, c)
    tols = vd.propagated_bounds(a, xt, xs, att, SLOPE, gOut, DROP, seed)
    worst = 0.0
    for what, x, ref, tol in zip(("Out", "grad_xt", "grad_xs", "grad_att"), got, (ref_out, ref_gxt, ref_gxs, ref_gatt), tols):
        err = np.abs(x.astype(np.float64) - ref)
        worst = max(worst, float((err / tol).max()))
        assert x.shape == ref.shape and np.all(err <= tol), f"{what}: worst err / tolerance {float((err / tol).max()):.3g}"
    print(f"multi-edge operator k={k} H={H} dropout={DROP}: worst err / tolerance {worst:.3g}")


# ---- (e) the branch without the remap

@pytest.mark.parametrize("family,k,H,T", E_CASES, ids=_ids(E_CASES))
def test_without_the_remap_the_same_bits_the_other_row_count_and_gatt_by_its_partials(family, k, H, T):
    """Which workgroup runs a group does not decide what it computes: Out, P, gXt, gXs and dz have the bits of the default plan's run.
    dAttWork is stored at blockIdx.x, so its rows move and its count is 741 where the remap's padded grid gives 748; check_att holds
    it under the layout without the remap.  gAtt sums the rows in another order and is held by check_att alone."""
    a = walk_graph(T)
    o = operands(family, k, H, a, shift_of(family, k, H))
    d = to_dev(o)
    base = run(family, plan(T, k), a, d, k, H)
    got = run(family, plan(T, k, remap=False), a, d, k, H)
    torch.cuda.synchronize()
    for key in KEYS:
        assert torch.equal(_bits(got[key]), _bits(base[key])), f"{key}: the plan without the remap gives other bits"
    assert (base["att_work"].numel(), got["att_work"].numel()) == (748 * k, 741 * k)
    got, lay = to_host(got), layout(T, k, remap=False)
    assert lay[1] == 741
    rows_written(got["att_work"], lay, k, f"no remap {family}")
    each = check64(family, a, o, got, f"no remap {family} k={k} H={H}", layout=lay)
    assert "att_work" in each
    with pytest.raises(AssertionError, match="dAttWork"):  # and the layout with the remap is another
        v2.check_att(a, o["xt"], o["xs"], o["att"], got["p"], o["g"], SLOPE, np.concatenate([got["att_work"], np.zeros(7 * k, np.float32)]), got["gatt"],
                     layout(T, k), drop=drop_of(family))


# ---- (f) the captured graph, dP = NULL and a backward without gAtt

def test_at_budget_512_a_captured_graph_a_forward_without_p_and_a_backward_without_gatt():
    family, k, H, T = F_CASE
    a1, a, p = walk_graph(1), walk_graph(T), plan(F_CASE[3], F_CASE[1])
    d = _tiled(to_dev(operands(family, k, H, a1, shift_of(family, k, H))), T)
    eager = run(family, p, a, d, k, H)
    assert torch.equal(_bits(run(family, p, a, d, k, H, with_p=False)["out"]), _bits(eager["out"]))
    part = _outputs(p, a, k, H)
    _launch(family, p, d, part, want=(True, True, False))
    torch.cuda.synchronize()
    assert bool((part["att_work"] == SENTINEL).all()) and bool((part["gatt"] == SENTINEL).all()), "a backward without gAtt wrote dAttWork or gAtt"
    for key in ("gxt", "gxs", "dz"):
        assert torch.equal(_bits(part[key]), _bits(eager[key])), f"{key}: without gAtt the bits differ"
    outs = _outputs(p, a, k, H)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=side):  # one stream: the four launches are a chain
        _launch(family, p, d, outs)
    for t in outs.values():
        t.fill_(SENTINEL)
    graph_.replay()
    torch.cuda.synchronize()
    for key in ALL:
        assert torch.equal(_bits(outs[key]), _bits(eager[key])), f"{key}: the replay differs from the eager run"

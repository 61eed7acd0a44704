"""Hub rows cut by schedule window on the GPU (flex_plan_tuning.hub_row; plan_build.cpp, cut_hub_rows): the pieces of a long row run
among the rows of the schedule window their columns belong to, in ordinary chunks beside ordinary rows and row bundles, and the row is
summed from its partial slots as before.  The device code is the flat kernels' and the fix-up's, unchanged; what is new is where a
piece sits in the stream, so every case runs the plan's self-check, holds C to the float64 bound of tests/f64ref.py (a bound on any
order of the sum) and asks for identical bits from two launches.

The input is tests/hub_graphs.py's: 4096 vertices in natural order, 16 windows of 256 positions, short rows everywhere (bundles and
moved pieces share chunks), eight long rows spread over all windows and four planted ones -- a row whose every record moves, a row
with exactly one moved piece that is also a column of its own window, a moved run of two budgets, and a padded moved piece that ends
on +inf."""
import numpy as np
import pytest

import flex_amd
from f64ref import assert_within_f64_bound
from hub_graphs import KNOBS, N, OFF, expected_moves, hub_graph
from util import random_B

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def graph():
    return hub_graph()


def launch_twice(plan, a, B, k):
    Bd = torch.from_numpy(B).cuda()
    out = []
    for fill in (-7.0, 3.0):  # every row must be written, whatever C held
        C = torch.full((a.m, k), fill, device="cuda")
        plan(Bd, out=C)
        torch.cuda.synchronize()
        out.append(C)
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32)), "two launches differ"
    return out[0].cpu().numpy()


def check(a, k, route, seed=0, **kw):
    p = flex_amd.Plan(a, k, **kw)
    p.self_check()
    i = p.info()
    assert i["n_moved_pieces"] > 0 and i["moved_records"] > 0, i
    B = random_B(a.n, k, seed=seed + k)
    assert_within_f64_bound(a, B, launch_twice(p, a, B, k), route=f"{route} (moved pieces {i['n_moved_pieces']}, partials {i['n_partials']}, "
                                                                 f"bundles {i['n_bundles']}, packed {i['rec_packed']})")
    return p


@pytest.mark.parametrize("k,lanes", [(16, 8), (32, 8), (128, 8), (100, 0), (102, 0)])
@pytest.mark.parametrize("rec_pack", [1, 2])
@pytest.mark.parametrize("split_rows", [1, 2])
def test_every_width_packed_or_not_summed_in_the_launch_or_after(graph, k, lanes, rec_pack, split_rows):
    """G = 8 at k = 16, 32 and 128 (four column tiles); k = 100 is the flat kernel with a partly filled last tile, k = 102 the generic
    kernel (never packed)."""
    tn = dict(KNOBS, rec_pack=rec_pack, split_rows=split_rows, **({"lanes_per_nz": lanes} if lanes else {}))
    p = check(graph, k, f"k={k} rec_pack={rec_pack} split_rows={split_rows}", tuning=tn)
    i, t = p.info(), p.tuning()
    assert t["split_rows"] == split_rows and i["rec_packed"] == (1 if rec_pack == 1 and k % 4 == 0 else 0)
    assert not lanes or i["lanes_per_nz"] == lanes
    assert i["moved_records"] == expected_moves(graph)[1]
    if k in (16, 32):
        assert i["n_bundles"] > 0  # short rows in bundles, moved pieces between them


def test_same_sum_as_the_uncut_plan_within_the_bound_and_other_bits(graph):
    """The cut changes the order a hub row is summed in, nothing else: rows that are not cut come out bit for bit."""
    k = 64
    B = random_B(N, k, seed=11)
    on = launch_twice(flex_amd.Plan(graph, k, tuning=KNOBS), graph, B, k)
    off = launch_twice(flex_amd.Plan(graph, k, tuning=OFF), graph, B, k)
    short = np.diff(graph.rowPtr.astype(np.int64)) < KNOBS["hub_row"]
    assert np.array_equal(on[short].view(np.uint32), off[short].view(np.uint32))
    assert_within_f64_bound(graph, B, on, route="cut")
    assert_within_f64_bound(graph, B, off, route="uncut")


def test_bf16_operands_on_the_same_plan(graph):
    """flex_spmm_bf16 on the plan of the same input and knobs (bf16 B and C, fp32 partial sums, spmm_fixup_bf16_kernel)."""
    import spmm_bf16_ref as ref
    k = 128
    p = flex_amd.Plan(graph, k, tuning=dict(KNOBS, lanes_per_nz=8), bf16=True)
    p.self_check()
    i = p.info()
    assert i["n_moved_pieces"] > 0 and i["bf16"] == 1 and i["moved_records"] == expected_moves(graph)[1]
    B = ref.rounded(random_B(N, k, seed=12))
    Bd = torch.from_numpy(ref.to_bf16(B).view(np.int16)).cuda().view(torch.bfloat16)
    bits = []
    for _ in range(2):
        C = p(Bd)
        torch.cuda.synchronize()
        bits.append(C.contiguous().view(torch.int16).cpu().numpy().view(np.uint16))
    assert np.array_equal(bits[0], bits[1]), "two launches differ"
    msg, worst = ref.check(graph, B, bits[0], "bf16, moved pieces")
    print(f"bf16: worst err / bound {worst:.3g}")
    assert msg is None, msg


def test_mapped_plan(graph):
    """A mapped loader (vo_mp): the plan reads B and writes C in the original order, the windows are those of the loader's ids."""
    k = 32
    vo = np.random.default_rng(5).permutation(N).astype(np.int32)
    p = flex_amd.Plan(graph, k, vo_mp=vo, tuning=KNOBS)
    p.self_check()
    assert p.info()["moved_records"] == expected_moves(graph)[1]
    B = random_B(N, k, seed=13)
    C = launch_twice(p, graph, B, k)
    # row r' of the loader's matrix is original row vo[r'], column c' original column vo[c']: C[vo] = A' B[vo]
    assert_within_f64_bound(graph, B[vo], C[vo], route="mapped")


def test_community_order(graph):
    check(graph, 128, "cluster order", order=flex_amd.FLEX_ORDER_CLUSTER, tuning=KNOBS)


def test_more_than_256_pieces_on_one_row(graph):
    for split_rows in (1, 2):
        p = check(graph, 128, f"piece_records=8 split_rows={split_rows}", tuning=dict(KNOBS, piece_records=8, split_rows=split_rows))
        assert p.info()["n_moved_pieces"] > 300


def test_tiny_pieces_among_empty_rows():
    """100 moved pieces of 4 records among the 256 empty rows of their window: more tasks than a chunk may hold before its budget is
    used up (the planner's limit of 63 tasks per wave)."""
    a = hub_graph(seed=1, tiny_pieces=True)
    for extra in ({"chunk_records": 512, "row_cost": 1}, {"chunk_records": 512, "row_cost": 1, "bundle": 2}):
        for k in (32, 128):
            check(a, k, f"tiny pieces {extra} k={k}", tuning=dict(KNOBS, **extra))

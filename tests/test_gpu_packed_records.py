"""The packed record stream on the GPU (flex_plan_tuning.rec_pack; spmm_kernels.hip, stage_window_packed).  The arithmetic of a packed
plan is the unpacked plan's -- same FMAs in the same order, same stores -- so every case asks for BIT identity between C of the plan built
with rec_pack = 1 and C of the same plan built with rec_pack = 2, and holds the result to the float64 bound of tests/f64ref.py.

Shapes: the smallest that reach each piece of the decoder.  About 4 000 rows of degree about 200 give chunks of one full window, tasks
that start in the middle of a chunk and of a lane's words, one row of 1 500 records kept whole (three windows at G = 8, six at G = 16:
the running column across windows) and one of 3 000 cut into pieces.

G = 32 exists at k = 128 only: the tile width is capped by k (4 G <= the next power of two of k), so lanes_per_nz = 32 at k = 64 is the
16-lane tile again, which (16, 64) covers.  The one-slot tile (G = 64: differences loaded record by record, windows that start at odd
records) runs k = 512 as two tiles, the sixteen-slot tile (G = 4) k = 16; both on the first 1 000 of the same rows, the row of 1 500
records among them, so that the float64 reference of the widest case stays below a gigabyte.

k = 100: the issue behind this file expected it to run the generic kernel and to come out unpacked.  It does not: k % 4 == 0 runs the
flat kernel with a partly filled last tile, and is packed when asked.  It is tested as that; the generic kernel's shapes (k = 102: never
packed, rec_packed = 0) and a packed plan launched with operands that are not 16-byte aligned (the generic kernel decodes the stream
itself) are tested next to it."""
import numpy as np
import pytest

import flex_amd
from f64ref import assert_within_f64_bound
from util import random_B, random_csr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def both(a, k, order=flex_amd.FLEX_ORDER_NATURAL, **knobs):
    packed = flex_amd.Plan(a, k, order=order, tuning=dict(knobs, rec_pack=1))
    plain = flex_amd.Plan(a, k, order=order, tuning=dict(knobs, rec_pack=2))
    assert packed.info()["rec_packed"] == 1 and packed.tuning()["rec_pack"] == 1, packed.tuning()
    assert plain.info()["rec_packed"] == 0 and plain.tuning()["rec_pack"] == 2
    packed.self_check()
    return packed, plain


def run(plan, a, B, k):
    C = torch.full((a.m, k), -7.0, device="cuda")  # every row must be written
    plan(B, out=C)
    torch.cuda.synchronize()
    return C


def check(a, k, B, packed, plain, route):
    Bd = torch.from_numpy(B).cuda()
    Cp, Cu = run(packed, a, Bd, k), run(plain, a, Bd, k)
    assert torch.equal(Cp.view(torch.int32), Cu.view(torch.int32)), f"{route}: {int((Cp.view(torch.int32) != Cu.view(torch.int32)).sum())} entries differ"
    assert_within_f64_bound(a, B, Cp.cpu().numpy(), route=route)


@pytest.fixture(scope="module")
def rows200():
    return random_csr(4000, 4000, 200, seed=21, long_rows={7: 1500, 2000: 3000}, empty_frac=0.02)


@pytest.mark.parametrize("lanes,k", [(8, 64), (8, 128), (16, 64), (16, 128), (32, 128)])
def test_windows_tasks_and_the_running_column(rows200, lanes, k):
    a = rows200
    packed, plain = both(a, k, lanes_per_nz=lanes, long_row=2000)
    info, ri = packed.info(), packed.record_info()
    assert info["lanes_per_nz"] == lanes and info["n_split_rows"] == 1 and ri["wide_records"] == 0 and ri["exceptions"] == 0
    window = 512 if lanes == 8 else 256
    assert info["n_records"] / info["n_chunks"] > 0.6 * min(window, packed.tuning()["chunk_records"])  # chunks about one window long
    assert info["n_tasks"] > 1.5 * info["n_chunks"]  # tasks start inside chunks
    check(a, k, random_B(a.n, k, seed=k + lanes), packed, plain, f"G={lanes} k={k}")


@pytest.mark.parametrize("lanes,k", [(64, 512), (64, 256), (4, 16)])
def test_the_one_slot_and_the_sixteen_slot_tile(rows200, lanes, k):
    """G = 64: one record per step, so tasks and windows start at odd records and the staging step loads record by record; G = 4: sixteen
    records per step, 512-record windows.  Row 7 (1 500 records, kept whole) carries the running column across windows."""
    a = flex_amd.HostCsr(rows200.rowPtr[:1001], rows200.col[:rows200.rowPtr[1000]], rows200.vals[:rows200.rowPtr[1000]], n=rows200.n)
    packed, plain = both(a, k, lanes_per_nz=lanes, long_row=2000, chunk_records=512)  # chunks of two or three rows: two windows at G = 64
    info, ri = packed.info(), packed.record_info()
    assert info["lanes_per_nz"] == lanes and info["n_split_rows"] == 0 and ri["wide_records"] == 0 and ri["exceptions"] == 0
    assert info["n_tasks"] > 1.5 * info["n_chunks"]
    if lanes == 64:
        rec_first = packed.records().shape[0]
        assert rec_first == a.nnz  # no padding: a task starts wherever its predecessor ends, odd records included
    check(a, k, random_B(a.n, k, seed=k + lanes), packed, plain, f"G={lanes} k={k}")


def test_exceptions_several_per_chunk():
    """64 rows over 300 000 columns in no order: nearly every difference needs its high half, from a task's second record on."""
    a = random_csr(64, 300_000, 300, seed=22, empty_frac=0.0, sorted_cols=False)
    for lanes, k in ((8, 64), (16, 128)):
        packed, plain = both(a, k, lanes_per_nz=lanes)
        ri = packed.record_info()
        assert ri["exceptions"] > 0.5 * a.nnz and ri["exceptions"] > 4 * packed.info()["n_chunks"], ri
        rp, col = a.rowPtr.astype(np.int64), a.col.astype(np.int64)  # natural order: a task starts where its row does
        assert np.any(np.abs(col[rp[:-1] + 1] - col[rp[:-1]]) >= 65536)  # one on a task's second record
        check(a, k, random_B(a.n, k, seed=3), packed, plain, f"exceptions G={lanes}")


def test_bundle_chunks_stay_wide_next_to_packed_ones():
    a = random_csr(3000, 3000, 6, seed=23, long_rows={5: 900, 1500: 400, 2999: 2500})
    for k in (32, 64):
        packed, plain = both(a, k, bundle=1)
        ri = packed.record_info()
        assert packed.info()["n_bundles"] > 100 and 0 < ri["wide_records"] < ri["records"], ri
        check(a, k, random_B(a.n, k, seed=4), packed, plain, f"bundles k={k}")


def test_empty_rows_before_between_and_after_tasks():
    rng = np.random.default_rng(24)
    m, n = 1200, 50_000
    deg = rng.integers(30, 90, size=m)
    deg[:9] = 0
    deg[400:470] = 0
    deg[rng.random(m) < 0.15] = 0
    deg[-11:] = 0
    rp = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(deg, out=rp[1:])
    col = np.concatenate([np.sort(rng.choice(n, size=d, replace=False)) for d in deg if d]).astype(np.uint32)
    a = flex_amd.HostCsr(rp.astype(np.uint32), col, rng.uniform(-1, 1, len(col)).astype(np.float32), n=n)
    for lanes, k in ((8, 64), (32, 128)):
        packed, plain = both(a, k, lanes_per_nz=lanes, bundle=2)
        check(a, k, random_B(a.n, k, seed=5), packed, plain, f"empty rows G={lanes}")


def test_k_100_and_the_generic_kernel(rows200):
    a = flex_amd.HostCsr(rows200.rowPtr[:501], rows200.col[:rows200.rowPtr[500]], rows200.vals[:rows200.rowPtr[500]], n=rows200.n)
    # k = 100: the flat kernel, last tile partly filled
    packed, plain = both(a, 100)
    check(a, 100, random_B(a.n, 100, seed=6), packed, plain, "k=100")
    # k = 102: the generic kernel's shape -- the plan declines the knob
    p = flex_amd.Plan(a, 102, tuning={"rec_pack": 1})
    assert p.info()["rec_packed"] == 0 and p.tuning()["rec_pack"] == 2
    B = random_B(a.n, 102, seed=7)
    assert_within_f64_bound(a, B, run(p, a, torch.from_numpy(B).cuda(), 102).cpu().numpy(), route="k=102")
    # a packed plan, operands off by one float: the generic kernel decodes the packed stream (exceptions included)
    wide = random_csr(300, 200_000, 40, seed=25, sorted_cols=False)
    for mat, k in ((a, 64), (wide, 64)):
        packed, plain = both(mat, k, lanes_per_nz=8)
        B = random_B(mat.n, k, seed=8)
        outs = []
        for plan in (packed, plain):
            bb = torch.zeros(mat.n * k + 1, device="cuda")
            bb[1:] = torch.from_numpy(B).cuda().ravel()
            cc = torch.full((mat.m * k + 1,), -7.0, device="cuda")
            plan.spmm(bb[1:].data_ptr(), cc[1:].data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            outs.append(cc[1:].reshape(mat.m, k).clone())
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
        assert_within_f64_bound(mat, B, outs[0].cpu().numpy(), route="unaligned, packed")

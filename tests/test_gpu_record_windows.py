"""The edges of a record window on the GPU (spmm_device.h: stage_n, stage_packed_n, tail_cases; spmm_kernels.hip: spmm_fixup_kernel,
the float4 form).  The staging step loads a window of 8-byte records two per lane (16-byte loads) wherever the tile's padding aligns
it, a packed window pair by pair, with fewer loads for short windows, and the step loop ends a window with exactly the gathers it has
steps left.  Every case is checked two ways: against the float64 bound of tests/f64ref.py, and bit for bit between rec_pack on
and off and between rec_nt on and off (the same sums in the same order).

Window lengths come from a LADDER: row j holds S j - (j % 3) records (S = 64 / G records per step; padded to S j; S j where S = 1), j = 1 .. 2 W / S + 2 U
(W = the window, U = gathers per block), and chunk_records = 1 makes every row a chunk of its own.  So there is a window of every
length from S to W in steps of S -- exactly S, one wave load's worth (128 or 256 records) and that plus S, half a window, a full one --
every step count residue mod U = 4 and 8 in a window's last block, and rows of up to two windows and a rest, whose packed columns
run on across the windows.  The same ladder with a chunk budget of three windows packs several rows into a chunk: tasks start inside
windows, at every record slot of a lane's words that S allows, and chunks span several windows.

Columns: "near" rows lie sorted inside 60 000 columns (no difference needs its high half); "far" rows are spread unsorted over 200 000
(nearly every difference is an exception: at every record position mod 8, a window's first and last slot included); "mixed" rows are
near rows with two jumps of 70 000 columns at random records (one or two exceptions per row, anywhere in a window).

Both offset forms: the plain plan's records hold byte offsets (n ldb 4 <= 2^32); the same matrix planned on a B of ldb = 5376 words
(4.3 GB, allocated once, never initialised beyond the k columns in use) holds column ids and runs the 64-bit row addressing.

Split rows: rows of exactly 2, 7, 8, 9 and 17 pieces (long_row = piece_records = 64), summed by the fix-up kernel: its float4 form at
k = 32 (eight rows per wave), 128 (two), 100 (two, on 50 lanes) and 320 (one, two trips), its scalar form behind the generic kernel at
k = 30; wherever the flat kernel runs, the in-launch piece sum (split_rows = 1) must give the same bits."""
import numpy as np
import pytest

import flex_amd
from f64ref import assert_within_f64_bound

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 200_000          # columns: differences of 65 536 and more exist
WIDE_LDB = 5376      # N x 5376 x 4 > 2^32: column ids in the records, 64-bit row addressing
TILES = [(4, 16), (8, 32), (16, 64), (32, 128), (64, 256)]  # (lanes per record, k): one column tile each


def window_of(G):
    return 512 if G <= 8 else 256


def ladder(G, mode, seed):
    S, W, U = 64 // G, window_of(G), 8  # U = 8 covers the residues of 4 as well
    rng = np.random.default_rng(seed)
    lens = [S * j - (j % 3 if S > 1 else 0) for j in range(1, 2 * W // S + 2 * U + 1)]  # padded to S j
    rng.shuffle(lens)
    cols = []
    for n in lens:
        if mode == "near":
            c = np.sort(rng.integers(0, 60_000, size=n))
        elif mode == "far":
            c = rng.integers(0, N, size=n)
        else:
            c = np.sort(rng.integers(0, 60_000, size=n))
            for at in rng.integers(1, max(n, 2), size=2):  # two jumps of 70 000 at random records: one exception each
                c[at:] += 70_000
        cols.append(c)
    rp = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=rp[1:])
    col = np.concatenate(cols).astype(np.uint32)
    return flex_amd.HostCsr(rp.astype(np.uint32), col, rng.uniform(-1, 1, len(col)).astype(np.float32), n=N)


@pytest.fixture(scope="module")
def dense():
    """B for the widest tile (narrower ones take its first k columns), and the 4.3 GB buffer of the 64-bit form."""
    B = np.random.default_rng(77).uniform(-1, 1, size=(N, 256)).astype(np.float32)
    wide = torch.empty(N * WIDE_LDB, dtype=torch.float32, device="cuda").view(N, WIDE_LDB)
    return B, wide


def operand(dense, k, form):
    B, wide = dense
    Bk = np.ascontiguousarray(B[:, :k])
    if form == "off32":
        return Bk, torch.from_numpy(Bk).cuda(), None
    wide[:, :k] = torch.from_numpy(Bk).cuda()
    return Bk, wide, WIDE_LDB


def run(plan, a, k, Bd):
    C = torch.full((a.m, k), -7.0, device="cuda")  # every row must be written
    plan.spmm(Bd.data_ptr(), C.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return C


def same_bits(x, y):
    return torch.equal(x.view(torch.int32), y.view(torch.int32))


def four_ways(a, k, Bk, Bd, ldb, route, **knobs):
    """rec_pack on / off x rec_nt on / off: four plans, one result, within the float64 bound."""
    outs = {}
    for pack in (1, 2):
        for nt in (1, 2):
            plan = flex_amd.Plan(a, k, ldb=ldb, tuning=dict(knobs, rec_pack=pack, rec_nt=nt))
            info, tn = plan.info(), plan.tuning()
            assert info["rec_packed"] == (pack == 1) and tn["rec_nt"] == nt and info["lanes_per_nz"] == knobs["lanes_per_nz"], (info, tn)
            plan.self_check()
            outs[pack, nt] = run(plan, a, k, Bd)
            last = plan
    first = outs[1, 1]
    for key, C in outs.items():
        assert same_bits(first, C), f"{route}: rec_pack, rec_nt = {key} differs from (1, 1) in {int((first.view(torch.int32) != C.view(torch.int32)).sum())} entries"
    assert_within_f64_bound(a, Bk, first.cpu().numpy(), route=route)
    return last


def exception_slots(a, W):
    """Where the packed stream of a ladder plan (a row = a task = a chunk, natural order) holds exceptions: the window slot of every
    record whose column differs from its predecessor's in the task by 65 536 or more, modulo 2^32 (plan_build.cpp)."""
    rp, col = a.rowPtr.astype(np.int64), a.col.astype(np.int64)
    pos = np.arange(a.nnz) - np.repeat(rp[:-1], np.diff(rp))  # record index inside its row = inside its chunk
    d = np.zeros(a.nnz, dtype=np.int64)
    d[1:] = (col[1:] - col[:-1]) % (1 << 32)
    return pos[(pos > 0) & (d >= 65536)] % W


def chunks_by_cost(a, S, budget, row_cost=16, max_tasks=63):
    """pack_tasks_into_chunks (plan_build.cpp) on whole rows in natural order: (first record of the chunk, first record of the task)
    for every task."""
    out, pos, cost, first, zb = [], 0, 0, None, 0
    for t, n in enumerate(np.diff(a.rowPtr.astype(np.int64))):
        if first is None or cost >= budget or t - first >= max_tasks:
            first, cost, zb = t, 0, pos
        cost += int(n) + row_cost
        out.append((zb, pos))
        pos += (int(n) + S - 1) // S * S
    return out


@pytest.mark.parametrize("form", ["off32", "wide64"])
@pytest.mark.parametrize("mode", ["near", "far", "mixed"])
@pytest.mark.parametrize("G,k", TILES)
def test_a_window_of_every_length(dense, G, k, mode, form):
    a = ladder(G, mode, seed=G)
    Bk, Bd, ldb = operand(dense, k, form)
    unrolls = (0, 8) if G in (8, 16) else (0,)  # unroll = 8: the eight-gather block on the narrow tiles, seven partial cases
    for unroll in unrolls:
        knobs = dict(lanes_per_nz=G, chunk_records=1, long_row=1 << 20, bundle=2)
        if unroll:
            knobs["unroll"] = unroll
        plan = four_ways(a, k, Bk, Bd, ldb, f"ladder G={G} {mode} {form} unroll={unroll}", **knobs)
        info = plan.info()
        assert info["n_chunks"] == info["n_tasks"] == a.m and info["n_split_rows"] == 0  # a row, a chunk
        S = 64 // G
        assert info["n_records"] == sum((int(d) + S - 1) // S * S for d in np.diff(a.rowPtr.astype(np.int64)))
    ri = flex_amd.Plan(a, k, ldb=ldb, tuning=dict(lanes_per_nz=G, chunk_records=1, long_row=1 << 20, bundle=2, rec_pack=1)).record_info()
    W = window_of(G)
    slots = exception_slots(a, W)
    assert ri["exceptions"] == len(slots)  # the host model of where they are is the planner's
    if mode == "near":
        assert ri["exceptions"] == 0
    elif mode == "far":
        assert ri["exceptions"] > 0.5 * a.nnz
        # at every record position mod 8, in a window's first slot (of a second window) and in its last
        assert set((slots % 8).tolist()) == set(range(8)) and (slots == 0).any() and (slots == W - 1).any()
    else:
        assert 0 < ri["exceptions"] < 0.5 * a.nnz
        assert set((slots % 8).tolist()) == set(range(8))
    # window lengths (records, after padding): exactly S, one wave load's worth and that plus S, half a window, a full one; and the
    # steps left for a window's last block take every residue mod 8 (hence mod 4)
    padded = (np.diff(a.rowPtr.astype(np.int64)) + S - 1) // S * S
    last = np.where(padded % W == 0, W, padded % W)  # records of a row's last window
    for want in {S, 128, 128 + S, 256, 256 + S, W // 2, W} - {n for n in (128 + S, 256, 256 + S) if n > W}:
        assert (last == want).any() or want < S, want
    assert set(((last // S) % 8).tolist()) == set(range(8)) and (padded > 2 * W).any()


@pytest.mark.parametrize("form", ["off32", "wide64"])
@pytest.mark.parametrize("G,k", TILES)
def test_chunks_of_several_rows_and_several_windows(dense, G, k, form):
    """A budget of three windows: rows share chunks, so tasks start inside windows and the running column crosses them."""
    Bk, Bd, ldb = operand(dense, k, form)
    for mode in ("far", "mixed"):
        a = ladder(G, mode, seed=100 + G)
        plan = four_ways(a, k, Bk, Bd, ldb, f"three windows G={G} {mode} {form}", lanes_per_nz=G, chunk_records=3 * window_of(G),
                         long_row=1 << 20, bundle=2)
        info = plan.info()
        assert info["n_split_rows"] == 0 and info["n_tasks"] == a.m
        assert info["n_records"] / info["n_chunks"] > 2 * window_of(G)  # chunks of more than two windows on average
        assert info["n_tasks"] > 2 * info["n_chunks"]
        # where tasks start inside a window: every slot of a lane's 8 records that whole steps allow (multiples of S mod 8), in windows
        # after a chunk's first as well
        S, W = 64 // G, window_of(G)
        starts = chunks_by_cost(a, S, 3 * W)
        assert len({zb for zb, _ in starts}) == info["n_chunks"]  # the host model of the chunks is the planner's
        inside = np.array([(tb - zb) for zb, tb in starts if tb > zb])
        assert set((inside % W % 8).tolist()) == set(range(0, 8, S))  # S = 8, 16: {0}
        assert (inside >= W).any() and (inside % W != 0).any()


def split_graph(seed):
    """1 500 rows of 1 to 40 nonzeros, and rows of 2, 7, 8, 9 and 17 times 64 among them."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(1, 41, size=1500)
    pieces = {100: 2, 400: 7, 401: 8, 900: 9, 1499: 17}
    for r, q in pieces.items():
        deg[r] = 64 * q
    rp = np.zeros(len(deg) + 1, dtype=np.int64)
    np.cumsum(deg, out=rp[1:])
    col = np.concatenate([np.sort(rng.integers(0, N, size=d)) for d in deg]).astype(np.uint32)
    return flex_amd.HostCsr(rp.astype(np.uint32), col, rng.uniform(-1, 1, len(col)).astype(np.float32), n=N), pieces


@pytest.mark.parametrize("k", [32, 128, 100, 320, 30])
def test_split_rows_of_2_7_8_9_and_17_pieces(k):
    a, pieces = split_graph(5)
    Bk = np.random.default_rng(k).uniform(-1, 1, size=(N, k)).astype(np.float32)
    Bd = torch.from_numpy(Bk).cuda()
    knobs = dict(long_row=64, piece_records=64, bundle=2, split_rows=2)
    if k % 4:  # the generic kernel: never packed, always the fix-up kernel -- its scalar form
        plan = flex_amd.Plan(a, k, tuning=knobs)
        assert plan.info()["rec_packed"] == 0
        C = run(plan, a, k, Bd)
        info = plan.info()
    else:
        knobs["lanes_per_nz"] = {32: 8, 128: 32, 100: 32, 320: 64}[k]
        plan = four_ways(a, k, Bk, Bd, None, f"split rows k={k}", **knobs)
        info = plan.info()
        C = run(plan, a, k, Bd)
        for pack in (1, 2):
            fused = flex_amd.Plan(a, k, tuning=dict(knobs, split_rows=1, rec_pack=pack))
            assert fused.tuning()["split_rows"] == 1 and fused.info()["rec_packed"] == (pack == 1)
            for _ in range(3):  # the arrival counters re-arm themselves
                assert same_bits(C, run(fused, a, k, Bd)), f"k={k} rec_pack={pack}: the in-launch piece sum and the fix-up kernel differ"
    assert info["n_split_rows"] == len(pieces) and info["n_partials"] == sum(pieces.values()), info
    assert_within_f64_bound(a, Bk, C.cpu().numpy(), route=f"split rows k={k}")


def test_split_rows_unaligned_c_takes_the_scalar_fixup():
    """C one float off a 16-byte boundary: the generic kernel and the scalar fix-up, on a packed plan of k = 32."""
    a, pieces = split_graph(6)
    k = 32
    Bk = np.random.default_rng(9).uniform(-1, 1, size=(N, k)).astype(np.float32)
    Bd = torch.from_numpy(Bk).cuda()
    plan = flex_amd.Plan(a, k, tuning=dict(long_row=64, piece_records=64, bundle=2, split_rows=2, lanes_per_nz=8, rec_pack=1))
    aligned = run(plan, a, k, Bd)
    cc = torch.full((a.m * k + 1,), -7.0, device="cuda")
    plan.spmm(Bd.data_ptr(), cc[1:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert plan.info()["n_split_rows"] == len(pieces)
    assert_within_f64_bound(a, Bk, cc[1:].reshape(a.m, k).cpu().numpy(), route="unaligned C")
    assert_within_f64_bound(a, Bk, aligned.cpu().numpy(), route="aligned C")
    split = sorted(pieces)
    # a split row's pieces are the same partial sums either way (the flat and the generic kernel sum a piece in different orders, the
    # fix-up forms do not): the scalar form on the aligned pieces is covered by k = 30 above, so here only the bound is asked of each
    assert float(cc[0]) == -7.0 and torch.isfinite(cc[1:].reshape(a.m, k)[split]).all()

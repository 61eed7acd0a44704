"""The graphs on which the fused-attention walks run under group budgets above the floor (tests/test_attention_walks_host.py and
tests/test_gpu_attention_walks.py), beside tests/attention_forms.py.

internal.h: attention_group_budget(cost) = cost / 4096 rounded up to 64, clamped to 64 .. 2048, cost = entries + rows (entries + columns
for the column walk).  The four graphs the other attention files share all plan at 64; these plan at 128, 512 and 2048:

    walk_graph(1)    the lift of budget_base(): 70 000 rows and columns, 213 658 entries, every class of row and of column
    walk_graph(7)    7 copies of it on the diagonal
    walk_graph(30)   30 copies: the clamp

and multi_edge_graph() is thresholds_lifted with its columns shuffled within every row and a tenth of its entries repeated in the same
row: unsorted rows and multi-edges, where "in a's CSR order" and "ordered by column" differ.

BUDGETS and MIN_ITEMS_PER_GROUP are declarations, written down from a run of the host simulator, not computed by the rule they check:
tests/test_attention_walks_host.py holds every plan to them."""
import numpy as np

from flex_amd.binding import HostCsr
from fused_attention_backward_ref import both_sides
from fused_attention_ref import coo, threshold_graph

BASE_ROWS = 35_000
BOUNDARY_ROWS = (511, 512, 513, 514, 700, 1500)  # slot / wave / block boundaries (internal.h: kAtWaveRow = 512) and two block rows
# T -> the group budget of both walks, at every k
BUDGETS = {1: 128, 7: 512, 30: 2048}
# T -> the least items / groups of both walks at k = 8 (W = 4: 16 rows per slot item), rounded down to what the cases claim
MIN_ITEMS_PER_GROUP = {1: 1.5, 7: 7.5, 30: 33.0}
_graphs = {}


def budget_base(seed=1):
    """A seeded random pattern of 35 000 x 35 000: row lengths uniform in 0 .. 6; 1 row in 200 reset to 33 .. 79 entries (a wave row);
    six rows of 511, 512, 513, 514, 700 and 1500 entries; then a tenth of the rows emptied (the six kept); columns sorted within a row
    and chosen without replacement."""
    rng = np.random.default_rng([seed, 35])
    m = n = BASE_ROWS
    deg = rng.integers(0, 7, m)
    wave = rng.random(m) < 1 / 200
    deg[wave] = rng.integers(33, 80, int(wave.sum()))
    special = rng.choice(m, len(BOUNDARY_ROWS), replace=False)
    emptied = rng.random(m) < 0.1
    deg[emptied] = 0
    deg[special] = BOUNDARY_ROWS
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    col = np.empty(int(rp[-1]), np.uint32)
    for r in np.flatnonzero(deg):
        col[rp[r]:rp[r + 1]] = np.sort(rng.choice(n, deg[r], replace=False))
    return HostCsr(rp, col, rng.uniform(-1, 1, len(col)).astype(np.float32), n=n)


def tiled(g, T):
    """The block-diagonal graph of T copies of g: copy t has its rows, columns and entries shifted by t m, t n and t nnz."""
    rp = g.rowPtr.astype(np.int64)
    rowptr = np.concatenate([[0]] + [rp[1:] + t * g.nnz for t in range(T)]).astype(np.uint32)
    col = np.concatenate([g.col.astype(np.int64) + t * g.n for t in range(T)]).astype(np.uint32)
    return HostCsr(rowptr, col, np.tile(g.vals, T), n=T * g.n)


def walk_graph(T, seed=1):
    """tiled(both_sides(budget_base(seed)), T), made once."""
    if (T, seed) not in _graphs:
        _graphs[(T, seed)] = both_sides(budget_base(seed)) if T == 1 else tiled(walk_graph(1, seed), T)
    return _graphs[(T, seed)]


def tile_rows(x, T):
    """A row or edge operand of walk_graph(1) repeated for the T copies."""
    return np.ascontiguousarray(np.tile(x, (T,) + (1,) * (x.ndim - 1)))


# ---- the check of the copies: every copy's block of an output has the bits of the budget-128 run

def _bits(x):
    """The bits of a float32 array or tensor as int32, of bf16 bits (uint16) or a bfloat16 tensor as int16: a torch tensor."""
    import torch
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x.view(np.int32) if x.dtype == np.float32 else x.view(np.int16))
    return x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def assert_copies(what, key, got, base, T, empty=None):
    """got ([T rows, ...]: numpy, or a torch tensor on any device) holds, in each of its T blocks of rows, the bits of base ([rows, ...]);
    the first differing (copy, row, column) is reported.  An output that started at a sentinel and was not written differs too.
    empty (bool [rows]): these rows of every copy are +0 bits."""
    g, b = _bits(got), _bits(base)
    rows = b.shape[0]
    assert g.shape[0] == T * rows and g.shape[1:] == b.shape[1:] and g.dtype == b.dtype, f"{what}: {key} is {tuple(g.shape)} {g.dtype}, {T} copies of {tuple(b.shape)} {b.dtype}"
    g, b = g.reshape(T, rows, -1), b.reshape(1, rows, -1).to(g.device)
    differ = g != b
    if bool(differ.any()):
        c, r, j = (int(v) for v in differ.nonzero()[0])
        raise AssertionError(f"{what}: {key} has not the bits of the one-copy run: first at copy {c}, row {r}, column {j} "
                             f"({int(g[c, r, j])} for {int(b[0, r, j])}); {int(differ.sum())} elements differ")
    if empty is not None:
        import torch
        e = torch.from_numpy(np.asarray(empty, bool)).to(g.device)
        assert not bool(g[:, e].any()), f"{what}: {key} is not +0 on a line without entries"


# ---- a numpy restatement of the work list (plan_build.cpp, build_attention_walk), for models of kernels that walk it wrongly

def slots_of(k):
    """The slots of a wave: 64 lanes over slots of W lanes (internal.h, sddmm_lanes)."""
    w = 4
    while 4 * w < k and w < 64:
        w <<= 1
    return 64 // w


def walk_model(ptr, k, budget):
    """(items [n, 4] = (first entry, entries, first line, lines) of the grouped items, grp [groups + 1], blocks [n_b, 4]) of the walk
    over the lines of `ptr` (the row pointer, or the column pointer for the column walk) under a group budget."""
    ptr = np.asarray(ptr, np.int64)
    slots = slots_of(k)
    items, blocks, grp = [], [], []
    cost = [0]

    def add(first, cnt, line, lines):
        if not grp or cost[0] + cnt + lines > budget:
            grp.append(len(items))
            cost[0] = 0
        items.append((first, cnt, line, lines))
        cost[0] += cnt + lines

    run = [0, 0, 0]  # first line, lines, entries of the slot item being filled

    def close():
        if run[1]:
            add(int(ptr[run[0]]), run[2], run[0], run[1])
        run[1] = run[2] = 0

    for r, ln in enumerate(np.diff(ptr).tolist()):
        if ln > 32:
            close()
            (add if ln <= 512 else lambda *it: blocks.append(it))(int(ptr[r]), ln, r, 1)
            continue
        if run[1] == slots:
            close()
        if run[1] == 0:
            run[0] = r
        run[2] += ln
        run[1] += 1
    close()
    grp.append(len(items))
    return np.array(items, np.int64).reshape(-1, 4), np.array(grp, np.int64), np.array(blocks, np.int64).reshape(-1, 4)


def walk_places(ptr, k, budget):
    """dict of per-line arrays over the lines of ptr: item (the grouped item of the line, -1 on a block line), group (-1 likewise),
    later (the line's item is not the first of its group), and shift (entries of the first item of the group, 0 on the first item and on
    block lines); n_groups."""
    items, grp, _ = walk_model(ptr, k, budget)
    n = len(ptr) - 1
    item_of = np.full(n, -1, np.int64)
    item_of[np.repeat(items[:, 2], items[:, 3]) + (np.arange(int(items[:, 3].sum())) - np.repeat(np.cumsum(items[:, 3]) - items[:, 3], items[:, 3]))] = \
        np.repeat(np.arange(len(items)), items[:, 3])
    group_of_item = np.searchsorted(grp, np.arange(len(items)), side="right") - 1
    first_of_group = grp[group_of_item]
    on = item_of >= 0
    group = np.where(on, group_of_item[item_of], -1)
    later = on & (item_of != first_of_group[item_of])
    shift = np.where(later, items[first_of_group[item_of], 1], 0)
    return dict(item=item_of, group=group, later=later, shift=shift, n_groups=len(grp) - 1, items=items, grp=grp)


def multi_edge_graph(seed=3):
    """thresholds_lifted with the columns of every row shuffled, and a tenth of the entries repeated in their row (the copy is put at a
    random place of the row): rows cross 32 -> 33 and 512 -> 513 by the repeats alone.  (graph, first [nnz]): first[e] is the earliest
    entry of e's row with e's column, e itself where the pair occurs once."""
    if ("multi", seed) in _graphs:
        return _graphs[("multi", seed)]
    a = both_sides(threshold_graph())
    rng = np.random.default_rng([seed, 77])
    row, col, rp = coo(a)
    again = rng.random(a.nnz) < 0.1
    rows = np.concatenate([row, row[again]])
    cols = np.concatenate([col, col[again]])
    order = np.lexsort((rng.random(len(rows)), rows))  # by row, a random order inside it
    rows, cols = rows[order], cols[order]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=a.m))]).astype(np.uint32)
    g = HostCsr(rowptr, cols.astype(np.uint32), rng.uniform(-1, 1, len(cols)).astype(np.float32), n=a.n)
    key = rows * a.n + cols
    by_key = np.argsort(key, kind="stable")
    new = np.concatenate([[True], key[by_key][1:] != key[by_key][:-1]])
    first = np.empty(len(key), np.int64)
    first[by_key] = by_key[np.maximum.accumulate(np.where(new, np.arange(len(key)), 0))]
    _graphs[("multi", seed)] = (g, first)
    return g, first

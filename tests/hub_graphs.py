"""Inputs of the hub-row tests (tests/test_hub_pieces_host.py, tests/test_gpu_hub_pieces.py): hub rows cut by schedule window
(flex_plan_tuning.hub_row; plan_build.cpp, cut_hub_rows).

N = 4096 vertices in natural order, windows of W = 256 schedule positions (16 of them), short rows everywhere and a dozen planted long
rows.  The knobs KNOBS force the cut at this size: rows of 256 records or more, runs of 4 or more, a chunk budget of 128 records, and
rows or runs longer than 128 records cut by length (long_row; at this size the planner would otherwise keep rows of up to 384 records
whole, and no window of 256 columns could hold a run longer than one budget)."""
import numpy as np

import flex_amd

N, W = 4096, 256
KNOBS = {"hub_row": 256, "hub_window": W, "hub_min_run": 4, "chunk_records": 128, "long_row": 128}
OFF = dict(KNOBS, hub_row=1)

# planted rows
SPREAD = {5: 3000, 700: 600, 1024: 900, 1500: 1300, 2047: 2000, 2222: 750, 2900: 2500, 4000: 1100}  # columns over all windows
EMPTY_HOME = 10      # window 0: 100 columns each in windows 3, 7 and 9, none near the row
ONE_MOVED = 300      # window 1: 200 columns of its own window (its own column 300 among them), 60 of window 5, 3 of window 9 (too few to move)
LONG_RUN = 2600      # window 10: 250 columns of window 2 (a moved run of two budgets), 100 of its own window
NONFINITE = 1800     # window 7: 252 columns of its own window, 5 of window 11 -- a moved piece that is padded, its last value +inf


def _in_window(rng, w, count):
    return w * W + np.sort(rng.choice(W, size=count, replace=False))


def hub_graph(seed=0, tiny_pieces=False):
    """tiny_pieces: rows 800..899 (window 3) also hold all 256 columns of their own window and 4 columns of window 14, whose own 256
    rows are empty: 100 moved pieces of 4 records among empty rows -- more than 63 tasks before any chunk budget is used up."""
    rng = np.random.default_rng(seed)
    rows = {}
    for r in range(N):
        d = 0 if rng.random() < 0.08 else int(rng.poisson(5))
        rows[r] = np.sort(rng.choice(N, size=d, replace=False))
    for r, d in SPREAD.items():
        rows[r] = np.sort(rng.choice(N, size=d, replace=False))
    rows[EMPTY_HOME] = np.concatenate([_in_window(rng, w, 100) for w in (3, 7, 9)])
    others = np.setdiff1d(np.arange(W, 2 * W), [ONE_MOVED])
    own = np.sort(np.append(rng.choice(others, size=199, replace=False), ONE_MOVED))
    rows[ONE_MOVED] = np.concatenate([own, _in_window(rng, 5, 60), _in_window(rng, 9, 3)])
    rows[LONG_RUN] = np.concatenate([_in_window(rng, 2, 250), _in_window(rng, 10, 100)])
    rows[NONFINITE] = np.concatenate([_in_window(rng, 7, 252), _in_window(rng, 11, 5)])
    if tiny_pieces:
        for r in range(800, 900):
            rows[r] = np.concatenate([np.arange(3 * W, 4 * W), _in_window(rng, 14, 4)])
        for r in range(14 * W, 15 * W):
            rows[r] = np.zeros(0, np.int64)
    rp = np.zeros(N + 1, np.int64)
    np.cumsum([len(rows[r]) for r in range(N)], out=rp[1:])
    col = np.concatenate([rows[r] for r in range(N)]).astype(np.uint32)
    vals = rng.uniform(-1, 1, len(col)).astype(np.float32)
    vals[rp[NONFINITE + 1] - 1] = np.inf
    return flex_amd.HostCsr(rp.astype(np.uint32), col, vals, n=N)


def expected_moves(a, knobs=KNOBS, pos=None):
    """(moved runs, moved records, hub rows with an empty home part) by the rule of cut_hub_rows, from the CSR alone.  pos: schedule
    position of every vertex (None: its id)."""
    rp, col = a.rowPtr.astype(np.int64), a.col.astype(np.int64)
    pos = np.arange(a.m) if pos is None else np.asarray(pos)
    runs = records = empty_home = 0
    for r in np.nonzero(np.diff(rp) >= knobs["hub_row"])[0]:
        w, cnt = np.unique(pos[col[rp[r]:rp[r + 1]]] // knobs["hub_window"], return_counts=True)
        moves = (cnt >= knobs["hub_min_run"]) & (w != pos[r] // knobs["hub_window"])
        runs += int(moves.sum())
        records += int(cnt[moves].sum())
        empty_home += int(moves.any() and cnt[moves].sum() == rp[r + 1] - rp[r])
    return runs, records, empty_home


def expected_moved_pieces(a, slots, knobs=KNOBS):
    """Moved pieces by the rules of cut_hub_rows and cut_run, from the CSR alone: a moved run of more than long_row records is cut
    into min(ceil(len / piece), 256) parts of equal length rounded up to whole steps of `slots` records (piece: piece_records, else
    the chunk budget, in whole steps)."""
    rp, col = a.rowPtr.astype(np.int64), a.col.astype(np.int64)
    piece = max(slots, knobs.get("piece_records", knobs["chunk_records"]) // slots * slots)
    n = 0
    for r in np.nonzero(np.diff(rp) >= knobs["hub_row"])[0]:
        w, cnt = np.unique(col[rp[r]:rp[r + 1]] // knobs["hub_window"], return_counts=True)
        for c in cnt[(cnt >= knobs["hub_min_run"]) & (w != r // knobs["hub_window"])]:
            if c <= knobs["long_row"]:
                n += 1
                continue
            parts = min(-(-int(c) // piece), 256)
            per = -(-(-(-int(c) // parts)) // slots) * slots
            n += -(-int(c) // per)
    return n

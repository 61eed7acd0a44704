"""FLEX_PLAN_BF16 (include/flex_spmm.h) WITHOUT a GPU, through the host-simulated library: a bf16 plan is the fp32 plan
of the row width in 4-byte words (same tile, records, chunks, pieces), its refusals return their stated codes and leave *out NULL, the
other plan flags work on it, and the checker of tests/spmm_bf16_ref.py rejects planted faults and accepts float64 rounded once."""
import ctypes as C
import os

import numpy as np
import pytest

import f64ref
import flex_amd
import spmm_bf16_ref as ref
from conftest import GOLDEN
from flex_amd import binding

import hostsim  # tests/hostsim: the project's own module -- a failure to import it is a failure

OK, INVALID, UNSUPPORTED = 0, -1, -4
FORCED = {"mfma": 2, "blocks": 2, "split_rows": 2}  # what a bf16 plan forces


@pytest.fixture(scope="module")
def sim():
    so = os.environ.get("FLEX_HOSTSIM_LIB") or hostsim.build()
    old_so, old_lib = binding._SO, binding._lib
    binding._SO, binding._lib = so, None
    L = binding.lib()
    yield L
    binding._SO, binding._lib = old_so, old_lib


def _degree3(m=3000):
    rng = np.random.default_rng(3)
    col = np.stack([rng.permutation(m)[:3] for _ in range(m)]).astype(np.uint32)
    return flex_amd.HostCsr((np.arange(m + 1) * 3).astype(np.uint32), col.ravel(), rng.uniform(-1, 1, 3 * m).astype(np.float32), n=m)


def _with_empty_rows():
    a, _, _, _ = ref.case("k64_g8", "empty")
    return a


def graphs():
    return {
        "pubmed": lambda: flex_amd.csv_load(os.path.join(GOLDEN, "pubmed.csv")),
        "scenario": lambda: f64ref.scenario("wide", k=8, m=512)[0],  # rows of 400, 200 and 97 entries: longer than the chunk budget
        "degree3": _degree3,
        "empty_rows": _with_empty_rows,
    }


# ---- a. planning in words

@pytest.mark.parametrize("k", [8, 32, 64, 128, 256, 512])
@pytest.mark.parametrize("name", list(graphs()))
def test_a_bf16_plan_is_the_fp32_plan_of_the_word_width(sim, name, k):
    a = graphs()[name]()
    tn = dict(f64ref.SPLIT) if name == "scenario" else {}
    if name == "degree3":
        tn["bundle"] = 1
    ld = k + 16
    for ldb, ldc in ((None, None), (ld, ld + 8)):
        h = flex_amd.Plan(a, k, ldb=ldb, ldc=ldc, tuning=tn, bf16=True)
        w = flex_amd.Plan(a, k // 2, ldb=ldb and ldb // 2, ldc=ldc and ldc // 2, tuning={**tn, **FORCED})
        h.self_check()
        hi, wi = h.info(), w.info()
        assert hi["bf16"] == 1 and wi["bf16"] == 0
        assert hi["k"] == k and wi["k"] == k // 2  # elements, both
        for key in ("lanes_per_nz", "n_records", "n_tasks", "n_chunks", "n_slots", "n_split_rows", "n_partials", "n_bundles", "rec_packed", "two_d",
                    "n_tiles", "n_blocks"):
            assert hi[key] == wi[key], (key, hi[key], wi[key])
        assert hi["n_tiles"] == 0 and hi["n_blocks"] == 0
        ht, wt = h.tuning(), w.tuning()
        assert ht == wt, {f: (ht[f], wt[f]) for f in ht if ht[f] != wt[f]}
        assert ht["mfma"] == 2 and ht["split_rows"] == 2  # as resolved; no tile and no block exists (above)
        assert h.record_info() == w.record_info()
        # the records carry the B-row byte offsets (or column ids where the offsets need 64 bits): off32 and ldb in words are in them
        assert np.array_equal(h.records(), w.records())
        # the partial sums are fp32, one per ELEMENT: n_partials x k floats against n_partials x k / 2
        floats = lambda n, width: max(1, n * width)  # noqa: E731
        assert hi["device_bytes"] - wi["device_bytes"] == 4 * (floats(hi["n_partials"], k) - floats(hi["n_partials"], k // 2))
        if name == "scenario":
            assert hi["n_partials"] > 0
        if name == "degree3" and hi["lanes_per_nz"] <= 16:
            assert hi["n_bundles"] > 0
    print(f"{name} k={k}: lanes_per_nz {hi['lanes_per_nz']}, records {hi['n_records']}, partials {hi['n_partials']}, bundles {hi['n_bundles']}")


def test_a_64_bit_offsets_start_where_the_bf16_rows_pass_4_gib(sim):
    """off32 is decided on n x ldb x 2 bytes: the records of a plan just below hold byte offsets, just above column ids."""
    rng = np.random.default_rng(5)
    n, ldb = 1 << 16, 1 << 15  # n x ldb x 2 = 4 GiB exactly: the largest 32-bit plan
    col = rng.integers(0, n, size=(64, 4)).astype(np.uint32)
    col[0, 0] = n - 1
    rp = (np.arange(65) * 4).astype(np.uint32)
    vals = rng.uniform(-1, 1, 256).astype(np.float32)
    for cols, off32 in ((n, True), (n + 8, False)):
        a = flex_amd.HostCsr(rp, col.ravel(), vals, n=cols)
        h = flex_amd.Plan(a, 64, ldb=ldb, ldc=64, bf16=True)
        h.self_check()
        x = h.records()[:, 0].astype(np.int64)
        assert x.max() == ((n - 1) * ldb * 2 if off32 else n - 1)
        assert np.array_equal(h.records(), flex_amd.Plan(a, 32, ldb=ldb // 2, ldc=32, tuning=FORCED).records())


# ---- b. refusals

def _create_ex(L, a, k, flags=0, ldb=0, ldc=0, tuning=None):
    """flex_plan_create_ex with *out preset to a non-NULL value: (status, *out afterwards)."""
    v = a.view()
    tn = binding._tuning(tuning or {})
    d = binding._PlanDesc(C.sizeof(binding._PlanDesc), C.pointer(v), k, ldb, ldc, 0, flags | binding.FLEX_PLAN_BF16, 0, 0, None, None,
                          None if tn is None else C.pointer(tn))
    h = C.c_void_p(0xDEAD0)
    rc = L.flex_plan_create_ex(C.byref(h), C.byref(d))
    return rc, h


@pytest.mark.parametrize("what,kw", [
    ("k % 8", dict(k=36)), ("k % 8 (4)", dict(k=4)), ("ldb % 8", dict(k=32, ldb=36)), ("ldc % 8", dict(k=32, ldc=44)),
    ("mfma = 1", dict(k=32, tuning={"mfma": 1})), ("blocks = 1", dict(k=64, tuning={"blocks": 1})),
    ("split_rows = 1", dict(k=32, tuning={"split_rows": 1})), ("two_d = 1", dict(k=32, tuning={"two_d": 1, "panel_kb": 1})),
    ("mutable values", dict(k=32, flags=binding.FLEX_PLAN_MUTABLE_VALUES)), ("attention", dict(k=32, flags=binding.FLEX_PLAN_ATTENTION)),
    ("attention backward", dict(k=32, flags=binding.FLEX_PLAN_ATTENTION | binding.FLEX_PLAN_ATTENTION_BACKWARD)),
    ("autotune", dict(k=32, flags=binding.FLEX_PLAN_AUTOTUNE)),
])
def test_b_refusals_are_unsupported_and_leave_out_null(sim, what, kw):
    a = f64ref.scenario("wide", k=8, m=512)[0]
    rc, h = _create_ex(sim, a, **kw)
    assert rc == UNSUPPORTED, (what, rc)
    assert h.value is None, what
    # the same request without the flag's conflict is a plan
    rc, h = _create_ex(sim, a, 32)
    assert rc == OK and h.value
    sim.flex_plan_destroy(h)


def test_b_calls_on_the_wrong_kind_of_plan(sim):
    a = f64ref.scenario("wide", k=8, m=512)[0]
    h = flex_amd.Plan(a, 64, order=flex_amd.FLEX_ORDER_RCM | flex_amd.FLEX_PLAN_STATS, tuning=f64ref.SPLIT, bf16=True)
    sim.hostsim_launch_log(1)  # launchers would report FLEX_OK and log: a refusal must come before them
    try:
        assert sim.flex_spmm(h._h, 0x1000, 0x2000, None) == INVALID
        im = binding._Imbalance()
        assert sim.flex_plan_measure_imbalance(h._h, 0x1000, 0x2000, None, C.byref(im)) == INVALID
        sim.hostsim_launch_log_read.restype = C.c_char_p
        assert sim.hostsim_launch_log_read().decode() == ""
    finally:
        sim.hostsim_launch_log(0)
    ki = binding._KernelInfo()
    assert sim.flex_plan_kernel_info(h._h, C.byref(ki)) == UNSUPPORTED
    assert sim.flex_plan_is_bf16(h._h) == 1 and sim.flex_plan_is_bf16(None) == INVALID
    # what reads the plan works, and reports the plan of the word width
    h.self_check()
    w = flex_amd.Plan(a, 32, order=flex_amd.FLEX_ORDER_RCM | flex_amd.FLEX_PLAN_STATS, tuning={**f64ref.SPLIT, **FORCED})
    assert h.stats() == w.stats() and h.tuning() == w.tuning() and h.record_info() == w.record_info()
    assert np.array_equal(h.records(), w.records())
    assert w.info()["bf16"] == 0 and sim.flex_plan_is_bf16(w._h) == 0


# ---- c. flag combinations

def test_c_transposed_row_range_and_mapped_bf16_plans(sim):
    a = f64ref.scenario("wide", k=8, m=512)[0]
    tn = dict(f64ref.SPLIT)
    wide = {**tn, **FORCED}
    # transposed: the plan of A^T at the word width
    t, tw = flex_amd.Plan(a, 64, transpose=True, tuning=tn, bf16=True), flex_amd.Plan(a, 32, transpose=True, tuning=wide)
    t.self_check()
    assert np.array_equal(t.records(), tw.records()) and t.info()["n_partials"] == tw.info()["n_partials"]
    # a row shard, with a column map
    cm = np.random.default_rng(1).permutation(a.n).astype(np.int32)
    for rows in ((0, 100), (100, 512), (37, 37)):
        s, sw = flex_amd.Plan(a, 64, rows=rows, col_map=cm, tuning=tn, bf16=True), flex_amd.Plan(a, 32, rows=rows, col_map=cm, tuning=wide)
        s.self_check()
        assert s.info()["m"] == rows[1] - rows[0] and np.array_equal(s.records(), sw.records())
    # mapped (a reordered graph planned with its map), with leading dimensions
    vo, ap = flex_amd.perm_csr(a, flex_amd.order_rcm(a))
    m_, mw = flex_amd.Plan(ap, 64, vo_mp=vo, ldb=72, ldc=80, tuning=tn, bf16=True), flex_amd.Plan(ap, 32, vo_mp=vo, ldb=36, ldc=40, tuning=wide)
    m_.self_check()
    assert np.array_equal(m_.records(), mw.records())
    # the XCD interleave and an order
    x = flex_amd.Plan(a, 128, order=flex_amd.FLEX_ORDER_CLUSTER | flex_amd.FLEX_PLAN_XCD_INTERLEAVE, bf16=True)
    x.self_check()


# ---- d. the checker

def _probe():
    """A matrix whose float64 result sits where each fault shows.  B is all ones (k = 8), so C64[r, :] = the sum of row r's values."""
    rows = [
        [1 + 2.0 ** -7 - 2.0 ** -10],             # 0: truncation gives 1, rounding 1 + 2^-7
        [1 + 3 * 2.0 ** -8 - 2.0 ** -13],         # 1: through 11 bits it becomes the tie 1 + 3 2^-8 and then 1 + 2^-6; once: 1 + 2^-7
        [1 + 2.0 ** -9] * 100 + [-1.0] * 100,     # 2: every term rounded to bf16 first: 0 instead of 100 2^-9
        [1 + 2.0 ** -9 + 2.0 ** -12] * 8 + [-8.0],  # 3: nine pieces of one term, each rounded to bf16 before they are added: 0
        [],                                        # 4: an empty row
        [1.0, 2.0],                                # 5: its first column meets a NaN in B
    ]
    n = 256
    cols, c = [], 0
    for r in rows:
        cols.append(list(range(c, c + len(r))))
        c += len(r)
    rp = np.cumsum([0] + [len(r) for r in rows])
    a = flex_amd.HostCsr(rp.astype(np.uint32), np.array(sum(cols, []), np.uint32), np.array(sum(rows, []), np.float32), n=n)
    B = np.ones((n, 8), np.float32)
    B[cols[5][0], 3] = np.nan
    return a, B


def _rn(x, bits):
    """x (float64, positive normal range) rounded to `bits` significant bits, ties to even."""
    m, e = np.frexp(x)
    return np.ldexp(np.rint(np.ldexp(m, bits)), e - bits)


def test_d_the_checker_rejects_planted_faults():
    a, B = _probe()
    c64 = f64ref.spmm_f64(a, B)
    good = ref.f64_to_bf16(c64)
    msg, worst = ref.check(a, B, good, "rounded once")
    assert msg is None and worst <= 1.0, msg

    def rejected(bits, needle):
        msg, _ = ref.check(a, B, bits, "fault")
        assert msg is not None and needle in msg, msg

    trunc = good.copy()
    trunc[0] = (c64[0].astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    assert trunc[0, 0] == 0x3F80 and good[0, 0] == 0x3F81
    rejected(trunc, "beyond the bf16 bound")
    twice = good.copy()
    twice[1] = ref.f64_to_bf16(_rn(c64[1], 11))
    assert twice[1, 0] == 0x3F82 and good[1, 0] == 0x3F81
    rejected(twice, "beyond the bf16 bound")
    per_term = good.copy()
    terms = ref.rounded(a.vals[a.rowPtr[2]:a.rowPtr[3]])  # B is 1
    per_term[2] = ref.to_bf16(np.float32(terms.astype(np.float64).sum()))
    assert per_term[2, 0] == 0
    rejected(per_term, "beyond the bf16 bound")
    pieces = good.copy()
    pieces[3] = ref.to_bf16(np.float32(ref.rounded(a.vals[a.rowPtr[3]:a.rowPtr[4]]).astype(np.float64).sum()))
    assert pieces[3, 0] == 0 and good[3, 0] != 0
    rejected(pieces, "beyond the bf16 bound")
    moved = good.copy()
    moved[5, 3], moved[5, 4] = good[5, 4], good[5, 3]
    rejected(moved, "wrong class")
    minus = good.copy()
    minus[4] = 0x8000
    rejected(minus, "empty row")


@pytest.mark.parametrize("pair", list(ref.PAIRS))
def test_d_the_checker_accepts_float64_rounded_once_on_every_gpu_case(pair):
    worst = 0.0
    for graph in ref.GRAPHS:
        a, B, _, _ = ref.case(pair, graph)
        c64, bound32 = ref.case_reference(pair, graph)
        msg, w = ref.check(a, B, ref.f64_to_bf16(c64), f"{pair} {graph}", ref=(c64, bound32))
        assert msg is None, msg
        worst = max(worst, w)
        # the case is not vacuous: finite entries to judge, and where the scenario plants them, non-finite ones
        assert np.isfinite(c64).any()
        if ref.values_of(pair, graph) in ("nonfinite_A", "nonfinite_B"):
            assert (~np.isfinite(c64)).any()
    print(f"{pair}: float64 rounded once to bf16, worst err / bound {worst:.3g}")
    assert 0.0 < worst <= 1.0

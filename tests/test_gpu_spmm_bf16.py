"""flex_spmm_bf16 on the GPU (include/flex_spmm.h, FLEX_PLAN_BF16): every element of C against float64 within the bound
of tests/spmm_bf16_ref.py on every form of spmm_flat_bf16_kernel and spmm_fixup_bf16_kernel, bit-identical results where the fp32
engine promises them, the leading dimensions, the other plan flags, the guards, SparseOperator(..., bf16=True) and 64-bit addressing at
every tile width.  The cases are tests/spmm_bf16_ref.py's and tests/attention_forms.py's, which tests/test_attention_routes.py holds to
the kernels they launch.
Every test prints the worst err / bound it saw (pytest -s)."""
import numpy as np
import pytest

import attention_forms as forms
import f64ref
import flex_amd
import spmm_bf16_ref as ref
from flex_amd import Plan

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SPLIT = forms.SPMM_BF16_SPLIT


def dev_bf16(x):
    """fp32 array of bf16 numbers -> a cuda bfloat16 tensor of the same numbers."""
    return torch.from_numpy(ref.to_bf16(x).view(np.int16)).cuda().view(torch.bfloat16)


def bits_of(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def run(p, B):
    C = p(dev_bf16(B))
    torch.cuda.synchronize()
    return bits_of(C)


def accept(a, B, bits, what, ref_=None):
    msg, worst = ref.check(a, B, bits, what, ref=ref_)
    print(f"{what}: worst err / bound {worst:.3g}")
    assert msg is None, msg
    return worst


def transposed(a):
    """The CSR of A^T by a stable sort (what FLEX_PLAN_TRANSPOSE plans)."""
    row = np.repeat(np.arange(a.m), np.diff(a.rowPtr.astype(np.int64)))
    order = np.argsort(a.col, kind="stable")
    rp = np.zeros(a.n + 1, np.int64)
    np.cumsum(np.bincount(a.col, minlength=a.n), out=rp[1:])
    return flex_amd.HostCsr(rp.astype(np.uint32), row[order].astype(np.uint32), a.vals[order], n=a.m)


# ---- 1. every element against float64

@pytest.mark.parametrize("pair,graph", ref.CASES, ids=[f"{p}-{g}" for p, g in ref.CASES])
def test_1_every_element_of_c_within_the_bound(pair, graph):
    a, B, tn, lanes = ref.case(pair, graph)
    p = Plan(a, B.shape[1], tuning=tn, bf16=True)
    i = p.info()
    assert i["bf16"] == 1 and i["lanes_per_nz"] == (lanes or i["lanes_per_nz"]) and i["n_tiles"] == 0 and i["n_blocks"] == 0
    lanes = i["lanes_per_nz"]
    if pair in ("k512_rule", "k512_g32", "k256_group"):
        assert B.shape[1] >= 2 * 8 * lanes  # two column tiles or more
    if graph == "deg3" and lanes <= 16:
        assert i["n_bundles"] > 0
    if graph == "deg40":
        assert i["n_bundles"] == 0
    if graph == "long":
        assert i["n_partials"] > 1 and i["n_split_rows"] >= 1  # pieces, summed by spmm_fixup_bf16_kernel
    if graph in ref.PACK_GRAPHS:
        assert i["rec_packed"] == (1 if graph == "pack1" else 0)
    accept(a, B, run(p, B), f"{pair} {graph} ({ref.values_of(pair, graph)}; lanes {lanes}, bundles {i['n_bundles']}, partials {i['n_partials']}, "
                            f"packed {i['rec_packed']})", ref.case_reference(pair, graph))


# ---- 2. packed and unpacked plans of one case

@pytest.mark.parametrize("pair", ["k512_rule", "k64_g8", "k256_group"])
def test_2_packed_and_unpacked_plans_give_the_same_bits(pair):
    a, B, tn, _ = ref.case(pair, "pack1")
    tn = {**tn, **SPLIT}
    p1, p2 = Plan(a, B.shape[1], tuning={**tn, "rec_pack": 1}, bf16=True), Plan(a, B.shape[1], tuning={**tn, "rec_pack": 2}, bf16=True)
    assert p1.info()["rec_packed"] == 1 and p2.info()["rec_packed"] == 0 and p1.info()["n_partials"] > 0
    c1, c2 = run(p1, B), run(p2, B)
    assert np.array_equal(c1, c2)
    accept(a, B, c1, f"{pair} packed, split rows")


# ---- 3. repeatability

def test_3_two_runs_and_a_graph_replay_are_bit_identical():
    a, B, tn, _ = ref.case("k128_g16", "long")
    p = Plan(a, 128, tuning=tn, bf16=True)
    Bd = dev_bf16(B)
    C = torch.zeros((a.m, 128), dtype=torch.bfloat16, device="cuda")
    first = run(p, B)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        p(Bd, out=C)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(C), first)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        p(Bd, out=C)
    C.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(C), first)
    accept(a, B, first, "k128_g16 long, replayed")


# ---- 4. leading dimensions

@pytest.mark.parametrize("pair,graph", [("k40_g8", "long"), ("k128_g16", "deg3"), ("k512_rule", "pack1")])
def test_4_leading_dimensions_keep_what_lies_past_k(pair, graph):
    a, B, tn, _ = ref.case(pair, graph)
    k = B.shape[1]
    ldb, ldc = k + 8, k + 24
    p = Plan(a, k, ldb=ldb, ldc=ldc, tuning=tn, bf16=True)
    Bw = np.full((a.n, ldb), np.nan, np.float32)  # what lies past k in B is never read
    Bw[:, :k] = B
    Cd = torch.full((a.m, ldc), -7.0, dtype=torch.bfloat16, device="cuda")
    planted = bits_of(Cd)[0, 0]
    Bd = dev_bf16(Bw)
    p.spmm_bf16(Bd.data_ptr(), Cd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = bits_of(Cd)
    assert np.all(got[:, k:] == planted)
    accept(a, B, np.ascontiguousarray(got[:, :k]), f"{pair} {graph} ldb {ldb} ldc {ldc}", ref.case_reference(pair, graph))


# ---- 5. other plan flags

def _square_case(k, values="wide"):
    a, B = f64ref.scenario(values, k=k, m=512)
    return a, ref.rounded(B)


def test_5_a_transposed_plan_is_the_plan_of_the_transposed_csr():
    a, B = _square_case(64)
    at = transposed(a)
    got = run(Plan(a, 64, transpose=True, tuning=SPLIT, bf16=True), B)
    assert np.array_equal(got, run(Plan(at, 64, tuning=SPLIT, bf16=True), B))
    accept(at, B, got, "transposed k64")


def test_5_row_shards_against_the_full_plan():
    a, B = _square_case(128)
    full = run(Plan(a, 128, tuning=SPLIT, bf16=True), B)
    ref_ = ref.reference(a, B)
    bounds = flex_amd.shard_rows(a, 128, 3)
    got = np.concatenate([run(Plan(a, 128, rows=(int(bounds[i]), int(bounds[i + 1])), tuning=SPLIT, bf16=True), B) for i in range(3)])
    accept(a, B, got, "three row shards k128", ref_)
    print(f"row shards bit-identical to the full plan: {np.array_equal(got, full)} ({int((got != full).sum())} elements differ)")


def test_5_a_mapped_plan_against_float64():
    a, B = _square_case(64, "nonfinite_B_wide_A")
    vo, ap = flex_amd.perm_csr(a, flex_amd.order_rcm(a))
    got = run(Plan(ap, 64, vo_mp=vo, tuning=SPLIT, bf16=True), B)  # reads B and writes C in the ORIGINAL numbering
    accept(a, B, got, "mapped (RCM) k64")


# ---- 6. guards

def test_6_misaligned_operands_are_refused_and_c_is_untouched():
    a, B, tn, _ = ref.case("k64_g8", "deg40")
    p = Plan(a, 64, tuning=tn, bf16=True)
    Bd = torch.zeros(a.n * 64 + 8, dtype=torch.bfloat16, device="cuda")
    Cd = torch.full((a.m * 64 + 8,), 3.0, dtype=torch.bfloat16, device="cuda")
    before = bits_of(Cd)
    for ob, oc in ((2, 0), (0, 2), (8, 4)):  # bytes off 16-byte alignment
        with pytest.raises(flex_amd.FlexError, match="not supported"):
            p.spmm_bf16(Bd.data_ptr() + ob, Cd.data_ptr() + oc, 0)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(Cd), before)
    with pytest.raises(flex_amd.FlexError, match="invalid argument"):  # flex_spmm on a bf16 plan, flex_spmm_bf16 on an fp32 plan
        p.spmm(Bd.data_ptr(), Cd.data_ptr(), 0)
    with pytest.raises(flex_amd.FlexError, match="invalid argument"):
        Plan(a, 64, tuning=tn).spmm_bf16(Bd.data_ptr(), Cd.data_ptr(), 0)
    with pytest.raises(flex_amd.FlexError, match="not supported"):
        p.kernel_info()
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(Cd), before)


def test_6_one_plan_on_two_streams_at_once_is_refused():
    """As test_gpu_spmm.py tests flex_spmm: a plan with split rows refuses a launch on another stream while its latest is pending."""
    a, B, tn, _ = ref.case("k128_g16", "long")
    p = Plan(a, 128, tuning=tn, bf16=True)
    assert p.info()["n_partials"] > 0
    want = run(p, B)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d = dev_bf16(B)
    c1, c2 = (torch.empty((a.m, 128), dtype=torch.bfloat16, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        torch.cuda._sleep(400_000_000)  # ~0.2 s of device time in front of the launch: it IS in flight when the next call comes
    p.spmm_bf16(d.data_ptr(), c1.data_ptr(), s1.cuda_stream)
    p.spmm_bf16(d.data_ptr(), c1.data_ptr(), s1.cuda_stream)  # same stream: ordered by the stream, accepted
    with pytest.raises(flex_amd.FlexError, match="invalid argument"):
        p.spmm_bf16(d.data_ptr(), c2.data_ptr(), s2.cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(c1), want)
    p.spmm_bf16(d.data_ptr(), c2.data_ptr(), s2.cuda_stream)  # the first stream has drained: another stream is fine now
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(c2), want)


# ---- 7. the operator

@pytest.mark.parametrize("k", [32, 128])
def test_7_sparse_operator_forward_and_backward(k):
    a, Bn = _square_case(k, "zeros")
    Bn = np.where(np.isfinite(Bn), Bn, np.float32(1.0))  # float64 autograd needs finite operands; the stored zeros of A stay
    g = ref.rounded(np.random.default_rng(k).uniform(-1, 1, (a.m, k)).astype(np.float32))
    op = flex_amd.SparseOperator(a, k, tuning=SPLIT, bf16=True)
    B = dev_bf16(Bn).requires_grad_(True)
    out = op(B)
    assert out.dtype == torch.bfloat16
    out.backward(dev_bf16(g))
    torch.cuda.synchronize()
    assert B.grad.dtype == torch.bfloat16
    # float64 torch autograd on the widened operands
    A64 = torch.zeros((a.m, a.n), dtype=torch.float64)
    row = np.repeat(np.arange(a.m), np.diff(a.rowPtr.astype(np.int64)))
    A64.index_put_((torch.from_numpy(row), torch.from_numpy(a.col.astype(np.int64))), torch.from_numpy(a.vals.astype(np.float64)), accumulate=True)
    B64 = torch.from_numpy(Bn.astype(np.float64)).requires_grad_(True)
    out64 = A64 @ B64
    out64.backward(torch.from_numpy(g.astype(np.float64)))
    at = transposed(a)
    accept(a, Bn, bits_of(out.detach()), f"operator k{k} out", (out64.detach().numpy(), f64ref.f64_bound(a, Bn)))
    accept(at, g, bits_of(B.grad), f"operator k{k} B.grad", (B64.grad.numpy(), f64ref.f64_bound(at, g)))
    # dtypes and what the bf16 operator does not offer
    with pytest.raises(TypeError):
        op(B.detach().float())
    with pytest.raises(TypeError):
        flex_amd.SparseOperator(a, k)(B.detach())
    with pytest.raises(NotImplementedError):
        op(B.detach(), values=torch.zeros(a.nnz, device="cuda"))
    for kw in ({"learn_values": True}, {"learn_values": True, "fused_attention": True}):
        with pytest.raises(NotImplementedError):
            flex_amd.SparseOperator(a, k, bf16=True, **kw)


# ---- 8. 64-bit addressing

@pytest.fixture(scope="module")
def big_b():
    """n = 2^16 + 8 rows of 2^15 bf16, just above 4 GiB, every element NaN: made once; a test fills the rows it uses and puts NaN back."""
    n_big, ldb = forms.WIDE64_N, forms.WIDE64_LDB
    try:
        big = torch.full((n_big * ldb,), float("nan"), dtype=torch.bfloat16, device="cuda")
    except RuntimeError as e:  # torch.OutOfMemoryError is one
        pytest.skip(f"no room for a B of {n_big * ldb * 2 / 2 ** 30:.2f} GiB: {e}")
    yield big.view(n_big, ldb)
    del big


def _run_on_big_b(p, big_b, cmap, B, m):
    """C bits of p on the large B with row cmap[c] holding row c of B; the rows are NaN again afterwards."""
    k, rows = B.shape[1], torch.from_numpy(cmap).cuda()
    big_b[rows, :k] = dev_bf16(B)
    try:
        C = torch.empty((m, k), dtype=torch.bfloat16, device="cuda")
        p.spmm_bf16(big_b.data_ptr(), C.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        big_b[rows, :k] = float("nan")
    return bits_of(C)


def test_8_rows_of_b_past_4_gib(big_b):
    """n x ldb x 2 bytes just above 4 GiB: the plan keeps column ids and the kernel forms 64-bit row addresses (OFF32 false, G = 16).
    Rows of B at and above the 4 GiB mark are used together with their aliases 4 GiB below (what a wrapped 32-bit offset would read);
    every row the scenario does not use is NaN."""
    k, ldb, n_big = 128, forms.WIDE64_LDB, forms.WIDE64_N
    assert (ldb, n_big) == (1 << 15, (1 << 16) + 8)
    a, B = _square_case(k)
    cmap = forms.wide64_map(a.n)  # column c of the scenario reads row cmap[c] of the large B
    assert np.array_equal(cmap[:16], np.concatenate([(1 << 16) + np.arange(8), np.arange(8)])) and len(np.unique(cmap)) == a.n
    a_big = f64ref.embed_cols(a, cmap, n_big)
    p = Plan(a_big, k, ldb=ldb, tuning={"lanes_per_nz": 16}, bf16=True)
    assert p.info()["lanes_per_nz"] == 16 and int(p.records()[:, 0].max()) == n_big - 1  # column ids, not byte offsets
    accept(a, B, _run_on_big_b(p, big_b, cmap, B, a.m), "B past 4 GiB, k128 G16")


@pytest.mark.parametrize("c", forms.SPMM_BF16_WIDE64_CASES, ids=forms.case_id)
def test_8_rows_of_b_past_4_gib_at_every_tile_width(big_b, c):
    """spmm_flat_bf16_kernel<G, false, ...> for every G, on the same construction.  "split": f64ref's scenario cut into pieces, so that
    the pieces and spmm_fixup_bf16_kernel run on this route; "bundle": rows of 3 entries, whose bundles store their rows of C from here."""
    a, B, a_big, cmap, tn = forms.wide64_case(c)
    k, G = c["k"], c["G"]
    p = Plan(a_big, k, ldb=forms.WIDE64_LDB, tuning=tn, bf16=True)
    i = p.info()
    assert i["lanes_per_nz"] == G and int(p.records()[:, 0].max()) == forms.WIDE64_N - 1  # the forced tile; column ids, not byte offsets
    if c["wide64"] == "split":
        assert i["n_partials"] > 0 and i["n_split_rows"] >= 1
    else:
        assert i["n_bundles"] > 0 and i["n_partials"] == 0
    accept(a, B, _run_on_big_b(p, big_b, cmap, B, a.m),
           f"B past 4 GiB, {c['wide64']} k{k} G{G} (bundles {i['n_bundles']}, partials {i['n_partials']})")

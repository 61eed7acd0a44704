"""Which kernel each float64 route launches, checked without a GPU, and the checkers of the address-mark tests checked against the faults
they target.

Every route of tests/f64ref.py (ROUTES, and the address tables of tests/test_gpu_address_limits.py) declares the kernel instantiations
its plans launch.  A plan is created on the host simulator (tests/hostsim) from each scenario and launched on fake 16-byte-aligned
operands (one float off for the unaligned routes) with the shim's launch log on; the log must equal the declaration.  A planner rule
that sent a route to another kernel would otherwise go unseen: its float64 test would still pass, on the wrong kernel.  Every SpMM kernel
that libflex_spmm.so ships must be declared by some route, so a new instantiation needs a route before the suite passes.

The kernels of flex::values and flex::softmax (the value refresh, the SDDMM, the edge softmax) get the same treatment through the cases of
tests/values_marks.py, which tests/test_gpu_values_address_limits.py runs at the 2 and 4 GiB marks: every case is launched on the host
simulator, whose stand-ins pick the instantiation by the library's own rules (internal.h: sddmm_pick, refresh_passes, softmax_vec), every
shipped instantiation needs a case, and numpy models of the addressing faults those cases target fail the checkers they use.

The kernels of flex::attention (gat:: included) and flex::spmm_bf16 -- the fused attention in all its forms and the bf16 SpMM -- are
outside both censuses here; tests/test_attention_routes.py holds them to the cases of tests/attention_forms.py by the same rule."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from f64ref import (ADDRESS_TABLES, BIG_LDB, C_MARK4, C_ROWS, FAKE_B, FAKE_C, ROUTES, SCENARIOS, TOP32_N, WIDE64_N, BigB, address_case,
                    address_plans, block_map, block_slots, check_f64_bound, embed_cols, embed_rows, fake_launch, plan_for_route,
                    scenario, sign_extend32, spmm_big_b, wrap32)
from flex_amd import binding
from sddmm_ref import _gb, assert_sddmm_within_bound, sddmm64
from softmax_ref import check_forward, forward_fp32, scores
from values_marks import (ENTRY_ALIAS, ENTRY_K, ENTRY_OPS, ENTRY_SCALE, SDDMM_TABLES, EntryArray, alias_entry, alias_row, entry_csr,
                          entry_filler, entry_graph, entry_launch, entry_plan, sddmm_case, sddmm_launch, sddmm_model, sddmm_plan)
import values_marks

hostsim = pytest.importorskip("hostsim")


@pytest.fixture(scope="module")
def sim():
    so = os.environ.get("FLEX_HOSTSIM_LIB") or hostsim.build()
    old_so, old_lib = binding._SO, binding._lib
    binding._SO, binding._lib = so, None
    yield binding.lib()
    binding._SO, binding._lib = old_so, old_lib


def _launched(L, plan, spec):
    return hostsim.launch_log(L, lambda: fake_launch([plan], spec.get("unaligned", False), spec.get("stamped", False)))


# ---- the launch log ---------------------------------------------------------------------------------------------------------

def test_the_launch_log_is_off_by_default(sim):
    """Without the log the shim refuses every launch (test_planner_host.py::test_hostsim_cannot_compute), and after it the same."""
    a, _ = scenario("wide", k=32)
    p = plan_for_route("flat_g8", a)[0]
    assert hostsim.launch_log(sim, lambda: p.spmm(0x1000, 0x2000, 0)) == ["spmm_flat_kernel<8, true, 4, 4, false>"]
    with pytest.raises(binding.FlexError, match="not supported"):
        p.spmm(0x1000, 0x2000, 0)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_route_launches_the_kernels_it_declares(sim, route):
    spec = ROUTES[route]
    for name in SCENARIOS:
        a, _ = scenario(name, k=spec["k"], m=spec.get("m", 512), pattern=spec.get("pattern", "random"))
        for p in plan_for_route(route, a):
            assert _launched(sim, p, spec) == spec["kernels"], (route, name)


@pytest.mark.parametrize("table,route", [(t, r) for t, routes in ADDRESS_TABLES.items() for r in routes])
def test_every_address_route_launches_the_kernels_it_declares(sim, table, route):
    """The big B (n = 2^22 at ldb 256: 32-bit offsets; n = 2^22 + 8192: 64-bit) and the big C (2^20 + 4096 rows at ldc 1024)."""
    spec = ADDRESS_TABLES[table][route]
    for name in SCENARIOS:
        _, _, a_big = address_case(table, route, name)
        for p in address_plans(table, route, a_big):
            p.self_check()
            assert _launched(sim, p, spec) == spec["kernels"], (table, route, name)
            if route.startswith("blocks"):  # hot blocks need 32-bit B offsets: where they are possible they must be taken
                assert (p.info()["n_blocks"] > 0) == (table != "wide64"), (table, route, name, p.info()["n_blocks"])


# ---- every shipped SpMM kernel has a route ------------------------------------------------------------------------------------

EXEMPT = {"gather_rows_kernel<true>", "gather_rows_kernel<false>"}  # test_gpu_spmm.py::test_gather_rows_is_a_bitwise_copy


def shipped_kernels(so):
    """The kernel handles of a built library, as `nm -C` names them without namespace and parameters; the HBM probe's are left out."""
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-C", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        sym = line.split(" ", 2)[-1]
        if "__device_stub__" in sym or "flex::(anonymous namespace)::" not in sym:
            continue
        name = sym.split("flex::(anonymous namespace)::", 1)[1].split("(", 1)[0]
        if name.endswith("_kernel") or "_kernel<" in name:
            names.add(name)
    return {n for n in names if not n.startswith("probe_")}


def declared_kernels():
    kernels = {k for spec in ROUTES.values() for k in spec["kernels"]}
    return kernels | {k for routes in ADDRESS_TABLES.values() for spec in routes.values() for k in spec["kernels"]}


def test_every_shipped_spmm_kernel_is_declared_by_a_route():
    so = os.path.join(os.path.dirname(binding.__file__), "lib", "libflex_spmm.so")  # the GPU build, whatever binding points at
    assert os.path.exists(so), f"{so} is not built"
    shipped = shipped_kernels(so)
    assert len(shipped) == 37, sorted(shipped)  # a new instantiation: give it a route, then count it here
    missing = shipped - EXEMPT - declared_kernels()
    assert not missing, f"kernels no route launches: {sorted(missing)}"
    assert declared_kernels() <= shipped, sorted(declared_kernels() - shipped)


# ---- the embedding, and the faults the address-mark tests target --------------------------------------------------------------

def test_the_block_maps_reach_the_marks():
    top = block_map(512, "top32")
    assert top.max() == TOP32_N - 1 and (top >= 1 << 21).mean() > 0.8 and len(np.unique(top)) == 512
    wide = block_map(512, "wide64")
    win = wide[wide >= TOP32_N]
    assert len(win) == 256 and win.max() < WIDE64_N and set((win - TOP32_N).tolist()) <= set(wide.tolist())
    rows = block_map(512, "c_side")
    assert len(np.unique(rows)) == 512 and rows.max() < C_ROWS
    assert ((rows >= 1 << 19) & (rows < C_MARK4)).any() and (rows < 1 << 19).any()
    assert set((rows[rows >= C_MARK4] - C_MARK4).tolist()) <= set(rows.tolist())
    for table in ("top32", "wide64", "c_side"):
        assert np.all(block_slots(table, 16) % 32 == 0)


def _b_case(name, table):
    a, B = scenario(name, k=8, m=512, pattern="block" if name != "cancel" else "random")
    cmap = block_map(a.n, table)
    return a, B, embed_cols(a, cmap, TOP32_N if table == "top32" else WIDE64_N), BigB(B, cmap)


@pytest.mark.parametrize("table", ["top32", "wide64"])
@pytest.mark.parametrize("name", SCENARIOS)
def test_the_embedding_passes_the_bound(name, table):
    """The identity model (every column read where it was put) gives the scenario's own result."""
    a, B, a_big, big = _b_case(name, table)
    msg = check_f64_bound(a, B, spmm_big_b(a_big, big), route=f"embedded {table}")
    assert msg is None, msg
    C = oracle.spmm(a_big.rowPtr, np.searchsorted(np.unique(a_big.col), a_big.col).astype(np.uint32), a_big.vals,
                    big.rows(np.unique(a_big.col)))
    assert check_f64_bound(a, B, C, route=f"embedded {table}, fp32 oracle") is None


@pytest.mark.parametrize("name", ["wide", "cancel", "zeros", "huge", "nonfinite_A"])
def test_a_32bit_wrap_of_64bit_offsets_fails(name):
    """wide64: a column c >= 2^22 read through a 32-bit byte offset lands on c - 2^22, a used row that holds other values."""
    a, B, a_big, big = _b_case(name, "wide64")
    assert np.any(wrap32(a_big.col) != a_big.col)
    assert check_f64_bound(a, B, spmm_big_b(a_big, big, read=wrap32)) is not None


@pytest.mark.parametrize("name", ["wide", "cancel", "zeros", "huge", "products_underflow"])
def test_a_sign_extended_32bit_offset_fails(name):
    """top32: a byte offset >= 2^31 sign-extended lands up to 2 GiB in front of B, in the NaN guard."""
    a, B, a_big, big = _b_case(name, "top32")
    assert np.any(sign_extend32(a_big.col) < 0)
    msg = check_f64_bound(a, B, spmm_big_b(a_big, big, read=sign_extend32))
    assert msg is not None and "wrong class" in msg, msg


def c_readback(a, B, rmap, wrap_rows=False, sentinel=np.float32(-7.0)):
    """What the C-side test reads back (C[rmap[r], :k]) from a model of the big C after a right kernel, or one that wrote rows >= 2^20
    to r - 2^20 (wrap_rows); every row starts as the sentinel, as on the GPU."""
    C = spmm_big_b(embed_cols(a, np.arange(a.n), a.n), BigB(B, np.arange(a.n)))
    big = {}
    for r, row in zip(rmap.tolist(), C):
        big[r - C_MARK4 if wrap_rows and r >= C_MARK4 else r] = row
    return np.stack([big.get(r, np.full(B.shape[1], sentinel, np.float32)) for r in rmap.tolist()])


@pytest.mark.parametrize("name", ["wide", "cancel", "zeros", "huge", "nonfinite_B_wide_A"])
def test_a_c_row_wrap_fails(name):
    """c_side: rows >= 2^20 written to r - 2^20 (a 32-bit byte offset of C) leave their own rows at the sentinel and overwrite their
    aliases; the identity model passes, and the embedded A keeps every row where the map put it."""
    a, B = scenario(name, k=8, m=512)
    rmap = block_map(a.m, "c_side")
    a_big = embed_rows(a, rmap, C_ROWS)
    rp = a_big.rowPtr.astype(np.int64)
    assert np.array_equal(np.diff(rp)[rmap], np.diff(a.rowPtr.astype(np.int64))) and rp[-1] == a.nnz
    assert check_f64_bound(a, B, c_readback(a, B, rmap)) is None
    assert check_f64_bound(a, B, c_readback(a, B, rmap, wrap_rows=True)) is not None


# ---- the values and softmax kernels: every case launches what it declares, every shipped instantiation has a case ------------------

FAKE_G, FAKE_OUT = 0x7F8000000000, 0x7FC000000000


@pytest.mark.parametrize("table,case", [(t, c) for t, cases in SDDMM_TABLES.items() for c in cases])
def test_every_sddmm_case_launches_the_kernel_it_declares(sim, table, case):
    _, a_big, _, _, _ = sddmm_case(table, case)
    p = sddmm_plan(table, case, a_big)
    p.self_check()
    log = hostsim.launch_log(sim, lambda: sddmm_launch(table, case, p, FAKE_G, FAKE_B, FAKE_OUT))
    assert log == SDDMM_TABLES[table][case]["kernels"], (table, case)


def test_every_entry_side_call_launches_the_kernels_it_declares(sim):
    """On a stand-in with a small filler: the selection does not look at the entry numbers."""
    g = entry_graph()
    p = entry_plan(entry_csr(g, entry_filler(g, 1 << 20, "block")))
    p.self_check()
    for op, spec in ENTRY_OPS.items():
        log = hostsim.launch_log(sim, lambda: entry_launch(op, p, FAKE_B, FAKE_C, FAKE_OUT, FAKE_G, FAKE_B, FAKE_C))
        assert log == spec["kernels"], op
    with pytest.raises(binding.FlexError, match="not supported"):  # and without the log the stand-ins refuse, like every launcher
        p.sddmm_ptr(FAKE_G, FAKE_B, FAKE_OUT)


def shipped_values_kernels(so):
    """The kernel handles (data symbols, not the launchers' code) of flex::values and flex::softmax in a built library, as `nm -C`
    names them without namespace and parameters."""
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-C", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        _, kind, sym = line.split(" ", 2)
        if kind in "tTwW" or "__device_stub__" in sym:
            continue
        for ns in ("flex::values::", "flex::softmax::"):
            if ns in sym:
                names.add(sym.split(ns, 1)[1].split("(", 1)[0])
    return names


def test_every_shipped_values_and_softmax_kernel_is_declared_by_a_case():
    so = os.path.join(os.path.dirname(binding.__file__), "lib", "libflex_spmm.so")  # the GPU build, whatever binding points at
    assert os.path.exists(so), f"{so} is not built"
    shipped = shipped_values_kernels(so)
    assert len(shipped) == 26, sorted(shipped)  # 2 refresh + 20 sddmm_slots + 4 edge_softmax_rows; a new one: give it a case, then count it
    declared = {k for k in values_marks.declared_kernels() if not k.startswith("spmm_")}
    assert declared == shipped, (sorted(shipped - declared), sorted(declared - shipped))
    at_marks = {k for t in ("top32", "wide64") for spec in SDDMM_TABLES[t].values() for k in spec["kernels"]}
    assert {k for k in shipped if k.startswith("sddmm_slots")} == at_marks  # every SDDMM instantiation runs on the 4 GiB B


# ---- the faults the values address-mark tests target -------------------------------------------------------------------------------

def _coo(a):
    return np.repeat(np.arange(a.m, dtype=np.int64), np.diff(a.rowPtr.astype(np.int64))), a.col.astype(np.int64)


def _sddmm_small(kind, k=8):
    a, _ = scenario("wide", k=k, m=512)
    G, B = _gb(kind, a.m, a.n, k, 1)
    rows, cols = _coo(a)
    return a, G, B, rows, cols, sddmm64(rows, cols, G, B)


@pytest.mark.parametrize("kind", ["uniform", "wide"])
@pytest.mark.parametrize("table", ["top32", "wide64"])
def test_sddmm_b_row_faults_fail(table, kind):
    """B read through a 32-bit wrap of a 64-bit plan's offsets (wide64: other values) or a sign-extended 32-bit offset (top32: the NaN
    guard); the identity model passes."""
    a, G, B, rows, cols, (ref, T) = _sddmm_small(kind)
    cmap = block_map(a.n, table)
    big_g, big_b = BigB(G, np.arange(a.m)), BigB(B, cmap)
    assert_sddmm_within_bound(sddmm_model(rows, cmap[cols], big_g, big_b), ref, T, 8, "identity")
    fault, why = (wrap32, "beyond the bound") if table == "wide64" else (sign_extend32, "wrong class")
    assert np.any(fault(cmap[cols]) != cmap[cols])
    with pytest.raises(AssertionError, match=why):
        assert_sddmm_within_bound(sddmm_model(rows, cmap[cols], big_g, big_b, read_b=fault), ref, T, 8, table)


@pytest.mark.parametrize("kind", ["uniform", "wide", "nonfinite"])
def test_sddmm_g_row_wrap_fails(kind):
    """G rows >= 2^20 read at r - 2^20 (a 32-bit byte offset of G at ldc 1024): the alias is another used row."""
    a, G, B, rows, cols, (ref, T) = _sddmm_small(kind)
    rmap = block_map(a.m, "c_side")
    big_g, big_b = BigB(G, rmap), BigB(B, np.arange(a.n))
    assert_sddmm_within_bound(sddmm_model(rmap[rows], cols, big_g, big_b), ref, T, 8, "identity")
    assert np.any(alias_row(rmap[rows]) != rmap[rows])
    with pytest.raises(AssertionError):
        assert_sddmm_within_bound(sddmm_model(rmap[rows], cols, big_g, big_b, read_g=alias_row), ref, T, 8, "g wrap")


def _entry_case():
    g = entry_graph()
    F = entry_filler(g, "4GiB", "block")  # arithmetic only: nothing of 4 GiB is made here
    e = np.arange(F, F + g.nnz, dtype=np.int64)
    assert e[0] < ENTRY_ALIAS < e[-1]
    return g, F, e


def test_an_entry_output_written_at_the_alias_fails():
    """out[e] written at e - 2^30: the shard's own entries keep the sentinel (the bound fails) and entries outside it change."""
    g, F, e = _entry_case()
    G, B = _gb("uniform", g.m, g.n, ENTRY_K, 2)
    rows, cols = _coo(g)
    ref, T = sddmm64(rows, cols, G, B)
    val = sddmm_model(rows, cols, BigB(G, np.arange(g.m)), BigB(B, np.arange(g.n)))
    for fault in (False, True):
        out = EntryArray(-7.0)
        out.write(alias_entry(e) if fault else e, val)
        if not fault:
            assert_sddmm_within_bound(out.read(e), ref, T, ENTRY_K, "identity")
            assert out.changed_outside(F, F + g.nnz) == 0
        else:
            with pytest.raises(AssertionError):
                assert_sddmm_within_bound(out.read(e), ref, T, ENTRY_K, "written at the alias")
            assert out.changed_outside(F, F + g.nnz) == int((e >= ENTRY_ALIAS).sum())


@pytest.mark.parametrize("kind", ["spread80", "masked30", "poisoned"])
def test_softmax_scores_read_at_the_alias_fail(kind):
    """Scores read at e - 2^30, where the GPU test keeps other finite values: the forward check fails; read where they are, it passes."""
    g, F, e = _entry_case()
    rp = F + g.rowPtr.astype(np.int64)
    s = scores(kind, rp, seed=41)
    x = EntryArray(np.nan)
    x.write(e, s)
    past = e[e >= ENTRY_ALIAS]
    x.write(past - ENTRY_ALIAS, np.random.default_rng(7).uniform(-3, 3, len(past)).astype(np.float32))
    check_forward(rp, s, ENTRY_SCALE, forward_fp32(rp, x.read(e), ENTRY_SCALE), "identity")
    with pytest.raises(AssertionError):
        check_forward(rp, s, ENTRY_SCALE, forward_fp32(rp, x.read(alias_entry(e)), ENTRY_SCALE), "read at the alias")

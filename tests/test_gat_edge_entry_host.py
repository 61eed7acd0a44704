"""The return code and the launches of the entry points of the fused GAT attention with a per-edge score term for every way their
arguments can be wrong (tests/gat_edge_entry_table.py), on a host-simulator build: tests/hostsim's library with ONE more source,
tests/hostsim_gat_edge/launchers.cpp, which includes the library's own attention_gat_edge_entry.h and defines logging stand-ins for its
two row launchers.  The column launch is the GAT family's, which tests/hostsim/shim.cpp answers in its own log.  tests/hostsim/ is not
edited and still builds.  The real library answers the same table in tests/test_gpu_gat_edge.py.  No GPU."""
import ctypes
import os
import re

import pytest

import gat_edge_entry_table as table
from flex_amd import binding
from fused_attention_backward_ref import both_sides
from fused_attention_ref import threshold_graph

hostsim = pytest.importorskip("hostsim")

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "flex_amd", "csrc")
_SRC = os.path.join(_HERE, "hostsim_gat_edge", "launchers.cpp")
_OUT = os.path.join(_HERE, "hostsim_gat_edge", "_build", "libflex_hostsim_gat_edge.so")
_HEADERS = [os.path.join(_CSRC, "attention_gat_edge_entry.h")]
HEADER = os.path.join(_HERE, "..", "include", "flex_spmm.h")


def _build():
    """hostsim.build() knows its own sources only: a library older than one of the files that are ours is made again"""
    if os.path.exists(_OUT) and any(os.path.getmtime(f) > os.path.getmtime(_OUT) for f in [_SRC] + _HEADERS):
        os.remove(_OUT)
    return hostsim.build(extra_flags=(_SRC,), out=_OUT)


@pytest.fixture(scope="module")
def sim():
    so = _build()
    old_so, old_lib = binding._SO, binding._lib
    binding._SO, binding._lib = so, None
    yield binding.lib()
    binding._SO, binding._lib = old_so, old_lib


@pytest.fixture(scope="module")
def sim_plans(sim):
    return table.plans(both_sides(threshold_graph()))


def fake_address(i):
    return 0x7F0000000000 + (i << 36)  # 16-byte aligned, never dereferenced


OPS = {a: fake_address(i) for i, a in enumerate(table.OPERANDS)}


def _named(line):
    """the work array's address in a line of the row launcher's log, as the operand it is (or lies 4 bytes into)"""
    def name(m):
        addr = int(m.group(1), 16)
        return "work=" + next(a for a, base in OPS.items() if base <= addr < base + 16)
    return re.sub(r"work=(0x[0-9a-f]+)", name, line)


def launch_log(L, fn):
    """what fn() launched, in order: the row launchers of this build's own source, then the column launchers of the shim (an entry point
    runs its row launch before its column launch)"""
    L.hostsim_gat_edge_log_read.restype = ctypes.c_char_p
    L.hostsim_launch_log.argtypes = [ctypes.c_int]
    L.hostsim_launch_log_read.restype = ctypes.c_char_p
    L.hostsim_gat_edge_log_clear()
    L.hostsim_launch_log(1)
    try:
        fn()
        return [_named(x) for x in L.hostsim_gat_edge_log_read().decode().splitlines()] + L.hostsim_launch_log_read().decode().splitlines()
    finally:
        L.hostsim_launch_log(0)


def test_the_header_declares_the_two_calls_and_no_pinned_pattern_sees_them():
    header = open(HEADER).read()
    assert set(re.findall(r"^int (flex_edge_gat_\w*)\(", header, re.M)) == set(table.ENTRIES)
    pinned = (r"flex_(gat_)?attention\w*$", r"flex_gatv2_\w*$", r"flex_dropout_gatv2_\w*$")
    assert not any(re.match(pat, n) for pat in pinned for n in table.ENTRIES)
    for name in table.ENTRIES:
        rows = [row for row, *_ in table.rows_of(name)]
        assert len(rows) == len(set(rows)) and {"valid", "null_plan", "null_Ee", "p_1", "p_nan", "shard"} <= set(rows), name
    back = [row for row, *_ in table.rows_of(table.BACKWARD)]
    assert {"both_work_arrays_null", "work_is_p_without_gee", "gee_is_p"} <= set(back)


@pytest.mark.parametrize("drop", [table.DROP, 0.0], ids=["p0.5", "p0"])
@pytest.mark.parametrize("name", table.ENTRIES)
def test_every_refusal_keeps_its_code_its_precedence_and_its_launches(sim, sim_plans, name, drop):
    """At p = 0.5 the row launches are the DROP-on kernels and the column launch the GAT dropout family's; at p == 0 the same codes, the
    DROP-off kernels and the undropped column launch."""
    fn = binding._values_fn(name)
    for row, change, code, launches in table.rows_of(name, drop):
        handle, args = table.arguments(name, change, sim_plans, OPS, drop)
        got = []
        log = launch_log(sim, lambda: got.append(fn(handle, *args, 0)))
        assert (got[0], log) == (code, launches), f"{name}, p = {drop}, row {row}"
        if drop == 0 and "drop" not in change:
            assert all(", false>" in x or x.startswith("gat::") for x in log), (row, log)


@pytest.mark.parametrize("drop", [table.DROP, 0.0], ids=["p0.5", "p0"])
def test_which_launches_run_for_each_subset_of_wanted_gradients(sim, sim_plans, drop):
    """The rows iff gEl, gEr or gEe is wanted, the columns iff gEr or gV; the work array is gEe where it is wanted, else dWork."""
    fn = binding._values_fn(table.BACKWARD)
    for mask in range(16):
        want = [bool(mask >> i & 1) for i in range(4)]
        change = {key: None for key, w in zip(("GEl", "GEr", "GEe", "GV"), want) if not w}
        handle, args = table.arguments(table.BACKWARD, change, sim_plans, OPS, drop)
        log = launch_log(sim, lambda: fn(handle, *args, 0))
        assert log == table.backward_launches(*want, drop=drop), want
        assert len(log) == (want[0] or want[1] or want[2]) + (want[1] or want[3]), want
        rows = [x for x in log if x.startswith("gat_edge::")]
        assert all(("work=GEe" in x) == want[2] and ("work=Work" in x) != want[2] and ("+gel" in x) == want[0] for x in rows), (want, log)


def test_the_existing_simulator_still_builds_and_loads_without_the_new_calls():
    old_so, old_lib = binding._SO, binding._lib
    try:
        binding._SO, binding._lib = os.environ.get("FLEX_HOSTSIM_LIB") or hostsim.build(), None
        L = binding.lib()
        assert hasattr(L, "flex_gat_attention") and not hasattr(L, "flex_edge_gat_attention")
    finally:
        binding._SO, binding._lib = old_so, old_lib

"""The return code and the launches of the GATv2 entry points for every way their arguments can be wrong (tests/gatv2_entry_table.py), on
a host-simulator build: tests/hostsim's library with ONE more source, tests/hostsim_gatv2/launchers.cpp, which includes the library's
own flex_amd/csrc/attention_gatv2_entry.h and defines stand-in launchers that log the instantiation they would launch.  tests/hostsim/
is not edited: hostsim.build() places its extra flags in front of the sources on the compiler's line, so a path there is compiled as
one more source.  The real library answers the same table in tests/test_gpu_gatv2_attention.py.  No GPU."""
import os
import re

import pytest

import gatv2_entry_table as table
from flex_amd import binding
from fused_attention_backward_ref import both_sides
from fused_attention_ref import threshold_graph

hostsim = pytest.importorskip("hostsim")

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hostsim_gatv2", "launchers.cpp")
_OUT = os.path.join(_HERE, "hostsim_gatv2", "_build", "libflex_hostsim_gatv2.so")
_ENTRY = os.path.join(_HERE, "..", "flex_amd", "csrc", "attention_gatv2_entry.h")
HEADER = os.path.join(_HERE, "..", "include", "flex_spmm.h")


def _build():
    """hostsim.build() knows its own sources only: a library older than one of the two files that are ours is made again"""
    if os.path.exists(_OUT) and any(os.path.getmtime(f) > os.path.getmtime(_OUT) for f in (_SRC, _ENTRY)):
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


def launch_log(L, fn):
    """what fn() launched through the GATv2 launchers of L, in order"""
    import ctypes
    L.hostsim_gatv2_log_read.restype = ctypes.c_char_p
    L.hostsim_gatv2_log_clear()
    fn()
    return L.hostsim_gatv2_log_read().decode().splitlines()


def fake_address(i):
    return 0x7F0000000000 + (i << 36)  # 16-byte aligned, never dereferenced


def test_the_table_has_every_gatv2_call_of_the_header_and_none_of_them_is_one_of_the_22():
    header = open(HEADER).read()
    names = set(re.findall(r"^int (flex_gatv2_\w*)\(", header, re.M))
    assert names == set(table.ENTRIES) | {"flex_gatv2_attention_work_size"}
    assert not any(re.match(r"flex_(gat_)?attention\w*$", n) for n in names)
    assert len(set(re.findall(r"^int (flex_(?:gat_)?attention\w*)\(", header, re.M))) == 22
    for name in table.ENTRIES:
        rows = [row for row, *_ in table.rows_of(name)]
        assert "valid" in rows and "null_plan" in rows and len(rows) == len(set(rows)), name
        assert all(f"null_{a}" in rows for a in table.NEED[name]) and all(f"{a}_4_bytes_off" in rows for a in table.ALIGNED[name])
    assert {row for row, *_ in table.ROWS} <= {row for name in table.ENTRIES for row, *_ in table.rows_of(name)}


@pytest.mark.parametrize("name", table.ENTRIES)
def test_every_refusal_keeps_its_code_its_precedence_and_its_launches(sim, sim_plans, name):
    fn = binding._values_fn(name)
    ops = {a: fake_address(i) for i, a in enumerate(table.OPERANDS)}
    for row, change, code, launches in table.rows_of(name):
        handle, args = table.arguments(name, change, sim_plans, ops)
        got = []
        log = launch_log(sim, lambda: got.append(fn(handle, *args, 0)))
        assert (got[0], log) == (code, launches), f"{name}, row {row}"


def test_which_launches_run_for_each_subset_of_wanted_gradients(sim, sim_plans):
    fn = binding._values_fn(table.BACKWARD)
    ops = {a: fake_address(i) for i, a in enumerate(table.OPERANDS)}
    seen = set()
    for mask in range(8):
        want = [bool(mask >> i & 1) for i in range(3)]
        change = {key: None for key, w in zip(("GXt", "GXs", "GAtt"), want) if not w}
        handle, args = table.arguments(table.BACKWARD, change, sim_plans, ops)
        log = launch_log(sim, lambda: fn(handle, *args, 0))
        assert log == table.backward_launches(*want), want
        assert len(log) == (0 if mask == 0 else 1 + want[1] + want[2])  # the rows whenever anything is wanted, the columns for gXs, the reduction for gAtt
        seen.add(tuple(log))
    assert len(seen) == 8


def test_the_work_size_is_k_floats_per_workgroup_of_the_row_launch(sim, sim_plans):
    import ctypes
    fn = binding._values_fn("flex_gatv2_attention_work_size")
    n = ctypes.c_uint64(99)
    assert fn(None, ctypes.byref(n)) == table.INVALID and fn(sim_plans["valid"]._h, None) == table.INVALID
    assert fn(sim_plans["unflagged"]._h, ctypes.byref(n)) == table.INVALID and n.value == 99
    assert fn(sim_plans["empty"]._h, ctypes.byref(n)) == table.OK and n.value == 0
    p = sim_plans["valid"]
    assert fn(p._h, ctypes.byref(n)) == table.OK
    i = p.attention_info()
    wgs = -(-i["groups"] // 4)  # four waves to a workgroup, one group to a wave; under the XCD remap a multiple of eight workgroups
    assert n.value in {(i["rows_block"] + w) * table.K for w in (wgs, -(-wgs // 8) * 8)} and n.value > 0
    assert n.value == p.gatv2_attention_work_size()


def test_the_existing_simulator_still_loads_without_the_new_symbols():
    """binding looks the attention calls up at first use: tests/hostsim's own library has no flex_gatv2_* and needs none"""
    so = os.environ.get("FLEX_HOSTSIM_LIB") or hostsim.build()
    old_so, old_lib = binding._SO, binding._lib
    binding._SO, binding._lib = so, None
    try:
        L = binding.lib()
        assert not hasattr(L, "flex_gatv2_attention") and hasattr(L, "flex_gat_attention")
    finally:
        binding._SO, binding._lib = old_so, old_lib

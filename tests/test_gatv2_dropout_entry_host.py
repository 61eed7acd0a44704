"""The return code and the launches of the GATv2 dropout entry points for every way their arguments can be wrong
(tests/gatv2_dropout_entry_table.py), on a host-simulator build: tests/hostsim's library with ONE more source,
tests/hostsim_gatv2_dropout/launchers.cpp, which includes the library's own attention_gatv2_entry.h and
attention_gatv2_dropout_entry.h and defines logging stand-ins for all seven launchers.  tests/hostsim/ and tests/hostsim_gatv2/ are not
edited, and both still build.  The real library answers the same table in tests/test_gpu_gatv2_dropout.py.  No GPU."""
import ctypes
import os
import re

import pytest

import gatv2_dropout_entry_table as table
import gatv2_entry_table as base
from flex_amd import binding
from fused_attention_backward_ref import both_sides
from fused_attention_ref import threshold_graph

hostsim = pytest.importorskip("hostsim")

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "flex_amd", "csrc")
_SRC = os.path.join(_HERE, "hostsim_gatv2_dropout", "launchers.cpp")
_OUT = os.path.join(_HERE, "hostsim_gatv2_dropout", "_build", "libflex_hostsim_gatv2_dropout.so")
_HEADERS = [os.path.join(_CSRC, f) for f in ("attention_gatv2_common.h", "attention_gatv2_entry.h", "attention_gatv2_dropout_entry.h")]
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


def launch_log(L, fn):
    """what fn() launched through the GATv2 launchers of L, in order"""
    L.hostsim_gatv2_dropout_log_read.restype = ctypes.c_char_p
    L.hostsim_gatv2_dropout_log_clear()
    fn()
    return L.hostsim_gatv2_dropout_log_read().decode().splitlines()


def fake_address(i):
    return 0x7F0000000000 + (i << 36)  # 16-byte aligned, never dereferenced


OPS = {a: fake_address(i) for i, a in enumerate(table.OPERANDS)}


def test_the_header_declares_the_two_calls_and_no_pinned_pattern_sees_them():
    header = open(HEADER).read()
    assert set(re.findall(r"^int (flex_dropout_gatv2_\w*)\(", header, re.M)) == set(table.ENTRIES)
    assert not any(re.match(r"flex_(gat_)?attention\w*$", n) or re.match(r"flex_gatv2_\w*$", n) for n in table.ENTRIES)
    for name in table.ENTRIES:
        rows = [row for row, *_ in table.rows_of(name)]
        assert len(rows) == len(set(rows)) and {"valid", "null_plan", "p_negative", "p_1", "p_above_1", "p_nan", "p_inf"} <= set(rows), name
        assert [row for row, *_ in base.rows_of(table.UNDROPPED[name])] == rows[:-len(table.P_ROWS)]  # every row of the undropped table, in its order


@pytest.mark.parametrize("drop", [table.DROP, 0.0], ids=["p0.5", "p0"])
@pytest.mark.parametrize("name", table.ENTRIES)
def test_every_refusal_keeps_its_code_its_precedence_and_its_launches(sim, sim_plans, name, drop):
    """At p = 0.5 the launches are the dropout kernels (and gatv2::gatt_reduce); at p == 0 the same codes, and the gatv2:: kernels."""
    fn = binding._values_fn(name)
    for row, change, code, launches in table.rows_of(name, drop):
        handle, args = table.arguments(name, change, sim_plans, OPS, drop)
        got = []
        log = launch_log(sim, lambda: got.append(fn(handle, *args, 0)))
        assert (got[0], log) == (code, launches), f"{name}, p = {drop}, row {row}"
        assert all(x.startswith("gatv2::") for x in log) if drop == 0 and "drop" not in change else True


def test_the_undropped_entry_points_of_this_build_answer_their_own_table(sim, sim_plans):
    """Both entry headers are in this build: the undropped calls run on the same stand-ins as in tests/hostsim_gatv2."""
    for name in base.ENTRIES:
        fn = binding._values_fn(name)
        for row, change, code, launches in base.rows_of(name):
            handle, args = base.arguments(name, change, sim_plans, OPS)
            got = []
            log = launch_log(sim, lambda: got.append(fn(handle, *args, 0)))
            assert (got[0], log) == (code, launches), f"{name}, row {row}"


@pytest.mark.parametrize("drop", [table.DROP, 0.0], ids=["p0.5", "p0"])
def test_which_launches_run_for_each_subset_of_wanted_gradients(sim, sim_plans, drop):
    fn = binding._values_fn(table.BACKWARD)
    seen = set()
    for mask in range(8):
        want = [bool(mask >> i & 1) for i in range(3)]
        change = {key: None for key, w in zip(("GXt", "GXs", "GAtt"), want) if not w}
        handle, args = table.arguments(table.BACKWARD, change, sim_plans, OPS, drop)
        log = launch_log(sim, lambda: fn(handle, *args, 0))
        assert log == table.backward_launches(*want, drop=drop), want
        assert len(log) == (0 if mask == 0 else 1 + want[1] + want[2])  # the rows whenever anything is wanted, the columns for gXs, the reduction for gAtt
        space = "gatv2::" if drop == 0 else "gatv2_dropout::"
        assert all(x.startswith(space) or x == "gatv2::gatt_reduce" for x in log)
        seen.add(tuple(log))
    assert len(seen) == 8


def test_the_existing_simulators_still_build_and_load():
    """tests/hostsim's own library has neither family of GATv2 calls; tests/hostsim_gatv2's, whose launchers.cpp defines the four
    undropped launchers alone, links against attention_gatv2_entry.h as it is now and has the undropped calls only."""
    import test_gatv2_entry_host as plain
    old_so, old_lib = binding._SO, binding._lib
    try:
        for so, has, has_not in ((os.environ.get("FLEX_HOSTSIM_LIB") or hostsim.build(), "flex_gat_attention", "flex_gatv2_attention"),
                                 (plain._build(), "flex_gatv2_attention", "flex_dropout_gatv2_attention")):
            binding._SO, binding._lib = so, None
            L = binding.lib()
            assert hasattr(L, has) and not hasattr(L, has_not), so
    finally:
        binding._SO, binding._lib = old_so, old_lib

"""The refusal table of the GATv2 entry points (flex_amd/csrc/attention_gatv2_entry.h): per row what it changes in a valid call, and
for the forward and the backward the code it must get and what is launched.  tests/test_gatv2_entry_host.py runs it on a host-simulator
build, tests/test_gpu_gatv2_attention.py on the real library.  The order it pins is flex_gat_attention's: plan, flag, heads and slope;
head split; empty plan (FLEX_OK); NULL operands and dWork == dP; alignment (FLEX_ERR_UNSUPPORTED); no output wanted (FLEX_OK).

Graph and shapes: both_sides(threshold_graph()), which is square, k = 32 (the (W, NS) = (8, 1) form), H = 4; a plan of k = 24 for a head
of 12 columns; a row-range shard.  A launch is named as `nm -C` names its kernel below namespace flex; the row launch of the backward
says behind its name what it was asked for beside dz ("+gxt", "+gatt")."""
import numpy as np

import flex_amd
from flex_amd import binding

OK, INVALID, UNSUPPORTED = 0, -1, -4  # include/flex_spmm.h: FLEX_OK, FLEX_ERR_INVALID, FLEX_ERR_UNSUPPORTED
K, H, SLOPE = 32, 4, 0.2
ENTRIES = {"flex_gatv2_attention": "heads Xt Xs Att slope Out P".split(),
           "flex_gatv2_attention_backward": "heads Xt Xs Att P G slope GXt GXs GAtt Work AttWork".split()}
NEED = {"flex_gatv2_attention": ("Xt", "Xs", "Att", "Out"), "flex_gatv2_attention_backward": ("Xt", "Xs", "Att", "P", "G", "Work")}
ALIGNED = {"flex_gatv2_attention": ("Xt", "Xs", "Att", "Out"), "flex_gatv2_attention_backward": ("Xt", "Xs", "Att", "G", "GXt", "GXs", "AttWork")}
OPERANDS = ("Xt", "Xs", "Att", "Out", "P", "G", "GXt", "GXs", "GAtt", "Work", "AttWork")
WRITTEN = {"flex_gatv2_attention": ("Out", "P"), "flex_gatv2_attention_backward": ("GXt", "GXs", "GAtt", "Work", "AttWork")}
FORWARD, BACKWARD = tuple(ENTRIES)


def backward_launches(gxt, gxs, gatt, form="8, 1"):
    """what flex_gatv2_attention_backward launches for the gradients that are wanted"""
    if not (gxt or gxs or gatt):
        return []
    return ([f"gatv2::rows_backward<{form}>" + (" +gxt" if gxt else "") + (" +gatt" if gatt else "")]
            + ([f"gatv2::columns_backward<{form}>"] if gxs else []) + (["gatv2::gatt_reduce"] if gatt else []))


VALID = {FORWARD: ["gatv2::rows<8, 1>"], BACKWARD: backward_launches(True, True, True)}
NO_OUTPUT = {"GXt": None, "GXs": None, "GAtt": None}

# (row, the change, {entry point: (code, launches)}): "plan" -> which plan, "off" -> the operand moved 4 bytes, "same" -> (operand, the
# operand whose address it takes), "all_null" -> every pointer NULL, any other key -> the argument's new value
BOTH = lambda code, launches=(): {FORWARD: (code, list(launches)), BACKWARD: (code, list(launches))}  # noqa: E731
ROWS = [
    ("valid", {}, {FORWARD: (OK, VALID[FORWARD]), BACKWARD: (OK, VALID[BACKWARD])}),
    ("null_plan", {"plan": None}, BOTH(INVALID)),
    ("plan_without_the_flags", {"plan": "unflagged"}, BOTH(INVALID)),
    ("plan_without_the_backward_flag", {"plan": "no_backward"}, {FORWARD: (OK, VALID[FORWARD]), BACKWARD: (INVALID, [])}),
    ("heads_0", {"heads": 0}, BOTH(INVALID)),
    ("heads_negative", {"heads": -2}, BOTH(INVALID)),
    ("slope_0", {"slope": 0.0}, BOTH(INVALID)),
    ("slope_1.5", {"slope": 1.5}, BOTH(INVALID)),
    ("slope_nan", {"slope": float("nan")}, BOTH(INVALID)),
    ("slope_1", {"slope": 1.0}, {FORWARD: (OK, VALID[FORWARD]), BACKWARD: (OK, VALID[BACKWARD])}),
    ("heads_5", {"heads": 5}, BOTH(UNSUPPORTED)),                                # 32 columns in 5 heads
    ("heads_of_12_columns", {"plan": "k24", "heads": 2}, BOTH(UNSUPPORTED)),     # d = 12 is no power of two
    ("slope_0_and_heads_5", {"slope": 0.0, "heads": 5}, BOTH(INVALID)),          # the slope comes before the head split
    ("empty_plan_all_null", {"plan": "empty", "all_null": True}, BOTH(OK)),      # FLEX_OK before the NULL-operand check
    ("empty_plan_heads_5", {"plan": "empty", "all_null": True, "heads": 5}, BOTH(UNSUPPORTED)),
    ("empty_plan_slope_0", {"plan": "empty", "all_null": True, "slope": 0.0}, BOTH(INVALID)),
    # null_<operand> and <operand>_4_bytes_off: one row per operand, made by rows_of
    ("work_is_p", {"same": ("Work", "P")}, {BACKWARD: (INVALID, [])}),
    ("gatt_without_attwork", {"AttWork": None}, {BACKWARD: (INVALID, [])}),
    ("attwork_is_not_needed_without_gatt", {"AttWork": None, "GAtt": None}, {BACKWARD: (OK, backward_launches(True, True, False))}),
    ("attwork_4_bytes_off_without_gatt", {"off": "AttWork", "GAtt": None}, {BACKWARD: (OK, backward_launches(True, True, False))}),
    ("null_work_and_xs_4_bytes_off", {"Work": None, "off": "Xs"}, {BACKWARD: (INVALID, [])}),   # NULL operands before the alignment
    ("null_out_and_xs_4_bytes_off", {"Out": None, "off": "Xs"}, {FORWARD: (INVALID, [])}),
    ("no_p", {"P": None}, {FORWARD: (OK, VALID[FORWARD])}),
    ("no_output", dict(NO_OUTPUT), {BACKWARD: (OK, [])}),
    ("no_output_and_no_attwork", {**NO_OUTPUT, "AttWork": None}, {BACKWARD: (OK, [])}),
    ("xs_4_bytes_off_and_no_output", {"off": "Xs", **NO_OUTPUT}, {BACKWARD: (UNSUPPORTED, [])}),  # the alignment before "no output wanted"
    ("xt_is_xs", {"same": ("Xt", "Xs")}, {FORWARD: (OK, VALID[FORWARD]), BACKWARD: (OK, VALID[BACKWARD])}),
    ("shard", {"plan": "shard"}, {FORWARD: (OK, VALID[FORWARD]), BACKWARD: (INVALID, [])}),
] + [(f"want_{'xt' * x}{'xs' * s}{'att' * t}", {key: None for key, w in zip(("GXt", "GXs", "GAtt"), (x, s, t)) if not w},
      {BACKWARD: (OK, backward_launches(x, s, t))}) for x in (0, 1) for s in (0, 1) for t in (0, 1) if 0 < x + s + t < 3]


def rows_of(name):
    """(row, change, code, launches) of every row that reaches entry point `name`"""
    made = [(f"null_{a}", {a: None}, {name: (INVALID, [])}) for a in NEED[name]]
    made += [(f"{a}_4_bytes_off", {"off": a}, {name: (UNSUPPORTED, [])}) for a in ALIGNED[name]]
    for row, change, expect in made + ROWS:
        if name in expect:
            yield row, change, expect[name][0], expect[name][1]


def arguments(name, change, plans, ops):
    """(plan handle, the arguments after it and before the stream) of a row: the valid call's `ops` (operand -> address) with its change"""
    ops = dict(ops, heads=H, slope=SLOPE)
    if change.get("all_null"):
        ops.update({a: None for a in OPERANDS})
    for a, value in change.items():
        if a == "off":
            ops[value] += 4
        elif a == "same":
            ops[value[0]] = ops[value[1]]
        elif a not in ("plan", "all_null"):
            ops[a] = value
    which = change.get("plan", "valid")
    plan = None if which is None else plans[which]
    return (None if plan is None else plan._h), [ops[a] for a in ENTRIES[name]]


SHARD = (17, 101)


def plans(a):
    empty = binding.HostCsr(np.zeros(a.m + 1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=a.n)
    return {"valid": flex_amd.Plan(a, K, attention=True, attention_backward=True), "unflagged": flex_amd.Plan(a, K),
            "no_backward": flex_amd.Plan(a, K, attention=True), "empty": flex_amd.Plan(empty, K, attention=True, attention_backward=True),
            "k24": flex_amd.Plan(a, 24, attention=True, attention_backward=True), "shard": flex_amd.Plan(a, K, rows=SHARD, attention=True)}

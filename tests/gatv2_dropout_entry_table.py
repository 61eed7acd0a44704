"""The refusal table of the GATv2 dropout entry points (flex_amd/csrc/attention_gatv2_dropout_entry.h): every row of
tests/gatv2_entry_table.py -- the undropped calls' refusals, code for code and in their order -- with the two new arguments drop_p and
seed in the call, plus the rows of drop_p itself, which is checked beside the slope: before the head split and before the empty plan's
FLEX_OK.  tests/test_gatv2_dropout_entry_host.py runs it on a host-simulator build, tests/test_gpu_gatv2_dropout.py on the real
library.  At drop_p > 0 a row or column launch is the dropout kernel of the same form (gatv2_dropout::), the reduction of gAtt stays
gatv2::gatt_reduce; at drop_p == 0 every launch is the undropped call's."""
import gatv2_entry_table as base
from gatv2_entry_table import INVALID, OK, UNSUPPORTED, H, K, OPERANDS, SLOPE, plans  # noqa: F401

FORWARD, BACKWARD = "flex_dropout_gatv2_attention", "flex_dropout_gatv2_attention_backward"
ENTRIES = {FORWARD: "heads Xt Xs Att slope drop seed Out P".split(),
           BACKWARD: "heads Xt Xs Att P G slope drop seed GXt GXs GAtt Work AttWork".split()}
UNDROPPED = {FORWARD: base.FORWARD, BACKWARD: base.BACKWARD}
WRITTEN = {name: base.WRITTEN[UNDROPPED[name]] for name in ENTRIES}
DROP, SEED = 0.5, 0x0123456789ABCDEF

# (row, the change, the code of both entry points; nothing is launched)
P_ROWS = [
    ("p_negative", {"drop": -0.25}, INVALID),
    ("p_1", {"drop": 1.0}, INVALID),
    ("p_above_1", {"drop": 1.5}, INVALID),
    ("p_nan", {"drop": float("nan")}, INVALID),
    ("p_inf", {"drop": float("inf")}, INVALID),
    ("p_1_and_heads_5", {"drop": 1.0, "heads": 5}, INVALID),                                  # p comes before the head split
    ("p_1_on_an_empty_plan", {"plan": "empty", "all_null": True, "drop": 1.0}, INVALID),      # and before the empty plan's FLEX_OK
    ("p_1_and_a_null_operand", {"drop": 1.0, "Xs": None}, INVALID),
    ("p_1_and_xs_4_bytes_off", {"drop": 1.0, "off": "Xs"}, INVALID),                          # and before the alignment
]


def dropped(launches):
    """the launches of a call at drop_p > 0 from the undropped call's"""
    return [x if x == "gatv2::gatt_reduce" else x.replace("gatv2::", "gatv2_dropout::") for x in launches]


def backward_launches(gxt, gxs, gatt, drop=DROP):
    base_ = base.backward_launches(gxt, gxs, gatt)
    return base_ if drop == 0 else dropped(base_)


def rows_of(name, drop=DROP):
    """(row, change, code, launches) of every row that reaches entry point `name`, called at drop_p = drop where the row sets none"""
    for row, change, code, launches in base.rows_of(UNDROPPED[name]):
        yield row, change, code, (launches if drop == 0 else dropped(launches))
    for row, change, code in P_ROWS:
        yield row, change, code, []


def arguments(name, change, plans_, ops, drop=DROP):
    """(plan handle, the arguments after it and before the stream) of a row: gatv2_entry_table.arguments with drop_p and seed"""
    ops = dict(ops, heads=H, slope=SLOPE, drop=drop, seed=SEED)
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
    plan = None if which is None else plans_[which]
    return (None if plan is None else plan._h), [ops[a] for a in ENTRIES[name]]

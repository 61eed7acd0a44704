"""The refusal table of the entry points of the fused GAT attention with a per-edge score term
(flex_amd/csrc/attention_gat_edge_entry.h): per row what it changes in a valid call, and for the forward and the backward the code it
must get and what is launched.  tests/test_gat_edge_entry_host.py runs it on a host-simulator build, tests/test_gpu_gat_edge.py on the
real library.  The order it pins is gat_forward's and gat_backward's of attention_entry.h: plan, flag, heads, slope and drop_p; head
split; empty plan (FLEX_OK); NULL operands (dEe among them), both work pointers NULL and the work array equal to dP; alignment
(FLEX_ERR_UNSUPPORTED); no output wanted (FLEX_OK).

Graph and shapes: gatv2_entry_table's -- both_sides(threshold_graph()), k = 32 (the (W, NS) = (8, 1) form), H = 4, a plan of k = 24 for a
head of 12 columns, a row-range shard.  A launch is named as `nm -C` names its kernel below namespace flex.  The row launch of the
backward says behind its name whether it was handed gEl ("+gel") and which operand is its work array ("work=GEe" or "work=Work"); the
column launch is the GAT family's: gat_dropout::gat_dropout_columns_backward at drop_p > 0, gat::gat_columns_backward at drop_p == 0."""
from gatv2_entry_table import INVALID, OK, UNSUPPORTED, H, K, SLOPE, plans  # noqa: F401

FORWARD, BACKWARD = "flex_edge_gat_attention", "flex_edge_gat_attention_backward"
ENTRIES = {FORWARD: "heads El Er Ee V slope drop seed Out P".split(),
           BACKWARD: "heads El Er Ee V P G slope drop seed GEl GEr GEe GV Work".split()}
NEED = {FORWARD: ("El", "Er", "Ee", "V", "Out"), BACKWARD: ("El", "Er", "Ee", "V", "P", "G")}
ALIGNED = {FORWARD: ("V", "Out"), BACKWARD: ("V", "G", "GV")}
UNALIGNED_OK = {FORWARD: ("El", "Er", "Ee", "P"), BACKWARD: ("El", "Er", "Ee", "P", "GEl", "GEr", "GEe", "Work")}  # the alignment of a float is enough
OPERANDS = ("El", "Er", "Ee", "V", "Out", "P", "G", "GEl", "GEr", "GEe", "GV", "Work")
WRITTEN = {FORWARD: ("Out", "P"), BACKWARD: ("GEl", "GEr", "GEe", "GV", "Work")}
DROP, SEED = 0.5, 0x0123456789ABCDEF
FORM = "8, 1"


def forward_launches(drop=DROP, with_p=True):
    return [f"gat_edge::gat_edge_rows<{FORM}, {'true' if drop else 'false'}>" + ("" if with_p else " -p")]


def backward_launches(gel, ger, gee, gv, drop=DROP, work="Work"):
    """what flex_edge_gat_attention_backward launches for the gradients that are wanted; `work`: the operand that serves as the work
    array when gEe is not wanted"""
    out = []
    if gel or ger or gee:
        out.append(f"gat_edge::gat_edge_rows_backward<{FORM}, {'true' if drop else 'false'}>" + (" +gel" if gel else "") + f" work={'GEe' if gee else work}")
    if ger or gv:
        out.append(f"gat_dropout::gat_dropout_columns_backward<{FORM}>" if drop else f"gat::gat_columns_backward<{FORM}>")
    return out


def _valid(drop):
    return {FORWARD: (OK, forward_launches(drop)), BACKWARD: (OK, backward_launches(True, True, True, True, drop))}


NO_OUTPUT = {"GEl": None, "GEr": None, "GEe": None, "GV": None}
BOTH = lambda code: {FORWARD: (code, []), BACKWARD: (code, [])}  # noqa: E731


def rows(drop=DROP):
    """(row, the change, {entry point: (code, launches)}) at drop_p = drop where the row sets none: "plan" -> which plan, "off" -> the
    operand moved 4 bytes, "same" -> (operand, the operand whose address it takes), "all_null" -> every pointer NULL, any other key ->
    the argument's new value"""
    valid = _valid(drop)
    bl = lambda *w, **kw: backward_launches(*w, drop=drop, **kw)  # noqa: E731
    table = [
        ("valid", {}, valid),
        ("null_plan", {"plan": None}, BOTH(INVALID)),
        ("plan_without_the_flags", {"plan": "unflagged"}, BOTH(INVALID)),
        ("plan_without_the_backward_flag", {"plan": "no_backward"}, {FORWARD: valid[FORWARD], BACKWARD: (INVALID, [])}),
        ("heads_0", {"heads": 0}, BOTH(INVALID)),
        ("heads_negative", {"heads": -2}, BOTH(INVALID)),
        ("slope_0", {"slope": 0.0}, BOTH(INVALID)),
        ("slope_negative", {"slope": -1.0}, BOTH(INVALID)),
        ("slope_1.5", {"slope": 1.5}, BOTH(INVALID)),
        ("slope_nan", {"slope": float("nan")}, BOTH(INVALID)),
        ("slope_inf", {"slope": float("inf")}, BOTH(INVALID)),
        ("slope_1", {"slope": 1.0}, valid),
        ("p_negative", {"drop": -0.25}, BOTH(INVALID)),
        ("p_1", {"drop": 1.0}, BOTH(INVALID)),
        ("p_above_1", {"drop": 1.5}, BOTH(INVALID)),
        ("p_nan", {"drop": float("nan")}, BOTH(INVALID)),
        ("p_inf", {"drop": float("inf")}, BOTH(INVALID)),
        ("heads_5", {"heads": 5}, BOTH(UNSUPPORTED)),                                # 32 columns in 5 heads
        ("heads_of_12_columns", {"plan": "k24", "heads": 2}, BOTH(UNSUPPORTED)),     # d = 12 is no power of two
        ("slope_0_and_heads_5", {"slope": 0.0, "heads": 5}, BOTH(INVALID)),          # the slope comes before the head split
        ("p_1_and_heads_5", {"drop": 1.0, "heads": 5}, BOTH(INVALID)),               # and so does drop_p
        ("empty_plan_all_null", {"plan": "empty", "all_null": True}, BOTH(OK)),      # FLEX_OK before the NULL-operand check
        ("empty_plan_heads_5", {"plan": "empty", "all_null": True, "heads": 5}, BOTH(UNSUPPORTED)),
        ("empty_plan_slope_0", {"plan": "empty", "all_null": True, "slope": 0.0}, BOTH(INVALID)),
        ("p_1_on_an_empty_plan", {"plan": "empty", "all_null": True, "drop": 1.0}, BOTH(INVALID)),
        ("p_1_and_a_null_operand", {"drop": 1.0, "Ee": None}, BOTH(INVALID)),
        ("p_1_and_v_4_bytes_off", {"drop": 1.0, "off": "V"}, BOTH(INVALID)),         # and before the alignment
        # null_<operand>, <operand>_4_bytes_off: one row per operand, made by rows_of
        ("both_work_arrays_null", {"GEe": None, "Work": None}, {BACKWARD: (INVALID, [])}),
        ("both_work_arrays_null_and_no_output", {**NO_OUTPUT, "Work": None}, {BACKWARD: (INVALID, [])}),
        ("work_is_p_without_gee", {"GEe": None, "same": ("Work", "P")}, {BACKWARD: (INVALID, [])}),
        ("gee_is_p", {"same": ("GEe", "P")}, {BACKWARD: (INVALID, [])}),                  # dGradEe is the work array whenever it is given
        ("work_is_p_beside_gee", {"same": ("Work", "P")}, {BACKWARD: valid[BACKWARD]}),   # dWork is not used then, whatever it is
        ("no_work_beside_gee", {"Work": None}, {BACKWARD: valid[BACKWARD]}),
        ("no_gee", {"GEe": None}, {BACKWARD: (OK, bl(True, True, False, True))}),
        ("null_ee_and_v_4_bytes_off", {"Ee": None, "off": "V"}, BOTH(INVALID)),      # NULL operands before the alignment
        ("both_work_arrays_null_and_v_4_bytes_off", {"GEe": None, "Work": None, "off": "V"}, {BACKWARD: (INVALID, [])}),
        ("no_p", {"P": None}, {FORWARD: (OK, forward_launches(drop, with_p=False))}),
        ("no_output", dict(NO_OUTPUT), {BACKWARD: (OK, [])}),
        ("v_4_bytes_off_and_no_output", {"off": "V", **NO_OUTPUT}, {BACKWARD: (UNSUPPORTED, [])}),  # the alignment before "no output wanted"
        ("shard", {"plan": "shard"}, {FORWARD: valid[FORWARD], BACKWARD: (INVALID, [])}),
    ]
    for mask in range(1, 15):  # every proper subset of the four gradients
        w = [bool(mask >> i & 1) for i in range(4)]
        change = {key: None for key, on in zip(("GEl", "GEr", "GEe", "GV"), w) if not on}
        table.append(("want_" + "_".join(n for n, on in zip(("el", "er", "ee", "v"), w) if on), change, {BACKWARD: (OK, bl(*w))}))
    return table


def rows_of(name, drop=DROP):
    """(row, change, code, launches) of every row that reaches entry point `name`"""
    valid = _valid(drop)
    made = [(f"null_{a}", {a: None}, {name: (INVALID, [])}) for a in NEED[name]]
    made += [(f"{a}_4_bytes_off", {"off": a}, {name: (UNSUPPORTED, [])}) for a in ALIGNED[name]]
    made += [(f"{a}_4_bytes_off", {"off": a}, {name: valid[name]}) for a in UNALIGNED_OK[name]]
    for row, change, expect in made + rows(drop):
        if name in expect:
            yield row, change, expect[name][0], expect[name][1]


def arguments(name, change, plans_, ops, drop=DROP):
    """(plan handle, the arguments after it and before the stream) of a row: the valid call's `ops` (operand -> address) with its change"""
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

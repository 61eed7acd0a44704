"""The return code and the launches of every fused-attention entry point, for every way its arguments can be wrong: one table, run on
the host simulator (every test here but the last) and on the real library (the last, marked gpu).

The entry points are one source for both builds (flex_amd/csrc/attention_entry.h: the library compiles it into attention_kernels.hip's
object, the simulator into tests/hostsim/shim.cpp's), so the two runs agree by construction; if they ever disagree, a build is wrong.
What the table pins is the order of precedence of the refusals, which differs between the single-head pair, the per-head family (heads,
bf16, the two bias forms and the four dropout calls) and GAT (fp32 and bf16 V rows, with and without dropout).  The expected codes were
written down from the entry points as they stood in the attention_*_kernels.hip files before they moved -- the first twelve at commit
03f89bd, the ten dropout and bf16-GAT calls at commit 4b269a3: ENTRIES names, per entry point, that file and the line of each check
there, every row of ROWS names the check that answers it, and a failing row prints both.

Graph and shapes: both_sides(threshold_graph()), k = 32 (the (W, NS) = (8, 1) form), H = 4 for the per-head families, drop_p = 0.5 in a
valid call; fake operands on the simulator, as attention_forms.fake_launch has them."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import attention_forms as forms
import flex_amd
from flex_amd import binding
from fused_attention_backward_ref import both_sides
from fused_attention_ref import threshold_graph

OK, INVALID, UNSUPPORTED = 0, -1, -4  # include/flex_spmm.h: FLEX_OK, FLEX_ERR_INVALID, FLEX_ERR_UNSUPPORTED
K, H = 32, 4
DROP_P, SEED = 0.5, 0x0123456789ABCDEF

# ---- the 22 entry points: arguments after the plan and before the stream (GAT's el, er, gEl, gEr stand under Q, K, GQ, GK and its
# slope under scale), the operands that must not be NULL, and what a valid call launches at k = 32

FWD, BWD = "Q K V scale Out P", "Q K V P G scale GQ GK GV Work"
FWD_BIAS, BWD_BIAS = "Q K V Bias scale Out P", "Q K V P G scale GQ GK GV GB Work"
FWD_DROP, BWD_DROP = "Q K V Bias scale drop_p seed Out P", "Q K V P G scale drop_p seed GQ GK GV GB Work"
FWD_GAT_DROP, BWD_GAT_DROP = "Q K V scale drop_p seed Out P", "Q K V P G scale drop_p seed GQ GK GV Work"
SINGLE_GENERIC = {False: ["attention_rows<8, 1, false>"], True: ["attention_rows_backward<8, 1, false>", "attention_columns_backward<8, 1, false>"]}


def _entry(kind, backward, elem, args, file, lines, kernels, at="03f89bd", **launches):
    """launches: what the entry point launches in a call other than the valid one, by the name a row of ROWS gives that call."""
    must = ("Q", "K", "V", "G", "Work") + (() if kind == "dropout" else ("Bias",))  # the dropout calls take a NULL bias
    need = [a for a in args.split() if a in must or a == ("P" if backward else "Out")]
    return {"kind": kind, "backward": backward, "elem": elem, "args": args.split(), "need": need, "file": file, "lines": lines, "at": at,
            "kernels": kernels, "launches": {"valid": kernels, "generic": SINGLE_GENERIC[backward], **launches}}


def _three(rows, rows_bwd, cols_bwd, backward):
    return [rows_bwd, cols_bwd] if backward else [rows]


def _dropout_entry(backward, elem):
    """One of the four dot-product dropout calls: the dropped kernels with and without the bias, and at drop_p = 0 the kernels of the
    undropped call on the same operands (with a bias: the bias call; without: the per-head call, whose one head on fp32 rows is the
    single-head pair)."""
    e, plain = ("float", "attention_heads") if elem == "fp32" else ("unsigned short", "attention_bf16")
    drop = lambda b: _three(f"dropout::attention_dropout_rows<8, 1, {b}, {e}>", f"dropout::attention_dropout_rows_backward<8, 1, {b}, {e}>",
                            f"dropout::attention_dropout_columns_backward<8, 1, {e}>", backward)
    heads = lambda stem, tail: _three(f"{stem}_rows<8, 1{tail}>", f"{stem}_rows_backward<8, 1{tail}>", f"{stem}_columns_backward<8, 1{tail}>", backward)
    lines = ({"plan": 135, "scale": 136, "drop_p": 136, "split": 138, "empty": 139, "null": 140, "bias_alias": 141, "align": 143, "no_out": 144,
              "p0": 145, "launch": 151} if backward else
             {"plan": 113, "scale": 114, "drop_p": 114, "split": 116, "empty": 117, "null": 118, "align": 120, "p0": 121, "launch": 124})
    return _entry("dropout", backward, elem, "heads " + (BWD_DROP if backward else FWD_DROP), "attention_dropout_kernels.hip", lines, drop("true"),
                  at="4b269a3", no_bias=drop("false"),
                  p0=_three(f"attention_bias_rows<8, 1, {e}>", f"attention_bias_rows_backward<8, 1, {e}>", f"{plain}_columns_backward<8, 1>", backward),
                  p0_no_bias=heads(plain, ""), p0_no_bias_one_head=heads("attention", ", true") if elem == "fp32" else heads(plain, ""))


def _gat_entry(backward, elem, drop):
    """One of the six GAT calls after the first two: fp32 with dropout, bf16 without and with."""
    if elem == "fp32":
        file, stem, tail, plain_tail = "attention_gat_dropout_kernels.hip", "gat_dropout::gat_dropout", "", None
        lines = ({"plan": 176, "split": 178, "empty": 179, "null": 180, "align": 183, "no_out": 184, "p0": 185, "launch": 191} if backward else
                 {"plan": 155, "split": 157, "empty": 158, "null": 159, "align": 161, "p0": 162, "launch": 165})
    else:
        file, stem, tail, plain_tail = "attention_gat_bf16_kernels.hip", "gat_bf16::gat_bf16", ", true" if drop else ", false", ", false"
        lines = ({"plan": 189, "split": 191, "empty": 192, "null": 193, "align": 196, "no_out": 197, "p0": 198, "launch": 205} if backward else
                 {"plan": 168, "split": 170, "empty": 171, "null": 172, "align": 174, "p0": 175, "launch": 179})
    lines |= {"scale": lines["plan"], "drop_p": lines["plan"]}  # the slope and drop_p stand in the check of the plan and the heads
    names = lambda s, t: _three(f"{s}_rows<8, 1{t}>", f"{s}_rows_backward<8, 1{t}>", f"{s}_columns_backward<8, 1{t}>", backward)
    args = (BWD_GAT_DROP if backward else FWD_GAT_DROP) if drop else (BWD if backward else FWD)
    p0 = {"p0": names("gat::gat", "") if elem == "fp32" else names(stem, plain_tail)} if drop else {}
    return _entry("gat_dropout" if drop else "gat", backward, elem, "heads " + args, file, lines, names(stem, tail), at="4b269a3", **p0)


# "lines": where each check of an entry point stood in "file" at commit "at".  "plan": NULL plan, missing flag, heads < 1 (GAT: and the slope
# and drop_p); "drop_p": the dropout probability, beside the scale or the slope; "p0": drop_p == 0 hands over to the undropped kernels;
# "one_head": heads == 1 forwards to the single-head call; "split": head_split_lg; "empty": no entries; "null": a NULL operand or
# dWork == dP; "bias_alias": dGradBias == dP or dWork; "align": the refusal of the non-vector form; "no_out": no output wanted;
# "launch": the launches (the single-head pair: of the 16-byte or of the generic form)
ENTRIES = {
    "flex_attention": _entry("single", False, "fp32", FWD, "attention_kernels.hip",
                             {"plan": 209, "scale": 210, "empty": 211, "null": 212, "launch": 221}, ["attention_rows<8, 1, true>"]),
    "flex_attention_backward": _entry("single", True, "fp32", BWD, "attention_backward_kernels.hip",
                                      {"plan": 312, "scale": 313, "empty": 314, "null": 315, "no_out": 317, "launch": 330},
                                      ["attention_rows_backward<8, 1, true>", "attention_columns_backward<8, 1, true>"]),
    "flex_attention_heads": _entry("heads", False, "fp32", "heads " + FWD, "attention_heads_kernels.hip",
                                   {"plan": 68, "one_head": 69, "scale": 70, "split": 72, "empty": 73, "null": 74, "align": 76, "launch": 83},
                                   ["attention_heads_rows<8, 1>"]),
    "flex_attention_heads_backward": _entry("heads", True, "fp32", "heads " + BWD, "attention_heads_kernels.hip",
                                            {"plan": 91, "one_head": 92, "scale": 93, "split": 95, "empty": 96, "null": 97, "align": 100, "no_out": 101,
                                             "launch": 111},
                                            ["attention_heads_rows_backward<8, 1>", "attention_heads_columns_backward<8, 1>"]),
    "flex_attention_bf16": _entry("perhead", False, "bf16", "heads " + FWD, "attention_bf16_kernels.hip",
                                  {"plan": 85, "scale": 86, "split": 88, "empty": 89, "null": 90, "align": 92, "launch": 99}, ["attention_bf16_rows<8, 1>"]),
    "flex_attention_bf16_backward": _entry("perhead", True, "bf16", "heads " + BWD, "attention_bf16_kernels.hip",
                                           {"plan": 108, "scale": 109, "split": 111, "empty": 112, "null": 113, "align": 115, "no_out": 116, "launch": 126},
                                           ["attention_bf16_rows_backward<8, 1>", "attention_bf16_columns_backward<8, 1>"]),
    # bias_forward<E> and bias_backward<E>, which the four entry points at lines 118-138 of the file call
    "flex_attention_bias": _entry("perhead", False, "fp32", "heads " + FWD_BIAS, "attention_bias_kernels.hip",
                                  {"plan": 62, "scale": 63, "split": 65, "empty": 66, "null": 67, "align": 69, "launch": 76},
                                  ["attention_bias_rows<8, 1, float>"]),
    "flex_attention_bias_backward": _entry("perhead", True, "fp32", "heads " + BWD_BIAS, "attention_bias_kernels.hip",
                                           {"plan": 85, "scale": 86, "split": 88, "empty": 89, "null": 90, "bias_alias": 91, "align": 93, "no_out": 94,
                                            "launch": 101},
                                           ["attention_bias_rows_backward<8, 1, float>", "attention_heads_columns_backward<8, 1>"]),
    "flex_attention_bf16_bias": _entry("perhead", False, "bf16", "heads " + FWD_BIAS, "attention_bias_kernels.hip",
                                       {"plan": 62, "scale": 63, "split": 65, "empty": 66, "null": 67, "align": 69, "launch": 76},
                                       ["attention_bias_rows<8, 1, unsigned short>"]),
    "flex_attention_bf16_bias_backward": _entry("perhead", True, "bf16", "heads " + BWD_BIAS, "attention_bias_kernels.hip",
                                                {"plan": 85, "scale": 86, "split": 88, "empty": 89, "null": 90, "bias_alias": 91, "align": 93, "no_out": 94,
                                                 "launch": 101},
                                                ["attention_bias_rows_backward<8, 1, unsigned short>", "attention_bf16_columns_backward<8, 1>"]),
    "flex_gat_attention": _entry("gat", False, "fp32", "heads " + FWD, "attention_gat_kernels.hip",
                                 {"plan": 469, "scale": 469, "split": 471, "empty": 472, "null": 473, "align": 475, "launch": 481}, ["gat::gat_rows<8, 1>"]),
    "flex_gat_attention_backward": _entry("gat", True, "fp32", "heads " + BWD, "attention_gat_kernels.hip",
                                          {"plan": 489, "scale": 489, "split": 491, "empty": 492, "null": 493, "align": 496, "no_out": 497, "launch": 506},
                                          ["gat::gat_rows_backward<8, 1>", "gat::gat_columns_backward<8, 1>"]),
    "flex_attention_dropout": _dropout_entry(False, "fp32"),
    "flex_attention_dropout_backward": _dropout_entry(True, "fp32"),
    "flex_attention_bf16_dropout": _dropout_entry(False, "bf16"),
    "flex_attention_bf16_dropout_backward": _dropout_entry(True, "bf16"),
    "flex_gat_attention_dropout": _gat_entry(False, "fp32", True),
    "flex_gat_attention_dropout_backward": _gat_entry(True, "fp32", True),
    "flex_gat_attention_bf16": _gat_entry(False, "bf16", False),
    "flex_gat_attention_bf16_backward": _gat_entry(True, "bf16", False),
    "flex_gat_attention_bf16_dropout": _gat_entry(False, "bf16", True),
    "flex_gat_attention_bf16_dropout_backward": _gat_entry(True, "bf16", True),
}

# ---- the table.  A row: its name, what it changes in a valid call (a dict: "plan" -> which plan, "off" -> the operand moved 4 bytes,
# "same" -> (operand, the operand whose address it takes), any other key -> the argument's new value), and per kind of entry point
# (check that answers, code, what is launched: None = nothing, "valid" = the entry point's kernels, "generic" = the single-head
# pair's generic form, any other name = that entry of the entry point's "launches").  The kinds: "single", "heads" (flex_attention_heads
# and its backward, which forward heads == 1), "perhead" (bf16 and the bias forms), "dropout" (the four dot-product dropout calls), "gat"
# (fp32 and bf16 V rows) and "gat_dropout" (the same with dropout).  A row reaches the entry points of the kinds it names that have the
# arguments it names; a row that takes outputs away reaches the backward calls.
DOT = ("single", "heads", "perhead", "dropout")
GAT = ("gat", "gat_dropout")
DROP = ("dropout", "gat_dropout")
ALL = DOT + GAT
PER_HEAD = ("heads", "perhead", "dropout") + GAT
NO_OUTPUT = {"GQ": None, "GK": None, "GV": None, "GB": None}


def _same(check, code, launch=None, kinds=ALL):
    return {kind: (check, code, launch) for kind in kinds}


ROWS = [
    ("valid", {}, _same("launch", OK, "valid")),
    ("null_plan", {"plan": None}, _same("plan", INVALID)),
    ("plan_without_the_flag", {"plan": "unflagged"}, _same("plan", INVALID)),
    ("heads_0", {"heads": 0}, _same("plan", INVALID, kinds=PER_HEAD)),
    # scale (GAT: slope) comes before the head split and before the empty plan's early exit
    ("scale_0", {"scale": 0.0}, _same("scale", INVALID, kinds=DOT)),
    ("scale_nan", {"scale": float("nan")}, _same("scale", INVALID, kinds=DOT)),
    ("scale_inf", {"scale": float("inf")}, _same("scale", INVALID, kinds=DOT)),
    ("slope_0", {"scale": 0.0}, _same("scale", INVALID, kinds=GAT)),
    ("slope_1.5", {"scale": 1.5}, _same("scale", INVALID, kinds=GAT)),
    ("heads_5", {"heads": 5}, _same("split", UNSUPPORTED, kinds=PER_HEAD)),  # 32 columns in 5 heads
    ("scale_0_and_heads_5", {"scale": 0.0, "heads": 5}, _same("scale", INVALID, kinds=PER_HEAD)),
    # FLEX_OK before the NULL-operand check; a bad head split is still refused on it
    ("empty_plan_all_null", {"plan": "empty", "all_null": True}, _same("empty", OK)),
    ("empty_plan_heads_5", {"plan": "empty", "all_null": True, "heads": 5}, _same("split", UNSUPPORTED, kinds=PER_HEAD)),
    # null_<operand>: one row per operand the entry point needs, made by _rows_of
    ("work_is_p", {"same": ("Work", "P")}, _same("null", INVALID)),
    ("gbias_is_p", {"same": ("GB", "P")}, _same("bias_alias", INVALID)),
    ("gbias_is_work", {"same": ("GB", "Work")}, _same("bias_alias", INVALID)),
    # V four bytes off: the single-head pair runs the generic form, everything else refuses
    ("v_4_bytes_off", {"off": "V"}, {"single": ("launch", OK, "generic"), **_same("align", UNSUPPORTED, kinds=PER_HEAD)}),
    ("gv_4_bytes_off", {"off": "GV"}, {"single": ("launch", OK, "generic"), **_same("align", UNSUPPORTED, kinds=PER_HEAD)}),
    ("no_output", NO_OUTPUT, _same("no_out", OK)),
    # the single-head backward looks at the outputs first, the per-head family and GAT at the alignment first
    ("v_4_bytes_off_and_no_output", {"off": "V", **NO_OUTPUT},
     {"single": ("no_out", OK, None), **_same("align", UNSUPPORTED, kinds=PER_HEAD)}),
    ("null_work_and_v_4_bytes_off", {"Work": None, "off": "V"}, _same("null", INVALID)),
    # heads == 1 of flex_attention_heads and its backward is the single-head call, generic form included; the others run it themselves
    ("one_head_v_4_bytes_off", {"heads": 1, "off": "V"}, {"heads": ("one_head", OK, "generic"), **_same("align", UNSUPPORTED, kinds=("perhead", "dropout") + GAT)}),
    ("one_head_scale_0", {"heads": 1, "scale": 0.0}, {"heads": ("one_head", INVALID, None), **_same("scale", INVALID, kinds=("perhead", "dropout") + GAT)}),
    # drop_p is answered beside the scale (GAT: beside the slope, in the check of the plan): before the head split and the empty plan's exit
    ("drop_p_1", {"drop_p": 1.0}, _same("drop_p", INVALID, kinds=DROP)),
    ("drop_p_negative", {"drop_p": -0.1}, _same("drop_p", INVALID, kinds=DROP)),
    ("drop_p_nan", {"drop_p": float("nan")}, _same("drop_p", INVALID, kinds=DROP)),
    ("drop_p_1_and_heads_5", {"drop_p": 1.0, "heads": 5}, _same("drop_p", INVALID, kinds=DROP)),
    ("empty_plan_all_null_drop_p_1", {"plan": "empty", "all_null": True, "drop_p": 1.0}, _same("drop_p", INVALID, kinds=DROP)),
    # the bias of the dot-product dropout calls is optional: NULL runs the kernels without it
    ("no_bias", {"Bias": None}, _same("launch", OK, "no_bias", kinds=("dropout",))),
    ("no_gbias", {"GB": None}, _same("launch", OK, "no_bias", kinds=("dropout",))),
    # drop_p == 0 runs the undropped kernels, and only after every refusal: a misaligned operand is refused for one head too (the
    # single-head call would run its generic form on it), and nothing runs where no output is wanted
    ("drop_p_0", {"drop_p": 0.0}, _same("p0", OK, "p0", kinds=DROP)),
    ("drop_p_0_no_bias", {"drop_p": 0.0, "Bias": None}, _same("p0", OK, "p0_no_bias", kinds=("dropout",))),
    ("drop_p_0_no_gbias", {"drop_p": 0.0, "GB": None}, _same("p0", OK, "p0_no_bias", kinds=("dropout",))),
    ("drop_p_0_one_head_no_bias", {"drop_p": 0.0, "heads": 1, "Bias": None}, _same("p0", OK, "p0_no_bias_one_head", kinds=("dropout",))),
    ("drop_p_0_one_head_no_gbias", {"drop_p": 0.0, "heads": 1, "GB": None}, _same("p0", OK, "p0_no_bias_one_head", kinds=("dropout",))),
    ("drop_p_0_v_4_bytes_off", {"drop_p": 0.0, "off": "V"}, _same("align", UNSUPPORTED, kinds=DROP)),
    ("drop_p_0_gv_4_bytes_off", {"drop_p": 0.0, "off": "GV"}, _same("align", UNSUPPORTED, kinds=DROP)),
    ("drop_p_0_one_head_v_4_bytes_off", {"drop_p": 0.0, "heads": 1, "off": "V"}, _same("align", UNSUPPORTED, kinds=DROP)),
    ("drop_p_0_one_head_no_bias_v_4_bytes_off", {"drop_p": 0.0, "heads": 1, "Bias": None, "off": "V"}, _same("align", UNSUPPORTED, kinds=("dropout",))),
    ("drop_p_0_one_head_no_gbias_v_4_bytes_off", {"drop_p": 0.0, "heads": 1, "GB": None, "off": "V"}, _same("align", UNSUPPORTED, kinds=("dropout",))),
    ("drop_p_0_no_output", {"drop_p": 0.0, **NO_OUTPUT}, _same("no_out", OK, kinds=DROP)),
]


def _rows_of(name):
    """(row name, change, check, code, the kernels launched) of every row of the table that reaches entry point `name`."""
    e = ENTRIES[name]
    for row, change, expect in [(f"null_{a}", {a: None}, _same("null", INVALID)) for a in e["need"]] + ROWS:
        named = [a for a in change if a not in ("plan", "all_null", "off", "same")] + [change[m] for m in ("off",) if m in change] + list(change.get("same", ()))
        if NO_OUTPUT.items() <= change.items():  # taking every output away: one that the entry point does not have changes nothing
            named.remove("GB")
        if e["kind"] not in expect or any(a not in e["args"] for a in named):
            continue
        if any(a in NO_OUTPUT for a in named) and not e["backward"]:
            continue
        check, code, launch = expect[e["kind"]]
        kernels = [] if launch is None else e["launches"][launch]
        yield row, change, check, code, kernels


def _arguments(e, change, plans, ops):
    """(plan handle, the arguments after it) of a row: the valid call's `ops` (name -> address) with the row's change."""
    ops = dict(ops, heads=H, scale=forms.SLOPE if e["kind"] in GAT else forms.SCALE, drop_p=DROP_P, seed=SEED)
    if change.get("all_null"):
        ops.update({a: None for a in e["args"] if a not in ("heads", "scale", "drop_p", "seed")})
    for a, value in change.items():
        if a == "off":
            ops[value] += 4
        elif a == "same":
            ops[value[0]] = ops[value[1]]
        elif a not in ("plan", "all_null"):
            ops[a] = value
    which = change.get("plan", "valid")
    plan = None if which is None else plans["no_backward" if which == "unflagged" and e["backward"] else which]
    return (None if plan is None else plan._h), [ops[a] for a in e["args"]]


def _plans(a):
    empty = binding.HostCsr(np.zeros(a.m + 1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=a.n)
    return {"valid": flex_amd.Plan(a, K, attention=True, attention_backward=True), "unflagged": flex_amd.Plan(a, K),
            "no_backward": flex_amd.Plan(a, K, attention=True), "empty": flex_amd.Plan(empty, K, attention=True, attention_backward=True)}


def _where(name, row, check):
    e = ENTRIES[name]
    return f"{name}, row {row}: answered by '{check}', {e['file']}:{e['lines'][check]} at {e['at']}"


OPERANDS = ("Q", "K", "V", "Out", "G", "P", "Work", "Bias", "GB", "GQ", "GK", "GV")

# ---- on the host simulator

hostsim = pytest.importorskip("hostsim")


@pytest.fixture(scope="module")
def sim():
    so = os.environ.get("FLEX_HOSTSIM_LIB") or hostsim.build()
    old_so, old_lib = binding._SO, binding._lib
    binding._SO, binding._lib = so, None
    yield binding.lib()
    binding._SO, binding._lib = old_so, old_lib


@pytest.fixture(scope="module")
def sim_plans(sim):
    return _plans(both_sides(threshold_graph()))


def test_the_table_has_every_entry_point_and_every_row_reaches_some():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "flex_spmm.h")).read()
    assert set(re.findall(r"^int (flex_(?:gat_)?attention\w*)\(", header, re.M)) == set(ENTRIES)
    reached = {row for name in ENTRIES for row, *_ in _rows_of(name)}
    assert {row for row, *_ in ROWS} <= reached
    for name in ENTRIES:
        rows = [row for row, *_ in _rows_of(name)]
        assert "valid" in rows and "null_plan" in rows and len(rows) == len(set(rows)), name
        assert ("no_output" in rows) == ("v_4_bytes_off_and_no_output" in rows) == ("work_is_p" in rows) == ENTRIES[name]["backward"], name


@pytest.mark.parametrize("name", ENTRIES)
def test_every_refusal_of_an_entry_point_keeps_its_code_its_precedence_and_its_launches(sim, sim_plans, name):
    e = ENTRIES[name]
    fn = binding._values_fn(name)
    ops = {a: forms.fake_address(i) for i, a in enumerate(OPERANDS)}
    for row, change, check, code, kernels in _rows_of(name):
        handle, args = _arguments(e, change, sim_plans, ops)
        got = []
        log = hostsim.launch_log(sim, lambda: got.append(fn(handle, *args, 0)))
        assert (got[0], log) == (code, kernels), _where(name, row, check)
    # without the log the launchers refuse: a valid call is "not supported", and a refusal of the entry point still comes first
    handle, args = _arguments(e, {}, sim_plans, ops)
    assert fn(handle, *args, 0) == UNSUPPORTED
    assert fn(None, *args, 0) == INVALID


def test_the_simulator_defines_every_attention_launcher(sim):
    """In a simulator build the launchers of the dropout and bf16-GAT families are weak references (internal.h, FLEX_SIM_OPTIONAL), so a
    stand-in that the shim forgot is not an error when the library loads: it is one here, by name, before any call jumps through it."""
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-C", "--undefined-only", binding._SO], capture_output=True, text=True, check=True).stdout
    assert [line.split(None, 1)[1] for line in out.splitlines() if "flex::attention::launch_" in line] == []


def test_the_shim_defines_no_attention_entry_point():
    shim = open(os.path.join(os.path.dirname(hostsim.__file__), "shim.cpp")).read()
    assert re.search(r"^int flex_(gat_)?attention", shim, re.M) is None
    assert re.search(r'^#include "attention_entry.h"', shim, re.M)


# ---- on the real library

SENTINEL = -12345.0


@pytest.mark.gpu
def test_the_real_library_answers_the_table_as_the_simulator_does():
    """Every row of the table on a real plan of the same graph and real tensors of its shapes.  A row that expects no launch must leave
    every writable operand as it was (a sentinel); of the rows that launch, the valid call of each entry point runs -- one forward and
    one backward per family -- and must write its outputs; the others (the generic form behind a misaligned operand, heads == 1) are
    the single-head kernels on operands that tests/test_gpu_fused_attention*.py run, and are not launched again here.  A row never
    hands a kernel a pointer it may not use: a refused row is refused before any launch, whatever its pointers."""
    import torch
    a = both_sides(threshold_graph())
    plans = _plans(a)
    stream = torch.cuda.current_stream().cuda_stream
    rng = torch.Generator(device="cuda").manual_seed(5)
    for name, e in ENTRIES.items():
        fn = binding._values_fn(name)
        rows_dtype = torch.bfloat16 if e["elem"] == "bf16" else torch.float32
        edge = (a.nnz,) if e["kind"] == "single" else (a.nnz, H)
        shapes = {x: (a.m, K) for x in ("Q", "K", "V", "Out", "G", "GQ", "GK", "GV")} | {x: edge for x in ("P", "Work", "Bias", "GB")}
        rows = ("V", "Out", "G", "GV") if e["kind"] in GAT else ("Q", "K", "V", "Out", "G", "GQ", "GK", "GV")  # the operands of the element type
        if e["kind"] in GAT:
            shapes |= {x: (a.m, H) for x in ("Q", "K", "GQ", "GK")}  # el, er and their gradients, floats (the lifted graph is square: m == n)
        shapes = {x: shape for x, shape in shapes.items() if x in e["args"]}
        written = [x for x in ("Out", "GQ", "GK", "GV", "GB", "Work") if x in e["args"]] + ([] if e["backward"] else ["P"])
        # every writable operand lies in one buffer filled with a sentinel, so "nothing was written" is one comparison per row; each
        # operand is 256-byte aligned and has four elements of slack, so an address 4 bytes on stays inside
        dtypes = {x: rows_dtype if x in rows else torch.float32 for x in shapes}
        nbytes = {x: -(-(int(np.prod(shapes[x])) + 4) * dtypes[x].itemsize // 256) * 256 for x in shapes}
        outputs = torch.empty(sum(nbytes[x] for x in written), dtype=torch.uint8, device="cuda")
        t, at = {}, 0
        for x in shapes:
            if x in written:
                t[x] = outputs[at:at + nbytes[x]].view(dtypes[x])
                t[x].fill_(SENTINEL)
                at += nbytes[x]
            else:
                t[x] = torch.full((nbytes[x] // dtypes[x].itemsize,), 0.01, dtype=dtypes[x], device="cuda")
                if x != "P":
                    t[x].copy_(torch.rand(t[x].shape, generator=rng, device="cuda"))
        clean = outputs.clone()
        ops = {x: t[x].data_ptr() for x in t}

        for row, change, check, code, kernels in _rows_of(name):
            if kernels and row != "valid":
                assert code == OK, _where(name, row, check)  # a launching row: run on the simulator and by the single-head GPU files
                continue
            handle, args = _arguments(e, change, plans, ops)
            got = fn(handle, *args, stream)
            assert got == code, _where(name, row, check)
            if not kernels:
                assert torch.equal(outputs, clean), _where(name, row, check) + ": it wrote something"
            else:
                assert all(bool((t[x] != t[x].new_full((), SENTINEL)).any()) for x in written), _where(name, row, check) + ": an output was not written"
                outputs.copy_(clean)

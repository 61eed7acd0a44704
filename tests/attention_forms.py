"""The one table of the fused-attention and bf16-SpMM cases that the GPU files run against float64, with the kernel instantiations each
case launches (beside tests/values_marks.py, which does the same for flex::values and flex::softmax).

Families: "single" (flex_attention / flex_attention_backward; tests/test_gpu_fused_attention.py and _backward.py), "heads"
(test_gpu_multihead_attention.py), "gat" (test_gpu_gat_attention.py), "bf16" (test_gpu_attention_bf16.py), "bias_fp32" and "bias_bf16"
(test_gpu_attention_bias.py) and "spmm_bf16" (test_gpu_spmm_bf16.py).  The GPU files take their k, (k, H) and case tables from here;
tests/test_attention_routes.py launches every case on the host simulator, whose stand-ins name the instantiation by the library's own
rules (internal.h: attention_pick, head_split_lg), compares the launch log with the declaration, and holds the union of the declarations
to the kernel handles that `nm -C` finds in flex::attention:: and flex::spmm_bf16:: of the built library.

A declaration is written down, not computed by the rule it checks: FORM_OF_K lists the (W, NS) form of every k that a case uses, and a
case says by its operands (k, leading dimensions, pointer offset) whether the 16-byte form serves."""
import numpy as np

import f64ref
import spmm_bf16_ref

# ---- the (W, NS) form of every k of the tables below: slots of W lanes x 4 columns, NS slabs of 4 W columns
FORM_OF_K = {
    4: (4, 1), 6: (4, 1), 8: (4, 1), 16: (4, 1),
    20: (8, 1), 30: (8, 1), 32: (8, 1),
    48: (16, 1), 50: (16, 1), 64: (16, 1),
    96: (32, 1), 100: (32, 1), 101: (32, 1), 128: (32, 1),
    250: (64, 1), 256: (64, 1),
    300: (64, 2), 301: (64, 2), 512: (64, 2),
    600: (64, 4), 601: (64, 4), 1023: (64, 4), 1024: (64, 4),
}
FORMS = [(4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4)]


def _form(form, tail=""):
    return f"<{form[0]}, {form[1]}{tail}>"


def _vec(vec):
    return ", true" if vec else ", false"


# ---- single head (fp32): the only family with a generic (VEC = false) form, taken when k, a leading dimension or an operand's address
# is no multiple of 4 floats

SINGLE_KS = (8, 32, 100, 128, 256)                # dense and aligned, every graph and scale
SINGLE_OTHER_KS = (30, 64, 300, 600)              # the thresholds graph: k = 30 is generic
SINGLE_STRIDED_KS = (30, 32)                      # padded (k + 4, k + 8), odd (k + 3, k + 1) and one float off 16 bytes
# one k per form that is no multiple of 4: W 4, 16, 32 and 64, two slabs, three slabs of the four-slab form (one idle), four slabs with
# one column short (W 8 is SINGLE_OTHER_KS's 30)
GENERIC_ODD_KS = (6, 50, 101, 250, 301, 601, 1023)
# the aligned k that reach the same forms through a misaligned operand or odd leading dimensions (W 8: SINGLE_STRIDED_KS's 32)
GENERIC_ALIGNED_KS = (8, 64, 128, 256, 512, 1024)
ALL_WANTED = (True, True, True)
ROW_KERNEL_ALONE, COLUMN_KERNEL_ALONE = (True, False, False), (False, False, True)  # gQ alone; gV alone


def single_kernels(k, vec, want=ALL_WANTED):
    """What flex_attention and then flex_attention_backward with the gradients `want` = (gQ, gK, gV) launch."""
    tail = _form(FORM_OF_K[k], _vec(vec))
    names = ["attention_rows" + tail]
    if want[0] or want[1]:
        names.append("attention_rows_backward" + tail)
    if want[1] or want[2]:
        names.append("attention_columns_backward" + tail)
    return names


def _single(k, vec, ldb=None, ldc=None, off=0, want=ALL_WANTED):
    """vec: the case's own statement that the 16-byte form serves (k, both leading dimensions and every operand's address allow it)."""
    ldb, ldc = ldb or k, ldc or k
    return {"family": "single", "k": k, "H": 1, "elem": "fp32", "ldb": ldb, "ldc": ldc, "off": off, "want": want, "kernels": single_kernels(k, vec, want)}


ALONE = (ROW_KERNEL_ALONE, COLUMN_KERNEL_ALONE)
SINGLE_CASES = (
    [_single(k, True) for k in SINGLE_KS + (64, 300, 600)]
    + [_single(k, False) for k in (30,) + GENERIC_ODD_KS]
    + [_single(32, True, 36, 40), _single(30, False, 34, 38)]
    + [_single(k, False, k + 3, k + 1) for k in SINGLE_STRIDED_KS + GENERIC_ODD_KS + GENERIC_ALIGNED_KS]
    + [_single(k, False, off=1) for k in SINGLE_STRIDED_KS + GENERIC_ALIGNED_KS]
    # each backward kernel alone: at k = 32 (16-byte form) on dense rows, the generic forms on padded rows (odd k) or one float off
    + [_single(32, True, want=w) for w in ALONE]
    + [_single(k, False, k + 3, k + 1, want=w) for k in GENERIC_ODD_KS for w in ALONE]
    + [_single(k, False, off=1, want=w) for k in GENERIC_ALIGNED_KS for w in ALONE]
)

# ---- the per-head families: only the vector form is built.  (k, H): H heads of d = k / H columns
HEADS_PAIRS = [(8, 2), (16, 4), (32, 4), (48, 3), (64, 4), (96, 3), (128, 2), (128, 8), (256, 4), (512, 4), (1024, 4), (1024, 64)]
# (32, 4) and (20, 5) are the W = 8 slot; the second has d = 4 and lanes past k.  New pairs are appended: the scenario rotation of a case
# is keyed on the index of its pair
GAT_PAIRS = [(4, 1), (8, 2), (16, 4), (48, 3), (64, 8), (96, 3), (128, 1), (128, 8), (256, 1), (512, 2), (1024, 4), (1024, 64), (32, 4), (20, 5)]
# every (W, NS) form, idle lanes past k (48), d = 4 and d = 256, H = 1
BF16_PAIRS = [(4, 1), (64, 1), (8, 2), (32, 4), (48, 3), (128, 8), (256, 4), (512, 4), (1024, 64)]
BIAS_PAIRS = [(4, 1), (64, 1), (8, 2), (32, 4), (48, 3), (128, 8), (256, 4), (512, 4), (1024, 64)]


def _per_head(family, elem, rows, rows_bwd, cols_bwd, tail=""):
    def make(k, H):
        form = FORM_OF_K[k]
        return {"family": family, "k": k, "H": H, "elem": elem, "ldb": k, "ldc": k, "off": 0, "want": ALL_WANTED + ((True,) if "bias" in family else ()),
                "kernels": [rows + _form(form, tail), rows_bwd + _form(form, tail), cols_bwd + _form(form)]}
    return make


HEADS_CASES = [_per_head("heads", "fp32", "attention_heads_rows", "attention_heads_rows_backward", "attention_heads_columns_backward")(k, H)
               for k, H in HEADS_PAIRS]
GAT_CASES = [_per_head("gat", "fp32", "gat::gat_rows", "gat::gat_rows_backward", "gat::gat_columns_backward")(k, H) for k, H in GAT_PAIRS]
BF16_CASES = [_per_head("bf16", "bf16", "attention_bf16_rows", "attention_bf16_rows_backward", "attention_bf16_columns_backward")(k, H)
              for k, H in BF16_PAIRS]
# the biased column backward does not see the bias: it is the unbiased one of the element type
BIAS_FP32_CASES = [_per_head("bias_fp32", "fp32", "attention_bias_rows", "attention_bias_rows_backward", "attention_heads_columns_backward", ", float")(k, H)
                   for k, H in BIAS_PAIRS]
BIAS_BF16_CASES = [_per_head("bias_bf16", "bf16", "attention_bias_rows", "attention_bias_rows_backward", "attention_bf16_columns_backward",
                             ", unsigned short")(k, H) for k, H in BIAS_PAIRS]

# ---- the bf16 SpMM: spmm_flat_bf16_kernel<G, OFF32, U, 4> and, where the plan has split rows, spmm_fixup_bf16_kernel

UNROLL_OF_G = {4: 4, 8: 4, 16: 4, 32: 8, 64: 8}
SPMM_BF16_SPLIT = {"long_row": 24, "piece_records": 16}  # tuning under which the rows of 400, 200 and 97 entries of f64ref's pattern are cut
SPMM_BF16_RULE_G = {"k512_rule": 16}                     # the tile the planner's rule picks where the pair does not force one
SPMM_BF16_SPLIT_GRAPHS = ("long", "pack1", "pack2")      # the graphs of spmm_bf16_ref with rows long enough to be cut under the default tuning


def flat_bf16(G, off32):
    return f"spmm_flat_bf16_kernel<{G}, {'true' if off32 else 'false'}, {UNROLL_OF_G[G]}, 4>"


FIXUP_BF16 = "spmm_fixup_bf16_kernel"

SPMM_BF16_CASES = [
    {"family": "spmm_bf16", "pair": pair, "graph": graph, "k": spmm_bf16_ref.PAIRS[pair][0], "elem": "bf16",
     "kernels": [flat_bf16(spmm_bf16_ref.PAIRS[pair][2] or SPMM_BF16_RULE_G[pair], True)] + ([FIXUP_BF16] if graph in SPMM_BF16_SPLIT_GRAPHS else [])}
    for pair, graph in spmm_bf16_ref.CASES
]

# Rows of B past 4 GiB (64-bit row addresses, OFF32 false) at every tile width: n = 2^16 + 8 rows at ldb = 2^15 elements, the rows at and
# above the mark used together with their aliases 4 GiB below.  k: the smallest at which the plan keeps the forced tile (the planner
# narrows a tile that is more than twice as wide as the row; 128 for G = 16 as tests/test_gpu_spmm_bf16.py always had it), so the wide
# tiles have lanes past the row's end.  "split": f64ref's scenario under SPMM_BF16_SPLIT, so that
# the pieces and the fix-up run on this route; "bundle": short rows, whose bundles store with 64-bit row addresses of C's rows as well.
WIDE64_LDB, WIDE64_N = 1 << 15, (1 << 16) + 8
WIDE64_K = {4: 8, 8: 8, 16: 128, 32: 136, 64: 264}
SPMM_BF16_WIDE64_CASES = (
    [{"family": "spmm_bf16", "wide64": "split", "G": G, "k": k, "elem": "bf16", "kernels": [flat_bf16(G, False), FIXUP_BF16]} for G, k in WIDE64_K.items()]
    + [{"family": "spmm_bf16", "wide64": "bundle", "G": 8, "k": 64, "elem": "bf16", "kernels": [flat_bf16(8, False)]}]
)

CASES = SINGLE_CASES + HEADS_CASES + GAT_CASES + BF16_CASES + BIAS_FP32_CASES + BIAS_BF16_CASES + SPMM_BF16_CASES + SPMM_BF16_WIDE64_CASES

# ---- the per-head families on padded rows (tests/test_gpu_attention_layouts.py): one (k, H) per (W, NS) form, ldb = k + 4, ldc = k + 8.
# A padded plan takes the vector form and launches what its dense twin launches: each case is the twin's, with the leading dimensions.
# Not part of CASES: the census counts every instantiation once through the dense cases, and drops a case from them to see it orphaned
LAYOUT_DOT_PAIRS = [(8, 2), (32, 4), (48, 3), (128, 8), (256, 4), (512, 4), (1024, 64)]
LAYOUT_GAT_PAIRS = [(4, 1), (32, 4), (48, 3), (128, 8), (256, 1), (512, 2), (1024, 4)]


def _padded(cases, pairs):
    twin = {(c["k"], c["H"]): c for c in cases}
    return [dict(twin[k, H], ldb=k + 4, ldc=k + 8) for k, H in pairs]


LAYOUT_CASES = (_padded(HEADS_CASES, LAYOUT_DOT_PAIRS) + _padded(GAT_CASES, LAYOUT_GAT_PAIRS) + _padded(BF16_CASES, LAYOUT_DOT_PAIRS)
                + _padded(BIAS_FP32_CASES, LAYOUT_DOT_PAIRS) + _padded(BIAS_BF16_CASES, LAYOUT_DOT_PAIRS))


def case_id(c):
    if c["family"] == "spmm_bf16":
        return f"spmm_bf16-wide64-{c['wide64']}-g{c['G']}" if "wide64" in c else f"spmm_bf16-{c['pair']}-{c['graph']}"
    want = "".join("qkvb"[i] for i, w in enumerate(c["want"]) if w)
    return f"{c['family']}-k{c['k']}-h{c['H']}-ldb{c['ldb']}-ldc{c['ldc']}-off{c['off']}-{want}"


def declared_kernels(cases=None):
    """Every instantiation some case launches."""
    return {n for c in (CASES if cases is None else cases) for n in c["kernels"]}


def wide64_map(n):
    """Column c of a scenario of n columns reads row wide64_map(n)[c] of the large B: 8 rows at and above 4 GiB, their aliases 4 GiB
    below, and the rest spread under the mark."""
    rest = np.unique(np.linspace(8, (1 << 16) - 1, n - 16).astype(np.int64))
    assert len(rest) == n - 16
    return np.concatenate([(1 << 16) + np.arange(8), np.arange(8), rest])


def wide64_case(c):
    """(a, B, a_big, cmap, tuning) of a case of SPMM_BF16_WIDE64_CASES: the scenario, and its CSR with the columns moved to cmap."""
    if c["wide64"] == "split":
        a, B = f64ref.scenario("wide", k=c["k"], m=512)
        B, tn = spmm_bf16_ref.rounded(B), {"lanes_per_nz": c["G"], **SPMM_BF16_SPLIT}
    else:
        a, B, tn, lanes = spmm_bf16_ref.case(f"k{c['k']}_g{c['G']}", "deg3")
        assert lanes == c["G"] and tn.get("bundle") == 1
    cmap = wide64_map(a.n)
    return a, B, f64ref.embed_cols(a, cmap, WIDE64_N), cmap, tn


# ---- launching a case on fake operands (the host simulator with its launch log on: nothing is read or written)

SCALE, SLOPE = 0.25, 0.2


def fake_address(i, off=0):
    """A 16-byte aligned address of operand i's own, `off` floats further."""
    return 0x7F0000000000 + (i << 36) + 4 * off


def attention_plan(c, a):
    import flex_amd
    return flex_amd.Plan(a, c["k"], attention=True, attention_backward=True, ldb=c["ldb"], ldc=c["ldc"])


def fake_launch(c, p):
    """The forward and then the backward of an attention case on plan p (the bf16 SpMM: its one call), every row operand `off` floats
    off 16 bytes, the gradients the case does not want NULL."""
    if c["family"] == "spmm_bf16":
        p.spmm_bf16(fake_address(0), fake_address(1))
        return
    off, H, want = c["off"], c["H"], c["want"]
    q, k, v, out, g = (fake_address(i, off) for i in range(5))
    pr, work, bias, gb = (fake_address(i, off) for i in range(5, 9))
    grads = [fake_address(9 + i, off) if w else None for i, w in enumerate(want[:3])]
    if c["family"] in ("single", "heads"):
        heads = None if c["family"] == "single" else H
        p.attention_ptr(q, k, v, SCALE, out, pr, heads=heads)
        p.attention_backward_ptr(q, k, v, pr, g, SCALE, *grads, work, heads=heads)
    elif c["family"] == "gat":
        p.gat_attention_ptr(H, q, k, v, SLOPE, out, pr)  # q, k: el and er
        p.gat_attention_backward_ptr(H, q, k, v, pr, g, SLOPE, *grads, work)
    elif c["family"] == "bf16":
        p.attention_bf16_ptr(q, k, v, SCALE, out, pr, heads=H)
        p.attention_bf16_backward_ptr(q, k, v, pr, g, SCALE, *grads, work, heads=H)
    else:
        fwd, bwd = ((p.attention_bias_ptr, p.attention_bias_backward_ptr) if c["family"] == "bias_fp32" else
                    (p.attention_bf16_bias_ptr, p.attention_bf16_bias_backward_ptr))
        fwd(q, k, v, bias, SCALE, out, pr, heads=H)
        bwd(q, k, v, pr, g, SCALE, *grads, gb if want[3] else None, work, heads=H)

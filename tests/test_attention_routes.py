"""Which kernel instantiation every float64 case of the fused attention and of the bf16 SpMM launches, checked without a GPU, and the
census of flex::attention (with gat) and flex::spmm_bf16 -- tests/test_kernel_routes.py's rule for the namespaces it does not see.

Every case of tests/attention_forms.py -- the table the GPU files take their k, (k, H) and case lists from -- is launched on the host
simulator (tests/hostsim) on fake operands of the declared alignment with the shim's launch log on.  The stand-ins name what the real
entry point would launch by the library's own rules (internal.h: attention_pick, head_split_lg); the log must equal the case's
declaration.  `nm -C` of the built libflex_spmm.so lists the kernel handles of the two namespaces: the declarations and the handles must
be the same set, and the counts are pinned, so a new instantiation fails here until a case runs it against float64 -- and a case that
leaves the table orphans its kernels.  A model of the pick rule that takes W from the next wider form fails the launch check."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import attention_forms as forms
import flex_amd
from flex_amd import binding
from fused_attention_backward_ref import both_sides
from fused_attention_ref import threshold_graph

hostsim = pytest.importorskip("hostsim")

ATTENTION_CASES = [c for c in forms.CASES if c["family"] != "spmm_bf16"]


@pytest.fixture(scope="module")
def sim():
    so = os.environ.get("FLEX_HOSTSIM_LIB") or hostsim.build()
    old_so, old_lib = binding._SO, binding._lib
    binding._SO, binding._lib = so, None
    yield binding.lib()
    binding._SO, binding._lib = old_so, old_lib


@pytest.fixture(scope="module")
def lifted():
    return both_sides(threshold_graph())


_plans = {}


def _plan(c, a):
    key = (c["k"], c["ldb"], c["ldc"])
    if key not in _plans:
        _plans[key] = forms.attention_plan(c, a)
    return _plans[key]


# ---- the launch log of the new stand-ins

def test_the_stand_ins_refuse_without_the_log_and_a_refusal_comes_before_any_log_line(sim, lifted):
    c = forms.HEADS_CASES[2]
    p = _plan(c, lifted)
    with pytest.raises(binding.FlexError, match="not supported"):  # the log is off: no launcher computes anything here
        forms.fake_launch(c, p)
    plain = flex_amd.Plan(lifted, c["k"])  # not an attention plan: invalid, whatever the log
    bad_split = dict(c, H=5)               # 32 columns in 5 heads
    sim.hostsim_launch_log_read.restype = __import__("ctypes").c_char_p
    for case, plan, why in ((c, plain, "invalid"), (bad_split, p, "not supported"), (dict(c, off=1), p, "not supported")):
        sim.hostsim_launch_log(1)
        try:
            with pytest.raises(binding.FlexError, match=why):
                forms.fake_launch(case, plan)
            assert sim.hostsim_launch_log_read().decode() == "", (why, case)
        finally:
            sim.hostsim_launch_log(0)
    assert hostsim.launch_log(sim, lambda: forms.fake_launch(c, p)) == c["kernels"]


@pytest.mark.parametrize("c", ATTENTION_CASES, ids=forms.case_id)
def test_every_attention_case_launches_the_kernels_it_declares(sim, lifted, c):
    p = _plan(c, lifted)
    assert hostsim.launch_log(sim, lambda: forms.fake_launch(c, p)) == c["kernels"]


@pytest.mark.parametrize("c", forms.LAYOUT_CASES, ids=forms.case_id)
def test_every_layout_case_launches_the_kernels_it_declares(sim, lifted, c):
    """A padded per-head plan (ldb = k + 4, ldc = k + 8: multiples of four elements) takes the vector form -- the only one these families
    have -- and is neither refused nor rerouted: it launches what its dense twin launches."""
    assert (c["ldb"], c["ldc"]) == (c["k"] + 4, c["k"] + 8) and c not in forms.CASES
    twin = [d for d in forms.CASES if d["family"] == c["family"] and (d["k"], d["H"], d["ldb"], d["ldc"]) == (c["k"], c["H"], c["k"], c["k"])]
    assert len(twin) == 1 and twin[0]["kernels"] == c["kernels"] and twin[0]["want"] == c["want"]
    p = _plan(c, lifted)
    assert hostsim.launch_log(sim, lambda: forms.fake_launch(c, p)) == c["kernels"]
    odd = flex_amd.Plan(lifted, c["k"], attention=True, attention_backward=True, ldb=c["k"] + 6, ldc=c["ldc"])  # ldb % 4 == 2: refused, nothing logged
    with pytest.raises(binding.FlexError, match="not supported"):
        hostsim.launch_log(sim, lambda: forms.fake_launch(c, odd))
    odd.destroy()


def test_the_layout_cases_run_every_form_of_every_per_head_family_the_table_knows():
    families = {}
    for c in forms.LAYOUT_CASES:
        families.setdefault(c["family"], []).append(forms.FORM_OF_K[c["k"]])
    assert set(families) == {"heads", "gat", "bf16", "bias_fp32", "bias_bf16"} and all(f == forms.FORMS for f in families.values())


@pytest.mark.parametrize("c", forms.SPMM_BF16_CASES, ids=forms.case_id)
def test_every_bf16_spmm_case_launches_the_kernels_it_declares(sim, c):
    import spmm_bf16_ref as ref
    a, B, tn, _ = ref.case(c["pair"], c["graph"])
    p = flex_amd.Plan(a, c["k"], tuning=tn, bf16=True)
    assert hostsim.launch_log(sim, lambda: forms.fake_launch(c, p)) == c["kernels"]
    assert (p.info()["n_partials"] > 0) == (forms.FIXUP_BF16 in c["kernels"])


@pytest.mark.parametrize("c", forms.SPMM_BF16_WIDE64_CASES, ids=forms.case_id)
def test_every_bf16_spmm_case_past_4_gib_launches_the_kernels_it_declares(sim, c):
    """Nothing of 4 GiB is made here: the plan holds column ids and the launch is logged."""
    a, B, a_big, cmap, tn = forms.wide64_case(c)
    p = flex_amd.Plan(a_big, c["k"], ldb=forms.WIDE64_LDB, tuning=tn, bf16=True)
    p.self_check()
    i = p.info()
    assert i["lanes_per_nz"] == c["G"] and int(p.records()[:, 0].max()) == forms.WIDE64_N - 1  # column ids, not byte offsets
    assert (i["n_partials"] > 0) == (c["wide64"] == "split") and (c["wide64"] != "bundle" or i["n_bundles"] > 0)
    assert hostsim.launch_log(sim, lambda: forms.fake_launch(c, p)) == c["kernels"]


# ---- the census

def shipped_attention_kernels(so):
    """The kernel handles (data symbols, not the launchers' code) of flex::attention (gat:: included, and kept in the name) and of
    flex::spmm_bf16 in a built library, as `nm -C` names them without the outer namespaces and the parameters."""
    nm = shutil.which("nm") or "/usr/bin/nm"
    out = subprocess.run([nm, "-C", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        _, kind, sym = line.split(" ", 2)
        if kind in "tTwW" or "__device_stub__" in sym:
            continue
        head = sym.split("(", 1)[0]
        for ns in ("flex::attention::", "flex::spmm_bf16::"):
            if ns in head:
                names.add(head.split(ns, 1)[1])
    return names


def orphans(shipped, cases):
    """(shipped kernels no case declares, declared kernels that are not shipped)"""
    declared = forms.declared_kernels(cases)
    return sorted(shipped - declared), sorted(declared - shipped)


def test_every_shipped_attention_and_bf16_spmm_kernel_is_declared_by_a_case():
    so = os.path.join(os.path.dirname(binding.__file__), "lib", "libflex_spmm.so")  # the GPU build, whatever binding points at
    assert os.path.exists(so), f"{so} is not built"
    shipped = shipped_attention_kernels(so)
    attention = {n for n in shipped if not n.startswith("spmm_")}
    # 7 (W, NS) forms x (42: three single-head kernels, VEC true and false; 21 heads; 21 bf16; 21 GAT; 28: the biased row kernels of both
    # element types) and 10 flat bf16 SpMM + the fix-up; a new one: give it a case that a GPU test runs against float64, then count it
    assert len(attention) == 133 and len(shipped) - len(attention) == 11, sorted(shipped)
    missing, unknown = orphans(shipped, forms.CASES)
    assert not missing and not unknown, (f"kernels no case launches: {missing}", f"declared but not shipped: {unknown}")
    # the instantiations that no test had launched before this table: the generic single-head forms but W = 8, the wide-offset bf16 tiles
    generic = {f"{kern}<{W}, {NS}, false>" for kern in ("attention_rows", "attention_rows_backward", "attention_columns_backward")
               for W, NS in forms.FORMS}
    assert len(generic) == 21 and generic <= forms.declared_kernels(forms.SINGLE_CASES)
    wide = {forms.flat_bf16(G, False) for G in (4, 8, 16, 32, 64)}
    assert wide <= forms.declared_kernels(forms.SPMM_BF16_WIDE64_CASES) and wide <= shipped
    for family in (forms.HEADS_CASES, forms.GAT_CASES, forms.BF16_CASES, forms.BIAS_FP32_CASES, forms.BIAS_BF16_CASES):
        assert {forms.FORM_OF_K[c["k"]] for c in family} == set(forms.FORMS)  # every per-head family runs all seven forms


def test_a_case_that_leaves_the_table_orphans_its_kernels():
    """On the declarations alone (the table is not edited): without the one case that runs a form, the census names its kernels."""
    shipped = forms.declared_kernels()
    lone = [c for c in forms.GAT_CASES if c["k"] == 512]
    assert len(lone) == 1
    missing, unknown = orphans(shipped, [c for c in forms.CASES if c is not lone[0]])
    assert missing == sorted(lone[0]["kernels"]) and not unknown


# ---- the launch check has teeth

def pick_model(k, wider=False):
    """(W, NS) of a k by a numpy model of attention_pick; wider: W taken from the next wider form."""
    W = int(np.clip(2 ** np.ceil(np.log2(k / 4)), 4, 64))
    if wider:
        W = min(2 * W, 128)
    slabs = int(np.ceil(k / (4 * W)))
    return W, 1 if slabs <= 1 else 2 if slabs == 2 else 4


def test_the_model_of_the_pick_rule_agrees_and_w_from_the_next_wider_form_fails_the_launch_check(sim, lifted):
    for c in ATTENTION_CASES:
        log = hostsim.launch_log(sim, lambda: forms.fake_launch(c, _plan(c, lifted)))
        right, wrong = pick_model(c["k"]), pick_model(c["k"], wider=True)
        assert right == forms.FORM_OF_K[c["k"]] and wrong != right, c
        assert log == c["kernels"]
        assert log != [n.replace("<%d, %d" % right, "<%d, %d" % wrong) for n in c["kernels"]], forms.case_id(c)

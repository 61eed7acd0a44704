"""The contract of the torch-level attention wrappers of flex_amd.binding.Plan, family by family (Q/K/V: attention, heads, bf16, bias,
dropout; el/er/V: GAT, dropout, bf16, edge; xt/xs/att: GATv2, dropout), without a launch: every <name>_ptr method is shadowed on the
plan instance by a recorder, and what the wrapper hands it is held to the table below -- the operands in the order of the _ptr
signature, the scalars, heads and torch's current stream; a missing out or gradient allocated with the right shape, dtype and device
(zero on a plan without entries), a given one returned by identity; `want` leaving None results and None pointers; the work arrays
allocated only where the call needs them; and an operand of the wrong dtype or shape refused by AssertionError before the call."""
import contextlib
import inspect
from typing import NamedTuple

import numpy as np
import pytest

import flex_amd
from flex_amd import binding

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K, H = 8, 2
SCALE, SLOPE, DROP, SEED = 0.375, 0.25, 0.5, 0x123456789ABCDEF0
MASK64 = 0xFFFFFFFFFFFFFFFF
STREAM = "<stream>"
F32, BF16 = torch.float32, torch.bfloat16


class Case(NamedTuple):
    name: str                  # the Plan method; it must call name + "_ptr" once
    ops: dict                  # its positional tensor operands in call order: token -> (kind of shape, dtype)
    scalars: tuple             # the positional scalars that follow them
    kw: dict                   # keyword arguments; a (kind, dtype) value is a tensor operand whose token is the keyword
    outs: tuple                # ((keyword, kind, dtype), ...): `out` of a forward, the gradients of a backward in `want` order
    probs: "tuple | None"      # forward: (keyword, kind) of the optional alpha array, token "P"
    work: "str | None"         # backward: the kind of the work array
    ptr: tuple                 # what name + "_ptr" receives, in the order of its signature: tokens, scalars, STREAM, "heads"
    heads: int
    ptr_heads: "int | None"
    no_work_if: "str | None" = None    # the gradient that serves as the work array where it is wanted
    att_work_if: "str | None" = None   # the gradient that needs att_work

    @property
    def id(self):
        return self.name + ("" if self.heads == H else "-one_head") + ("" if self.name != "attention_dropout" or "bias" in self.kw else "-no_bias")


# ---- the table: what each _ptr method receives

P_QKV = ("Q", "K", "V", SCALE, "out", "P", STREAM, "heads")
P_QKV_B = ("Q", "K", "V", "P", "G", SCALE, "grad_q", "grad_k", "grad_v", "work", STREAM, "heads")
P_BIAS = ("Q", "K", "V", "bias", SCALE, "out", "P", STREAM, "heads")
P_BIAS_B = ("Q", "K", "V", "P", "G", SCALE, "grad_q", "grad_k", "grad_v", "grad_bias", "work", STREAM, "heads")
P_DROP = ("Q", "K", "V", "bias", SCALE, DROP, SEED, "out", "P", STREAM, "heads")
P_DROP_B = ("Q", "K", "V", "P", "G", SCALE, DROP, SEED, "grad_q", "grad_k", "grad_v", "grad_bias", "work", STREAM, "heads")
P_GAT = ("heads", "el", "er", "V", SLOPE, "out", "P", STREAM)
P_GAT_B = ("heads", "el", "er", "V", "P", "G", SLOPE, "grad_el", "grad_er", "grad_v", "work", STREAM)
P_GAT_DROP = ("heads", "el", "er", "V", SLOPE, DROP, SEED, "out", "P", STREAM)
P_GAT_DROP_B = ("heads", "el", "er", "V", "P", "G", SLOPE, DROP, SEED, "grad_el", "grad_er", "grad_v", "work", STREAM)
P_EDGE = ("heads", "el", "er", "ee", "V", SLOPE, DROP, SEED, "out", "P", STREAM)
P_EDGE_B = ("heads", "el", "er", "ee", "V", "P", "G", SLOPE, DROP, SEED, "grad_el", "grad_er", "grad_ee", "grad_v", "work", STREAM)
P_GATV2 = ("heads", "xt", "xs", "att", SLOPE, "out", "P", STREAM)
P_GATV2_B = ("heads", "xt", "xs", "att", "P", "G", SLOPE, "grad_xt", "grad_xs", "grad_att", "work", "att_work", STREAM)
P_GATV2_DROP = ("heads", "xt", "xs", "att", SLOPE, DROP, SEED, "out", "P", STREAM)
P_GATV2_DROP_B = ("heads", "xt", "xs", "att", "P", "G", SLOPE, DROP, SEED, "grad_xt", "grad_xs", "grad_att", "work", "att_work", STREAM)


def _forward(name, ops, scalars, ptr, dt=F32, probs="p", pkind="eH", heads=H, ptr_heads=H, pass_heads=False, **kw):
    kw.update({"heads": heads} if pass_heads else {})
    return Case(name, ops, scalars, kw, (("out", "mk", dt),), (probs, pkind), None, ptr, heads, ptr_heads)


def _backward(name, ops, scalars, grads, ptr, work="eH", heads=H, ptr_heads=H, no_work_if=None, att_work_if=None, pass_heads=False, **kw):
    kw.update({"heads": heads} if pass_heads else {})
    return Case(name, ops, scalars, kw, grads, None, work, ptr, heads, ptr_heads, no_work_if, att_work_if)


def _cases():
    cases = []
    for bf, dt in (("", F32), ("_bf16", BF16)):
        qkv = {"Q": ("mk", dt), "K": ("nk", dt), "V": ("nk", dt)}
        qkv_b = {**qkv, "P": ("eH", F32), "G": ("mk", dt)}
        g_qkv = (("grad_q", "mk", dt), ("grad_k", "nk", dt), ("grad_v", "nk", dt))
        g_bias = g_qkv + (("grad_bias", "eH", F32),)
        gat = {"el": ("mH", F32), "er": ("nH", F32), "V": ("nk", dt)}
        gat_b = {**gat, "P": ("eH", F32), "G": ("mk", dt)}
        g_gat = (("grad_el", "mH", F32), ("grad_er", "nH", F32), ("grad_v", "nk", dt))
        cases += [
            _forward(f"attention{bf}", qkv, (SCALE,), P_QKV, dt, pass_heads=True),
            _backward(f"attention{bf}_backward", qkv_b, (SCALE,), g_qkv, P_QKV_B, pass_heads=True),
            _forward(f"attention{bf}_bias", {**qkv, "bias": ("eH", F32)}, (SCALE,), P_BIAS, dt, pass_heads=True),
            _backward(f"attention{bf}_bias_backward", qkv_b, (SCALE,), g_bias, P_BIAS_B, pass_heads=True),
            _forward(f"attention{bf}_dropout", qkv, (SCALE, DROP, SEED), P_DROP, dt, probs="probs", pass_heads=True, bias=("eH", F32)),
            _backward(f"attention{bf}_dropout_backward", qkv_b, (SCALE, DROP, SEED), g_bias, P_DROP_B, pass_heads=True),
            _forward(f"gat_attention{bf}", gat, (SLOPE,), P_GAT, dt),
            _backward(f"gat_attention{bf}_backward", gat_b, (SLOPE,), g_gat, P_GAT_B),
            _forward(f"gat_attention{bf}_dropout", gat, (SLOPE, DROP, SEED), P_GAT_DROP, dt, probs="probs"),
            _backward(f"gat_attention{bf}_dropout_backward", gat_b, (SLOPE, DROP, SEED), g_gat, P_GAT_DROP_B),
        ]
    qkv1 = {"Q": ("mk", F32), "K": ("nk", F32), "V": ("nk", F32)}
    g_qkv1 = (("grad_q", "mk", F32), ("grad_k", "nk", F32), ("grad_v", "nk", F32))
    edge = {"el": ("mH", F32), "er": ("nH", F32), "ee": ("eH", F32), "V": ("nk", F32)}
    g_edge = (("grad_el", "mH", F32), ("grad_er", "nH", F32), ("grad_ee", "eH", F32), ("grad_v", "nk", F32))
    gatv2 = {"xt": ("mk", F32), "xs": ("nk", F32), "att": ("att", F32)}
    gatv2_b = {**gatv2, "P": ("eH", F32), "G": ("mk", F32)}
    g_gatv2 = (("grad_xt", "mk", F32), ("grad_xs", "nk", F32), ("grad_att", "att", F32))
    cases += [
        # heads == 1: attention() and attention_backward() call flex_attention{,_backward} (heads=None), P and work are [nnz]
        _forward("attention", qkv1, (SCALE,), P_QKV, pkind="e", heads=1, ptr_heads=None),
        _backward("attention_backward", {**qkv1, "P": ("e", F32), "G": ("mk", F32)}, (SCALE,), g_qkv1, P_QKV_B, work="e", heads=1, ptr_heads=None),
        _forward("attention_dropout", qkv1, (SCALE, DROP, SEED), P_DROP, probs="probs", pass_heads=True),  # no bias: a None pointer
        _forward("gat_edge_attention", edge, (SLOPE, DROP, SEED), P_EDGE, probs="probs"),
        _backward("gat_edge_attention_backward", {**edge, "P": ("eH", F32), "G": ("mk", F32)}, (SLOPE, DROP, SEED), g_edge, P_EDGE_B,
                  no_work_if="grad_ee"),
        _forward("gatv2_attention", gatv2, (SLOPE,), P_GATV2),
        _backward("gatv2_attention_backward", gatv2_b, (SLOPE,), g_gatv2, P_GATV2_B, att_work_if="grad_att"),
        _forward("gatv2_attention_dropout", gatv2, (SLOPE, DROP, SEED), P_GATV2_DROP, probs="probs"),
        _backward("gatv2_attention_dropout_backward", gatv2_b, (SLOPE, DROP, SEED), g_gatv2, P_GATV2_DROP_B, att_work_if="grad_att"),
    ]
    return cases


CASES = _cases()
BACKWARD = [c for c in CASES if c.work is not None]
WRAPPERS = sorted({c.name for c in CASES})
_ids = {"ids": lambda c: c.id}


def test_the_table_names_every_wrapper_with_a_ptr_companion():
    ptr = sorted(n[:-4] for n in vars(binding.Plan) if n.endswith("_ptr") and ("attention" in n))
    assert WRAPPERS == ptr and len(WRAPPERS) == 26
    assert all(callable(getattr(binding.Plan, n)) for n in WRAPPERS)


# ---- the plans: an 8 x 8 graph with 20 entries (one row and one column without any) and one without entries

_plans = {}


def plan(empty=False):
    if empty not in _plans:
        if empty:
            a = binding.HostCsr(np.zeros(9, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), n=8)
        else:
            rng = np.random.default_rng(8)
            deg = [3, 0, 5, 2, 1, 4, 2, 3]
            col = np.concatenate([np.sort(rng.choice(7, d, replace=False)) for d in deg])
            a = binding.HostCsr(np.concatenate([[0], np.cumsum(deg)]), col, np.ones(len(col), np.float32), n=8)
        _plans[empty] = (flex_amd.Plan(a, K, attention=True, attention_backward=True), a)
    return _plans[empty]


def _shape(a, kind, heads):
    return {"mk": (a.m, K), "nk": (a.n, K), "mH": (a.m, heads), "nH": (a.n, heads), "eH": (a.nnz, heads), "e": (a.nnz,),
            "att": (heads, K // heads)}[kind]


@contextlib.contextmanager
def _allocations():
    """The tensors torch.empty and torch.zeros hand out inside the block, kept alive so that no address is used twice."""
    log, real = [], {f: getattr(torch, f) for f in ("empty", "zeros")}

    def spy(f):
        def alloc(*args, **kw):
            log.append(real[f](*args, **kw))
            return log[-1]
        return alloc

    for f in real:
        setattr(torch, f, spy(f))
    try:
        yield log
    finally:
        for f, fn in real.items():
            setattr(torch, f, fn)


class Run(NamedTuple):
    outs: tuple      # the wrapper's result as a tuple: (out,) or the gradients
    calls: list      # [(names, values)] of the _ptr call, bound to its signature, pointers decoded to tokens
    given: dict      # the optional tensors that were passed in
    want: tuple      # per output: wanted


def _run(c, empty=False, want=None, give=(), swap=None, scalars=None, raw=None):
    """Calls wrapper c.name with name + "_ptr" shadowed on the plan instance.  give: the optional tensors to pass ("P", "work",
    "att_work" and keywords of c.outs); swap: {token: tensor} replaces operands; want: passed where it is not None."""
    p, a = plan(empty)
    tensors = {t: torch.zeros(_shape(a, kind, c.heads), dtype=dt, device="cuda") for t, (kind, dt) in c.ops.items()}
    kw = {}
    for k, v in c.kw.items():
        if isinstance(v, tuple):
            tensors[k] = torch.zeros(_shape(a, v[0], c.heads), dtype=v[1], device="cuda")
        else:
            kw[k] = v
    tensors.update(swap or {})
    given = {}
    for k, kind, dt in c.outs:
        if k in give:
            given[k] = torch.ones(_shape(a, kind, c.heads), dtype=dt, device="cuda")
    if "P" in give and c.probs:
        given[c.probs[0]] = torch.ones(_shape(a, c.probs[1], c.heads), dtype=F32, device="cuda")
    if "work" in give:
        given["work"] = torch.ones(_shape(a, c.work, c.heads), dtype=F32, device="cuda")
    if "att_work" in give:
        given["att_work"] = torch.ones(max(p.gatv2_attention_work_size(), 1), dtype=F32, device="cuda")
    kw.update({k: tensors[k] for k in c.kw if k in tensors}, **given)
    default = inspect.signature(getattr(binding.Plan, c.name)).parameters
    if want is not None:
        kw["want"] = want
    eff = tuple(want if want is not None else default["want"].default) if c.work else (True,)
    eff = eff + (False,) * (len(c.outs) - len(eff))
    raw = [] if raw is None else raw
    setattr(p, c.name + "_ptr", lambda *args, **kwargs: raw.append((args, kwargs)))
    try:
        with _allocations() as made:
            res = getattr(p, c.name)(*(tensors[t] for t in c.ops), *(c.scalars if scalars is None else scalars), **kw)
    finally:
        delattr(p, c.name + "_ptr")
    outs = res if c.work else (res,)
    # pointers back to tokens: operands, what came back, and what the wrapper allocated for itself and kept
    names = {t.data_ptr(): tok for tok, t in tensors.items()}
    names.update({t.data_ptr(): "P" if c.probs and k == c.probs[0] else k for k, t in given.items()})
    names.update({t.data_ptr(): k for (k, _, _), t in zip(c.outs, outs) if t is not None})
    for t in made:
        if not any(t is o for o in outs) and t.dtype == F32 and t.is_cuda:
            if c.work and tuple(t.shape) == _shape(a, c.work, c.heads):
                names.setdefault(t.data_ptr(), "work")
            elif c.att_work_if and t.dim() == 1 and t.numel() == max(p.gatv2_attention_work_size(), 1):
                names.setdefault(t.data_ptr(), "att_work")
    sig = inspect.signature(getattr(binding.Plan, c.name + "_ptr"))
    calls = []
    for args, kwargs in raw:
        b = sig.bind(p, *args, **kwargs)
        b.apply_defaults()
        items = list(b.arguments.items())[1:]
        calls.append(([k for k, _ in items], [v if not k.endswith("_ptr") or v is None else names.get(v, hex(v)) for k, v in items]))
    return Run(tuple(outs), calls, given, eff)


def _expected(c, run, stream):
    """c.ptr with every token resolved: a tensor's token where the call has to pass it, None where it must not."""
    wanted = {k for (k, _, _), w in zip(c.outs, run.want) if w}
    present = set(c.ops) | {k for k, v in c.kw.items() if isinstance(v, tuple)} | wanted | ({"P"} if c.probs and c.probs[0] in run.given else set())
    if "work" in run.given or (c.work and c.no_work_if not in wanted):
        present.add("work")
    if c.att_work_if in wanted:
        present.add("att_work")
    return [c.ptr_heads if t == "heads" else stream if t == STREAM else (t if t in present else None) if isinstance(t, str) else t for t in c.ptr]


def _check_outputs(c, run, a, zero=False):
    for (k, kind, dt), t, w in zip(c.outs, run.outs, run.want):
        if not w:
            assert t is None, f"{c.name}: {k} is not wanted and came back"
            continue
        assert t.is_cuda and t.is_contiguous() and t.dtype == dt and tuple(t.shape) == _shape(a, kind, c.heads), (c.name, k, t.dtype, t.shape)
        if k in run.given:
            assert t is run.given[k], f"{c.name}: a given {k} is not the one that comes back"
        if zero:
            assert not bool(t.float().count_nonzero()), f"{c.name}: a new {k} on a plan without entries is not zero"


# ---- 1. argument order, scalars, heads, the stream; outputs allocated

@pytest.mark.parametrize("c", CASES, **_ids)
def test_the_ptr_call_has_the_tables_arguments_and_new_outputs(c):
    _, a = plan()
    streams = [None, torch.cuda.Stream()]
    assert streams[1].cuda_stream != torch.cuda.current_stream().cuda_stream
    for s in streams:
        with torch.cuda.stream(s) if s is not None else contextlib.nullcontext():
            handle = torch.cuda.current_stream().cuda_stream
            for give in ((), ("P",)):
                run = _run(c, give=give)
                assert len(run.calls) == 1
                assert run.calls[0][1] == _expected(c, run, handle), (c.id, give, run.calls[0])
                _check_outputs(c, run, a)


@pytest.mark.parametrize("c", CASES, **_ids)
def test_given_outputs_and_work_arrays_are_used_and_returned_by_identity(c):
    _, a = plan()
    give = tuple(k for k, _, _ in c.outs) + (("P",) if c.probs else ("work",)) + (("att_work",) if c.att_work_if else ())
    run = _run(c, give=give, want=(True,) * len(c.outs) if c.work else None)
    assert len(run.calls) == 1 and run.calls[0][1] == _expected(c, run, torch.cuda.current_stream().cuda_stream), (c.id, run.calls[0])
    _check_outputs(c, run, a)
    assert all(t is run.given[k] for (k, _, _), t in zip(c.outs, run.outs))


@pytest.mark.parametrize("c", CASES, **_ids)
def test_new_outputs_on_a_plan_without_entries_are_zero(c):
    _, a = plan(empty=True)
    run = _run(c, empty=True, want=(True,) * len(c.outs) if c.work else None)
    assert len(run.calls) == 1
    _check_outputs(c, run, a, zero=True)


# ---- 2. want

@pytest.mark.parametrize("c", BACKWARD, **_ids)
def test_an_output_that_want_leaves_out_is_none_and_so_is_its_pointer(c):
    _, a = plan()
    n = len(c.outs)
    patterns = [tuple(j != i for j in range(n)) for i in range(n)] + [(True,) * n]
    if "dropout_backward" in c.name and n == 4:
        patterns.append((True, True, True))  # three flags: no gBias
    for want in patterns:
        run = _run(c, want=want)
        exp = _expected(c, run, torch.cuda.current_stream().cuda_stream)
        assert len(run.calls) == 1 and run.calls[0][1] == exp, (c.id, want, run.calls[0])
        _check_outputs(c, run, a)
        got = dict(zip(*run.calls[0]))
        if c.no_work_if:  # gat_edge_attention_backward: gEe is the work array where it is wanted
            assert (got["dWork_ptr"] is None) == want[2] and (got["dWork_ptr"] == "work") == (not want[2])
        if c.att_work_if:
            assert (got["dAttWork_ptr"] == "att_work") == want[2] and (got["dAttWork_ptr"] is None) == (not want[2])


def test_the_default_want_of_the_dropout_backward_has_no_bias_gradient():
    for name in ("attention_dropout_backward", "attention_bf16_dropout_backward"):
        c = next(c for c in CASES if c.name == name)
        run = _run(c)
        assert run.want == (True, True, True, False) and run.outs[3] is None and dict(zip(*run.calls[0]))["dGradBias_ptr"] is None


# ---- 3. bad operands

def _operands(c):
    return {**c.ops, **{k: v for k, v in c.kw.items() if isinstance(v, tuple)}}


@pytest.mark.parametrize("c", CASES, **_ids)
def test_an_operand_of_the_wrong_dtype_or_shape_is_refused_before_the_call(c):
    _, a = plan()
    for tok, (kind, dt) in _operands(c).items():
        shape = _shape(a, kind, c.heads)
        for bad in (torch.zeros(shape, dtype=torch.float64, device="cuda"),
                    torch.zeros((shape[0] + 1,) + shape[1:], dtype=dt, device="cuda")):
            raw = []
            with pytest.raises(AssertionError):
                _run(c, swap={tok: bad}, raw=raw)
            assert raw == [], f"{c.name}: {tok} {bad.dtype} {tuple(bad.shape)} reached the library call"


# ---- 4. small cases

def test_a_one_dimensional_bias_is_taken_as_nnz_by_one_at_one_head():
    _, a = plan()
    for name in ("attention_bias", "attention_dropout"):
        c = next(c for c in CASES if c.name == name and "bias" in _operands(c))
        c = c._replace(heads=1, ptr_heads=1, kw={**c.kw, "heads": 1})
        bias = torch.zeros(a.nnz, device="cuda")
        run = _run(c, swap={"bias": bias})
        assert len(run.calls) == 1 and run.calls[0][1] == _expected(c, run, torch.cuda.current_stream().cuda_stream), run.calls[0]


@pytest.mark.parametrize("c", [c for c in CASES if SEED in c.scalars and c.name.startswith("gat")], **_ids)
def test_a_negative_seed_arrives_as_its_64_bit_twos_complement(c):
    run = _run(c, scalars=tuple(-3 if s == SEED else s for s in c.scalars))
    got = dict(zip(*run.calls[0]))
    assert got["seed"] == (-3) & MASK64 == 2 ** 64 - 3

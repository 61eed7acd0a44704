"""float64 reference and bound of the fused ReLU and dropout of the bf16 root layer (include/flex_axw.h: flex_axw_run_root_act_bf16), for
tests/test_gpu_axw_bf16_act.py, on top of a reference (ref, E) of tests/axw_bf16_root_ref.py: the kernel's fp32 z lies within E of ref.
ReLU is 1-Lipschitz, so relu(z) lies within E of relu(ref); the product with cs is one fp32 rounding, |fl(a cs) - a cs| <= 2^-24 cs a with
a <= relu(|ref| + E).  Hence the fp32-stage term cs (1 + 2^-23) E + 2^-24 cs relu(|ref| + E) around cs relu(ref), to which the one bf16
rounding is applied (axw_bf16_ref.check -> bound_bf16).  Dropped entries and padding columns are +0 bits exactly.  The backward's dZ is
exact arithmetic on bits: an fp32 product and to_bf16."""
import numpy as np

from attention_bf16_ref import from_bf16, to_bf16
from axw_bf16_ref import check
from flex_amd import binding


def cs_of(p):
    """1.0f / (1.0f - p) as the host computes it, in fp32"""
    return np.float32(1) / (np.float32(1) - np.float32(p))


def keep_mask(seed, p, n, c):
    """bool [n, c]: flex_dropout_mask over idx = row * c + col; p == 0 evaluates no hash and keeps everything"""
    return binding.dropout_mask(seed, p, 0, n * c).reshape(n, c).astype(bool) if p > 0 else np.ones((n, c), bool)


def act_reference(ref, E, p):
    """(cs relu(ref), the fp32-stage bound around it)"""
    cs = float(cs_of(p))
    with np.errstate(invalid="ignore", over="ignore"):
        return cs * np.maximum(ref, 0.0), cs * (1 + 2.0 ** -23) * E + 2.0 ** -24 * cs * np.maximum(np.abs(ref) + E, 0.0)


def check_act(ref, E, p, seed, out_bits, what=""):
    """(message or None, worst err / bound over the kept entries, share of nonzero entries, share of dropped entries) of bf16 bits Out
    [n x cp]: dropped entries and padding +0 bits, kept entries within the bound of act_reference."""
    (n, c), keep = ref.shape, keep_mask(seed, p, *ref.shape)
    if out_bits[:, :c][~keep].any():
        return f"[{what}] {int((out_bits[:, :c][~keep] != 0).sum())} dropped entries are not +0 bits", np.inf, 0.0, 0.0
    r, b = act_reference(ref, E, p)
    msg, worst = check(np.where(keep, r, 0.0), np.where(keep, b, 1.0), out_bits, what)  # a dropped entry: 0 against 0
    return msg, worst, float((out_bits[:, :c] != 0).mean()), float((~keep).mean())


def dz_bits(out_bits, dout, c, p):
    """bf16 bits [n x cp] of dZ = Out > 0 ? rn_bf16(fp32(dOut) cs) : +0, columns >= c +0; dout: fp32 [n x cp] of bf16 numbers"""
    with np.errstate(invalid="ignore", over="ignore"):
        z = np.where(from_bf16(out_bits) > 0, to_bf16(dout.astype(np.float32) * cs_of(p)), np.uint16(0))
    z[:, c:] = 0
    return z

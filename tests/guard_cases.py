"""The guarded optimiser step (include/rrnet_hip.h: rr_grad_norm / rr_guard_decide / rr_adam_step_guarded) restated in
numpy float64, and the input builders of tests/test_guard_gpu.py.

`sum_squares` is the plain float64 sum.  `device_order_sum` walks the SAME summation order as the two kernels (the header
states it): squares are exact in double and every addition rounds the same way wherever it runs, so this sum -- and with
it the clip factor that `decide` derives from it -- equals the device's bit for bit.  `decide` is §1 of the contract as
written, running products included; `adam_ema` is Adam and the EMA in float64."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = ("applied", "skipped", "clipped", "beta1_pow", "beta2_pow", "norm", "norm_max", "bad", "skip", "scale",
         "step_size", "bc2_sqrt", "ema_d", "ema_omd", "reserved0", "reserved1", "b1", "omb1", "b2", "omb2")
IX = {n: i for i, n in enumerate(SLOTS)}
EXACT_SLOTS = (0, 1, 2, 3, 4, 9, 10, 11, 12, 13)     # what the host restates exactly


def header_define(name):
    text = open(os.path.join(ROOT, "include", "rrnet_hip.h")).read()
    return int(re.search(r"(?m)^#define\s+%s\s+(\d+)\s*$" % name, text).group(1))


def nonfinite_mask(g):
    return (np.ascontiguousarray(g, dtype=np.float32).view(np.uint32) & np.uint32(0x7f800000)) == np.uint32(0x7f800000)


def sum_squares(g):
    """(float64 sum of the squares of the finite words, count of the NaN / Inf words)."""
    bad = nonfinite_mask(g)
    x = np.where(bad, 0.0, np.asarray(g, dtype=np.float64))
    return float(np.sum(x * x)), int(bad.sum())


def _butterfly(v):
    """xor butterfly over the last axis (64 lanes), offsets 32 .. 1: every lane ends with the wave's sum."""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def _block_sums(acc, threads):
    """acc [blocks, threads] per-lane sums -> [blocks]: butterfly per wave, then the waves added in order from 0."""
    w = _butterfly(acc.reshape(acc.shape[0], threads // 64, 64))
    t = np.zeros(acc.shape[0])
    for k in range(threads // 64):
        t = t + w[:, k]
    return t


def device_order_partials(g, blocks, threads):
    """partial[blocks] and bad[blocks] of rr_grad_norm, in its summation order."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    assert g.size % 4 == 0
    bad = nonfinite_mask(g)
    x = np.where(bad, 0.0, g.astype(np.float64))
    sq = x * x
    n4, total = g.size // 4, blocks * threads
    rounds = -(-n4 // total)
    pad = rounds * total * 4 - g.size
    sq = np.concatenate([sq, np.zeros(pad)]).reshape(rounds, total, 4)       # adding +0.0 changes no bit
    cnt = np.concatenate([bad, np.zeros(pad, dtype=bool)]).reshape(rounds, total, 4)
    acc = np.zeros(total)
    for r in range(rounds):
        for e in range(4):
            acc = acc + sq[r, :, e]
    return _block_sums(acc.reshape(blocks, threads), threads), cnt.sum(axis=(0, 2)).reshape(blocks, threads).sum(axis=1)


def device_order_sum(g, blocks, threads):
    """(S, B) as rr_guard_decide forms them from rr_grad_norm's partials."""
    if g.size == 0:
        return 0.0, 0
    partial, bad = device_order_partials(g, blocks, threads)
    rounds = -(-blocks // threads)
    p = np.concatenate([partial, np.zeros(rounds * threads - blocks)]).reshape(rounds, threads)
    acc = np.zeros(threads)
    for r in range(rounds):
        acc = acc + p[r]
    return float(_block_sums(acc.reshape(1, threads), threads)[0]), int(bad.sum())


def fresh_ctl():
    ctl = np.zeros(len(SLOTS))
    ctl[IX["beta1_pow"]] = ctl[IX["beta2_pow"]] = 1.0
    return ctl


def _f32(x):
    return float(np.float32(x))


def decide(ctl, S, B, grad_scale=1.0, max_norm=math.inf, skip_nonfinite=False, lr=1e-3, beta1=0.9, beta2=0.999,
           ema_decay=0.0, ema_warmup=False):
    """rr_guard_decide on the host: returns the next record (the argument is not modified)."""
    c = np.array(ctl, dtype=np.float64)
    norm = math.inf if B > 0 else math.sqrt(S) * grad_scale
    skip = bool(skip_nonfinite) and (B > 0 or not math.isfinite(norm))
    c[IX["bad"]], c[IX["norm"]], c[IX["skip"]] = float(B), norm, 1.0 if skip else 0.0
    if skip:
        c[IX["skipped"]] += 1.0
        return c
    coef = 1.0
    if math.isfinite(max_norm) and math.isfinite(norm):
        coef = min(1.0, max_norm / (norm + 1e-6))
    if coef < 1.0:
        c[IX["clipped"]] += 1.0
    c[IX["applied"]] += 1.0
    c[IX["beta1_pow"]] *= beta1
    c[IX["beta2_pow"]] *= beta2
    applied = c[IX["applied"]]
    c[IX["scale"]] = _f32(grad_scale * coef)
    c[IX["step_size"]] = _f32(lr / (1.0 - c[IX["beta1_pow"]]))
    c[IX["bc2_sqrt"]] = _f32(math.sqrt(1.0 - c[IX["beta2_pow"]]))
    d = ema_decay
    if ema_warmup:
        d = min(ema_decay, (1.0 + applied) / (10.0 + applied))
    c[IX["ema_d"]], c[IX["ema_omd"]] = _f32(d), _f32(1.0 - d)
    c[IX["reserved0"]] = c[IX["reserved1"]] = 0.0
    c[IX["b1"]], c[IX["omb1"]], c[IX["b2"]], c[IX["omb2"]] = _f32(beta1), _f32(1.0 - beta1), _f32(beta2), _f32(1.0 - beta2)
    if math.isfinite(norm):
        c[IX["norm_max"]] = max(c[IX["norm_max"]], norm)
    return c


def adam_ema(p, m, v, ema, g, ctl, eps=1e-8):
    """rr_adam_step_guarded in float64 with the constants of `ctl` -> (p, m, v, ema); ema may be None.  A skip returns the
    arguments."""
    if ctl[IX["skip"]] != 0.0:
        return p, m, v, ema
    gg = np.asarray(g, dtype=np.float64) * ctl[IX["scale"]]
    m = m * ctl[IX["b1"]] + gg * ctl[IX["omb1"]]
    v = v * ctl[IX["b2"]] + gg * gg * ctl[IX["omb2"]]
    p = p - ctl[IX["step_size"]] * (m / (np.sqrt(v) / ctl[IX["bc2_sqrt"]] + eps))
    if ema is not None:
        ema = ema * ctl[IX["ema_d"]] + p * ctl[IX["ema_omd"]]
    return p, m, v, ema


# ---- input builders -------------------------------------------------------------------------------------------------
def gradient(n, seed, scale=1.0):
    """n float32 words with magnitudes over several binades (so that the order of a float32 sum would matter)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n) * np.exp2(rng.integers(-6, 3, n)) * scale
    return g.astype(np.float32)


def sizes(blocks_of, threads):
    """The n of the GPU cases, named, from the exported block count and the kernel's thread count: 4 words; one workgroup
    exactly full, one vector less, one vector more; a partial last workgroup; the grid-stride loop taken more than once
    (an unrolled pair of rounds and a tail) at the grid cap, which is more partials than the decide kernel has lanes."""
    per_block = 4 * threads
    cap_n = per_block
    while blocks_of(cap_n * 2) > blocks_of(cap_n):        # smallest power-of-two multiple that reaches the cap
        cap_n *= 2
    cap = blocks_of(cap_n * 2)
    cases = {
        "one-vector": 4,
        "block-full": per_block,
        "block-minus-vector": per_block - 4,
        "block-plus-vector": per_block + 4,
        "partial-last-block": 5 * per_block + 4 * 37,
        # two full rounds of the whole grid (the kernel's two-deep unrolled loop runs once) and a partial third (its tail loop)
        "grid-stride-wraps": cap * per_block * 2 + per_block * 301 + 4 * 37,
    }
    assert blocks_of(cases["grid-stride-wraps"]) == cap and cap > threads
    assert cases["grid-stride-wraps"] <= 5_000_000
    return cases

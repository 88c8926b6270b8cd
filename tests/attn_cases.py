"""Shared by tests/test_attention_host.py, tests/test_attention_gpu.py and tools/gen_golden_attention.py: the cases of the
dilated-window attention (csrc/attn.hip), an independent float64 oracle of its rule, and the float32 yardstick.

The rule (include/rrnet_hip_attn.h).  q, k [n, h, w, ck], v [n, h, w, cv]; window (kh, kw), dilation (dh, dw), padding
(ph, pw), stride 1; oh = h + 2 ph - dh (kh - 1), cy = dh (kh // 2) - ph (likewise ow, cx).  Output (i, j), tap t = a kw + b reads
the source (y, x) = (i - ph + a dh, j - pw + b dw): logit[t] = q[i + cy, j + cx] . k[y, x] inside the map and 0 outside (a padded
tap is NOT masked: it enters the softmax with logit 0 and value 0), P = softmax_t, ctx[i, j] = sum_t P[t] v[y, x].

The oracle works on zero-padded copies of k and v and on slices of them — one slice per tap — not on F.unfold, which is what
the reference uses; tests/test_attention_host.py holds it against the golden file the reference wrote.  `window_rule(..,
dtype=np.float32)` is the yardstick: the same sums with every product rounded to float32 and added one term after another
in loop order (channels ascending, taps ascending; the helpers._seq32 convention), the exponential in float32.  What a
kernel may differ by is the summation order only, so its error is held to MARGIN times that chain's error."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "self_attention.npz")
MARGIN = 4.0                  # the project's margin where only the summation order differs (helpers.conv_accepts, dcn_fp64_ratios.txt)
RELU_MARGIN = 1e-4            # the golden's pre-ReLU BatchNorm outputs keep this distance from 0

# ops-level cases: n, ck, cv, (h, w), kernel, dilation, padding, scale of q and k
CASES = {
    "A": dict(n=2, ck=8, cv=12, hw=(7, 9), kernel=(3, 3), dilation=(2, 2), padding=(2, 2), scale=1.0),
    "B": dict(n=2, ck=8, cv=12, hw=(13, 11), kernel=(5, 5), dilation=(6, 6), padding=(12, 12), scale=1.0),
    "C": dict(n=1, ck=4, cv=4, hw=(6, 10), kernel=(2, 3), dilation=(1, 2), padding=(0, 2), scale=1.0),
    "D": dict(n=2, ck=64, cv=64, hw=(40, 72), kernel=(5, 5), dilation=(6, 6), padding=(12, 12), scale=1.0),
    # as A with q and k scaled: |logit| beyond 100, where exp() without the maximum subtracted overflows float32
    "E": dict(n=2, ck=8, cv=12, hw=(7, 9), kernel=(3, 3), dilation=(2, 2), padding=(2, 2), scale=7.0),
}
# module-level cases of the golden file (SelfAttentionModule, cin 16, ck 8, cv 12): geometries A and B; C (an even,
# rectangular kernel whose output is smaller than the map) is in the file for the oracle only
MODULE_CASES = {
    "A": dict(n=2, cin=16, ck=8, cv=12, hw=(7, 9), kernel=3, dilation=2, padding=2),
    "B": dict(n=1, cin=16, ck=8, cv=12, hw=(13, 11), kernel=5, dilation=6, padding=12),
    "C": dict(n=1, cin=8, ck=4, cv=4, hw=(6, 10), kernel=(2, 3), dilation=(1, 2), padding=(0, 2)),
}


def pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def geometry(h, w, kernel, dilation, padding):
    """-> (oh, ow, cy, cx)"""
    (kh, kw), (dh, dw), (ph, pw) = pair(kernel), pair(dilation), pair(padding)
    return h + 2 * ph - dh * (kh - 1), w + 2 * pw - dw * (kw - 1), dh * (kh // 2) - ph, dw * (kw // 2) - pw


def case_inputs(name):
    """-> q, k, v, dctx: float32-exact values as float64 arrays, NHWC."""
    c = CASES[name]
    rng = np.random.default_rng([2210, sorted(CASES).index("A" if name == "E" else name)])
    n, (h, w) = c["n"], c["hw"]
    oh, ow, _, _ = geometry(h, w, c["kernel"], c["dilation"], c["padding"])
    # q, k around 1 / sqrt(sqrt(ck)): logits of order 1, a softmax that is neither flat nor one-hot
    s = c["scale"] / c["ck"] ** 0.25
    q = (rng.standard_normal((n, h, w, c["ck"])) * s).astype(np.float32).astype(np.float64)
    k = (rng.standard_normal((n, h, w, c["ck"])) * s).astype(np.float32).astype(np.float64)
    v = rng.standard_normal((n, h, w, c["cv"])).astype(np.float32).astype(np.float64)
    dctx = rng.standard_normal((n, oh, ow, c["cv"])).astype(np.float32).astype(np.float64)
    return q, k, v, dctx


def _chain(terms, dtype):
    """Sum of a list of arrays: float64 -> np.sum's; float32 -> one term after another, in list order."""
    if dtype == np.float64:
        return np.sum(np.stack(terms, 0), 0)
    acc = terms[0].astype(np.float32)
    for t in terms[1:]:
        acc = (acc + t.astype(np.float32)).astype(np.float32)
    return acc


def _dot(a, b, dtype):
    """sum over the last axis of a * b: channels ascending in float32."""
    if dtype == np.float64:
        return (a * b).sum(-1)
    return _chain([(a[..., c] * b[..., c]).astype(np.float32) for c in range(a.shape[-1])], dtype)


def window_rule(q, k, v, kernel, dilation, padding, dctx=None, dtype=np.float64):
    """-> dict(ctx, p[, ds, dq, dk, dv]) by the rule above, every array of `dtype`.  Works on zero-padded copies of k, v (and of
    the gradients of k, v, which are cropped at the end); a tap is one slice."""
    (kh, kw), (dh, dw), (ph, pw) = pair(kernel), pair(dilation), pair(padding)
    q, k, v = (np.asarray(t, np.float64).astype(dtype) for t in (q, k, v))
    n, h, w, ck = q.shape
    oh, ow, cy, cx = geometry(h, w, kernel, dilation, padding)
    assert oh >= 1 and ow >= 1 and cy >= 0 and cx >= 0 and cy + oh <= h and cx + ow <= w
    padded = lambda t: np.pad(t, ((0, 0), (ph, ph), (pw, pw), (0, 0)))
    kp, vp = padded(k), padded(v)
    taps = [(a, b) for a in range(kh) for b in range(kw)]
    window = lambda t, a, b: t[:, a * dh:a * dh + oh, b * dw:b * dw + ow]
    qc = q[:, cy:cy + oh, cx:cx + ow]
    logit = np.stack([_dot(qc, window(kp, a, b), dtype) for a, b in taps], -1)
    e = np.exp(logit - logit.max(-1, keepdims=True)).astype(dtype)
    p = (e / _chain([e[..., t] for t in range(len(taps))], dtype)[..., None]).astype(dtype)
    out = dict(p=p, ctx=_chain([(p[..., t, None] * window(vp, a, b)).astype(dtype) for t, (a, b) in enumerate(taps)], dtype))
    if dctx is None:
        return out
    dctx = np.asarray(dctx, np.float64).astype(dtype)
    dp = np.stack([_dot(dctx, window(vp, a, b), dtype) for a, b in taps], -1)
    s = _chain([(p[..., t] * dp[..., t]).astype(dtype) for t in range(len(taps))], dtype)
    ds = (p * (dp - s[..., None]).astype(dtype)).astype(dtype)
    dq = np.zeros_like(q)
    dq[:, cy:cy + oh, cx:cx + ow] = _chain([(ds[..., t, None] * window(kp, a, b)).astype(dtype) for t, (a, b) in enumerate(taps)], dtype)
    dkp, dvp = np.zeros_like(kp), np.zeros_like(vp)
    for t, (a, b) in enumerate(taps):              # taps ascending: every source position adds its readers in that order
        wk, wv = window(dkp, a, b), window(dvp, a, b)
        wk += (ds[..., t, None] * qc).astype(dtype)
        wv += (p[..., t, None] * dctx).astype(dtype)
    crop = lambda t: np.ascontiguousarray(t[:, ph:ph + h, pw:pw + w])
    out.update(ds=ds, dq=dq, dk=crop(dkp), dv=crop(dvp))
    return out


def error_ratios(got, ref, seq):
    """(max-abs ratio, RMS ratio) of the error got - ref against the chained-float32 error seq - ref.  A zero yardstick asks
    for a zero error: the ratio is then 0 or inf."""
    eg = np.asarray(got, np.float64) - ref
    es = np.asarray(seq, np.float64) - ref
    ratio = lambda a, b: 0.0 if a == 0.0 else (float("inf") if b == 0.0 else a / b)
    return (ratio(float(np.abs(eg).max()), float(np.abs(es).max())),
            ratio(float(np.sqrt(np.mean(eg * eg))), float(np.sqrt(np.mean(es * es)))))


def accepts(ratios, margin=MARGIN):
    return all(np.isfinite(r) and r <= margin for r in ratios)


# ---- the golden file ------------------------------------------------------------------------------------------------
def load_golden():
    return dict(np.load(GOLDEN, allow_pickle=False))


def golden_state(g, tag):
    """{state_dict key: array} of case `tag`."""
    pre = tag + "/state/"
    return {k[len(pre):]: a for k, a in g.items() if k.startswith(pre)}


def nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))

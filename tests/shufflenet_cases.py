"""Shared by tests/test_shufflenet_host.py, tests/test_shufflenet_gpu.py and tools/gen_golden_shufflenet.py: the cases of the
depthwise 3x3 convolution and the channel shuffle (csrc/depthwise.hip), an independent float64 oracle of their
rules, the float32 yardstick, and ShuffleNetV2's unit built from them.

The rules (include/rrnet_hip_dw.h).  x [n, h, w, c], filter f [c, 3, 3], padding 1, stride s; P = (h - 1) / s + 1,
Q = (w - 1) / s + 1.
  forward        y[n, i, j, ch] = sum_{a, b} f[ch, a, b] x[n, i s - 1 + a, j s - 1 + b, ch] (+ bias[ch]), taps inside the map
  data gradient  dx[n, y, x, ch] = sum over the (a, b) with (y + 1 - a), (x + 1 - b) divisible by s, quotients i < P, j < Q, of
                 f[ch, a, b] dy[n, i, j, ch]
  weight grad.   df[ch, a, b] = sum_{n, i, j} x[n, i s - 1 + a, j s - 1 + b, ch] dy[n, i, j, ch]
  shuffle        channel_shuffle(cat(a, b), 2): out[p, 2 i] = a[p, i], out[p, 2 i + 1] = b[p, i]

The oracle works on zero-padded copies and on strided slices of them — one slice per tap — not on F.conv2d, which is what the
reference's nn.Conv2d(groups=c) runs; tests/test_shufflenet_host.py holds it against the golden file the reference wrote.
`dtype=np.float32` is the yardstick: the same sums with every product rounded to float32 and added one term after another in
loop order (taps a, b ascending; for the weight gradient n, i, j ascending; the helpers._seq32 convention).  What a kernel may
differ by is the summation order only, so its error is held to MARGIN times that chain's error."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "shufflenet.npz")
KEYS = os.path.join(HERE, "golden", "shufflenet_keys.json")
MARGIN = 4.0                  # the project's margin where only the summation order differs (attn_cases.accepts)
RELU_MARGIN = 1e-4            # the golden's pre-ReLU BatchNorm outputs keep this distance from 0
WIDTHS = (0.5, 1.0, 1.5, 2.0)

# kernel cases (n, h, w, c, s).  (1,1,1,*): a single tap inside the map; (1,2,3,4,2): an even side at stride 2 (the last
# row has no lower neighbour output); c = 488: ShuffleNetV2 x2.0's widest half, more channel vectors than half a workgroup;
# (2,33,65,88,1): 4290 pixels, more than one slab tile (64 pixels) and more than one weight-gradient tile (128 pixels)
DW_CASES = [(1, 1, 1, 4, 1), (1, 1, 1, 4, 2), (1, 2, 3, 4, 2), (2, 7, 9, 8, 1), (2, 8, 6, 24, 2), (3, 13, 17, 48, 2),
            (1, 5, 5, 488, 1), (2, 33, 65, 88, 1)]
# the golden's chain: InvertedResidual(24, 48, 2, 2) -> InvertedResidual(48, 48, 1, 1) on a 2 x 24 x 9 x 11 input
UNITS = ((24, 48, 2, 2), (48, 48, 1, 1))
UNIT_INPUT = (2, 24, 9, 11)
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def out_hw(h, w, s):
    return (h - 1) // s + 1, (w - 1) // s + 1


def dw_inputs(case, seed=0):
    """-> x [n,h,w,c], f [c,3,3], bias [c], dy [n,P,Q,c], df0 [c,3,3] (a gradient already in the target): float32-exact
    values as float64 arrays."""
    n, h, w, c, s = case
    p, q = out_hw(h, w, s)
    rng = np.random.default_rng([2310, seed, DW_CASES.index(case) if case in DW_CASES else 99])
    r = lambda *shape: rng.standard_normal(shape).astype(np.float32).astype(np.float64)
    return r(n, h, w, c), r(c, 3, 3), r(c), r(n, p, q, c), r(c, 3, 3)


def _chain(terms, dtype, axis=0):
    """Sum of stacked terms along `axis`: float64 -> np.sum's; float32 -> one term after another, in order."""
    if dtype == np.float64:
        return np.sum(terms, axis)
    return np.cumsum(terms.astype(np.float32), axis=axis, dtype=np.float32).take(-1, axis)


def _windows(tp, p, q, s):
    """The nine strided slices of a padded tensor [n, h + 2, w + 2, c], taps a, b ascending -> each [n, p, q, c]."""
    return [tp[:, a:a + (p - 1) * s + 1:s, b:b + (q - 1) * s + 1:s] for a in range(3) for b in range(3)]


def _pad(t):
    return np.pad(t, ((0, 0), (1, 1), (1, 1), (0, 0)))


def dw_fwd(x, f, s, bias=None, dtype=np.float64):
    x, f = np.asarray(x, np.float64).astype(dtype), np.asarray(f, np.float64).astype(dtype)
    p, q = out_hw(x.shape[1], x.shape[2], s)
    terms = np.stack([(f.reshape(-1, 9)[:, t] * win).astype(dtype) for t, win in enumerate(_windows(_pad(x), p, q, s))])
    y = _chain(terms, dtype)
    if bias is not None:
        y = (y + np.asarray(bias, np.float64).astype(dtype)).astype(dtype)
    return y


def dw_bwd_data(dy, f, s, h, w, dtype=np.float64):
    """A scatter into a zero-padded dx, taps ascending (every dx position then receives its taps in ascending order), cropped."""
    dy, f = np.asarray(dy, np.float64).astype(dtype), np.asarray(f, np.float64).astype(dtype)
    n, p, q, c = dy.shape
    assert (p, q) == out_hw(h, w, s)
    dxp = np.zeros((n, h + 2, w + 2, c), dtype)
    for t, win in enumerate(_windows(dxp, p, q, s)):
        win += (f.reshape(-1, 9)[:, t] * dy).astype(dtype)
    return np.ascontiguousarray(dxp[:, 1:1 + h, 1:1 + w])


def dw_bwd_weight(x, dy, s, df0=None, dtype=np.float64):
    """-> df [c, 3, 3] (+ df0 in front of the chain, as an accumulating call starts from the target's value)."""
    x, dy = np.asarray(x, np.float64).astype(dtype), np.asarray(dy, np.float64).astype(dtype)
    n, p, q, c = dy.shape
    out = np.empty((c, 9), dtype)
    for t, win in enumerate(_windows(_pad(x), p, q, s)):
        terms = (win * dy).astype(dtype).reshape(-1, c)
        if df0 is not None:
            terms = np.concatenate([np.asarray(df0, np.float64).astype(dtype).reshape(c, 9)[None, :, t], terms], 0)
        out[:, t] = _chain(terms, dtype)
    return out.reshape(c, 3, 3)


def interleave(a, b):
    out = np.empty(a.shape[:-1] + (2 * a.shape[-1],), a.dtype)
    out[..., 0::2], out[..., 1::2] = a, b
    return out


def deinterleave(g):
    return np.ascontiguousarray(g[..., 0::2]), np.ascontiguousarray(g[..., 1::2])


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


# ---- ShuffleNetV2's unit out of the rules above (float64, NHWC) -----------------------------------------------------------
def _pw(x, w):
    """1x1 convolution, w [k, c] -> (y, backward(dy) -> (dx, dw))."""
    return x @ w.T, lambda dy: (dy @ w, np.einsum("nhwk,nhwc->kc", dy, x))


def _bn(y, gamma, beta, mean_run, var_run, train):
    """-> (z, backward(dz) -> (dy, dgamma, dbeta), (new running mean, new running var)); eval mode: no backward."""
    if not train:
        inv = 1.0 / np.sqrt(var_run + BN_EPS)
        return (y - mean_run) * inv * gamma + beta, None, (mean_run, var_run)
    cnt = y.shape[0] * y.shape[1] * y.shape[2]
    mean = y.mean((0, 1, 2))
    var = ((y - mean) ** 2).mean((0, 1, 2))
    inv = 1.0 / np.sqrt(var + BN_EPS)
    xhat = (y - mean) * inv

    def backward(dz):
        dbeta, dgamma = dz.sum((0, 1, 2)), (dz * xhat).sum((0, 1, 2))
        return gamma * inv * (dz - dbeta / cnt - xhat * dgamma / cnt), dgamma, dbeta
    run = ((1 - BN_MOMENTUM) * mean_run + BN_MOMENTUM * mean, (1 - BN_MOMENTUM) * var_run + BN_MOMENTUM * var * cnt / (cnt - 1))
    return xhat * gamma + beta, backward, run


def _branch(x, state, prefix, layout, stride, train, grads, bufs, margins):
    """One nn.Sequential of the unit.  layout: 'dw_pw' (banch1) or 'pw_dw_pw' (banch2).  -> (out, backward(dout) -> dx)."""
    steps = {"dw_pw": (("dw", 0), ("bn", 1, False), ("pw", 2), ("bn", 3, True)),
             "pw_dw_pw": (("pw", 0), ("bn", 1, True), ("dw", 3), ("bn", 4, False), ("pw", 5), ("bn", 6, True))}[layout]
    backs = []
    for step in steps:
        key = "%s.%d." % (prefix, step[1])
        if step[0] == "pw":
            w = state[key + "weight"][:, :, 0, 0]
            x, back = _pw(x, w)
            backs.append(("pw", key, back))
        elif step[0] == "dw":
            f = state[key + "weight"][:, 0]
            xin = x
            x = dw_fwd(xin, f, stride)
            backs.append(("dw", key, (xin, f)))
        else:
            x, back, run = _bn(x, state[key + "weight"], state[key + "bias"], state[key + "running_mean"],
                               state[key + "running_var"], train)
            bufs[key + "running_mean"], bufs[key + "running_var"] = run
            bufs[key + "num_batches_tracked"] = state[key + "num_batches_tracked"] + (1 if train else 0)
            mask = None
            if step[2]:
                margins.append(float(np.abs(x).min()))
                mask = x > 0
                x = x * mask
            backs.append(("bn", key, (back, mask)))

    def backward(g):
        for kind, key, what in reversed(backs):
            if kind == "pw":
                g, grads[key + "weight"] = what(g)
                grads[key + "weight"] = grads[key + "weight"][:, :, None, None]
            elif kind == "dw":
                xin, f = what
                grads[key + "weight"] = dw_bwd_weight(xin, g, stride)[:, None]
                g = dw_bwd_data(g, f, stride, xin.shape[1], xin.shape[2])
            else:
                back, mask = what
                g, grads[key + "weight"], grads[key + "bias"] = back(g * mask if mask is not None else g)
        return g
    return x, backward


def unit(x, state, prefix, inp, oup, stride, benchmodel, train, grads, bufs, margins):
    """InvertedResidual(inp, oup, stride, benchmodel) on x [n, h, w, c] -> (out, backward(dout) -> dx)."""
    if benchmodel == 1:
        half = x.shape[-1] // 2
        b, back2 = _branch(x[..., half:], state, prefix + ".banch2", "pw_dw_pw", stride, train, grads, bufs, margins)

        def backward(g):
            da, db = deinterleave(g)
            return np.concatenate([da, back2(db)], -1)
        return interleave(x[..., :half], b), backward
    a, back1 = _branch(x, state, prefix + ".banch1", "dw_pw", stride, train, grads, bufs, margins)
    b, back2 = _branch(x, state, prefix + ".banch2", "pw_dw_pw", stride, train, grads, bufs, margins)

    def backward(g):
        da, db = deinterleave(g)
        return back1(da) + back2(db)
    return interleave(a, b), backward


def chain(x, state, gy=None, train=True):
    """The golden's two units (UNITS; state-dict keys '0.*', '1.*') on x [n, h, w, c] -> dict(y[, dx, grads], bufs, margin)."""
    grads, bufs, margins, backs = {}, {}, [], []
    for i, (inp, oup, stride, bench) in enumerate(UNITS):
        x, back = unit(x, state, str(i), inp, oup, stride, bench, train, grads, bufs, margins)
        backs.append(back)
    out = dict(y=x, bufs=bufs, margin=min(margins))
    if gy is not None:
        g = gy
        for back in reversed(backs):
            g = back(g)
        out.update(dx=g, grads=grads)
    return out


# ---- the golden files -----------------------------------------------------------------------------------------------
def load_golden():
    return dict(np.load(GOLDEN, allow_pickle=False))


def load_keys():
    """{width as str: [[key, [shape]], ...]} of the reference's ShuffleNetV2, in state_dict order."""
    with open(KEYS) as fh:
        return json.load(fh)


def golden_state(g, pre="state/"):
    return {k[len(pre):]: a for k, a in g.items() if k.startswith(pre)}


def nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def nchw(a):
    return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))

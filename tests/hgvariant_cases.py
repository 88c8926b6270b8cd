"""Plain-torch restatements (CPU, float64 or float32) of what the dense and the SE hourglass add to the hourglass, and the
case tables of tests/test_hgvariants_host.py and tests/test_hgvariants_gpu.py.

Restated from the reference's backbones/se_hourglass.py (SELayer :12-27, ResidualBlock :30-60, ConvBNRelu :64-79,
Hourglass :82-142, HourglassNet :145-217) and backbones/dense_hourglass.py (HourglassNet.forward :179-202), with the sizes the
reference hard-codes as arguments.  Module tree, attribute names and construction order are the reference's, so state_dict
keys and seeded default initialisation are the same; tests/golden/hgvariants.npz (tools/gen_golden_hgvariants.py) holds what the
reference's own classes computed, and test_hgvariants_host.py holds these restatements to it.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

U32 = 2.0 ** -24
HG_TINY = dict(n=2, inplanes=(32, 32, 48), layer_nums=(1, 1, 2), stem=16, num_feats=256)
DENSE_TINY = dict(HG_TINY, stem=128, inplanes=(256, 32, 48))      # the dense sums need 2 * stem == inplanes[0] == num_feats
HG104 = dict(n=5, inplanes=(256, 256, 384, 384, 384, 512), layer_nums=(2, 2, 2, 2, 2, 4), stem=128, num_feats=256)


# ----------------------------------------------------------------------------------------------------------------------
# modules
# ----------------------------------------------------------------------------------------------------------------------
class Undecided(Exception):
    """A ReLU input nearer to 0 than the margin: the site, the BatchNorm in front of it, the channels concerned."""

    def __init__(self, site, bn, channels):
        super().__init__(site)
        self.site, self.bn, self.channels = site, bn, channels


class ReluSites:
    """`with ReluSites() as sites:` records the input of every ReLU a restatement applies to a feature map, in order, and the
    BatchNorm whose per-channel bias shifts that input.  guard = (first site, margin): the first site from there on with an
    input nearer to 0 than the margin raises Undecided (settle_relus)."""
    active = None

    def __init__(self, guard=None):
        self.pre, self.guard = [], guard

    def __enter__(self):
        ReluSites.active = self
        return self

    def __exit__(self, *exc):
        ReluSites.active = None

    def relu(self, x, bn):
        i = len(self.pre)
        self.pre.append(x.detach())
        if self.guard is not None and i >= self.guard[0]:
            near = x.detach().abs() < self.guard[1]
            if bool(near.any()):
                raise Undecided(i, bn, near.any(0).any(-1).any(-1))
        return torch.relu(x)


def relu(x, bn):
    return torch.relu(x) if ReluSites.active is None else ReluSites.active.relu(x, bn)


RELU_MARGIN = 1e-3        # no ReLU input of a settled tiny network lies nearer to 0: 25x the float32 restatement's largest error at
#                           any ReLU input of these networks (4e-5, at features of size 10 and more)


def settle_relus(net, x, margin=RELU_MARGIN):
    """Moves BatchNorm biases of `net` (float64, float32-representable values) by multiples of 3 * margin until, in a train-mode
    forward on x, no ReLU input lies within `margin` of 0 — site by site in forward order: a bias only moves what comes
    after it.  A ReLU network's gradient jumps where such a decision flips (one flip moves a weight gradient of these
    networks by up to 14 % of its scale), so only a network without undecided inputs has a float64 gradient that a float32
    evaluation can be held to.  -> [(parameter name, channel, new value)], the biases that differ from before."""
    before = {k: v.clone() for k, v in net.state_dict().items()}
    net.train()
    first = 0
    for _ in range(20000):
        try:
            with torch.no_grad(), ReluSites(guard=(first, margin)):
                net(x)
            break
        except Undecided as e:
            first = e.site
            with torch.no_grad():
                e.bn.bias[e.channels] = (e.bn.bias[e.channels] + 3 * margin).float().double()
    else:
        raise RuntimeError("settle_relus did not converge")
    after = {k: v.clone() for k, v in net.state_dict().items()}
    net.load_state_dict({k: (after[k] if k.endswith(".bias") else before[k]) for k in before})     # (running statistics as they were)
    moved = []
    for k in before:
        if k.endswith(".bias"):
            for c in torch.nonzero(after[k] != before[k]).flatten().tolist():
                moved.append((k, c, float(after[k][c])))
    return moved


def apply_nudges(state, keys, channels, values):
    """det_fill's state dict with the settled biases put in (keys / channels / values: the golden's `<tag>/nudge_*` records)."""
    state = {k: v.clone() for k, v in state.items()}
    for k, c, v in zip(keys, channels, values):
        state[str(k)][int(c)] = float(v)
    return state


class SELayer(nn.Module):
    def __init__(self, channel, reduction=16):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Sequential(nn.Linear(channel, channel // reduction, bias=False), nn.ReLU(inplace=True),
                                nn.Linear(channel // reduction, channel, bias=False), nn.Sigmoid())

    def forward(self, x):
        return x * self.fc(x.mean((2, 3)))[:, :, None, None]


class Block(nn.Module):
    """The residual block; se=True: with the SELayer between bn2 and the add (constructed between bn2 and the skip)."""

    def __init__(self, inplanes, planes, stride=1, se=False):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        if se:
            self.se = SELayer(planes, 16)
        self.skip_connection = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride=stride, bias=False), nn.BatchNorm2d(planes)) \
            if (stride != 1 or inplanes != planes) else nn.Sequential()

    def forward(self, x):
        out = self.bn2(self.conv2(relu(self.bn1(self.conv1(x)), self.bn1)))
        if hasattr(self, "se"):
            out = self.se(out)
        return relu(out + self.skip_connection(x), self.bn2)


class CBR(nn.Module):
    def __init__(self, k, cin, cout, relu):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, padding=(k - 1) // 2, bias=False)
        self.bn = nn.BatchNorm2d(cout)
        self.with_relu = relu

    def forward(self, x):
        y = self.bn(self.conv(x))
        return relu(y, self.bn) if self.with_relu else y


class _ReLU(nn.Module):
    """The stem's ReLU; `bn`: a one-element list holding the BatchNorm in front of it (a list: not a submodule of this one)."""
    bn = (None,)

    def forward(self, x):
        return relu(x, self.bn[0])


def _seq(cin, cout, count, se, first_stride=1, widen_last=False):
    if widen_last:
        mods = [Block(cin, cin, se=se) for _ in range(count - 1)] + [Block(cin, cout, se=se)]
    else:
        mods = [Block(cin, cout, first_stride, se=se)] + [Block(cout, cout, se=se) for _ in range(count - 1)]
    return nn.Sequential(*mods)


class HG(nn.Module):
    def __init__(self, n, inplanes, layer_nums, se):
        super().__init__()
        cur, nxt, cn, nn_ = inplanes[0], inplanes[1], layer_nums[0], layer_nums[1]
        self.up1 = _seq(cur, cur, cn, se)
        self.max1 = nn.Sequential()
        self.low1 = _seq(cur, nxt, cn, se, first_stride=2)
        self.low2 = HG(n - 1, inplanes[1:], layer_nums[1:], se) if n > 1 else _seq(nxt, nxt, nn_, se)
        self.low3 = _seq(nxt, cur, cn, se, widen_last=True)
        self.up2 = nn.Upsample(scale_factor=2)

    def forward(self, x):
        up1 = self.up1(x)
        up2 = self.up2(self.low3(self.low2(self.low1(x))))
        return up1 + F.interpolate(up2, size=up1.shape[2:], mode="bilinear", align_corners=True)


class Net(nn.Module):
    """variant 'dense' | 'se' | 'plain' (the hourglass itself: the key lists of 'dense' are its)."""

    def __init__(self, variant, num_stacks=2, n=5, inplanes=HG104["inplanes"], layer_nums=HG104["layer_nums"], stem=128,
                 num_feats=256):
        super().__init__()
        se = variant == "se"
        self.variant, self.num_stacks = variant, num_stacks
        inplanes, layer_nums = list(inplanes), list(layer_nums)
        pre = [nn.Conv2d(3, stem, 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(stem), _ReLU(),
               Block(stem, 2 * stem, 1 if se else 2, se=se)]
        pre[2].bn = [pre[1]]
        self.pre_layer = nn.Sequential(*(pre + ([nn.MaxPool2d(2)] if se else [])))
        c0 = inplanes[0]
        self.hgs = nn.ModuleList([HG(n, inplanes, layer_nums, se) for _ in range(num_stacks)])
        self.convs = nn.ModuleList([CBR(3, c0, num_feats, relu=se) for _ in range(num_stacks)])
        self.residual = nn.ModuleList([Block(c0, c0, se=se) for _ in range(num_stacks - 1)])
        self.inter_ = nn.ModuleList([nn.Sequential(nn.Conv2d(c0, c0, 1, bias=False), nn.BatchNorm2d(c0)) for _ in range(num_stacks - 1)])
        self.conv_ = nn.ModuleList([nn.Sequential(nn.Conv2d(num_feats, c0, 1, bias=False), nn.BatchNorm2d(c0))
                                    for _ in range(num_stacks - 1)])

    def forward(self, x):
        pre = self.pre_layer(x)
        outs, skips = [], [pre]
        for i in range(self.num_stacks):
            feat = self.convs[i](self.hgs[i](pre))
            if self.variant == "dense":
                for s in skips:
                    feat = feat + s
                skips.append(feat)
            outs.append(feat)
            if i < self.num_stacks - 1:
                act = feat if self.variant == "se" else relu(feat, self.convs[i].bn)
                pre = self.residual[i](relu(self.inter_[i](pre) + self.conv_[i](act), self.inter_[i][1]))
        return outs


def tiny_net(variant, num_stacks):
    return Net(variant, num_stacks, **(DENSE_TINY if variant == "dense" else HG_TINY))


def full_momentum(net):
    """BatchNorm momentum 1 on every layer: after one train-mode pass the running statistics ARE that batch's, so the eval-mode
    pass that follows is normalised (features of O(1)) instead of running on the initial (0, 1)."""
    for m in net.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.momentum = 1.0
    return net


def key_shapes(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


# ----------------------------------------------------------------------------------------------------------------------
# golden records: what tools/gen_golden_hgvariants.py stores of a module run, and the same of a restatement
# ----------------------------------------------------------------------------------------------------------------------
BLOCK_CASES = {           # SE residual blocks: (inplanes, planes, stride), input shape
    "se_id": ((16, 16, 1), (2, 16, 12, 10)),
    "se_proj": ((8, 16, 1), (2, 8, 9, 11)),
    "se_s2_odd": ((8, 16, 2), (2, 8, 13, 11)),
}
NET_CASES = {             # tiny networks on 64x96: variant, stacks, batch
    "dense2": ("dense", 2, 1),
    "dense3": ("dense", 3, 1),              # the third stack is the only one with more than one earlier feature (sum_n)
    "se2": ("se", 2, 1),
}
NET_HW = (64, 96)
NET_CH_STRIDE = 64        # the networks' outputs are recorded at every 64th channel, ...
NET_PX_STRIDE = 4         # ... the input gradient at every 4th pixel of every 4th row,
NET_FULL_GRAD = ".se.fc."  # ... the SE weights' gradients whole, every parameter gradient as (sum, sum of squares)


def det_input(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).normal(0, 1, shape)).double()


def run_module(mod, x, gy_seed, train):
    """mod (float64) in train / eval mode on x, backward under a fixed upstream gradient per output
    -> (outputs, upstream gradients, dx, {name: grad})."""
    mod.train(train)
    mod.zero_grad()
    x = x.clone().requires_grad_()
    outs = mod(x)
    outs = list(outs) if isinstance(outs, (list, tuple)) else [outs]
    gys = [det_input(tuple(o.shape), gy_seed + i) for i, o in enumerate(outs)]
    torch.autograd.backward(outs, gys)
    return [o.detach() for o in outs], gys, x.grad.detach(), {k: p.grad.detach().clone() for k, p in mod.named_parameters()}


def block_record(tag, mod, x):
    """Whole tensors: train outputs and all gradients, eval outputs."""
    d = {}
    outs, _gys, gx, grads = run_module(mod, x, 44, True)
    d[tag + "/train/y"], d[tag + "/train/gx"] = outs[0], gx
    for k, g in grads.items():
        d[tag + "/train/grad/" + k] = g
    for k, b in mod.named_buffers():
        if b.is_floating_point():
            d[tag + "/train/buf/" + k] = b.detach().clone()
    with torch.no_grad():
        mod.eval()
        d[tag + "/eval/y"] = mod(x).detach()
    return {k: v.numpy() for k, v in d.items()}


def net_record(tag, mod, x):
    """The compact record of a tiny network (a whole one would be tens of MB): see NET_* above."""
    d = {}
    outs, _gys, gx, grads = run_module(mod, x, 77, True)
    for i, o in enumerate(outs):
        d["%s/train/y%d" % (tag, i)] = o[:, ::NET_CH_STRIDE]
    d[tag + "/train/gx"] = gx[:, :, ::NET_PX_STRIDE, ::NET_PX_STRIDE]
    keys = sorted(grads)
    d[tag + "/train/grad_sums"] = torch.stack([torch.stack([grads[k].sum(), (grads[k] ** 2).sum()]) for k in keys])
    for k in keys:
        if NET_FULL_GRAD in k:
            d[tag + "/train/grad/" + k] = grads[k]
    with torch.no_grad():
        mod.eval()
        for i, o in enumerate(mod(x)):
            d["%s/eval/y%d" % (tag, i)] = o[:, ::NET_CH_STRIDE]
    return {k: v.numpy() for k, v in d.items()}


# ----------------------------------------------------------------------------------------------------------------------
# kernel-level: squeeze, excite, scale + residual + ReLU
# ----------------------------------------------------------------------------------------------------------------------
SE_HW = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 300: (15, 20)}   # 300 rows: chunks of 128, 128 and 44 (the last
#                                                    one ends in the middle of a pass for every lane layout: 44 = 32 + 12 = 2 * 21 + 2)
SE_CR = [(4, 4), (32, 4), (32, 16), (48, 16), (256, 16), (512, 16)]       # (C, r): hidden widths 1, 8, 2, 3, 16, 32
SE_CASES = {"n%d_hw%d_c%d_r%d" % (n, hw, c, r): (n, SE_HW[hw], c, r, "plain")
            for n in (1, 3) for hw in SE_HW for (c, r) in SE_CR}
SE_CASES["empty_mask"] = (3, (8, 8), 32, 16, "empty")          # sample 1: u and skip negative everywhere, nothing passes the ReLU
SE_CASES["dskip_into"] = (3, (5, 13), 48, 16, "into")           # d skip added into a pre-filled target
MASK_MARGIN = 1e-3        # no pre-activation of a case lies nearer to 0: float32 cannot decide it otherwise than float64


def se_case(name):
    """-> dict of float64 CPU tensors u, skip, dout [n,c,h,w], w1 [c/r,c], w2 [c,c/r], into [n,c,h,w] | None."""
    import zlib
    n, (h, w), c, r, kind = SE_CASES[name]
    rng = np.random.default_rng([5, zlib.crc32(name.encode())])
    t = lambda *s: torch.from_numpy(rng.normal(0, 1, s)).float().double()         # float32-representable values
    u, skip, dout = t(n, c, h, w), t(n, c, h, w), t(n, c, h, w)
    w1 = t(c // r, c) / np.sqrt(c)
    w2 = t(c, c // r) / np.sqrt(max(c // r, 1))
    w1, w2 = w1.float().double(), w2.float().double()
    if kind == "empty":
        u[1], skip[1] = -u[1].abs() - 0.5, -skip[1].abs() - 0.5
    # keep every pre-activation MASK_MARGIN away from 0 (the squeeze's mean, hence s, does not depend on skip)
    for _ in range(2):
        pre = _se_forward(u, w1, w2, skip)[4]
        skip = torch.where(pre.abs() < 2 * MASK_MARGIN, skip + (0.01 if kind != "empty" else -0.01), skip).float().double()
    into = t(n, c, h, w) if kind == "into" else None
    return dict(u=u, skip=skip, dout=dout, w1=w1, w2=w2, into=into)


def _se_forward(u, w1, w2, skip):
    m = u.mean((2, 3))
    z1 = m @ w1.t()
    h = torch.relu(z1)
    s = torch.sigmoid(h @ w2.t())
    pre = u * s[:, :, None, None] + skip
    return m, h, s, z1, pre


def se_reference(case, dtype):
    """The node in plain torch at `dtype` -> dict of float64 numpy arrays: m, h, s, out, mask (bool), du, dskip, dw1, dw2, dm
    (the gradient of the mean), hmask (the hidden ReLU's)."""
    u, skip, w1, w2 = (case[k].to(dtype).clone().requires_grad_() for k in ("u", "skip", "w1", "w2"))
    m, h, s, z1, pre = _se_forward(u, w1, w2, skip)
    m.retain_grad()
    out = torch.relu(pre)
    out.backward(case["dout"].to(dtype))
    dskip = skip.grad if case["into"] is None else case["into"].to(dtype) + skip.grad
    res = dict(m=m, h=h, s=s, out=out, du=u.grad, dskip=dskip, dw1=w1.grad, dw2=w2.grad, dm=m.grad)
    res = {k: v.detach().double().numpy() for k, v in res.items()}
    res["mask"] = pre.detach().numpy() > 0
    res["hmask"] = z1.detach().numpy() > 0
    res["pre"] = pre.detach().double().numpy()
    return res


# ----------------------------------------------------------------------------------------------------------------------
# MaxPool2d(2)
# ----------------------------------------------------------------------------------------------------------------------
POOL_SIZES = [(1, 1), (2, 2), (5, 7), (8, 8), (9, 4)]
POOL_CHANNELS = [4, 48]


def pool_case(h, w, c, nan=True):
    """[2, c, h, w] float32: values from a small set (so windows tie often), planted all-equal windows, one NaN."""
    rng = np.random.default_rng([9, h, w, c])
    x = rng.integers(-3, 4, (2, c, h, w)).astype(np.float32) * 0.5
    if h >= 2 and w >= 2:
        x[0, :, 0:2, 0:2] = 1.25                                  # a four-way tie: the first tap wins
        x[1, 0, (h // 2) * 2 - 1, (w // 2) * 2 - 2] = 9.0          # last window, tap 2 ...
        x[1, 0, (h // 2) * 2 - 1, (w // 2) * 2 - 1] = 9.0          # ... ties with tap 3: tap 2 wins
        if nan:
            x[1, c - 1, 1, 0] = np.nan                            # a NaN wins its window
    return torch.from_numpy(x)


def pool_reference(x):
    """x [n,c,h,w] (any float dtype, CPU) -> (y, tap uint8 = ky * 2 + kx of the first maximum; a NaN wins, the last NaN of a window
    keeps the tap — ATen's update rule `v > max or isnan(v)`)."""
    n, c, h, w = x.shape
    oh, ow = h // 2, w // 2
    taps = [x[:, :, ky:2 * oh:2, kx:2 * ow:2] for ky in (0, 1) for kx in (0, 1)]
    y, tap = taps[0].clone(), torch.zeros(taps[0].shape, dtype=torch.uint8)
    for k in (1, 2, 3):
        upd = (taps[k] > y) | torch.isnan(taps[k])
        y = torch.where(upd, taps[k], y)
        tap = torch.where(upd, torch.full_like(tap, k), tap)
    return y, tap


def pool_backward_reference(dy, tap, h, w):
    n, c, oh, ow = dy.shape
    dx = torch.zeros((n, c, h, w), dtype=dy.dtype)
    for k in range(4):
        ky, kx = k >> 1, k & 1
        dx[:, :, ky:2 * oh:2, kx:2 * ow:2] = torch.where(tap == k, dy, torch.zeros_like(dy))
    return dx


# ----------------------------------------------------------------------------------------------------------------------
# tolerance rule of tests/test_retina_gpu.py
# ----------------------------------------------------------------------------------------------------------------------
def measured_tol(err32, ref):
    return max(4.0 * float(err32), 2.0 * U32 * float(np.abs(ref).max(initial=0.0)))


def judge(tag, got, ref64, ref32):
    got, ref64, ref32 = (np.asarray(a, dtype=np.float64) for a in (got, ref64, ref32))
    err32 = float(np.abs(ref32 - ref64).max(initial=0.0))
    tol = measured_tol(err32, ref64)
    err = float(np.abs(got - ref64).max(initial=0.0))
    print("  %-22s n=%-8d max|ref| %.3g  fp32 err %.3g  kernel err %.3g  tol %.3g"
          % (tag, got.size, float(np.abs(ref64).max(initial=0.0)), err32, err, tol))
    assert err <= tol, (tag, err, tol)

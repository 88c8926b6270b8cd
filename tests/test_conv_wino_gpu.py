"""GPU: the Winograd F(2x2,3x3) route (rrnet_amd/csrc/conv_wino.hip, include/rrnet_hip_wino.h) against float64, called through
its entry points BELOW the gate's pixel floor, at the smallest shapes that can break its kernels: odd maps (ragged tiles), an
image boundary inside a GEMM tile, channel counts that are no multiple of the K-step or of the GEMM tile, fewer tiles than a
GEMM tile, a map thinner than a Winograd tile.

Acceptance rule: the project's (helpers.conv_error_ratios / conv_accepts): max-abs and RMS error at 4096 seeded outputs, and
the RMS error over the whole tensor, as ratios to the error of a chained float32 sum of the same float32-rounded products, at
most CONV_MARGIN.  Every test prints its ratios (profiles/conv_wino_fp64_ratios.txt is one run's output).

What the route does NOT promise, and the direct route does: exact cancellation, the sign of zeros, and a non-finite
value staying within one tap of where it was — it reaches every output of the 2x2 tiles whose 4x4 window holds it."""
import functools

import numpy as np
import pytest
import torch

from helpers import (CONV_MARGIN, U32, conv_accepts, conv_bias_clear_of_zero, conv_error_ratios, conv_ref64, conv_sample_positions,
                     conv_tap_counts, conv_terms, conv_yardstick)

pytestmark = pytest.mark.gpu

# (n, c, h, w, k)
CASES = [(1, 128, 9, 13, 128),      # odd P and Q: ragged last tile row and column
         (2, 64, 8, 8, 132),        # the image boundary inside a GEMM tile (32 tiles of 128 rows); a ragged filter tile
         (1, 44, 12, 12, 40),       # C no multiple of the K-step, K below the narrow GEMM tile
         (1, 256, 16, 16, 256),
         (3, 64, 2, 2, 64),         # fewer tiles than a GEMM tile
         (3, 64, 1, 5, 64)]         # a map thinner than a Winograd tile
IDS = ["n%dc%dh%dw%dk%d" % c for c in CASES]
SENTINEL = -7.25e300
SLAB_CHAIN = 32                     # values per fp32 chain of wino_output_kernel (8 tiles x 4 pixels), double from there


def _dev(a):
    from rrnet_amd import ops
    return ops.to_nhwc(torch.as_tensor(a).float().cuda())


def _host(t):
    return t.detach().cpu().double()


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs (float32, CPU) and the float64 reference of case i: computed once, shared by its tests, never modified."""
    n, c, h, w, k = CASES[i]
    rng = np.random.default_rng(5000 + i)
    x = torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))
    wt = torch.from_numpy((rng.standard_normal((k, c, 3, 3)) / np.sqrt(9 * c)).astype(np.float32))
    gy = torch.from_numpy(rng.standard_normal((n, k, h, w)).astype(np.float32))
    y, dx, _ = conv_ref64(x, wt, None, 1, (1, 1), False, gy)
    return dict(x=x, w=wt, gy=gy, y=y, dx=dx)


def _filter(wd, flipped=False):
    """U of the device filter wd [K,C,3,3] (OHWI memory) through rr_wino_filter; flipped: of rr_weight_flip_transpose's copy."""
    from rrnet_amd import ops
    return ops._wino_filter(wd, flipped)


def _fprop(xd, u, n, h, w, c, k, bias=None, relu=False, out=None, accumulate=False, slab=None):
    """rr_conv_wino_fprop on x [n,c,h,w] (NHWC memory) -> y [n,k,h,w]."""
    from rrnet_amd import ops
    y = ops.empty_nhwc(n, k, h, w, xd.device) if out is None else out
    ws = ops._wino_ws(xd.device, n, h, w, c, k)
    ops._WINO.call("rr_conv_wino_fprop", xd, u, bias, y, slab, ws, ws.numel() * 4, n, h, w, c, k, int(relu), int(accumulate))
    return y


def _judge(tag, got, ref_all, idx, ref_s, max_seq, rms_seq, keep=None, margin=None):
    got, ref_all = got.numpy(), ref_all.numpy()
    assert np.abs(ref_s - ref_all[idx]).max() <= 1e-11 * max(np.abs(ref_s).max(), 1e-30), tag
    ga, ra = (got, ref_all) if keep is None else (got[keep], ref_all[keep])
    ratios = conv_error_ratios(got[idx], ref_s, max_seq, rms_seq, ga, ra)
    print("wino %s: max %.2f rms %.2f whole-tensor rms %.2f of the chained-fp32 yardstick (max %.2e rms %.2e), margin %g"
          % ((tag,) + ratios + (max_seq, rms_seq, CONV_MARGIN if margin is None else margin)))
    assert conv_accepts(ratios, margin), (tag, ratios)
    return ratios


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fprop_against_fp64(i):
    n, c, h, w, k = CASES[i]
    cs = _case(i)
    idx = conv_sample_positions((n, k, h, w), 11 * i + 1)
    yard = conv_yardstick(conv_terms("fprop", idx, cs["x"], cs["w"], None, 1, (1, 1)))
    y = _fprop(_dev(cs["x"]), _filter(_dev(cs["w"])), n, h, w, c, k)
    _judge("fprop %s" % IDS[i], _host(y), cs["y"], idx, *yard)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_dgrad_against_fp64_plain_and_accumulating(i):
    """The data gradient = the route on dy with the transform of the flipped / transposed filter (ops._dgrad_wino), plain and
    adding into a non-zero tensor (the starting value is the head column of the yardstick)."""
    from rrnet_amd import ops
    n, c, h, w, k = CASES[i]
    cs = _case(i)
    rng = np.random.default_rng(6000 + i)
    base = torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))
    idx = conv_sample_positions((n, c, h, w), 11 * i + 2)
    yard = conv_yardstick(conv_terms("dgrad", idx, None, cs["w"], cs["gy"], 1, (1, 1)), head=base.double().numpy()[idx])
    gyd, wd = _dev(cs["gy"]), _dev(cs["w"])
    dx = ops.empty_nhwc(n, c, h, w, "cuda")
    ops._dgrad_wino(gyd, wd, dx, (n, h, w, c, k, 3, 3, 1, 1, 0), 0.0, None)
    _judge("dgrad %s" % IDS[i], _host(dx), cs["dx"], idx, *yard[:3])
    acc = _dev(base).clone(memory_format=torch.channels_last)
    ops._dgrad_wino(gyd, wd, acc, (n, h, w, c, k, 3, 3, 1, 1, 1), 0.0, None)
    _judge("dgrad %s accumulate" % IDS[i], _host(acc), cs["dx"] + base.double(), idx, *yard[3:])


# ------------------------------------------------------------------------------------------------------------------
# epilogues
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1], ids=IDS[:2])
def test_bias_relu_and_statistics_slab(i):
    """bias + ReLU with the bias moved clear of zero (float32 and float64 agree on every mask bit), and the slab: every row
    written, the rows' sum against the float64 column sums of the kernel's OWN y.  Bound from the chains built: SLAB_CHAIN values
    per float32 chain, double from there: (SLAB_CHAIN + 1) u sum|y| and (SLAB_CHAIN + 2) u sum y^2 (+ the square's rounding)."""
    from rrnet_amd import _C
    n, c, h, w, k = CASES[i]
    cs = _case(i)
    rng = np.random.default_rng(7000 + i)
    b = conv_bias_clear_of_zero(cs["y"].numpy(), rng.standard_normal(k).astype(np.float32))
    ref = torch.relu(cs["y"] + torch.from_numpy(b).double().view(1, -1, 1, 1))
    idx = conv_sample_positions((n, k, h, w), 11 * i + 3)
    yard = conv_yardstick(conv_terms("fprop", idx, cs["x"], cs["w"], None, 1, (1, 1), bias=torch.from_numpy(b)), relu=True)
    nb = _C.call("rr_conv_stat_slab_bytes", n, h, w, k)
    slab = torch.full((nb // 8,), SENTINEL, dtype=torch.float64, device="cuda")
    y = _fprop(_dev(cs["x"]), _filter(_dev(cs["w"])), n, h, w, c, k, bias=torch.from_numpy(b).cuda(), relu=True, slab=slab)
    _judge("fprop %s bias relu" % IDS[i], _host(y), ref, idx, *yard)
    assert bool(((_host(y) > 0) == (ref > 0)).all())
    rows = slab.view(-1, 2, k)
    assert rows.shape[0] == -(-n * h * w // 128) and bool((rows != SENTINEL).all())
    yd = _host(y).permute(0, 2, 3, 1).reshape(-1, k)
    s1, s2, a1 = yd.sum(0), (yd * yd).sum(0), yd.abs().sum(0)
    got = rows.sum(0).cpu()
    b1, b2 = (SLAB_CHAIN + 1) * U32 * a1, (SLAB_CHAIN + 2) * U32 * s2
    e1, e2 = (got[0] - s1).abs(), (got[1] - s2).abs()
    print("wino slab %s (%d rows): error over bound: sum y %.3f, sum y^2 %.3f"
          % (IDS[i], rows.shape[0], float((e1 / (b1 + 1e-300)).max()), float((e2 / (b2 + 1e-300)).max())))
    assert bool((e1 <= b1).all()) and bool((e2 <= b2).all())


@pytest.mark.parametrize("acc", [False, True], ids=["plain", "accumulate"])
@pytest.mark.parametrize("mask", ["z", "scale"])
def test_link_sums_against_bn_bwd_reduce(mask, acc):
    """rr_conv_wino_dgrad_bnsum, with and without z, with and without accumulate: dx is bit-equal to the plain route's (same
    arithmetic, same stores), and the sums agree with rr_bn_bwd_reduce run on the stored gradient: each within its own bound
    against the float64 sums of that gradient — rr_bn_bwd_reduce's (tests/test_syncbn_gpu.py: float32 partials over 8 pixels: 9 u
    sum|d| and 12 u sum|d xhat| + 2 u |mean| invstd sum|d|), this kernel's the same form for chains of SLAB_CHAIN values."""
    from rrnet_amd import ops
    n, c, h, w, k = 2, 64, 9, 13, 132          # (c: dx's channels = the producer's)
    g = torch.Generator().manual_seed(31 + (mask == "z") + 2 * acc)
    dy = _dev(torch.randn(n, k, h, w, generator=g))
    wd = _dev(torch.randn(k, c, 3, 3, generator=g) / np.sqrt(9 * k))
    y = _dev(torch.randn(n, c, h, w, generator=g))
    res = _dev(torch.randn(n, c, h, w, generator=g))
    mean, var = (torch.randn(c, generator=g) * 0.1).cuda(), (torch.rand(c, generator=g) + 0.5).cuda()
    invstd = 1.0 / torch.sqrt(var)
    scale, shift = (torch.rand(c, generator=g).cuda() + 0.5) * invstd, torch.randn(c, generator=g).cuda() * 0.3
    link = ops.BnLink()
    link.y, link.mean, link.invstd = y, mean, invstd
    z = None
    if mask == "z":
        link.use_z = True
        z = torch.relu(y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) + res).contiguous(memory_format=torch.channels_last)
    else:
        link.msc, link.msh = scale, shift
    base = _dev(torch.randn(n, c, h, w, generator=g))
    geo = (n, h, w, c, k, 3, 3, 1, 1, int(acc))
    dx_plain = base.clone(memory_format=torch.channels_last)
    ops._dgrad_wino(dy, wd, dx_plain, geo, 0.0, None)
    dx = base.clone(memory_format=torch.channels_last)
    ops._dgrad_wino(dy, wd, dx, geo, 0.0, None, link, z)
    assert link.dz is dx and torch.equal(dx, dx_plain)
    ref = ops.bn_bwd_reduce(dx, z, y, mean, invstd, mask_scale=link.msc, mask_shift=link.msh)
    d = dx.double()
    d = d * ((z > 0) if mask == "z" else (torch.addcmul(shift.view(1, -1, 1, 1), y, scale.view(1, -1, 1, 1)) > 0))
    xh = (y.double() - mean.double().view(1, -1, 1, 1)) * invstd.double().view(1, -1, 1, 1)
    exp = torch.cat([d.sum((0, 2, 3)), (d * xh).sum((0, 2, 3))])
    a1, a2 = d.abs().sum((0, 2, 3)), (d * xh).abs().sum((0, 2, 3))
    lead = 2 * U32 * mean.double().abs() * invstd.double() * a1

    def over(got, chain):
        bound = torch.cat([(chain + 1) * U32 * a1, (chain + 4) * U32 * a2 + lead])
        return float(((got[:2 * c] - exp).abs() / bound.clamp_min(1e-300)).max())
    mine, theirs = over(link.sums, SLAB_CHAIN), over(ref, 8)
    print("wino link sums mask=%s acc=%d: error over bound %.3f (rr_bn_bwd_reduce on the stored gradient: %.3f)" % (mask, acc, mine, theirs))
    assert mine <= 1.0 and theirs <= 1.0


# ------------------------------------------------------------------------------------------------------------------
# inputs where convolution kernels go wrong
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 2, 5], ids=[IDS[0], IDS[2], IDS[5]])
def test_all_ones_count_the_taps(i):
    """x = w = 1: y = C x (taps of the pixel inside the image), bit for bit — the transforms are exact on small integers (G's
    halves give multiples of 1/4), so an off-by-one at a border or in a ragged tile changes a count."""
    n, c, h, w, k = CASES[i]
    in_h, reach_h, _ = conv_tap_counts(h, h, 3, 1, 1)
    in_w, reach_w, _ = conv_tap_counts(w, w, 3, 1, 1)
    y = _fprop(_dev(torch.ones(n, c, h, w)), _filter(_dev(torch.ones(k, c, 3, 3))), n, h, w, c, k)
    want = torch.from_numpy(c * np.outer(in_h, in_w)).double().expand(n, k, h, w)
    assert torch.equal(_host(y), want), float((_host(y) - want).abs().max())
    dx = _fprop(_dev(torch.ones(n, k, h, w)), _filter(_dev(torch.ones(k, c, 3, 3)), True), n, h, w, k, c)
    want = torch.from_numpy(k * np.outer(reach_h, reach_w)).double().expand(n, c, h, w)
    assert torch.equal(_host(dx), want), float((_host(dx) - want).abs().max())


def test_non_finite_inputs_reach_their_tiles_and_nothing_else():
    """One NaN and one +inf in x: non-finite at least at every output the element reaches through a tap, finite everywhere outside
    the 2x2 tiles whose 4x4 window holds it (the route's contract: up to two pixels further than a tap), finite in every other
    image; the finite outputs still meet the bound."""
    n, c, h, w, k = 3, 64, 9, 13, 64
    rng = np.random.default_rng(44)
    x = torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))
    wt = torch.from_numpy((rng.standard_normal((k, c, 3, 3)) / np.sqrt(9 * c)).astype(np.float32))
    pos = [(0, 5, 4, 7), (2, c - 3, 8, 0)]         # an interior pixel; the ragged last row at the left border
    xbad = x.clone()
    xbad[pos[0]], xbad[pos[1]] = float("nan"), float("inf")
    must = torch.zeros(n, 1, h, w, dtype=torch.bool)
    may = torch.zeros(n, 1, h, w, dtype=torch.bool)
    for (nn_, _, ph, pw) in pos:
        must[nn_, 0, max(ph - 1, 0):ph + 2, max(pw - 1, 0):pw + 2] = True
        for th in range((h + 1) // 2):
            for tw in range((w + 1) // 2):
                if 2 * th - 1 <= ph <= 2 * th + 2 and 2 * tw - 1 <= pw <= 2 * tw + 2:
                    may[nn_, 0, 2 * th:2 * th + 2, 2 * tw:2 * tw + 2] = True
    assert bool((must <= may).all()) and not bool(may[1].any()) and int(may.sum()) > int(must.sum())
    y = _host(_fprop(_dev(xbad), _filter(_dev(wt)), n, h, w, c, k))
    bad = ~torch.isfinite(y)
    assert bool((must.expand_as(bad) <= bad).all()), "a non-finite input is invisible at an output it reaches"
    assert bool((bad <= may.expand_as(bad)).all()), "a non-finite value outside the tiles whose window holds it"
    xz = x.clone()
    xz[pos[0]] = xz[pos[1]] = 0.0
    ref = conv_ref64(xz, wt, None, 1, (1, 1), False)[0]
    keep = (~may.expand_as(bad)).numpy()
    idx = conv_sample_positions((n, k, h, w), 45, keep=keep)
    yard = conv_yardstick(conv_terms("fprop", idx, xz, wt, None, 1, (1, 1)))
    hit = may.expand_as(bad)
    _judge("non-finite (%d non-finite, %d allowed)" % (int(bad.sum()), int(hit.sum())), torch.where(hit, torch.zeros_like(y), y), ref * (~hit),
           idx, *yard, keep=keep)


def test_per_pixel_scales_of_two_to_the_plus_minus_ten():
    """Every pixel of x scaled by its own 2^e, e in [-10, 10] (a pixel-to-pixel dynamic range of 2^20): the window transform adds
    pixels of different scales before the multiplication.  Same rule, same margin."""
    n, c, h, w, k = 1, 128, 9, 13, 128
    rng = np.random.default_rng(46)
    x = rng.standard_normal((n, c, h, w)) * np.ldexp(1.0, rng.integers(-10, 11, (n, 1, h, w)))
    x = torch.from_numpy(x.astype(np.float32))
    wt = torch.from_numpy((rng.standard_normal((k, c, 3, 3)) / np.sqrt(9 * c)).astype(np.float32))
    ref = conv_ref64(x, wt, None, 1, (1, 1), False)[0]
    idx = conv_sample_positions((n, k, h, w), 47)
    yard = conv_yardstick(conv_terms("fprop", idx, x, wt, None, 1, (1, 1)))
    y = _fprop(_dev(x), _filter(_dev(wt)), n, h, w, c, k)
    _judge("per-pixel scales 2^+-10", _host(y), ref, idx, *yard)


# ------------------------------------------------------------------------------------------------------------------
# one residual block, the route on and off
# ------------------------------------------------------------------------------------------------------------------
def _block_run(sd, x, gy, route_on):
    from rrnet_amd import ops
    from rrnet_amd.backbones.hourglass import ResidualBlock
    saved = ops._CONV_WINO, ops._WINO_BELOW_FLOOR
    ops._CONV_WINO = ops._WINO_BELOW_FLOOR = route_on
    try:
        mod = ResidualBlock(128, 128, 1)
        mod.load_state_dict(sd)
        mod = mod.cuda().to(memory_format=torch.channels_last).train()
        xd = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
        with ops.bf16_scope(0, force=True):
            y = mod(xd)
            y.backward(gy.cuda().contiguous(memory_format=torch.channels_last))
        torch.cuda.synchronize()
        out = {"y": y, "dx": xd.grad}
        out.update({"grad/" + kk: p.grad for kk, p in mod.named_parameters() if ".bn" in "." + kk})
        return {kk: v.detach().cpu().double() for kk, v in out.items()}
    finally:
        ops._CONV_WINO, ops._WINO_BELOW_FLOOR = saved


def test_residual_block_with_the_route_on_and_off():
    """ResidualBlock(128, 128) on 2 x 64 x 64, forward and backward (8192 output pixels: below the gate's measured floor, which
    tests/golden/conv_bwd_routes.json holds above this very shape — the arm with the route on runs under ops._WINO_BELOW_FLOOR, so
    both 3x3 layers and both data gradients take it), against oracle/model.py's block in float64.  Output, dx and the BatchNorm sums (dgamma, dbeta of bn1 / bn2):
    |on - off| <= |on - fp64| + |off - fp64| (which also says that neither arm holds a non-finite value), and the route's own
    distance to float64 stays within 4x the direct route's, in RMS — DESIGN 25 measures about 2x its rounding error at a
    convolution, which BatchNorm scales like the direct arm's.  Two runs with the route on: dx and the BatchNorm sums bit-equal
    (the weight gradients are float atomics on both routes)."""
    from oracle import model as om
    from rrnet_amd import ops
    from rrnet_amd.backbones.hourglass import ResidualBlock
    torch.manual_seed(77)
    sd = {kk: v.clone() for kk, v in ResidualBlock(128, 128, 1).state_dict().items()}
    for kk in sd:
        if kk.endswith("bn1.weight") or kk.endswith("bn2.weight"):
            sd[kk] = torch.rand_like(sd[kk]) + 0.5
        elif kk.endswith("bn1.bias") or kk.endswith("bn2.bias"):
            sd[kk] = torch.randn_like(sd[kk]) * 0.3
    x, gy = torch.randn(2, 128, 64, 64), torch.randn(2, 128, 64, 64)
    assert not ops.wino_takes(2, 64, 64, 128, 128, 3, 3, 1, (1, 1), stats=True)
    ops._WINO_BELOW_FLOOR = True
    try:
        assert ops.wino_takes(2, 64, 64, 128, 128, 3, 3, 1, (1, 1), stats=True) and ops.wino_takes(2, 64, 64, 128, 128, 3, 3, 1, (1, 1), link=True)
    finally:
        ops._WINO_BELOW_FLOOR = False
    stat = ("running_mean", "running_var", "num_batches_tracked")
    P = om.Params({"m." + kk: (v.clone() if kk.endswith(stat[2]) else v.double().clone().requires_grad_(not kk.endswith(stat)))
                   for kk, v in sd.items()}, training=True)
    x64 = x.double().requires_grad_()
    y64 = om.residual_block(P, "m", x64, 1)
    y64.backward(gy.double())
    ref = {"y": y64.detach(), "dx": x64.grad}
    ref.update({"grad/" + kk: P.sd["m." + kk].grad for kk in sd if ".bn" in "." + kk and not kk.endswith(stat)})
    on, off, again = _block_run(sd, x, gy, True), _block_run(sd, x, gy, False), _block_run(sd, x, gy, True)
    assert set(on) == set(ref) and len(ref) == 6
    for kk in sorted(ref):
        d_on, d_off, d = (on[kk] - ref[kk]).abs(), (off[kk] - ref[kk]).abs(), (on[kk] - off[kk]).abs()
        r_on, r_off = float(d_on.pow(2).mean().sqrt()), float(d_off.pow(2).mean().sqrt())
        print("wino block %s: rms distance to fp64: route on %.3e, off %.3e (ratio %.2f); max |on - off| %.3e"
              % (kk, r_on, r_off, r_on / max(r_off, 1e-300), float(d.max())))
        assert bool((d <= d_on + d_off).all()), kk
        assert r_on <= 4.0 * r_off, (kk, r_on, r_off)
        assert torch.equal(on[kk], again[kk]), kk
    assert float((on["y"] - off["y"]).abs().max()) > 0.0          # the two arms really ran different arithmetic

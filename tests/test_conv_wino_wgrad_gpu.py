"""GPU: the Winograd F(3x3,2x2) weight gradient (rr_conv_wino_wgrad: rrnet_amd/csrc/conv_wino.hip, the batch mode of
conv_wgrad_kernel in csrc/conv.hip, include/rrnet_hip_wino.h) against float64, through its entry point and through
ops.conv_wgrad BELOW the gate's pixel floor, at the smallest shapes at which each part can break.

Acceptance rule: the project's (helpers.conv_error_ratios / conv_accepts): max-abs and RMS error at 4096 seeded outputs and the
RMS error over the whole tensor, as ratios to the error of a chained float32 sum of the same float32-rounded products, at most
CONV_MARGIN.  Every test prints its ratios (profiles/conv_wino_wgrad_fp64_ratios.txt is one run's output).

What the route does NOT promise, and the direct route does: exact cancellation, the sign of zeros, and a non-finite
value staying at the taps that reach it — inside its (filter, channel) pair it may reach all nine taps."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from helpers import (CONV_MARGIN, conv_accepts, conv_error_ratios, conv_ref64, conv_sample_positions, conv_tap_counts, conv_terms,
                     conv_yardstick)

pytestmark = pytest.mark.gpu

# (n, c, h, w, k)
CASES = [(1, 128, 9, 13, 128),      # odd map, ragged tiles, T = 35: a ragged K tail on PIPE 1
         (2, 64, 8, 8, 132),        # a ragged filter tile, the image boundary inside a K-step, T = 32
         (1, 44, 12, 12, 40),       # C and K no multiples of 32
         (1, 256, 16, 16, 256),     # 2 x 2 output tiles, T = 64: PIPE 3
         (3, 64, 2, 2, 64),         # fewer tiles than a K-step
         (3, 64, 1, 5, 64),         # a map thinner than a tile
         (2, 64, 32, 32, 64),       # T = 512: two splits on PIPE 3
         (2, 64, 34, 30, 64)]       # T = 510: two splits with a ragged tail on PIPE 1
IDS = ["n%dc%dh%dw%dk%d" % c for c in CASES]
# what rr_conv_wino_wgrad_plan must report for them: (PIPE of the GEMM kernel, splits of T)
GEMM = [(1, 1), (3, 1), (1, 1), (3, 1), (1, 1), (1, 1), (3, 2), (1, 2)]
SENTINEL = 0x7FC12345               # a NaN pattern no kernel produces


def _dev(a):
    from rrnet_amd import ops
    return ops.to_nhwc(torch.as_tensor(a).float().cuda())


def _host(t):
    return t.detach().cpu().double()


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs (float32, CPU) and the float64 weight gradient of case i: computed once, shared by its tests, never modified."""
    n, c, h, w, k = CASES[i]
    rng = np.random.default_rng(8000 + i)
    x = torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))
    gy = torch.from_numpy(rng.standard_normal((n, k, h, w)).astype(np.float32))
    return dict(x=x, gy=gy, dw=_ref_dw(x, gy, k, c))


def _ref_dw(x, gy, k, c):
    return conv_ref64(x, torch.zeros(k, c, 3, 3), None, 1, (1, 1), False, gy)[2]


def _plan(n, h, w, c, k, r=3, s=3, stride=1, pad=(1, 1), out=(0, 0), flags=0, math=0):
    from rrnet_amd import _C, ops
    plan = (_C.c_int * 10)()
    ops._WINO.call("rr_conv_wino_wgrad_plan", math, n, h, w, c, k, r, s, stride, pad[0], pad[1], out[0], out[1], flags, plan)
    return list(plan)


def _entry(xd, gyd, dw):
    """rr_conv_wino_wgrad on x [n,c,h,w], dy [n,k,h,w] (NHWC memory): dw [k,c,3,3] (OHWI memory) += the gradient."""
    from rrnet_amd import ops
    n, c, h, w = xd.shape
    k = gyd.shape[1]
    ws = ops._wino_ws(xd.device, n, h, w, c, k, "rr_conv_wino_wgrad_ws_bytes")
    ops._WINO.call("rr_conv_wino_wgrad", xd, gyd, dw, ws, ws.numel() * 4, n, h, w, c, k)
    return dw


@contextlib.contextmanager
def _route(on=True, below_floor=True):
    """ops.conv_wgrad in fp32 arithmetic with the route's switches set; yields the list of timer keys the calls launch under."""
    from rrnet_amd import ops
    keys = []

    class Timer:
        def launch(self, name, flops, fn, detail=None, nbytes=0.0):
            keys.append(name)
            return fn()
    saved = ops._CONV_WINO_WGRAD, ops._WINO_WGRAD_BELOW_FLOOR, ops.TIMER
    ops._CONV_WINO_WGRAD, ops._WINO_WGRAD_BELOW_FLOOR, ops.TIMER = on, below_floor, Timer()
    try:
        with ops.bf16_scope(0, force=True):
            yield keys
    finally:
        ops._CONV_WINO_WGRAD, ops._WINO_WGRAD_BELOW_FLOOR, ops.TIMER = saved


def _through_ops(xd, gyd, dw, side=False):
    from rrnet_amd import functional as RF, ops
    ran_on = []

    def launch():
        ran_on.append(torch.cuda.current_stream(xd.device).cuda_stream)
        ops.conv_wgrad(xd, gyd, dw, 1, (1, 1))
    with _route() as keys:
        if side:
            RF._wgrad_async(launch, xd.device, xd, gyd)
        else:
            launch()
    torch.cuda.synchronize()
    assert keys == ["conv_wgrad<wino>"], keys
    here = torch.cuda.current_stream(xd.device).cuda_stream
    assert (ran_on[0] != here) == side, "the side-stream arm must launch on another stream than the caller's (RR_WGRAD_STREAM on)"
    assert (xd.device, ran_on[0]) in ops._WINO_WS            # ... from that stream's own workspace block
    return dw


def _judge(tag, got, ref_all, idx, ref_s, max_seq, rms_seq, keep=None):
    got, ref_all = got.numpy(), ref_all.numpy()
    assert np.abs(ref_s - ref_all[idx]).max() <= 1e-11 * max(np.abs(ref_s).max(), 1e-30), tag
    ga, ra = (got, ref_all) if keep is None else (got[keep], ref_all[keep])
    ratios = conv_error_ratios(got[idx], ref_s, max_seq, rms_seq, ga, ra)
    print("wino wgrad %s: max %.2f rms %.2f whole-tensor rms %.2f of the chained-fp32 yardstick (max %.2e rms %.2e), margin %g"
          % ((tag,) + ratios + (max_seq, rms_seq, CONV_MARGIN)))
    assert conv_accepts(ratios), (tag, ratios)
    return ratios


# ------------------------------------------------------------------------------------------------------------------
# 1. against float64
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_wgrad_against_fp64(i):
    """Into a zeroed dw and adding into a non-zero one (the starting value is the head column of the yardstick), through the entry
    point, through ops.conv_wgrad on the current stream, and through ops.conv_wgrad inside functional._wgrad_async's side stream."""
    from rrnet_amd import ops
    n, c, h, w, k = CASES[i]
    cs = _case(i)
    pl = _plan(n, h, w, c, k)
    assert pl[:2] == [0, 1] and (pl[4], pl[5]) == GEMM[i], pl
    rng = np.random.default_rng(8100 + i)
    base = torch.from_numpy((rng.standard_normal((k, c, 3, 3)) * float(cs["dw"].std())).astype(np.float32))
    idx = conv_sample_positions((k, c, 3, 3), 13 * i + 1)
    yard = conv_yardstick(conv_terms("wgrad", idx, cs["x"], (3, 3), cs["gy"], 1, (1, 1)), head=base.double().numpy()[idx])
    xd, gyd = _dev(cs["x"]), _dev(cs["gy"])
    runs = (("entry point", _entry), ("ops.conv_wgrad", _through_ops), ("ops.conv_wgrad, side stream", lambda *a: _through_ops(*a, side=True)))
    for name, run in runs:
        dw = run(xd, gyd, ops.zeros_nhwc(k, c, 3, 3, "cuda"))
        _judge("%s %s" % (IDS[i], name), _host(dw), cs["dw"], idx, *yard[:3])
        dw = run(xd, gyd, _dev(base).clone(memory_format=torch.channels_last))
        _judge("%s %s into a non-zero dw" % (IDS[i], name), _host(dw), cs["dw"] + base.double(), idx, *yard[3:])


# ------------------------------------------------------------------------------------------------------------------
# 2. - 4. inputs where convolution kernels go wrong
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 2, 5, 7], ids=[IDS[0], IDS[2], IDS[5], IDS[7]])
def test_all_ones_count_the_pixels(i):
    """x = dy = 1: dw[ko][c][r][s] = the number of pixels whose tap (r, s) lies inside the map, bit for bit — the transforms are
    exact on small integers (G's halves give multiples of 1/4), so an off-by-one at a border or in a ragged tile changes a count."""
    from rrnet_amd import ops
    n, c, h, w, k = CASES[i]
    taps_h, taps_w = conv_tap_counts(h, h, 3, 1, 1)[2], conv_tap_counts(w, w, 3, 1, 1)[2]
    dw = _entry(_dev(torch.ones(n, c, h, w)), _dev(torch.ones(n, k, h, w)), ops.zeros_nhwc(k, c, 3, 3, "cuda"))
    want = torch.from_numpy(n * np.outer(taps_h, taps_w)).double().expand(k, c, 3, 3)
    assert torch.equal(_host(dw), want), float((_host(dw) - want).abs().max())


def test_non_finite_inputs_stay_in_their_filter_and_channel():
    """One NaN in dy at filter ko: dw[ko'] is finite for every ko' != ko, and dw[ko] is non-finite at least where a tap reaches the
    pixel.  One +inf in x at channel c0: likewise dw[:, c'] for c' != c0.  Within the pair the value may reach all nine taps (the
    route's contract).  The finite part still meets the bound."""
    from rrnet_amd import ops
    n, c, h, w, k = 2, 64, 9, 13, 64
    rng = np.random.default_rng(91)
    x = torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))
    gy = torch.from_numpy(rng.standard_normal((n, k, h, w)).astype(np.float32))
    ref = _ref_dw(x, gy, k, c)
    ko, c0 = 37, c - 3
    # NaN in dy at an interior pixel: every tap of every channel reaches it
    gbad = gy.clone()
    gbad[0, ko, 4, 7] = float("nan")
    dw = _host(_entry(_dev(x), _dev(gbad), ops.zeros_nhwc(k, c, 3, 3, "cuda")))
    bad = ~torch.isfinite(dw)
    may = torch.zeros(k, c, 3, 3, dtype=torch.bool)
    may[ko] = True
    assert bool(bad[ko].all()), "a NaN of dy is invisible at a tap it reaches"
    assert bool((bad <= may).all()), "a non-finite value outside the filter that holds the NaN"
    keep = (~may).numpy()
    idx = conv_sample_positions((k, c, 3, 3), 92, keep=keep)
    yard = conv_yardstick(conv_terms("wgrad", idx, x, (3, 3), gy, 1, (1, 1)))
    _judge("NaN in dy (%d non-finite, %d allowed)" % (int(bad.sum()), int(may.sum())), torch.where(may, torch.zeros_like(dw), dw),
           ref * (~may), idx, *yard, keep=keep)
    # +inf in x in the ragged last row at the left border: x pixel (8, 0) meets dy pixel (9 - r, 1 - s), inside for r in {1, 2}, s in {0, 1}
    xbad = x.clone()
    xbad[1, c0, 8, 0] = float("inf")
    dw = _host(_entry(_dev(xbad), _dev(gy), ops.zeros_nhwc(k, c, 3, 3, "cuda")))
    bad = ~torch.isfinite(dw)
    may = torch.zeros(k, c, 3, 3, dtype=torch.bool)
    may[:, c0] = True
    must = torch.zeros(k, c, 3, 3, dtype=torch.bool)
    must[:, c0, 1:3, 0:2] = True
    assert bool((must <= bad).all()), "an inf of x is invisible at a tap that reaches it"
    assert bool((bad <= may).all()), "a non-finite value outside the channel that holds the inf"
    keep = (~may).numpy()
    idx = conv_sample_positions((k, c, 3, 3), 93, keep=keep)
    yard = conv_yardstick(conv_terms("wgrad", idx, x, (3, 3), gy, 1, (1, 1)))
    _judge("inf in x (%d non-finite, %d allowed)" % (int(bad.sum()), int(may.sum())), torch.where(may, torch.zeros_like(dw), dw),
           ref * (~may), idx, *yard, keep=keep)


@pytest.mark.parametrize("which", ["x", "dy", "x and dy"])
def test_per_pixel_scales_of_two_to_the_plus_minus_ten(which):
    """Every pixel of x, of dy, or of both scaled by its own 2^e, e in [-10, 10]: the transforms add pixels of different scales
    before the multiplication.  Same rule, same margin."""
    from rrnet_amd import ops
    n, c, h, w, k = 1, 128, 9, 13, 128
    rng = np.random.default_rng(94)
    sx = np.ldexp(1.0, rng.integers(-10, 11, (n, 1, h, w))) if "x" in which else 1.0
    sy = np.ldexp(1.0, rng.integers(-10, 11, (n, 1, h, w))) if "dy" in which else 1.0
    x = rng.standard_normal((n, c, h, w)) * sx
    gy = rng.standard_normal((n, k, h, w)) * sy
    x, gy = torch.from_numpy(x.astype(np.float32)), torch.from_numpy(gy.astype(np.float32))
    idx = conv_sample_positions((k, c, 3, 3), 95)
    yard = conv_yardstick(conv_terms("wgrad", idx, x, (3, 3), gy, 1, (1, 1)))
    dw = _entry(_dev(x), _dev(gy), ops.zeros_nhwc(k, c, 3, 3, "cuda"))
    _judge("per-pixel scales 2^+-10 on %s" % which, _host(dw), _ref_dw(x, gy, k, c), idx, *yard)


# ------------------------------------------------------------------------------------------------------------------
# 5. what the launches must not touch
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1, 7], ids=[IDS[0], IDS[1], IDS[7]])
def test_neighbouring_parameters_and_the_workspace_tail_are_untouched(i):
    """dw is a slice of one flat gradient buffer: the parameters in front of it and behind it are bit-unchanged, and so is the
    workspace beyond rr_conv_wino_wgrad_ws_bytes."""
    from rrnet_amd import ops
    n, c, h, w, k = CASES[i]
    cs = _case(i)
    guard, numel = 4096, k * c * 9
    flat = torch.full((2 * guard + numel,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    dw = flat[guard:guard + numel].view(k, 3, 3, c).permute(0, 3, 1, 2)
    assert ops.is_nhwc(dw)
    dw.zero_()
    need = ops._WINO.call("rr_conv_wino_wgrad_ws_bytes", n, h, w, c, k)
    assert need == 4 * (16 * n * ((h + 1) // 2) * ((w + 1) // 2) * (c + k) + 16 * k * c)
    ws = torch.full((need // 4 + guard,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    ops._WINO.call("rr_conv_wino_wgrad", _dev(cs["x"]), _dev(cs["gy"]), dw, ws, need, n, h, w, c, k)
    torch.cuda.synchronize()
    bits = flat.view(torch.int32)
    assert bool((bits[:guard] == SENTINEL).all()) and bool((bits[guard + numel:] == SENTINEL).all())
    assert bool((ws.view(torch.int32)[need // 4:] == SENTINEL).all())
    assert not bool((ws.view(torch.int32)[:need // 4] == SENTINEL).any())          # V, W and S are written in full
    idx = conv_sample_positions((k, c, 3, 3), 13 * i + 2)
    _judge("%s inside a flat buffer" % IDS[i], _host(dw), cs["dw"], idx, *conv_yardstick(conv_terms("wgrad", idx, cs["x"], (3, 3), cs["gy"], 1, (1, 1))))


# ------------------------------------------------------------------------------------------------------------------
# 6. the plan and the dispatch
# ------------------------------------------------------------------------------------------------------------------
def test_plan_refusals_and_the_floor():
    from rrnet_amd import _C, ops
    n, h, w, c, k = 2, 64, 64, 128, 128
    assert _plan(n, h, w, c, k)[:2] == [0, 1]                       # 8192 pixels: the floor, and only the floor
    assert _plan(8, 128, 128, 256, 256)[:2] == [1, 0]
    assert _plan(8, 128, 128, 256, 256)[4:8] == [3, 12, 86, 768]    # 1024 K-steps of 32 tiles over 64 x 12 workgroups
    for kw in (dict(stride=2), dict(r=1, s=1, pad=(0, 0)), dict(out=(h, w)), dict(flags=1), dict(math=1), dict(pad=(0, 0))):
        assert _plan(8, 128, 128, 256, 256, **kw)[:2] == [0, 0], kw
    for cc, kk in ((32, 128), (128, 32), (130, 128), (128, 130)):
        assert _plan(8, 128, 128, cc, kk)[:2] == [0, 0], (cc, kk)
    for i, (nn, cc, hh, ww, kk) in enumerate(CASES):
        assert _plan(nn, hh, ww, cc, kk)[:2] == [0, 1], IDS[i]
    assert not ops.wino_wgrad_takes(n, h, w, c, k, 3, 3, 1, (1, 1))
    # an entry point refuses what the plan refuses for another reason than the floor
    t = torch.zeros(16, device="cuda")
    with pytest.raises(_C.RRNetHipError):
        ops._WINO.call("rr_conv_wino_wgrad", t, t, t, t, 1 << 30, 1, 8, 8, 32, 64)
    with pytest.raises(_C.RRNetHipError):
        ops._WINO.call("rr_conv_wino_wgrad", t, t, t, t, 64, 1, 8, 8, 64, 64)          # a workspace too small


def test_dispatch_with_the_switch_off_is_the_direct_launch():
    """2 x 64 x 64 x 128 -> 128: with the switch off — and with it on, below the floor — ops.conv_wgrad makes exactly the one
    rr_conv_wgrad call it made before the route existed; with the test switch the route's two calls."""
    from rrnet_amd import ops
    n, c, h, w, k = 2, 128, 64, 64, 128
    g = torch.Generator().manual_seed(5)
    xd, gyd = _dev(torch.randn(n, c, h, w, generator=g)), _dev(torch.randn(n, k, h, w, generator=g))
    real_fn = ops._C.fn

    def recorded(on, below):
        log = []

        def fn(name, *a, **kw):
            f = real_fn(name, *a, **kw)

            def call(*args):
                log.append((name,) + tuple(v for v in args if isinstance(v, (int, float))))
                return f(*args)
            return call
        dw = ops.zeros_nhwc(k, c, 3, 3, "cuda")
        ops._C.fn = fn
        try:
            with _route(on, below) as keys:
                ops.conv_wgrad(xd, gyd, dw, 1, (1, 1))
        finally:
            ops._C.fn = real_fn
        torch.cuda.synchronize()
        return log, keys, dw
    direct = [("rr_conv_wgrad", n, h, w, c, k, 3, 3, 1, 1, 1, 0, 0)]
    log, keys, dw_off = recorded(False, True)
    assert log == direct and keys == ["conv_wgrad<BN=128>"], (log, keys)
    log, keys, _ = recorded(True, False)
    assert log == direct and keys == ["conv_wgrad<BN=128>"], (log, keys)
    log, keys, dw_on = recorded(True, True)
    assert [e[0] for e in log] == ["rr_conv_wino_wgrad_ws_bytes", "rr_conv_wino_wgrad"] and keys == ["conv_wgrad<wino>"], (log, keys)
    assert float((dw_on - dw_off).abs().max()) > 0.0            # the two arms really ran different arithmetic


# ------------------------------------------------------------------------------------------------------------------
# 7. one residual block, the route on and off
# ------------------------------------------------------------------------------------------------------------------
def _block_run(sd, x, gy, route_on):
    from rrnet_amd import ops
    from rrnet_amd.backbones.hourglass import ResidualBlock
    with _route(route_on, route_on) as keys:
        mod = ResidualBlock(128, 128, 1)
        mod.load_state_dict(sd)
        mod = mod.cuda().to(memory_format=torch.channels_last).train()
        xd = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
        y = mod(xd)
        y.backward(gy.cuda().contiguous(memory_format=torch.channels_last))
        torch.cuda.synchronize()
        out = {kk: p.grad.detach().cpu().double() for kk, p in mod.named_parameters() if p.dim() == 4 and p.shape[2] == 3}
    assert keys.count("conv_wgrad<wino>") == (2 if route_on else 0), keys
    return out


def test_residual_block_with_the_route_on_and_off():
    """ResidualBlock(128, 128) on 2 x 64 x 64 (8192 pixels: below the floor, so the arm with the route on runs under
    ops._WINO_WGRAD_BELOW_FLOOR), the weight gradients of both 3x3 layers against oracle/model.py's block in float64:
    |on - off| <= |on - fp64| + |off - fp64|, and the route's RMS distance to float64 within 4x the direct route's."""
    from oracle import model as om
    from rrnet_amd.backbones.hourglass import ResidualBlock
    torch.manual_seed(78)
    sd = {kk: v.clone() for kk, v in ResidualBlock(128, 128, 1).state_dict().items()}
    for kk in sd:
        if kk.endswith("bn1.weight") or kk.endswith("bn2.weight"):
            sd[kk] = torch.rand_like(sd[kk]) + 0.5
        elif kk.endswith("bn1.bias") or kk.endswith("bn2.bias"):
            sd[kk] = torch.randn_like(sd[kk]) * 0.3
    x, gy = torch.randn(2, 128, 64, 64), torch.randn(2, 128, 64, 64)
    stat = ("running_mean", "running_var", "num_batches_tracked")
    P = om.Params({"m." + kk: (v.clone() if kk.endswith(stat[2]) else v.double().clone().requires_grad_(not kk.endswith(stat)))
                   for kk, v in sd.items()}, training=True)
    y64 = om.residual_block(P, "m", x.double(), 1)
    y64.backward(gy.double())
    on, off = _block_run(sd, x, gy, True), _block_run(sd, x, gy, False)
    assert len(on) == 2 and set(on) == set(off)
    for kk in sorted(on):
        ref = P.sd["m." + kk].grad
        d_on, d_off, d = (on[kk] - ref).abs(), (off[kk] - ref).abs(), (on[kk] - off[kk]).abs()
        r_on, r_off = float(d_on.pow(2).mean().sqrt()), float(d_off.pow(2).mean().sqrt())
        print("wino wgrad block %s: rms distance to fp64: route on %.3e, off %.3e (ratio %.2f); max |on - off| %.3e"
              % (kk, r_on, r_off, r_on / max(r_off, 1e-300), float(d.max())))
        assert bool((d <= d_on + d_off).all()), kk
        assert r_on <= 4.0 * r_off, (kk, r_on, r_off)
        assert float(d.max()) > 0.0, kk

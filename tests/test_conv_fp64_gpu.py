"""GPU: the fp32 MFMA convolutions of rrnet_amd/csrc/conv.hip (fprop / dgrad / wgrad) against float64, on every host
dispatch route (helpers.conv_routes names the route of each shape; tests/test_host_logic.py checks that the grid reaches
every label).  The other convolution suites (bf16, f16x3, conv16) compare against THESE kernels, so this is their anchor.

Acceptance rule (helpers.seq32_error / conv_error_ratios / conv_accepts): at 4096 seeded outputs the kernel's max-abs and
RMS error against float64 must not exceed CONV_MARGIN x the error of a float32 sum that adds the same float32-rounded
products one after the other; the RMS error over the whole tensor is held to the same figure.  Every test prints its
ratios.  The statistics slab is judged on its own, against the float64 column sums of the kernel's OWN output."""
import functools

import numpy as np
import pytest
import torch

from helpers import (CONV64_ASYM_WGRAD, CONV64_GRID, CONV_MARGIN, CONV_SAMPLES, U32, conv_accepts, conv_bias_clear_of_zero,
                     conv_error_ratios, conv_ref64, conv_routes, conv_sample_positions, conv_tap_counts, conv_terms,
                     conv_yardstick)

pytestmark = pytest.mark.gpu

GRID_IDS = ["n%dc%dh%dw%dk%dr%ds%d_s%d" % c[:8] + ("_bias" if c[10] else "") + ("_relu" if c[11] else "") for c in CONV64_GRID]
SENTINEL = -7.25e300
SHAPE_A = (1, 256, 16, 16, 256, 3, 3, 1, 1, 1)          # split-K fprop / dgrad, pipelined wgrad
SHAPE_B = (2, 16, 7, 9, 24, 3, 3, 2, 1, 1)              # stride 2, odd H and W: the four parity classes
SPECIAL = [SHAPE_A, SHAPE_B]
SPECIAL_IDS = ["n%dc%dh%dw%dk%dr%ds%d_s%d" % c[:8] for c in SPECIAL]


def _f32mode():
    from rrnet_amd import ops
    return ops.bf16_scope(0, force=True)                # the fp32 kernels whatever RR_CONV_MATH says


def _dev(a):
    from rrnet_amd import ops
    return ops.to_nhwc(torch.as_tensor(a).float().cuda())


def _host(t):
    return t.detach().cpu().double()


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs (float32, CPU) and the float64 reference of grid case i: computed once, shared by its tests, never modified."""
    n, c, h, w, k, r, s, st, ph, pw, bias, relu, _, passes = CONV64_GRID[i]
    rng = np.random.default_rng(1000 + i)
    x = torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))
    wt = torch.from_numpy((rng.standard_normal((k, c, r, s)) / np.sqrt(c * r * s)).astype(np.float32))
    b = rng.standard_normal(k).astype(np.float32) if bias else None
    if relu:                                             # no output near 0: fp32 and fp64 agree on every ReLU mask bit
        b = conv_bias_clear_of_zero(conv_ref64(x, wt, None, st, (ph, pw), False)[0].numpy(), b)
    b = None if b is None else torch.from_numpy(b)
    p, q = (h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1
    gy = torch.from_numpy(rng.standard_normal((n, k, p, q)).astype(np.float32)) if passes != "f" else None
    y, dx, dw = conv_ref64(x, wt, b, st, (ph, pw), relu, gy)
    if relu:
        assert float(y[y > 0].min()) > 1e-3 and float(conv_ref64(x, wt, b, st, (ph, pw), False)[0].abs().min()) > 1e-3
        gy = gy * (y > 0).float()                        # what the layer's backward hands to the kernels
    return dict(x=x, w=wt, b=b, gy=gy, y=y, dx=dx, dw=dw)


def _routes(i, want_stats=False, **kw):
    n, c, h, w, k, r, s, st, ph, pw, bias, relu = CONV64_GRID[i][:12]
    return conv_routes(n, c, h, w, k, r, s, st, (ph, pw), bias, relu, want_stats, **kw)


def _judge(tag, got, ref_all, idx, ref_s, max_seq, rms_seq, keep=None):
    """Prints the three ratios of one tensor and asserts the acceptance rule.  keep: boolean mask of the elements judged."""
    got, ref_all = got.numpy(), ref_all.numpy()
    # the gathered products really are those of the reference's outputs
    assert np.abs(ref_s - ref_all[idx]).max() <= 1e-11 * max(np.abs(ref_s).max(), 1e-30), tag
    ga, ra = (got, ref_all) if keep is None else (got[keep], ref_all[keep])
    ratios = conv_error_ratios(got[idx], ref_s, max_seq, rms_seq, ga, ra)
    print("%s: max %.2f rms %.2f whole-tensor rms %.2f of the chained-fp32 yardstick (max %.2e rms %.2e), margin %g"
          % ((tag,) + ratios + (max_seq, rms_seq, CONV_MARGIN)))
    assert conv_accepts(ratios), (tag, ratios)
    return ratios


def _fprop_raw(xd, wd, bd, shape, st, ph, pw, relu, slab):
    from rrnet_amd import _C, ops
    n, c, h, w, k, r, s = shape
    p, q = ops.out_hw(h, w, r, s, st, ph, pw)
    y = ops.empty_nhwc(n, k, p, q, xd.device)
    _C.check(_C.fn("rr_conv_fprop")(_C.ptr(xd), _C.ptr(wd), _C.ptr(bd), _C.ptr(y), _C.ptr(slab), n, h, w, c, k, r, s, st, ph, pw,
                                    int(relu), _C.stream()), "rr_conv_fprop")
    return y


def _slab_for(n, p, q, k):
    from rrnet_amd import _C
    nb = _C.fn("rr_conv_stat_slab_bytes")(n, p, q, k)
    assert nb == -(-n * p * q // 128) * 2 * k * 8
    return torch.full((nb // 8,), SENTINEL, dtype=torch.float64, device="cuda")


def _check_slab(tag, slab, y, k, split):
    """The slab against the float64 column sums of the kernel's own y.  Fused epilogue (conv_igemm_kernel: s1 / s2 chain at
    most 64 rows per lane in fp32, then everything is double): |err| <= 65 u sum|y| and 66 u sum y^2 (64 additions, + the
    square's rounding).  Split-K (colstats_kernel, all double): 1e-12 of the same sums, only row 0 of the slab filled."""
    rows = slab.view(-1, 2, k)
    yd = _host(y).permute(0, 2, 3, 1).reshape(-1, k)
    s1, s2, a1 = yd.sum(0), (yd * yd).sum(0), yd.abs().sum(0)
    got = rows.sum(0).cpu()
    if split:
        assert float(rows[1:].abs().max() if rows.shape[0] > 1 else 0.0) == 0.0, tag     # the rows colstats_kernel does not fill
        b1, b2 = 1e-12 * a1, 1e-12 * s2
    else:
        assert bool((rows != SENTINEL).all()), tag                                         # every tile row, every column written
        b1, b2 = 65 * U32 * a1, 66 * U32 * s2
    e1, e2 = (got[0] - s1).abs(), (got[1] - s2).abs()
    tiny = 1e-300
    print("%s: slab (%s, %d rows) error over bound: sum y %.3f, sum y^2 %.3f" % (tag, "split-K" if split else "fused", rows.shape[0],
          float((e1 / (b1 + tiny)).max()), float((e2 / (b2 + tiny)).max())))
    assert bool((e1 <= b1).all()) and bool((e2 <= b2).all()), tag


@pytest.mark.parametrize("i", range(len(CONV64_GRID)), ids=GRID_IDS)
def test_fprop_against_fp64(i):
    from rrnet_amd import ops
    n, c, h, w, k, r, s, st, ph, pw, bias, relu, stats, _ = CONV64_GRID[i]
    cs = _case(i)
    idx = conv_sample_positions(tuple(cs["y"].shape), 7 * i + 1)
    yard = conv_yardstick(conv_terms("fprop", idx, cs["x"], cs["w"], None, st, (ph, pw), bias=cs["b"]), relu=relu)
    xd, wd = _dev(cs["x"]), _dev(cs["w"])
    bd = None if cs["b"] is None else cs["b"].cuda()
    with _f32mode():
        for ws in stats:
            route = sorted(_routes(i, ws)["fprop"])
            tag = "fprop %s stats=%d %s" % (GRID_IDS[i], ws, route)
            if ws:
                slab = _slab_for(n, cs["y"].shape[2], cs["y"].shape[3], k)
                y = _fprop_raw(xd, wd, bd, (n, c, h, w, k, r, s), st, ph, pw, relu, slab)
                _check_slab(tag, slab, y, k, "ksplit>1+stats" in route)
            else:
                y = ops.conv_fprop(xd, wd, bd, st, (ph, pw), relu)
            _judge(tag, _host(y), cs["y"], idx, *yard)
        if ops.conv_packable(xd, wd, st):             # the stem: packed taps + a 1x1 convolution on the vector kernels
            y, slab, _ = ops.conv_fprop_packed(xd, wd, st, (ph, pw), want_stats=True)
            _judge("fprop %s packed taps" % GRID_IDS[i], _host(y), cs["y"], idx, *yard)


@pytest.mark.parametrize("i", [j for j, c in enumerate(CONV64_GRID) if "d" in c[13]], ids=[g for g, c in zip(GRID_IDS, CONV64_GRID) if "d" in c[13]])
def test_dgrad_against_fp64(i):
    """Both data-gradient routes of ops.conv_dgrad (rr_conv_dgrad; stride 1: the forward kernel on the flipped filter), each
    plain and accumulating into a non-zero tensor."""
    from rrnet_amd import ops
    n, c, h, w, k, r, s, st, ph, pw = CONV64_GRID[i][:10]
    cs = _case(i)
    rng = np.random.default_rng(2000 + i)
    base = torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))
    idx = conv_sample_positions((n, c, h, w), 7 * i + 2)
    yard = conv_yardstick(conv_terms("dgrad", idx, None, cs["w"], cs["gy"], st, (ph, pw)), head=base.double().numpy()[idx])
    gyd, wd = _dev(cs["gy"]), _dev(cs["w"])
    rt = _routes(i)
    saved = ops._DGRAD_VIA_FPROP, ops._DGRAD_VIA_FPROP_MIN_PIXELS
    ops._DGRAD_VIA_FPROP_MIN_PIXELS = 0
    try:
        with _f32mode():
            for via in ((False, True) if rt["dgrad_via_fprop"] else (False,)):
                ops._DGRAD_VIA_FPROP = via
                tag = "dgrad %s %s" % (GRID_IDS[i], "via fprop %s" % sorted(rt["dgrad_via_fprop"]) if via else sorted(rt["dgrad"]))
                dx = ops.conv_dgrad(gyd, wd, (n, c, h, w), st, (ph, pw))
                _judge(tag, _host(dx), cs["dx"], idx, *yard[:3])
                acc = _dev(base).clone(memory_format=torch.channels_last)
                ops.conv_dgrad(gyd, wd, (n, c, h, w), st, (ph, pw), out=acc, accumulate=True)
                _judge(tag + " accumulate", _host(acc), cs["dx"] + base.double(), idx, *yard[3:])
    finally:
        ops._DGRAD_VIA_FPROP, ops._DGRAD_VIA_FPROP_MIN_PIXELS = saved


@pytest.mark.parametrize("i", [j for j, c in enumerate(CONV64_GRID) if "w" in c[13]], ids=[g for g, c in zip(GRID_IDS, CONV64_GRID) if "w" in c[13]])
def test_wgrad_against_fp64(i):
    """conv_wgrad_kernel ADDS (its epilogue is an atomic add into dw, also with one split): into a zeroed dw the result is
    the gradient, into a non-zero dw it is that tensor plus the gradient — judged with the starting value as one more term."""
    from rrnet_amd import ops
    n, c, h, w, k, r, s, st, ph, pw = CONV64_GRID[i][:10]
    cs = _case(i)
    rng = np.random.default_rng(3000 + i)
    base = torch.from_numpy((rng.standard_normal((k, c, r, s)) * float(cs["dw"].std())).astype(np.float32))
    idx = conv_sample_positions((k, c, r, s), 7 * i + 3)
    yard = conv_yardstick(conv_terms("wgrad", idx, cs["x"], (r, s), cs["gy"], st, (ph, pw)), head=base.double().numpy()[idx])
    xd, gyd = _dev(cs["x"]), _dev(cs["gy"])
    tag = "wgrad %s %s" % (GRID_IDS[i], sorted(_routes(i)["wgrad"]))
    with _f32mode():
        dw = ops.zeros_nhwc(k, c, r, s, "cuda")
        ops.conv_wgrad(xd, gyd, dw, st, (ph, pw))
        _judge(tag, _host(dw), cs["dw"], idx, *yard[:3])
        dw = _dev(base).clone(memory_format=torch.channels_last)
        ops.conv_wgrad(xd, gyd, dw, st, (ph, pw))
        _judge(tag + " into a non-zero dw", _host(dw), cs["dw"] + base.double(), idx, *yard[3:])
        if ops.conv_packable(xd, _dev(cs["w"]), st):   # the stem's weight gradient from the packed taps
            _, _, xp = ops.conv_fprop_packed(xd, _dev(cs["w"]), st, (ph, pw))
            dw = _dev(base).clone(memory_format=torch.channels_last)
            ops.conv_wgrad_packed(xp, gyd, dw)
            _judge(tag + " packed taps, non-zero dw", _host(dw), cs["dw"] + base.double(), idx, *yard[3:])


def test_wgrad_output_size_override_is_padding_at_the_far_edge():
    """rr_conv_wgrad with out_h / out_w one larger than symmetric padding gives (pad_h / pad_w are the leading pads) ==
    the weight gradient of the convolution on the input zero-padded by one more row and column at the far edge."""
    import torch.nn.functional as F
    from rrnet_amd import _C, ops
    n, c, h, w, k, r, s, st, ph, pw, oh, ow = CONV64_ASYM_WGRAD
    rng = np.random.default_rng(77)
    x = torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))
    gy = torch.from_numpy(rng.standard_normal((n, k, oh, ow)).astype(np.float32))
    far_h, far_w = (oh - 1) * st + r - (h + 2 * ph), (ow - 1) * st + s - (w + 2 * pw)
    assert far_h == 1 and far_w == 1
    _, _, dw_ref = conv_ref64(F.pad(x, (0, far_w, 0, far_h)), torch.zeros(k, c, r, s), None, st, (ph, pw), False, gy)
    idx = conv_sample_positions((k, c, r, s), 78)
    yard = conv_yardstick(conv_terms("wgrad", idx, x, (r, s), gy, st, (ph, pw)))
    xd, gyd = _dev(x), _dev(gy)
    dw = ops.zeros_nhwc(k, c, r, s, "cuda")
    _C.check(_C.fn("rr_conv_wgrad")(_C.ptr(xd), _C.ptr(gyd), _C.ptr(dw), n, h, w, c, k, r, s, st, ph, pw, oh, ow, _C.stream()), "rr_conv_wgrad")
    route = sorted(conv_routes(n, c, h, w, k, r, s, st, (ph, pw), False, False, False, oh, ow)["wgrad"])
    _judge("wgrad out_h/out_w override %s" % route, _host(dw), dw_ref, idx, *yard)


# ------------------------------------------------------------------------------------------------------------------
# inputs where convolution kernels go wrong
# ------------------------------------------------------------------------------------------------------------------
def _run_all(x, wt, gy, cfg, want_stats=(False, True)):
    """y per want_stats value, dx per data-gradient route, dw into zeros: every kernel route of one shape, as CPU float64."""
    from rrnet_amd import ops
    n, c, h, w, k, r, s, st, ph, pw = cfg
    xd, wd, gyd = _dev(x), _dev(wt), _dev(gy)
    out = {}
    saved = ops._DGRAD_VIA_FPROP, ops._DGRAD_VIA_FPROP_MIN_PIXELS
    ops._DGRAD_VIA_FPROP_MIN_PIXELS = 0
    try:
        with _f32mode():
            for ws in want_stats:
                res = ops.conv_fprop(xd, wd, None, st, (ph, pw), False, want_stats=ws)
                out["y stats=%d" % ws] = _host(res[0] if ws else res)
            for via in ((False, True) if st == 1 else (False,)):
                ops._DGRAD_VIA_FPROP = via
                out["dx via_fprop=%d" % via] = _host(ops.conv_dgrad(gyd, wd, (n, c, h, w), st, (ph, pw)))
            dw = ops.zeros_nhwc(k, c, r, s, "cuda")
            ops.conv_wgrad(xd, gyd, dw, st, (ph, pw))
            out["dw"] = _host(dw)
    finally:
        ops._DGRAD_VIA_FPROP, ops._DGRAD_VIA_FPROP_MIN_PIXELS = saved
    return out


def _ref_of(name, y, dx, dw):
    return y if name.startswith("y") else (dx if name.startswith("dx") else dw)


@pytest.mark.parametrize("cfg", SPECIAL, ids=SPECIAL_IDS)
def test_exact_cancellation_and_signed_zeros(cfg):
    """Operands of the form +-2^e, e in [-2, 2] (and +-0), paired over the channels so that the products of every tap cancel
    exactly in pairs: every partial sum, in any order and over any split, is a multiple of 2^-4 below 2^17, hence exact in
    float32.  The float64 answer is 0 except where one planted element (x for y, dy for dx) breaks a pair; the kernels —
    split-K atomics included — must return exactly 0 there and the planted outputs (and all of dw) bit for bit."""
    n, c, h, w, k, r, s, st, ph, pw = cfg
    rng = np.random.default_rng(41)
    p, q = (h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1

    def paired(shape, axis):                                 # +-2^e or +-0, the same value on channels 2i and 2i + 1
        half = list(shape)
        half[axis] //= 2
        v = np.ldexp(rng.choice([-1.0, 1.0], half), rng.integers(-2, 3, half))
        v[rng.random(half) < 0.1] = 0.0
        v[rng.random(half) < 0.05] = -0.0
        return np.repeat(v, 2, axis=axis)
    x, gy = paired((n, c, h, w), 1), paired((n, k, p, q), 1)
    mag = np.repeat(np.repeat(np.ldexp(1.0, rng.integers(-2, 3, (k // 2, c // 2, r, s))), 2, 0), 2, 1)
    sign = np.where(np.arange(k) % 2, -1.0, 1.0)[:, None, None, None] * np.where(np.arange(c) % 2, -1.0, 1.0)[None, :, None, None]
    wt = mag * sign                                          # w[k, 2i+1] = -w[k, 2i] and w[2j+1, c] = -w[2j, c]
    x[0, 5, h // 2, w // 3] += 8.0
    gy[n - 1, 2, p // 2, q // 2] += 8.0
    x, wt, gy = (torch.from_numpy(a.astype(np.float32)) for a in (x, wt, gy))
    y, dx, dw = conv_ref64(x, wt, None, st, (ph, pw), False, gy)
    planted_y = conv_ref64((x == x[0, 5, h // 2, w // 3]).double()[:, 5:6], torch.ones(1, 1, r, s), None, st, (ph, pw), False)[0]
    assert int((y != 0).sum()) > 0 and bool(((y != 0).any(1, keepdim=True) <= (planted_y > 0)).all())    # zero outside the planted field
    assert 0 < int((dx != 0).sum()) <= n * c * r * s
    for name, got in _run_all(x, wt, gy, cfg).items():
        ref = _ref_of(name, y, dx, dw)
        assert torch.equal(got, ref), (name, float((got - ref).abs().max()), int((got != ref).sum()))
        print("%s %s: bit-exact, %d non-zero of %d" % (SPECIAL_IDS[SPECIAL.index(cfg)], name, int((ref != 0).sum()), ref.numel()))


@pytest.mark.parametrize("cfg", SPECIAL, ids=SPECIAL_IDS)
def test_dynamic_range_across_channels(cfg):
    """One input channel scaled by 1e4 with its filter taps scaled by 1e-4, another the opposite way: same products in y,
    eight decades between the channels of dx and dw.  The bound is unchanged, being computed on the same terms."""
    n, c, h, w, k, r, s, st, ph, pw = cfg
    rng = np.random.default_rng(42)
    p, q = (h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1
    x = rng.standard_normal((n, c, h, w))
    wt = rng.standard_normal((k, c, r, s)) / np.sqrt(c * r * s)
    x[:, 0] *= 1e4; wt[:, 0] *= 1e-4; x[:, 1] *= 1e-4; wt[:, 1] *= 1e4
    x, wt = torch.from_numpy(x.astype(np.float32)), torch.from_numpy(wt.astype(np.float32))
    gy = torch.from_numpy(rng.standard_normal((n, k, p, q)).astype(np.float32))
    y, dx, dw = conv_ref64(x, wt, None, st, (ph, pw), False, gy)
    yards = {}
    for kind, ref in (("y", y), ("dx", dx), ("dw", dw)):
        idx = conv_sample_positions(tuple(ref.shape), 43)
        terms = conv_terms({"y": "fprop", "dx": "dgrad", "dw": "wgrad"}[kind], idx, x, (r, s) if kind == "dw" else wt, gy, st, (ph, pw))
        yards[kind] = (idx,) + conv_yardstick(terms)
    for name, got in _run_all(x, wt, gy, cfg).items():
        idx, ref_s, mx, rms = yards[name.split()[0]]
        _judge("dynamic range %s %s" % (SPECIAL_IDS[SPECIAL.index(cfg)], name), got, _ref_of(name, y, dx, dw), idx, ref_s, mx, rms)


@pytest.mark.parametrize("cfg", SPECIAL, ids=SPECIAL_IDS)
def test_all_ones_count_the_taps_inside_the_image(cfg):
    """x = w = dy = 1 (exact in fp32): y = C x (taps of the pixel inside the image), dx = K x ((output, tap) pairs reaching the
    pixel), dw = N x (outputs whose tap lies inside) — closed forms, bit for bit: an off-by-one in any border or parity class
    changes a count."""
    n, c, h, w, k, r, s, st, ph, pw = cfg
    p, q = (h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1
    in_h, reach_h, valid_h = conv_tap_counts(h, p, r, st, ph)
    in_w, reach_w, valid_w = conv_tap_counts(w, q, s, st, pw)
    want = {"y": torch.from_numpy(c * np.outer(in_h, in_w)).double().expand(n, k, p, q),
            "dx": torch.from_numpy(k * np.outer(reach_h, reach_w)).double().expand(n, c, h, w),
            "dw": torch.from_numpy(n * np.outer(valid_h, valid_w)).double().expand(k, c, r, s)}
    assert len(np.unique(np.outer(in_h, in_w))) > 1 and len(np.unique(np.outer(reach_h, reach_w))) > 1
    for name, got in _run_all(torch.ones(n, c, h, w), torch.ones(k, c, r, s), torch.ones(n, k, p, q), cfg).items():
        ref = want[name.split()[0]]
        assert torch.equal(got, ref), (name, float((got - ref).abs().max()), int((got != ref).sum()))


@pytest.mark.parametrize("cfg", SPECIAL, ids=SPECIAL_IDS)
def test_non_finite_inputs_stay_visible_and_do_not_leak(cfg):
    """One NaN and one +inf in x (fprop), in dy (dgrad, wgrad): exactly the outputs whose receptive field holds one are
    non-finite, every other output still meets the bound — nothing leaks across tiles or K slices."""
    n, c, h, w, k, r, s, st, ph, pw = cfg
    rng = np.random.default_rng(44)
    p, q = (h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1
    x = torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))
    wt = torch.from_numpy((rng.standard_normal((k, c, r, s)) / np.sqrt(c * r * s)).astype(np.float32))
    gy = torch.from_numpy(rng.standard_normal((n, k, p, q)).astype(np.float32))
    # interior positions (every tap of the marked dy pixels lies inside x: dw[k0], dw[k1] are non-finite throughout)
    xpos = [(0, 5, h // 4, w // 2), (n - 1, c - 3, (3 * h) // 4, w // 4)]
    gpos = [(0, 3, 1, q // 2), (n - 1, k - 2, p // 2, 1)]
    for (pp, qq) in [(g[2], g[3]) for g in gpos]:
        assert pp * st - ph >= 0 and pp * st - ph + r <= h and qq * st - pw >= 0 and qq * st - pw + s <= w
    xbad, gbad = x.clone(), gy.clone()
    xbad[xpos[0]], xbad[xpos[1]] = float("nan"), float("inf")
    gbad[gpos[0]], gbad[gpos[1]] = float("nan"), float("inf")
    ones = torch.ones(1, 1, r, s)
    xmark, gmark = torch.zeros(n, 1, h, w), torch.zeros(n, 1, p, q)
    for pos in xpos:
        xmark[pos[0], 0, pos[2], pos[3]] = 1
    for pos in gpos:
        gmark[pos[0], 0, pos[2], pos[3]] = 1
    hit_y = (conv_ref64(xmark, ones, None, st, (ph, pw), False)[0] > 0).expand(n, k, p, q)
    hit_dx = (conv_ref64(torch.zeros(n, 1, h, w), ones, None, st, (ph, pw), False, gmark)[1] > 0).expand(n, c, h, w)
    hit_dw = torch.zeros(k, c, r, s, dtype=torch.bool)
    hit_dw[gpos[0][1]] = hit_dw[gpos[1][1]] = True
    xz, gz = x.clone(), gy.clone()                          # the reference of the untouched outputs: the marked elements as 0
    xz[xpos[0]] = xz[xpos[1]] = 0.0
    gz[gpos[0]] = gz[gpos[1]] = 0.0
    y = conv_ref64(xz, wt, None, st, (ph, pw), False)[0]
    _, dx, dw = conv_ref64(x, wt, None, st, (ph, pw), False, gz)
    got_y = _run_all(xbad, wt, gy, cfg)
    got_g = _run_all(x, wt, gbad, cfg)
    for name in got_y:
        kind = name.split()[0]
        got = got_y[name] if kind == "y" else got_g[name]
        hit, ref = {"y": (hit_y, y), "dx": (hit_dx, dx), "dw": (hit_dw, dw)}[kind]
        bad = ~torch.isfinite(got)
        assert torch.equal(bad, hit), (name, int(bad.sum()), int(hit.sum()), int((bad != hit).sum()))
        keep = (~hit).numpy()
        idx = conv_sample_positions(tuple(ref.shape), 45, keep=keep)
        terms = conv_terms({"y": "fprop", "dx": "dgrad", "dw": "wgrad"}[kind], idx, xz if kind == "y" else x, (r, s) if kind == "dw" else wt,
                           gz, st, (ph, pw))
        _judge("non-finite %s %s (%d non-finite)" % (SPECIAL_IDS[SPECIAL.index(cfg)], name, int(hit.sum())),
               torch.where(hit, torch.zeros_like(got), got), ref * (~hit), idx, *conv_yardstick(terms), keep=keep)


# ------------------------------------------------------------------------------------------------------------------
# a statistic through finalize
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(80, 64), (79, 65)], ids=["M5120", "M5135"])
def test_mean_30_statistics_through_finalize(hw):
    """A 1x1 convolution whose output has per-channel mean 30 (from a constant input channel) and standard deviation 1,
    M a multiple of 128 and not; its slab through ops.bn_stats_finalize against a float64 BatchNorm over the kernel's own y.

    Bounds, from the slab's (test_fprop_against_fp64: |dS1| <= 65 u sum|y|, |dS2| <= 66 u sum y^2; the finalize kernel is
    double throughout and rounds mean / invstd to float once, relative u):
      mean   = S1 / M                 |d mean| <= 65 u E|y| + u |mean|
      var    = S2 / M - mean^2        |d var|  <= 66 u E[y^2] + 2 |mean| 65 u E|y| + (65 u E|y|)^2  =: B
               (~ 196 u * 901 = 1.05e-2 at mean 30, var 1: the one-pass variance loses (mean/std)^2 = 900 of the sums' accuracy)
      invstd = (var + eps)^-1/2       inside [ (var64 + eps + B)^-1/2 (1 - 2u), (var64 + eps - B)^-1/2 (1 + 2u) ]"""
    from rrnet_amd import ops
    h, w = hw
    c, k, eps = 64, 64, 1e-5
    rng = np.random.default_rng(h)
    x = rng.standard_normal((1, c, h, w)).astype(np.float32)
    x[:, 0] = 1.0
    wt = rng.standard_normal((k, c, 1, 1))
    wt[:, 0] = 0.0
    wt = (wt / np.sqrt((wt * wt).sum(1, keepdims=True))).astype(np.float32)       # unit norm over the random channels: variance 1
    wt[:, 0] = 30.0
    xd, wd = _dev(x), _dev(wt)
    with _f32mode():
        slab = _slab_for(1, h, w, k)
        y = _fprop_raw(xd, wd, None, (1, c, h, w, k, 1, 1), 1, 0, 0, False, slab)
    assert bool((slab != SENTINEL).all())
    one, zero = torch.ones(k, device="cuda"), torch.zeros(k, device="cuda")
    mean, invstd, _, _ = ops.bn_stats_finalize(slab, float(h * w), one, zero, zero.clone(), one.clone(), 0.1, eps)
    yd = _host(y).permute(0, 2, 3, 1).reshape(-1, k)
    m64 = yd.mean(0)
    var64 = ((yd - m64) ** 2).mean(0)
    assert float((m64 - 30).abs().max()) < 0.2 and float((var64 - 1).abs().max()) < 0.2
    ea, e2 = yd.abs().mean(0), (yd * yd).mean(0)
    b_mean = 65 * U32 * ea + U32 * m64.abs()
    b_var = 66 * U32 * e2 + 2 * m64.abs() * 65 * U32 * ea + (65 * U32 * ea) ** 2
    lo, hi = (var64 + eps + b_var) ** -0.5 * (1 - 2 * U32), (var64 + eps - b_var) ** -0.5 * (1 + 2 * U32)
    i64 = (var64 + eps) ** -0.5
    gm, gi = mean.cpu().double(), invstd.cpu().double()
    _, tm, ti = torch.native_batch_norm(y.cpu().contiguous(), None, None, None, None, True, 0.1, eps)
    print("mean-30 M=%d: |mean err| max %.2e (bound %.2e, torch CPU fp32 %.2e); invstd rel err max %.2e (bound %.2e, torch CPU fp32 %.2e)"
          % (h * w, float((gm - m64).abs().max()), float(b_mean.min()), float((tm.double() - m64).abs().max()),
             float(((gi - i64) / i64).abs().max()), float((b_var / (2 * (var64 + eps))).min()), float(((ti.double() - i64) / i64).abs().max())))
    assert bool(((gm - m64).abs() <= b_mean).all())
    assert bool((gi >= lo).all()) and bool((gi <= hi).all())

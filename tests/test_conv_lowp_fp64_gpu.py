"""GPU: the bf16 and f16x3 implicit-GEMM convolutions of rrnet_amd/csrc/conv_bf16.hip (conv_igemm_bf16_kernel in its tile widths,
plain / fused backward sums / strided destination, fp32 or ready-made 16-bit filter; conv_wgrad_bf16_kernel) against float64, on
every route rr_plan::fprop_plan (csrc/conv_plan.h) can send them.  The entry points are called through the C ABI, so that no size
threshold of rrnet_amd.ops reroutes a case; helpers.CONV16_GRID lays the cases out and tests/test_host_logic.py checks that they
reach every label of helpers.CONV16_ROUTE_LABELS in both arithmetics.

Reference: the operand images the contract defines (helpers.lowp_image: bf16 round-to-nearest-even; f16x3 hi + lo under the scale of
the maxima the entry point is handed) multiplied in float64 on the CPU — hi*hi + hi*lo + lo*hi for f16x3, oracle.split.conv2d in the
forward pass.  Acceptance: helpers.conv_accepts, unchanged from the fp32 suite — the products of the images are exact in float32, so
only fp32 accumulation separates a correct kernel from the reference, and the yardstick is the chained float32 sum of those same
products at 4096 seeded outputs (the three products of an f16x3 term as three terms).  Every judged tensor prints its ratios and route."""
import functools

import numpy as np
import pytest
import torch

from helpers import (CONV16_ASYM_WGRAD, CONV16_GRID, CONV16_LINKS, CONV16_MARGIN, LOWP_NAMES, MATH_BF16, MATH_F16X3, U32, conv16_case_labels,
                     conv16_dgrad_labels, conv16_wgrad_labels, conv_accepts, conv_bias_clear_of_zero, conv_error_ratios, conv_ref64,
                     conv_sample_positions, conv_tap_counts, conv_yardstick, lowp_fprop_ref64, lowp_grads_ref64, lowp_image, lowp_terms)

pytestmark = pytest.mark.gpu

MATHS = [MATH_BF16, MATH_F16X3]
MATH_IDS = [LOWP_NAMES[m] for m in MATHS]
GRID_IDS = ["n%dc%dh%dw%dk%dr%ds%d_s%d" % c[:8] + ("_bias" if c[10] else "") + ("_relu" if c[11] else "") for c in CONV16_GRID]
SENTINEL = -7.25e300
INF_BITS = 0x7f800000
SHAPE_A = (1, 256, 16, 16, 256, 3, 3, 1, 1, 1)          # stride 1: bn32 split-K forward and data gradient
SHAPE_B = (2, 16, 7, 9, 24, 3, 3, 2, 1, 1)              # stride 2, odd H and W: four parity classes of different sizes
SPECIAL = [SHAPE_A, SHAPE_B]
SPECIAL_IDS = ["n%dc%dh%dw%dk%dr%ds%d_s%d" % c[:8] for c in SPECIAL]


def _with(passes):
    return dict(argvalues=[j for j, c in enumerate(CONV16_GRID) if passes in c[13]],
                ids=[g for g, c in zip(GRID_IDS, CONV16_GRID) if passes in c[13]])


# ------------------------------------------------------------------------------------------------------------------
# the entry points, as rrnet_amd.ops calls them
# ------------------------------------------------------------------------------------------------------------------
def _dev(a):
    from rrnet_amd import ops
    return ops.to_nhwc(torch.as_tensor(a).float().cuda())


def _host(t):
    return t.detach().cpu().double()


def _nan_nhwc(n, c, h, w):
    """An output buffer of NaNs: an element the launch leaves alone fails every comparison."""
    return torch.full((n, h, w, c), float("nan"), device="cuda").permute(0, 3, 1, 2)


def _word(t):
    """rr_absmax_bits of t into a zeroed device word."""
    from rrnet_amd import _C
    word = torch.zeros(2, dtype=torch.int32, device="cuda")
    _C.check(_C.fn("rr_absmax_bits")(_C.ptr(t), t.numel(), _C.ptr(word), _C.stream()), "rr_absmax_bits")
    return word


def _filter_image(math, flat, word):
    """The ready-made 16-bit image of a filter given in the memory order the kernel reads: its bf16 copy, or the two fp16 parts of
    rr_weight_split_f16 under the maximum `word`."""
    from rrnet_amd import _C
    if math == MATH_BF16:
        return flat.to(torch.bfloat16)
    out = torch.empty(2 * flat.numel(), dtype=torch.float16, device="cuda")
    _C.check(_C.fn("rr_weight_split_f16")(_C.ptr(flat), flat.numel(), _C.ptr(word), _C.ptr(out), _C.stream()), "rr_weight_split_f16")
    return out


def _ohwi(wd):
    return wd.permute(0, 2, 3, 1).contiguous().view(-1)           # [k][r][s][c]: the memory of an OHWI filter, flat


def _fprop(math, xd, wd, bd, geo, relu, slab=None, image=False):
    from rrnet_amd import _C, ops
    n, c, h, w, k, r, s, st, ph, pw = geo
    p, q = ops.out_hw(h, w, r, s, st, ph, pw)
    y = _nan_nhwc(n, k, p, q)
    if math == MATH_BF16:
        img = _filter_image(math, _ohwi(wd), None) if image else None
        tail = (_C.ptr(img),)
    else:
        wx, ww = _word(xd), _word(wd)
        img = _filter_image(math, _ohwi(wd), ww) if image else None
        tail = (_C.ptr(wx), _C.ptr(ww), _C.ptr(img))
    name = "rr_conv_fprop_" + LOWP_NAMES[math]
    _C.check(_C.fn(name)(_C.ptr(xd), _C.ptr(wd), _C.ptr(bd), _C.ptr(y), _C.ptr(slab), n, h, w, c, k, r, s, st, ph, pw, int(relu), *tail,
                         _C.stream()), name)
    torch.cuda.synchronize()
    return y


def _flip(wd):
    from rrnet_amd import _C
    wt = torch.empty(wd.numel(), dtype=torch.float32, device="cuda")
    _C.check(_C.fn("rr_weight_flip_transpose")(_C.ptr(wd), _C.ptr(wt), *wd.shape, _C.stream()), "rr_weight_flip_transpose")
    return wt


def _dgrad(math, gyd, wd, geo, out=None, image=False, link=None):
    """rr_conv_dgrad_s1_* (stride 1, on the flipped filter) or rr_conv_dgrad_s2_* (stride 2) -> dx; `out`: accumulate into it.
    link: (entry point stem, the producer's arguments in front of the arithmetic's own) of the _bnsum / _relubias forms."""
    from rrnet_amd import _C
    n, c, h, w, k, r, s, st, ph, pw = geo
    dx = _nan_nhwc(n, c, h, w) if out is None else out
    sfx = LOWP_NAMES[math]
    held = () if math == MATH_BF16 else (_word(gyd), _word(wd))      # (locals: the words must outlive the launch, not its argument list)
    words = tuple(_C.ptr(t) for t in held)
    if st == 1:
        wt = _flip(wd)
        img = _filter_image(math, wt, None if math == MATH_BF16 else held[1]) if image else None
        stem, mid = link or ("rr_conv_dgrad_s1_", ())
        tail = words if stem.endswith("relubias_") else words + (_C.ptr(img),)
        name = stem + sfx
        _C.check(_C.fn(name)(_C.ptr(gyd), _C.ptr(wt), _C.ptr(dx), n, h, w, c, k, r, s, ph, pw, int(out is not None), *mid, *tail, _C.stream()), name)
    else:
        wsub = torch.empty(wd.numel(), dtype=torch.float32, device="cuda")
        name = "rr_conv_dgrad_s2_" + sfx
        _C.check(_C.fn(name)(_C.ptr(gyd), _C.ptr(wd), _C.ptr(dx), n, h, w, c, k, r, s, ph, pw, int(out is not None), _C.ptr(wsub), *words,
                             _C.stream()), name)
    torch.cuda.synchronize()
    return dx


def _wgrad(math, xd, gyd, dw, geo, out_hw=(0, 0)):
    from rrnet_amd import _C
    n, c, h, w, k, r, s, st, ph, pw = geo
    held = () if math == MATH_BF16 else (_word(xd), _word(gyd))
    words = tuple(_C.ptr(t) for t in held)
    name = "rr_conv_wgrad_" + LOWP_NAMES[math]
    _C.check(_C.fn(name)(_C.ptr(xd), _C.ptr(gyd), _C.ptr(dw), n, h, w, c, k, r, s, st, ph, pw, *out_hw, *words, _C.stream()), name)
    torch.cuda.synchronize()
    return dw


# ------------------------------------------------------------------------------------------------------------------
# inputs, references, the judge
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(i, math):
    """Inputs (float32, CPU), their images and the float64 references of grid case i under `math`: computed once, shared by the
    tests of the case, never modified."""
    n, c, h, w, k, r, s, st, ph, pw, bias, relu, _, passes = CONV16_GRID[i]
    rng = np.random.default_rng(5000 + i)
    x = torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))
    wt = torch.from_numpy((rng.standard_normal((k, c, r, s)) / np.sqrt(c * r * s)).astype(np.float32))
    b = rng.standard_normal(k).astype(np.float32) if bias else None
    p, q = (h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1
    gy = torch.from_numpy(rng.standard_normal((n, k, p, q)).astype(np.float32))
    xi, wi = lowp_image(math, x), lowp_image(math, wt)
    cs = dict(x=x, w=wt, xi=xi, wi=wi, b=None)
    if "f" in passes:
        if relu:                                            # no output near 0: the kernel and the reference agree on every ReLU mask bit
            b = conv_bias_clear_of_zero(lowp_fprop_ref64(math, xi, wi, None, st, (ph, pw), False).numpy(), b)
        cs["b"] = None if b is None else torch.from_numpy(b)
        cs["y"] = lowp_fprop_ref64(math, xi, wi, cs["b"], st, (ph, pw), relu)
        if relu:
            assert float(cs["y"][cs["y"] > 0].min()) > 1e-3
            gy = gy * (cs["y"] > 0).float()                 # what the layer's backward hands to the kernels
    if passes != "f":
        cs["gy"], cs["gi"] = gy, lowp_image(math, gy)
        cs["dx"], cs["dw"] = lowp_grads_ref64(math, xi, wi, cs["gi"], st, (ph, pw))
    return cs


def _judge(tag, got, ref_all, idx, ref_s, max_seq, rms_seq, keep=None):
    """Prints the three ratios of one tensor and asserts the acceptance rule.  keep: boolean mask of the elements judged."""
    got, ref_all = got.numpy(), ref_all.numpy()
    assert np.abs(ref_s - ref_all[idx]).max() <= 1e-11 * max(np.abs(ref_s).max(), 1e-30), tag     # the gathered products are the reference's
    ga, ra = (got, ref_all) if keep is None else (got[keep], ref_all[keep])
    ratios = conv_error_ratios(got[idx], ref_s, max_seq, rms_seq, ga, ra)
    print("%s: max %.2f rms %.2f whole-tensor rms %.2f of the chained-fp32 yardstick (max %.2e rms %.2e), margin %g"
          % ((tag,) + ratios + (max_seq, rms_seq, CONV16_MARGIN)))
    assert conv_accepts(ratios, CONV16_MARGIN), (tag, ratios)
    return ratios


def _slab_for(n, p, q, k):
    from rrnet_amd import _C
    nb = _C.fn("rr_conv_stat_slab_bytes")(n, p, q, k)
    assert nb == -(-n * p * q // 128) * 2 * k * 8
    return torch.full((nb // 8,), SENTINEL, dtype=torch.float64, device="cuda")


def _check_slab(tag, slab, y, k, split):
    """The slab against the float64 column sums of the kernel's own y.  The fused epilogue of conv_igemm_bf16_kernel chains s1 / s2
    in fp32 over the TM * 16 rows a lane holds — 32 at the 128-column tile, 16 at the 64- and 32-column ones, NOT the 64 of
    conv.hip's kernel — and is double from there on; derived as the fp32 suite derives its 65 u / 66 u from 64 rows:
    |err| <= 33 u sum|y| and 34 u sum y^2 (32 additions, + the square's rounding).  Split-K (the colstats pass of conv.hip, all
    double): 1e-12 of the same sums, only row 0 of the slab filled."""
    rows = slab.view(-1, 2, k)
    yd = _host(y).permute(0, 2, 3, 1).reshape(-1, k)
    s1, s2, a1 = yd.sum(0), (yd * yd).sum(0), yd.abs().sum(0)
    got = rows.sum(0).cpu()
    if split:
        assert float(rows[1:].abs().max() if rows.shape[0] > 1 else 0.0) == 0.0, tag
        b1, b2 = 1e-12 * a1, 1e-12 * s2
    else:
        assert bool((rows != SENTINEL).all()), tag          # every tile row, every column written
        b1, b2 = 33 * U32 * a1, 34 * U32 * s2
    e1, e2 = (got[0] - s1).abs(), (got[1] - s2).abs()
    print("%s: slab (%s, %d rows) error over bound: sum y %.3f, sum y^2 %.3f" % (tag, "split-K" if split else "fused", rows.shape[0],
          float((e1 / (b1 + 1e-300)).max()), float((e2 / (b2 + 1e-300)).max())))
    assert bool((e1 <= b1).all()) and bool((e2 <= b2).all()), tag


# ------------------------------------------------------------------------------------------------------------------
# the grid
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", MATHS, ids=MATH_IDS)
@pytest.mark.parametrize("i", **_with("f"))
def test_fprop_against_fp64(i, math):
    """rr_conv_fprop_bf16 / _f16x3 with and without the statistics slab, on the fp32 filter and on its ready-made 16-bit image
    (which the entry point ignores where the label says so: C % 8 != 0, f16x3 below the 128-column tile)."""
    n, c, h, w, k, r, s, st, ph, pw, bias, relu, stats, _ = CONV16_GRID[i]
    cs = _case(i, math)
    idx = conv_sample_positions(tuple(cs["y"].shape), 7 * i + 1)
    yard = conv_yardstick(lowp_terms(math, "fprop", idx, cs["xi"], cs["wi"], st, (ph, pw), bias=cs["b"]), relu=relu)
    xd, wd = _dev(cs["x"]), _dev(cs["w"])
    bd = None if cs["b"] is None else cs["b"].cuda()
    for ws in stats:
        route = sorted(conv16_case_labels(math, CONV16_GRID[i], ws)["fprop"])
        for image in (False, True):
            tag = "%s fprop %s stats=%d image=%d %s" % (LOWP_NAMES[math], GRID_IDS[i], ws, image, route)
            slab = _slab_for(n, cs["y"].shape[2], cs["y"].shape[3], k) if ws else None
            y = _fprop(math, xd, wd, bd, CONV16_GRID[i][:10], relu, slab, image)
            if ws:
                _check_slab(tag, slab, y, k, "ksplit>1+stats" in route)
            _judge(tag, _host(y), cs["y"], idx, *yard)


@pytest.mark.parametrize("math", MATHS, ids=MATH_IDS)
@pytest.mark.parametrize("i", **_with("d"))
def test_dgrad_against_fp64(i, math):
    """rr_conv_dgrad_s1_* (fp32 flipped filter and its ready-made image) / rr_conv_dgrad_s2_*, each into a buffer of NaNs and
    accumulating into a non-zero tensor, whose value counts as one more term.  A stride-2 call whose parity classes are partly
    empty must zero them in the plain form and leave them alone in the accumulating one."""
    n, c, h, w, k, r, s, st, ph, pw = geo = CONV16_GRID[i][:10]
    cs = _case(i, math)
    rng = np.random.default_rng(6000 + i)
    base = torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))
    idx = conv_sample_positions((n, c, h, w), 7 * i + 2)
    yard = conv_yardstick(lowp_terms(math, "dgrad", idx, cs["gi"], cs["wi"], st, (ph, pw)), head=base.double().numpy()[idx])
    gyd, wd = _dev(cs["gy"]), _dev(cs["w"])
    route = sorted(conv16_case_labels(math, CONV16_GRID[i])["dgrad"])
    for image in ((False, True) if st == 1 else (False,)):
        tag = "%s dgrad %s image=%d %s" % (LOWP_NAMES[math], GRID_IDS[i], image, route)
        _judge(tag, _host(_dgrad(math, gyd, wd, geo, image=image)), cs["dx"], idx, *yard[:3])
        acc = _dev(base).clone(memory_format=torch.channels_last)
        _dgrad(math, gyd, wd, geo, out=acc, image=image)
        _judge(tag + " accumulate", _host(acc), cs["dx"] + base.double(), idx, *yard[3:])


@pytest.mark.parametrize("math", MATHS, ids=MATH_IDS)
@pytest.mark.parametrize("i", **_with("w"))
def test_wgrad_against_fp64(i, math):
    """conv_wgrad_bf16_kernel ADDS (float atomics into dw, also with one split): into zeros, and into a non-zero dw."""
    from rrnet_amd import ops
    n, c, h, w, k, r, s, st, ph, pw = geo = CONV16_GRID[i][:10]
    cs = _case(i, math)
    rng = np.random.default_rng(7000 + i)
    base = torch.from_numpy((rng.standard_normal((k, c, r, s)) * float(cs["dw"].std())).astype(np.float32))
    idx = conv_sample_positions((k, c, r, s), 7 * i + 3)
    yard = conv_yardstick(lowp_terms(math, "wgrad", idx, cs["xi"], cs["gi"], st, (ph, pw), rs=(r, s)), head=base.double().numpy()[idx])
    xd, gyd = _dev(cs["x"]), _dev(cs["gy"])
    tag = "%s wgrad %s %s" % (LOWP_NAMES[math], GRID_IDS[i], sorted(conv16_case_labels(math, CONV16_GRID[i])["wgrad"]))
    _judge(tag, _host(_wgrad(math, xd, gyd, ops.zeros_nhwc(k, c, r, s, "cuda"), geo)), cs["dw"], idx, *yard[:3])
    dw = _dev(base).clone(memory_format=torch.channels_last)
    _judge(tag + " into a non-zero dw", _host(_wgrad(math, xd, gyd, dw, geo)), cs["dw"] + base.double(), idx, *yard[3:])


@pytest.mark.parametrize("math", MATHS, ids=MATH_IDS)
def test_wgrad_output_size_override_is_padding_at_the_far_edge(math):
    """rr_conv_wgrad_* with out_h / out_w one larger than symmetric padding gives == the weight gradient on the input zero-padded
    by one more row and column at the far edge."""
    from rrnet_amd import ops
    n, c, h, w, k, r, s, st, ph, pw, oh, ow = CONV16_ASYM_WGRAD
    rng = np.random.default_rng(77)
    x = torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))
    gy = torch.from_numpy(rng.standard_normal((n, k, oh, ow)).astype(np.float32))
    far = ((oh - 1) * st + r - (h + 2 * ph), (ow - 1) * st + s - (w + 2 * pw))
    assert far == (1, 1)
    xi, gi = lowp_image(math, x), lowp_image(math, gy)
    wi = lowp_image(math, torch.zeros(k, c, r, s))
    dw_ref = lowp_grads_ref64(math, xi, wi, gi, st, (ph, pw), far=far)[1]
    idx = conv_sample_positions((k, c, r, s), 78)
    yard = conv_yardstick(lowp_terms(math, "wgrad", idx, xi, gi, st, (ph, pw), rs=(r, s)))
    dw = _wgrad(math, _dev(x), _dev(gy), ops.zeros_nhwc(k, c, r, s, "cuda"), CONV16_ASYM_WGRAD[:10], (oh, ow))
    route = sorted(conv16_wgrad_labels(math, *CONV16_ASYM_WGRAD[:10], out_hw=(oh, ow)))
    _judge("%s wgrad out_h/out_w override %s" % (LOWP_NAMES[math], route), _host(dw), dw_ref, idx, *yard)


# ------------------------------------------------------------------------------------------------------------------
# stride-1 data gradients that carry their producer's backward sums
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", MATHS, ids=MATH_IDS)
@pytest.mark.parametrize("j", range(len(CONV16_LINKS)), ids=["n%dc%dh%dw%d_k%d_%s_%s" % (sh + (k, ln, ms)) for sh, k, ln, ms in CONV16_LINKS])
def test_dgrad_with_fused_producer_sums(j, math):
    """rr_conv_dgrad_s1_bnsum_* / _relubias_* at the 64- and 32-column tiles (the 128-column form keeps its tests in
    test_conv_bf16_gpu.py / test_conv_split_gpu.py), and one split-K case where the plan hands the sums to the reduce pass behind
    the launch.  dx against float64 (relu_bias: masked, exact zeros under the mask).  The sums against float64 sums over the
    kernel's OWN dx on the CPU — sum d | sum d * xhat, d = dx * mask, xhat = (y - mean) * invstd; relu_bias: the column sums of the
    stored dx — within 1e-5 of their scale.  The mask is (z > 0) or the sign of y * scale + shift, which the kernels take from ONE
    fma (rr_bn_affine): its sign is that of the exact value, evaluated here in float64."""
    from rrnet_amd import _C
    (n, c, h, w), k, link, mask_src = CONV16_LINKS[j]
    geo = (n, c, h, w, k, 3, 3, 1, 1, 1)
    rng = np.random.default_rng(8000 + j)
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    gy, wt = f32(rng.standard_normal((n, k, h, w))), f32(rng.standard_normal((k, c, 3, 3)) / np.sqrt(9 * k))
    base = f32(rng.standard_normal((n, c, h, w)))
    py = f32(rng.standard_normal((n, c, h, w)) * 1.5 + 0.3)
    mean, var = py.double().mean((0, 2, 3)), py.double().var((0, 2, 3), unbiased=False)
    mean, invstd = mean.float(), (1.0 / torch.sqrt(var + 1e-5)).float()
    msc, msh = f32(rng.uniform(0.5, 1.5, c)) * invstd, f32(rng.standard_normal(c) * 0.3)
    z = torch.relu(f32(rng.standard_normal((n, c, h, w))))
    ch = lambda v: v.double().view(1, -1, 1, 1)
    mask = {"affine": py.double() * ch(msc) + ch(msh) > 0, "z": z > 0, None: torch.ones(n, c, h, w, dtype=torch.bool)}[mask_src]
    assert 0.2 < float(mask.double().mean()) <= 1.0
    gi, wi = lowp_image(math, gy), lowp_image(math, wt)
    dx_ref = lowp_grads_ref64(math, lowp_image(math, torch.zeros(n, c, h, w)), wi, gi, 1, (1, 1))[0]
    keep = mask.numpy() if link == "relu_bias" else None
    idx = conv_sample_positions((n, c, h, w), 9 * j + 1, keep=keep)
    yard = conv_yardstick(lowp_terms(math, "dgrad", idx, gi, wi, 1, (1, 1)), head=base.double().numpy()[idx])
    gyd, wd, pyd, zd = _dev(gy), _dev(wt), _dev(py), _dev(z)
    dev = lambda v: None if v is None else v.cuda()
    route = sorted(conv16_dgrad_labels(math, *geo, link=link))
    for accumulate in (False, True):
        slab = torch.full((_C.fn("rr_conv_stat_slab_bytes")(n, h, w, c) // 8,), SENTINEL, dtype=torch.float64, device="cuda")
        sums = torch.zeros(2 * c, dtype=torch.float64, device="cuda")
        if link == "bn":
            md, id_, scd, shd = dev(mean), dev(invstd), dev(msc if mask_src == "affine" else None), dev(msh if mask_src == "affine" else None)
            mid = (_C.ptr(pyd), _C.ptr(zd if mask_src == "z" else None), _C.ptr(md), _C.ptr(id_), _C.ptr(scd), _C.ptr(shd), _C.ptr(slab), _C.ptr(sums))
            entry = ("rr_conv_dgrad_s1_bnsum_", mid)
        else:
            entry = ("rr_conv_dgrad_s1_relubias_", (_C.ptr(zd), _C.ptr(slab), _C.ptr(sums)))
        out = _dev(base).clone(memory_format=torch.channels_last) if accumulate else None
        dx = _host(_dgrad(math, gyd, wd, geo, out=out, link=entry))
        tag = "%s dgrad link %s accumulate=%d %s" % (LOWP_NAMES[math], CONV16_LINKS[j], accumulate, route)
        full = dx_ref + base.double() if accumulate else dx_ref
        if link == "relu_bias":
            assert float(dx[~mask].abs().max()) == 0.0, tag                      # exact zeros under the mask
            _judge(tag, dx, full * mask, idx, *(yard[3:] if accumulate else yard[:3]), keep=keep)
        else:
            _judge(tag, dx, full, idx, *(yard[3:] if accumulate else yard[:3]))
        d = dx * mask
        xhat = (py.double() - ch(mean)) * ch(invstd)
        want = torch.cat([d.sum((0, 2, 3)), (d * xhat).sum((0, 2, 3))])
        got = sums.cpu()
        rows = c if link == "relu_bias" else 2 * c                                # (relu_bias: the second row is not meaningful)
        err, scale = float((got[:rows] - want[:rows]).abs().max()), float(want[:rows].abs().max())
        print("%s: sums error %.2e of their scale (bound 1e-5)" % (tag, err / scale))
        assert err <= 1e-5 * scale, (tag, err, scale)


# ------------------------------------------------------------------------------------------------------------------
# inputs where convolution kernels go wrong
# ------------------------------------------------------------------------------------------------------------------
def _run_all(math, x, wt, gy, cfg):
    """Every route of one shape as CPU float64: y with and without statistics and on the filter image, dx, dw into zeros."""
    from rrnet_amd import ops
    n, c, h, w, k, r, s, st, ph, pw = cfg
    p, q = (h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1
    xd, wd, gyd = _dev(x), _dev(wt), _dev(gy)
    out = {"y stats=0": _host(_fprop(math, xd, wd, None, cfg, False)),
           "y stats=1": _host(_fprop(math, xd, wd, None, cfg, False, _slab_for(n, p, q, k))),
           "y image": _host(_fprop(math, xd, wd, None, cfg, False, image=True)),
           "dx": _host(_dgrad(math, gyd, wd, cfg)),
           "dw": _host(_wgrad(math, xd, gyd, ops.zeros_nhwc(k, c, r, s, "cuda"), cfg))}
    return out


def _exact_in(math, t):
    """True when every value of t is its own image: exact in bf16, or in ONE fp16 value after the tensor's scale (lo = 0)."""
    parts, scale = lowp_image(math, t)
    return bool(np.array_equal(parts[0] / scale, t.double().numpy())) and all(not p.any() for p in parts[1:])


def _refs(math, x, wt, gy, cfg, seed, bits=(None, None, None), keep=None):
    """{"y" | "dx" | "dw": (reference, sample positions, sampled sums, max_seq, rms_seq)} from the images of x, w, gy."""
    n, c, h, w, k, r, s, st, ph, pw = cfg
    xi, wi, gi = (lowp_image(math, t, b) for t, b in zip((x, wt, gy), bits))
    dx, dw = lowp_grads_ref64(math, xi, wi, gi, st, (ph, pw))
    refs = {"y": (lowp_fprop_ref64(math, xi, wi, None, st, (ph, pw), False), "fprop", xi, wi), "dx": (dx, "dgrad", gi, wi), "dw": (dw, "wgrad", xi, gi)}
    out = {}
    for kind, (ref, pas, a, b) in refs.items():
        idx = conv_sample_positions(tuple(ref.shape), seed, keep=None if keep is None else keep[kind])
        out[kind] = (ref, idx) + conv_yardstick(lowp_terms(math, pas, idx, a, b, st, (ph, pw), rs=(r, s)))
    return out


@pytest.mark.parametrize("math", MATHS, ids=MATH_IDS)
@pytest.mark.parametrize("cfg", SPECIAL, ids=SPECIAL_IDS)
def test_all_ones_count_the_taps_inside_the_image(cfg, math):
    """x = w = dy = 1 — exact in bf16; in f16x3 it lands on hi = 2^14, lo = 0: y = C x (taps inside the image), dx = K x ((output,
    tap) pairs reaching the pixel), dw = N x (outputs whose tap lies inside) — closed forms, bit for bit."""
    n, c, h, w, k, r, s, st, ph, pw = cfg
    p, q = (h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1
    parts, scale = lowp_image(math, torch.ones(4))
    assert float(parts[0][0]) == (1.0 if math == MATH_BF16 else 2.0 ** 14) and all(not pt.any() for pt in parts[1:])
    in_h, reach_h, valid_h = conv_tap_counts(h, p, r, st, ph)
    in_w, reach_w, valid_w = conv_tap_counts(w, q, s, st, pw)
    want = {"y": torch.from_numpy(c * np.outer(in_h, in_w)).double().expand(n, k, p, q),
            "dx": torch.from_numpy(k * np.outer(reach_h, reach_w)).double().expand(n, c, h, w),
            "dw": torch.from_numpy(n * np.outer(valid_h, valid_w)).double().expand(k, c, r, s)}
    assert len(np.unique(np.outer(in_h, in_w))) > 1 and len(np.unique(np.outer(reach_h, reach_w))) > 1
    for name, got in _run_all(math, torch.ones(n, c, h, w), torch.ones(k, c, r, s), torch.ones(n, k, p, q), cfg).items():
        ref = want[name.split()[0]]
        assert torch.equal(got, ref), (name, float((got - ref).abs().max()), int((got != ref).sum()))


@pytest.mark.parametrize("math", MATHS, ids=MATH_IDS)
@pytest.mark.parametrize("cfg", SPECIAL, ids=SPECIAL_IDS)
def test_exact_cancellation_and_signed_zeros(cfg, math):
    """The construction of the fp32 suite's test of this name: operands +-2^e, e in [-2, 2] (and +-0), paired over the channels so
    that the products of every tap cancel in pairs, one planted element (+8) in x and in dy.  Every value is exact in bf16, and in
    ONE fp16 value after the tensor's scale (asserted on the host), so every partial sum — in any order, over any split, scaled or
    not — is exact in fp32: exactly 0 outside the planted fields, the planted outputs and all of dw bit for bit."""
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
    wt = mag * sign
    x[0, 5, h // 2, w // 3] += 8.0
    gy[n - 1, 2, p // 2, q // 2] += 8.0
    x, wt, gy = (torch.from_numpy(a.astype(np.float32)) for a in (x, wt, gy))
    assert _exact_in(math, x) and _exact_in(math, wt) and _exact_in(math, gy)
    y, dx, dw = conv_ref64(x, wt, None, st, (ph, pw), False, gy)
    assert 0 < int((y != 0).sum()) <= n * k * r * s and 0 < int((dx != 0).sum()) <= n * c * r * s
    for name, got in _run_all(math, x, wt, gy, cfg).items():
        ref = {"y": y, "dx": dx, "dw": dw}[name.split()[0]]
        assert torch.equal(got, ref), (name, float((got - ref).abs().max()), int((got != ref).sum()))
        print("%s %s %s: bit-exact, %d non-zero of %d" % (LOWP_NAMES[math], SPECIAL_IDS[SPECIAL.index(cfg)], name, int((ref != 0).sum()), ref.numel()))


@pytest.mark.parametrize("math", MATHS, ids=MATH_IDS)
@pytest.mark.parametrize("cfg", SPECIAL, ids=SPECIAL_IDS)
def test_dynamic_range_across_channels(cfg, math):
    """One input channel scaled by 1e4 with its filter taps scaled by 1e-4, another the opposite way.  bf16: the fp32 suite's rule on
    the rounded operands.  f16x3: against the split reference, which models the per-tensor scale (the small channels keep fewer
    bits: that is the arithmetic's contract, not the kernel's error)."""
    n, c, h, w, k, r, s, st, ph, pw = cfg
    rng = np.random.default_rng(42)
    p, q = (h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1
    x = rng.standard_normal((n, c, h, w))
    wt = rng.standard_normal((k, c, r, s)) / np.sqrt(c * r * s)
    x[:, 0] *= 1e4; wt[:, 0] *= 1e-4; x[:, 1] *= 1e-4; wt[:, 1] *= 1e4
    x, wt = torch.from_numpy(x.astype(np.float32)), torch.from_numpy(wt.astype(np.float32))
    gy = torch.from_numpy(rng.standard_normal((n, k, p, q)).astype(np.float32))
    refs = _refs(math, x, wt, gy, cfg, 43)
    for name, got in _run_all(math, x, wt, gy, cfg).items():
        _judge("%s dynamic range %s %s" % (LOWP_NAMES[math], SPECIAL_IDS[SPECIAL.index(cfg)], name), got, *refs[name.split()[0]])


@pytest.mark.parametrize("math", MATHS, ids=MATH_IDS)
@pytest.mark.parametrize("cfg", SPECIAL, ids=SPECIAL_IDS)
def test_non_finite_inputs_stay_visible_and_do_not_leak(cfg, math):
    """One NaN and one +inf in x (fprop), in dy (dgrad, wgrad): exactly the outputs whose receptive field holds one are non-finite.
    bf16: every other output still meets the bound.  f16x3: the infinite maximum collapses that tensor's scale to 2^-114 (every
    finite value's image is 0), so the other outputs are judged against the split reference built with that same scale — and
    must be finite."""
    n, c, h, w, k, r, s, st, ph, pw = cfg
    rng = np.random.default_rng(44)
    p, q = (h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1
    x = torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))
    wt = torch.from_numpy((rng.standard_normal((k, c, r, s)) / np.sqrt(c * r * s)).astype(np.float32))
    gy = torch.from_numpy(rng.standard_normal((n, k, p, q)).astype(np.float32))
    xpos = [(0, 5, h // 4, w // 2), (n - 1, c - 3, (3 * h) // 4, w // 4)]
    gpos = [(0, 3, 1, q // 2), (n - 1, k - 2, p // 2, 1)]       # interior: every tap of the marked dy pixels lies inside x
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
    hit = {"y": (conv_ref64(xmark, ones, None, st, (ph, pw), False)[0] > 0).expand(n, k, p, q),
           "dx": (conv_ref64(torch.zeros(n, 1, h, w), ones, None, st, (ph, pw), False, gmark)[1] > 0).expand(n, c, h, w),
           "dw": torch.zeros(k, c, r, s, dtype=torch.bool)}
    hit["dw"][gpos[0][1]] = hit["dw"][gpos[1][1]] = True
    xz, gz = x.clone(), gy.clone()                          # the reference of the untouched outputs: the marked elements as 0
    xz[xpos[0]] = xz[xpos[1]] = 0.0
    gz[gpos[0]] = gz[gpos[1]] = 0.0
    keep = {kind: (~m).numpy() for kind, m in hit.items()}
    collapsed = INF_BITS if math == MATH_F16X3 else None
    refs_y = _refs(math, xz, wt, gy, cfg, 45, bits=(collapsed, None, None), keep=keep)       # x holds the non-finite values
    refs_g = _refs(math, x, wt, gz, cfg, 45, bits=(None, None, collapsed), keep=keep)        # dy holds them
    got_y, got_g = _run_all(math, xbad, wt, gy, cfg), _run_all(math, x, wt, gbad, cfg)
    for name in got_y:
        kind = name.split()[0]
        got = got_y[name] if kind == "y" else got_g[name]
        ref, idx, ref_s, mx, rms = (refs_y if kind == "y" else refs_g)[kind]
        bad = ~torch.isfinite(got)
        assert torch.equal(bad, hit[kind]), (name, int(bad.sum()), int(hit[kind].sum()), int((bad != hit[kind]).sum()))
        _judge("%s non-finite %s %s (%d non-finite)" % (LOWP_NAMES[math], SPECIAL_IDS[SPECIAL.index(cfg)], name, int(bad.sum())),
               torch.where(bad, torch.zeros_like(got), got), ref * (~hit[kind]), idx, ref_s, mx, rms, keep=keep[kind])

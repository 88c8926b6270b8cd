"""GPU: RetinaNet's own kernels (csrc/retina.hip: anchor assignment, focal / smooth-L1 losses and their gradients, box decode,
3x3/2 max-pool, bilinear upsample-add) and the RetinaNet convolution shapes on the existing convolution entries, against the
plain-torch restatements of tests/retina_cases.py evaluated in float64 on the CPU.

Tolerances are never read off the kernel.  Discrete results (states, argmax, positive counts, kept anchors, classes, pool
taps) must be equal.  Values follow the measured rule of tests/test_criterion_gpu.py: at most 4x the error of the same
restatement evaluated in float32 on the CPU against float64, with a floor of 2 u max|ref|, u = 2^-24; gradients are exactly
0 where float64 has 0.  Max-pool is bit-equal to ATen's CPU result (its backward where at most two terms meet, else within
(n + 1) u sum|term|).  The convolutions follow tests/test_conv_fp64_gpu.py's rule (helpers.conv_accepts).
Every test prints its figures (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

import retina_cases as rc
from helpers import (conv_accepts, conv_error_ratios, conv_ref64, conv_sample_positions, conv_terms, conv_yardstick)

pytestmark = pytest.mark.gpu
U32 = rc.U32
CL = torch.channels_last


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def measured_tol(err32, ref):
    return max(4.0 * float(err32), 2.0 * U32 * float(np.abs(ref).max(initial=0.0)))


def _judge(tag, got, ref64, ref32):
    got, ref64, ref32 = (np.asarray(a, dtype=np.float64) for a in (got, ref64, ref32))
    err32 = float(np.abs(ref32 - ref64).max(initial=0.0))
    tol = measured_tol(err32, ref64)
    err = float(np.abs(got - ref64).max(initial=0.0))
    print("  %-28s n=%-8d max|ref| %.3g  fp32 err %.3g  kernel err %.3g  tol %.3g"
          % (tag, got.size, float(np.abs(ref64).max(initial=0.0)), err32, err, tol))
    assert err <= tol, (tag, err, tol)


# --------------------------------------------------------------------------------------------------------------------
# criterion
# --------------------------------------------------------------------------------------------------------------------
CRIT_CASES = {                      # kind, image size, classes, seed, saturated logits
    "base_64x64": ("base", (64, 64), 10, 21, False),
    "base_40x104": ("base", (40, 104), 10, 22, False),
    "duplicate": ("duplicate", (64, 64), 10, 23, False),
    "bad_class": ("bad_class", (64, 64), 10, 24, False),
    "one_class": ("base", (72, 56), 1, 25, False),
    "saturated": ("base", (64, 64), 10, 26, True),
}
CRIT_CASES.update(rc.CRIT_ROUTE_CASES)   # every launch route; tests/test_retina_host.py proves each input sits on its route
W_CLS, W_LOC = 0.7, 1.3             # the two upstream scalars of the backward


@functools.lru_cache(maxsize=None)
def _crit_case(name):
    kind, size, classes, seed, sat = CRIT_CASES[name]
    annos, anchors = rc.criterion_inputs(kind, size, classes)
    loc, logits = rc.criterion_preds(annos.shape[0], anchors.shape[0], classes, seed, saturate=sat)
    r64 = rc.criterion_with_grads(loc, logits, annos, anchors, classes, torch.float64, W_CLS, W_LOC)
    r32 = rc.criterion_with_grads(loc, logits, annos, anchors, classes, torch.float32, W_CLS, W_LOC)
    return annos, anchors, loc, logits, classes, r64, r32


def test_criterion_inputs_have_the_stated_properties():
    """Checked on the float64 side before any kernel is looked at: anchor counts, the positive / ignored / negative split, the
    boxes that win nothing, the distance of every best IoU from the two thresholds, no tied annotations on a positive."""
    for size, count in rc.ANCHOR_COUNTS.items():
        assert rc.anchors_of(size).shape == (count, 4)
    for size, split in (((64, 64), (18, 25, 713)), ((40, 104), (16, 20, 810))):
        asg = rc.assign(rc.criterion_batch("base")[:1], rc.anchors_of(size), 10, torch.float64)
        st, best, iou = asg["state"][0], asg["max_iou"][0], asg["iou"][0]
        assert (int((st == 1).sum()), int((st == -1).sum()), int((st == 0).sum())) == split
        winners = set(asg["argmax"][0][st == 1].tolist())
        assert 2 not in winners and 3 not in winners                       # the padding row and the 3x4 box
        assert float((best - 0.4).abs().min()) > 1e-6 and float((best - 0.5).abs().min()) > 1e-6
        tied = (iou == best[None, :]).sum(dim=0) > 1
        assert not bool((tied & (st == 1)).any())


@pytest.mark.parametrize("name", list(CRIT_CASES))
def test_retina_criterion_vs_fp64(name):
    """rr_retina_assign + rr_retina_loss_fwd / _bwd through RF.retina_criterion, backward driven by 0.7 cls + 1.3 loc.
    Measured (float32 restatement on the CPU / kernel on an MI355X, both against float64), base_64x64: targets 8.6e-7 /
    8.6e-7 (max 2.89); cls_loss 2.7e-6 / 5.0e-6 of 103.7 (tolerance 1.2e-5); loc_loss 4.3e-8 / 1.7e-8 of 0.732; d loc 1.2e-8
    / 1.2e-8 (max 6.0e-3); d logits for 1e-3 <= p <= 0.99 1.4e-8 / 1.6e-8 (max 0.066), for p > 0.99 8.5e-9 / 1.2e-8.  The
    closest case is one_class: cls_loss 6.0e-7 / 1.3e-6 of 13.4 against a tolerance of 2.4e-6.  saturated: the float32 upper
    clamp 1 - 2^-23 is not float64's 1 - 1e-7, which moves the loss of 1747 by 18.2 in the restatement and the kernel alike.
    The routes of rc.CRIT_ROUTE_CASES, cls_loss: c4 2.1e-6 / 1.7e-6 of 41.8; c8 6.4e-6 / 1.3e-6 of 86.8; c12 1.3e-5 / 2.0e-6 of
    130; c12_swapped 1.2e-5 / 3.7e-6 of 128; c8_saturated 15.6 / 15.6 of 1490 (the clamp again); many_256 4.8e-8 / 1.9e-7 of
    2.14 (tolerance 2.6e-7, the closest of the new cases); many_257 2.9e-7 / 5.5e-8; many_513 5.4e-8 / 5.4e-8 of 2.08;
    exact_thresholds 2.6e-8 / 3.3e-8 of 0.776; one_block_100 1.4e-7 / 9.9e-8; one_anchor 3.6e-7 / 1.2e-7 of 3.60; block_cap
    5.4e-6 / 2.2e-6 of 77.8 with 518 positives, its last 13 rows d logits 3.7e-11 / 3.6e-11 (max 3.0e-4) and d loc 1.1e-10 /
    1.1e-10.  Every discrete result of every case is equal."""
    from rrnet_amd import functional as RF
    from rrnet_amd import ops
    annos, anchors, loc, logits, classes, r64, r32 = _crit_case(name)
    a64 = r64["asg"]
    print("\ncriterion %s: B=%d A=%d C=%d npos %s" % (name, logits.shape[0], logits.shape[1], classes, a64["npos"].tolist()))
    if CRIT_CASES[name][0] in ("base", "swapped"):
        assert int(a64["npos"][1]) == 0 and int(a64["npos"][0]) > 0        # one image without annotations
    an_d, ad = torch.from_numpy(annos).cuda(), anchors.cuda()
    before = an_d.clone()
    asg = ops.retina_assign(an_d, ad, classes)
    assert torch.equal(an_d, before)                                       # the annotations are not turned into xyxy in place
    assert np.array_equal(asg["state"].cpu().numpy(), a64["state"].numpy())
    assert np.array_equal(asg["argmax"].cpu().numpy(), a64["argmax"].numpy())
    assert np.array_equal(asg["npos"].cpu().numpy(), a64["npos"].numpy())
    assert np.array_equal(asg["cls"].cpu().numpy(), a64["cls"].numpy())
    if name == "exact_thresholds":                                         # 0.5 is positive, 2/5 is not below 0.4
        assert asg["state"][0].tolist() == rc.EXACT_STATE and asg["argmax"][0].tolist() == rc.EXACT_ARGMAX
    if name == "many_513":                                                 # rows 3 and 300 tie across a chunk boundary: 3 wins
        first, twin = rc.MANY_DUPLICATE
        got_arg, got_state = asg["argmax"].cpu(), asg["state"].cpu()
        assert int(((got_arg[0] == first) & (got_state[0] == 1)).sum()) > 0 and not bool((got_arg[0] == twin).any())
        assert int(((got_arg[1] == 512 - twin) & (got_state[1] == 1)).sum()) > 0 and not bool((got_arg[1] == 512 - first).any())
    if name == "bad_class":
        hit = (a64["argmax"] == 0) & (a64["state"] == 1)
        assert bool(hit.any()) and int(a64["cls"][hit].abs().max()) == 0    # positives of the bad box carry no class
    _judge("max_iou", _np(asg["max_iou"]), a64["max_iou"].numpy(), r32["asg"]["max_iou"].numpy())
    _judge("target", _np(asg["target"]), a64["target"].numpy(), r32["asg"]["target"].numpy())

    lo = torch.from_numpy(loc).cuda().requires_grad_()
    lg = torch.from_numpy(logits).cuda().requires_grad_()
    cls_loss, loc_loss = RF.retina_criterion(lo, lg, an_d, ad, classes)
    (W_CLS * cls_loss + W_LOC * loc_loss).backward()
    again = RF.retina_criterion(lo.detach(), lg.detach(), an_d, ad, classes)
    assert float(again[0]) == float(cls_loss.detach()) and float(again[1]) == float(loc_loss.detach())   # bit-identical run to run
    _judge("cls_loss", [float(cls_loss.detach())], [r64["cls_loss"]], [r32["cls_loss"]])
    _judge("loc_loss", [float(loc_loss.detach())], [r64["loc_loss"]], [r32["loc_loss"]])

    got_dl, got_dg = _np(lo.grad), _np(lg.grad)
    assert np.all(got_dl[r64["dloc"] == 0.0] == 0.0) and np.all(got_dg[r64["dlogits"] == 0.0] == 0.0)
    ignored = (a64["state"] == -1).numpy()
    assert np.all(got_dg[ignored] == 0.0) and np.all(got_dl[(a64["state"] != 1).numpy()] == 0.0)
    if CRIT_CASES[name][4]:
        sat = np.abs(logits) == 40.0
        assert sat.any() and np.all(got_dg[sat] == 0.0)                    # the clamp passes no gradient
    _judge("d loc", got_dl, r64["dloc"], r32["dloc"])
    p = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
    for tag, sel in (("p<1e-3", p < 1e-3), ("1e-3<=p<=0.99", (p >= 1e-3) & (p <= 0.99)), ("p>0.99", p > 0.99)):
        if sel.any():
            _judge("d logits " + tag, got_dg[sel], r64["dlogits"][sel], r32["dlogits"][sel])
    if name == "block_cap":
        # the three bands above cover every element; the rows that only the fifth turn of the stride loop reaches, on their own
        last = (4 * 1024 * 256) // classes
        assert last < logits.shape[1] and np.count_nonzero(r64["dlogits"][:, last:]) and np.count_nonzero(r64["dloc"][:, last:])
        _judge("d logits, last %d rows" % (logits.shape[1] - last), got_dg[:, last:], r64["dlogits"][:, last:], r32["dlogits"][:, last:])
        _judge("d loc, last rows", got_dl[:, last:], r64["dloc"][:, last:], r32["dloc"][:, last:])


# --------------------------------------------------------------------------------------------------------------------
# max-pool
# --------------------------------------------------------------------------------------------------------------------
POOL_MAPS = [(1, 1), (2, 3), (7, 9), (8, 8)]


def _pool_input(kind, n, c, h, w, seed):
    g = np.random.default_rng(seed)
    if kind == "constant":
        return np.full((n, c, h, w), 0.75, dtype=np.float32)
    x = g.standard_normal((n, c, h, w)).astype(np.float32)
    if kind == "negative":
        x = -np.abs(x) - 1.0
    if kind == "coarse":                                                    # few distinct values: many ties inside a window
        x = np.round(x * 1.5).astype(np.float32)
    return x


@pytest.mark.parametrize("kind", ["normal", "constant", "negative", "coarse"])
@pytest.mark.parametrize("c", [3, 4, 64])
@pytest.mark.parametrize("hw", POOL_MAPS)
def test_maxpool3x3s2_vs_aten(hw, c, kind):
    from rrnet_amd import ops
    h, w = hw
    n = 2
    x = torch.from_numpy(_pool_input(kind, n, c, h, w, 100 * h + w + c))
    xr = x.clone().requires_grad_()
    y_ref, tap_ref = rc.maxpool(xr)
    g = np.random.default_rng(7)
    dy = torch.from_numpy(g.standard_normal(tuple(y_ref.shape)).astype(np.float32))
    y_ref.backward(dy)
    xd = ops.to_nhwc(x.cuda())
    y, idx = ops.maxpool3x3s2_fwd(xd)
    assert tuple(y.shape) == tuple(y_ref.shape)
    assert np.array_equal(y.cpu().numpy().view(np.uint32), y_ref.detach().numpy().view(np.uint32))
    assert np.array_equal(idx.cpu().numpy(), tap_ref.numpy())                  # ATen's choice, ties included
    if kind == "negative":
        assert float(y.max()) < 0.0                                            # padding did not enter as 0
    dx = ops.maxpool3x3s2_bwd(ops.to_nhwc(dy.cuda()), idx, tuple(x.shape)).cpu()
    # how many windows name each input element, and the sum of |dy| over them
    ones = torch.ones_like(y_ref.detach()).requires_grad_(False)
    xc = x.clone().requires_grad_()
    rc.maxpool(xc)[0].backward(ones)
    count = xc.grad
    xa = x.clone().requires_grad_()
    rc.maxpool(xa)[0].backward(dy.abs())
    mass = xa.grad
    ref = xr.grad
    few = count <= 2
    assert np.array_equal(dx[few].numpy().view(np.uint32), ref[few].numpy().view(np.uint32))
    bound = (count + 1) * U32 * mass
    assert bool(((dx - ref).abs().double() <= bound.double())[~few].all())
    print("\nmaxpool %s c=%d %s: windows per element up to %d, backward max err %.3g"
          % (hw, c, kind, int(count.max()), float((dx - ref).abs().max())))


def test_maxpool_propagates_nan():
    from rrnet_amd import ops
    x = torch.from_numpy(_pool_input("normal", 1, 4, 7, 9, 5))
    x[0, 1, 3, 4] = float("nan")
    y_ref, tap_ref = rc.maxpool(x)
    y, idx = ops.maxpool3x3s2_fwd(ops.to_nhwc(x.cuda()))
    assert np.array_equal(torch.isnan(y).cpu().numpy(), torch.isnan(y_ref).numpy()) and bool(torch.isnan(y).any())
    assert np.array_equal(idx.cpu().numpy(), tap_ref.numpy())


# --------------------------------------------------------------------------------------------------------------------
# bilinear upsample-add
# --------------------------------------------------------------------------------------------------------------------
BILINEAR_CASES = [((1, 1), (1, 1)), ((3, 4), (5, 7)), ((4, 4), (8, 8)), ((5, 5), (9, 9)), ((4, 7), (7, 13)),
                  # one source pixel feeds everything; ratio above 4; shrinking; shrinking by a non-integer ratio; same size
                  ((1, 1), (4, 5)), ((2, 3), (9, 10)), ((8, 9), (4, 3)), ((7, 13), (4, 7)), ((5, 5), (5, 5))]


def _bilinear_ref(x, y, dout, dtype):
    xt = torch.from_numpy(x).to(dtype).requires_grad_()
    yt = torch.from_numpy(y).to(dtype).requires_grad_()
    out = rc.bilinear_add(xt, yt)
    out.backward(torch.from_numpy(dout).to(dtype))
    return [t.detach().numpy().astype(np.float64) for t in (out, xt.grad, yt.grad)]


@pytest.mark.parametrize("c", [256, 3, 4, 6])
@pytest.mark.parametrize("src,dst", BILINEAR_CASES)
def test_bilinear_add_vs_fp64(src, dst, c):
    """out and d x by the measured rule; d y is dout itself; at equal sizes out = y + x and d x = dout bit for bit; the
    adjoint identity sum(dout (out - y)) = sum(x d x): both sides summed in float64 from the kernel's results must agree
    within the sum of the two sides' bounds, each the measured rule's for that side (4x the float32 restatement's error of
    that sum, floor 2 u |sum|); the float64 restatement's own two sides agree to 1e-12.  Each side's distance from float64
    is printed, not asserted: one sum's float32 error is a single random number and can be small by chance (with C = 3,
    (1,1) -> (4,5): kernel 1.3e-7 / 4.6e-7, float32 restatement 0.9e-7 / 1.1e-7; (2,3) -> (9,10): 1.9e-6 / 2.7e-6 against
    1.8e-7 / 4.3e-7), while every element of out and d x is within its bound.
    Measured (float32 restatement on the CPU / kernel on an MI355X, both against float64), C = 256: (2,3) -> (9,10) out 7.3e-7
    / 5.5e-7, d x 2.8e-6 / 2.5e-6 (max 11.1), the two sides 2.7e-5 apart against a bound of 7.1e-5; (8,9) -> (4,3) out 3.0e-7
    / 3.0e-7, d x 0 / 0 (every weight is 1/4), sides 8.0e-6 apart (bound 3.6e-5); (7,13) -> (4,7) out 1.8e-6 / 1.8e-6, d x 1.1e-6
    / 1.1e-6, sides 1.0e-5 apart (bound 2.0e-4).  The two sides come closest to their bound at (5,5) -> (9,9), C = 256 (2.1e-5
    of 2.6e-5) and at (1,1) -> (4,5), C = 3 (6.0e-7 of 8.0e-7)."""
    from rrnet_amd import functional as RF
    g = np.random.default_rng(31 * src[0] + dst[1] + c)
    n = 2
    x = g.standard_normal((n, c) + src).astype(np.float32)
    y = g.standard_normal((n, c) + dst).astype(np.float32)
    dout = g.standard_normal((n, c) + dst).astype(np.float32)
    r64, r32 = _bilinear_ref(x, y, dout, torch.float64), _bilinear_ref(x, y, dout, torch.float32)
    xd = torch.from_numpy(x).cuda().contiguous(memory_format=CL).requires_grad_()
    yd = torch.from_numpy(y).cuda().contiguous(memory_format=CL).requires_grad_()
    out = RF.bilinear_add(xd, yd)
    out.backward(torch.from_numpy(dout).cuda().contiguous(memory_format=CL))
    print("\nbilinear-add %s -> %s c=%d" % (src, dst, c))
    _judge("out", _np(out), r64[0], r32[0])
    _judge("d x", _np(xd.grad), r64[1], r32[1])
    assert np.array_equal(yd.grad.cpu().numpy(), dout)                          # d y is dout itself
    if src == dst:
        assert np.array_equal(out.detach().cpu().numpy().view(np.uint32), (y + x).view(np.uint32))
        assert np.array_equal(xd.grad.cpu().numpy().view(np.uint32), dout.view(np.uint32))
    x64, y64, d64 = (a.astype(np.float64) for a in (x, y, dout))
    sides = [[float((d64 * (o - y64)).sum()), float((x64 * dx).sum())] for o, dx in ((_np(out), _np(xd.grad)), r64[:2], r32[:2])]
    assert abs(sides[1][0] - sides[1][1]) <= 1e-12 * float(np.abs(d64 * (r64[0] - y64)).sum())
    tol = sum(measured_tol(abs(s32 - s64), np.array([s64])) for s64, s32 in zip(sides[1], sides[2]))
    gap = abs(sides[0][0] - sides[0][1])
    print("  adjoint: sum(dout (out - y)) %.9g  sum(x dx) %.9g  differ by %.3g (float32 restatement %.3g), tol %.3g;  each side off "
          "float64 by %.3g / %.3g (float32 restatement %.3g / %.3g)"
          % (sides[0][0], sides[0][1], gap, abs(sides[2][0] - sides[2][1]), tol, abs(sides[0][0] - sides[1][0]),
             abs(sides[0][1] - sides[1][1]), abs(sides[2][0] - sides[1][0]), abs(sides[2][1] - sides[1][1])))
    assert gap <= tol, (gap, tol)


# --------------------------------------------------------------------------------------------------------------------
# decode
# --------------------------------------------------------------------------------------------------------------------
def _decode_inputs(a, c, seed, mode, b=2, thr=0.1):
    g = np.random.default_rng(seed)
    logits = (g.standard_normal((b, a, c)) * 2.0 - 2.5).astype(np.float32)
    if mode == "none":
        logits = (-5.0 - np.abs(logits)).astype(np.float32)
    if mode == "all":
        logits[..., 0] = 3.0
    if mode == "mixed" and c > 2:
        # first-maximum ties: on every third anchor a later class repeats the row's maximum
        top = logits.max(axis=2)
        first = logits.argmax(axis=2)
        rows = np.arange(a) % 3 == 0
        for i in range(b):
            sel = np.nonzero(rows & (first[i] < c - 1))[0]
            logits[i, sel, c - 1] = top[i, sel]
    if mode == "batch3":                                                        # some; the middle image nothing; the last everything
        logits[0] -= np.float32(2.0)
        logits[1] = (-5.0 - np.abs(logits[1])).astype(np.float32)
        logits[2, :, c - 1] = 3.0
    p = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
    logits[np.abs(p - thr) < 1e-5] = -3.0                                       # nothing within 1e-5 of the threshold
    if mode == "special":
        for i in range(b):
            for kind, rows in SPECIAL_ROWS.items():
                r = rows[i]
                if kind == "nan_all":
                    logits[i, r, :] = np.nan
                elif kind == "nan_first":                                       # NaN in class 0, class 4 far above the threshold
                    logits[i, r, 0], logits[i, r, 4] = np.nan, 6.0
                elif kind == "nan_later":                                       # NaN in class 3, class 5 far above the threshold
                    logits[i, r, 3], logits[i, r, 5] = np.nan, 6.0
                elif kind == "inf":                                             # probability exactly 1, class 3
                    logits[i, r, 2] = np.inf
    loc = (g.standard_normal((b, a, 4)) * 0.8).astype(np.float32)
    xy = g.uniform(0, 400, (a, 2))
    wh = g.uniform(4, 120, (a, 2))
    anchors = np.concatenate([xy, xy + wh], axis=1).astype(np.float32)
    return logits, loc, anchors


# mode "special" (A = 300, C = 10): the rows of image 0 / image 1 that carry a NaN or an infinite logit; they sit in the first,
# the second and the last wave of the first pass over 256 anchors and in the second pass, with kept rows on either side
SPECIAL_ROWS = {"nan_all": (5, 255), "nan_first": (70, 256), "nan_later": (130, 299), "inf": (64, 257)}
DECODE_CASES = [pytest.param(a, mode, 10, None, id="%d-%s" % (a, mode)) for a, mode in
                [(300, "none"), (1, "all"), (63, "mixed"), (64, "mixed"), (65, "mixed"), (1025, "mixed"), (777, "all")]]
DECODE_CASES += [pytest.param(a, "mixed", c, None, id="%d-mixed-c%d" % (a, c)) for c in (1, 4, 80) for a in (65, 1025)]
DECODE_CASES += [pytest.param(1025, "mixed", 10, thr, id="1025-mixed-thr%g" % thr) for thr in (0.05, 0.5)]
DECODE_CASES += [pytest.param(300, "batch3", 10, None, id="300-batch3"), pytest.param(300, "special", 10, None, id="300-special")]


@pytest.mark.parametrize("a,mode,c,thr", DECODE_CASES)
def test_retina_decode_vs_fp64(a, mode, c, thr):
    """rr_retina_decode against rc.decode in float64: counts, classes (first maximum), kept rows in anchor order, nothing
    behind the count.  C = 1 (the class loop does not run), 4, 10 and 80; the default threshold and 0.05 / 0.5 passed
    explicitly; B = 3 with an image that keeps nothing between two that keep rows.  "special": a NaN probability is the row's
    maximum wherever it stands (torch's max), so rows whose logits are all NaN, NaN in class 0, or NaN in class 3 beside a
    class at 6.0 are dropped, and a +inf logit is kept with probability exactly 1; the rows around them pack as without them.
    Measured (float32 restatement on the CPU / kernel on an MI355X, both against float64): special keeps 297 / 297 of 300,
    probabilities 7.4e-8 / 7.4e-8, boxes 4.1e-5 / 4.1e-5 (max 412); C = 80, A = 1025 keeps every row, 8.2e-8 / 8.2e-8 and 4.4e-5
    / 4.4e-5; C = 1 keeps 460 / 455 of 1025; threshold 0.5 keeps 688 / 664, 0.05 keeps 1024 / 1025; batch3 keeps 221, 0, 300.
    Before the kernel took a NaN for the maximum, special kept 298 / 298: `p > best` skipped the NaN in class 3 and the row
    stayed on the strength of its class at 6.0."""
    from rrnet_amd import ops
    b = 3 if mode == "batch3" else 2
    args = {} if thr is None else {"thr": thr}
    thr_used = 0.1 if thr is None else thr
    logits, loc, anchors = _decode_inputs(a, c, 1000 + a + (0 if c == 10 else 31 * c), mode, b=b, **args)
    p = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
    top_p = p.max(axis=2)                                                       # NaN where a row holds one
    assert float(np.abs(top_p[~np.isnan(top_p)] - thr_used).min()) > 1e-5
    assert bool(np.isnan(top_p).any()) == (mode == "special")
    dev = [torch.from_numpy(t).cuda() for t in (logits, loc, anchors)]
    rows, count = ops.retina_decode(*dev) if thr is None else ops.retina_decode(*dev, thr)
    rows, count = rows.cpu().numpy(), count.cpu().numpy()
    print("\ndecode A=%d %s C=%d threshold %g: kept %s" % (a, mode, c, thr_used, count.tolist()))
    ties = 0
    for i in range(logits.shape[0]):
        r64, keep64 = rc.decode(logits[i], loc[i], anchors, torch.float64, **args)
        r32, _ = rc.decode(logits[i], loc[i], anchors, torch.float32, **args)
        k = keep64.numel()
        if mode == "special":
            kept = keep64.tolist()
            for kind, at in SPECIAL_ROWS.items():
                assert (at[i] in kept) == (kind == "inf"), (kind, at[i])
                assert min(abs(r - at[i]) for r in kept if r != at[i]) == 1      # a kept neighbour: the packing is at stake
        assert int(count[i]) == k
        if mode == "none" or (mode == "batch3" and i == 1):
            assert k == 0
        if mode == "all" or (mode == "batch3" and i == 2):
            assert k == a
        if mode == "batch3" and i == 0:
            assert 0 < k < a
        got = rows[i, :k]
        assert np.array_equal(got[:, 5], r64[:, 5].numpy())                     # class + 1, first maximum
        top = logits[i].max(axis=1, keepdims=True)
        ties += int(((logits[i] == top).sum(axis=1) > 1)[keep64.numpy()].sum())
        if k:
            # the kept anchors, in anchor order: every row's probability is the one of its anchor
            _judge("prob", got[:, 4], r64[:, 4].numpy(), r32[:, 4].numpy())
            _judge("boxes", got[:, :4], r64[:, :4].numpy(), r32[:, :4].numpy())
        if mode == "special":
            at = keep64.tolist().index(SPECIAL_ROWS["inf"][i])
            assert got[at, 4] == 1.0 and got[at, 5] == 3.0
        assert not rows[i, k:].any()                                            # nothing behind the count
    if mode == "mixed" and a >= 63 and c > 2:
        assert ties > 0


# --------------------------------------------------------------------------------------------------------------------
# the RetinaNet convolution shapes on the existing entries
# --------------------------------------------------------------------------------------------------------------------
CONV_SHAPES = {                      # n, c, h, w, k, r, s, stride, pad, bias
    "stem_7x7s2_3_64": (2, 3, 40, 56, 64, 7, 7, 2, 3, False),
    "lateral_1x1_2048_256": (2, 2048, 3, 4, 256, 1, 1, 1, 0, True),
    "loc_3x3_256_36": (2, 256, 8, 10, 36, 3, 3, 1, 1, True),
    "cls_3x3_256_90": (2, 256, 8, 10, 90, 3, 3, 1, 1, True),
    # the ResNet bottlenecks: stride-2 projections (on an odd map; at 2048 outputs), the stride-2 3x3, the 1x1 pair at 2048
    "proj_1x1s2_256_512": (2, 256, 7, 9, 512, 1, 1, 2, 0, False),
    "proj_1x1s2_1024_2048": (2, 1024, 6, 8, 2048, 1, 1, 2, 0, False),
    "c2_3x3s2_512_512": (2, 512, 6, 8, 512, 3, 3, 2, 1, False),
    "c3_1x1_512_2048": (2, 512, 3, 4, 2048, 1, 1, 1, 0, False),
    "c1_1x1_2048_512": (2, 2048, 3, 4, 512, 1, 1, 1, 0, False),
}


@functools.lru_cache(maxsize=None)
def _conv_case(name):
    n, c, h, w, k, r, s, st, pad, bias = CONV_SHAPES[name]
    g = np.random.default_rng(sum(CONV_SHAPES[name][:7]))
    x = torch.from_numpy(g.standard_normal((n, c, h, w)).astype(np.float32))
    wt = torch.from_numpy((g.standard_normal((k, c, r, s)) / np.sqrt(c * r * s)).astype(np.float32))
    b = torch.from_numpy(g.standard_normal(k).astype(np.float32)) if bias else None
    p, q = (h + 2 * pad - r) // st + 1, (w + 2 * pad - s) // st + 1
    gy = torch.from_numpy(g.standard_normal((n, k, p, q)).astype(np.float32))
    y, dx, dw = conv_ref64(x, wt, b, st, (pad, pad), False, gy)
    return x, wt, b, gy, y, dx, dw


def _conv_judge(tag, got, ref_all, idx, ref_s, max_seq, rms_seq):
    got, ref_all = got.detach().cpu().double().numpy(), ref_all.numpy()
    ratios = conv_error_ratios(got[idx], ref_s, max_seq, rms_seq, got, ref_all)
    print("%s: max %.2f rms %.2f whole-tensor rms %.2f of the chained-fp32 yardstick" % ((tag,) + ratios))
    assert conv_accepts(ratios), (tag, ratios)


@pytest.mark.parametrize("name", list(CONV_SHAPES))
def test_retinanet_conv_shapes_vs_fp64(name):
    from rrnet_amd import ops
    n, c, h, w, k, r, s, st, pad, bias = CONV_SHAPES[name]
    x, wt, b, gy, y64, dx64, dw64 = _conv_case(name)
    xd, wd, gyd = (ops.to_nhwc(t.cuda()) for t in (x, wt, gy))
    bd = None if b is None else b.cuda()
    print()
    with ops.bf16_scope(0, force=True):
        idx = conv_sample_positions(tuple(y64.shape), 1)
        yard = conv_yardstick(conv_terms("fprop", idx, x, wt, None, st, (pad, pad), bias=b))
        _conv_judge("fprop " + name, ops.conv_fprop(xd, wd, bd, st, (pad, pad), False), y64, idx, *yard)
        idx = conv_sample_positions((n, c, h, w), 2)
        yard = conv_yardstick(conv_terms("dgrad", idx, None, wt, gy, st, (pad, pad)))
        _conv_judge("dgrad " + name, ops.conv_dgrad(gyd, wd, (n, c, h, w), st, (pad, pad)), dx64, idx, *yard)
        idx = conv_sample_positions((k, c, r, s), 3)
        yard = conv_yardstick(conv_terms("wgrad", idx, x, (r, s), gy, st, (pad, pad)))
        dw = ops.zeros_nhwc(k, c, r, s, "cuda")
        ops.conv_wgrad(xd, gyd, dw, st, (pad, pad))
        _conv_judge("wgrad " + name, dw, dw64, idx, *yard)


# --------------------------------------------------------------------------------------------------------------------
# BatchNorm backward sums at ResNet's 2048 channels (rr_bn_bwd_reduce beyond one workgroup's 1024 channels)
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["none", "z", "recomputed"])
@pytest.mark.parametrize("c,hw", [(2048, (3, 4)), (1280, (10, 11)), (1028, (5, 5))])
def test_bn_bwd_reduce_wide_channels_vs_fp64(c, hw, mask):
    """sums[0:C] = sum dy, sums[C:2C] = sum dy * xhat over the pixels, dy = dz masked by z > 0 (z given, or recomputed as
    y * scale + shift).  Derived bound per channel: xhat carries 2 roundings, the product 1, the kernel adds at most 8 terms
    in float32 before it goes on in double: |err| <= 12 u sum|term|.  The recomputed mask uses the kernel's own fused
    multiply-add, evaluated here in float64 on inputs kept 1e-3 away from 0."""
    from rrnet_amd import ops
    g = np.random.default_rng(c + hw[0])
    n = 2
    shape = (n, c) + hw
    dz = g.standard_normal(shape).astype(np.float32)
    y = g.standard_normal(shape).astype(np.float32)
    mean = (g.standard_normal(c) * 0.1).astype(np.float32)
    invstd = (1.0 + 0.2 * g.random(c)).astype(np.float32)
    scale = (0.5 + g.random(c)).astype(np.float32)
    shift = (g.standard_normal(c) * 0.3).astype(np.float32)
    pre = y.astype(np.float64) * scale[None, :, None, None] + shift[None, :, None, None]
    y = np.where(np.abs(pre) < 1e-3, y + np.float32(0.01), y).astype(np.float32)
    pre = y.astype(np.float64) * scale[None, :, None, None] + shift[None, :, None, None]
    assert float(np.abs(pre).min()) > 1e-4
    z = np.maximum(pre, 0).astype(np.float32)
    keep = np.ones(shape, bool) if mask == "none" else pre > 0
    dy = dz.astype(np.float64) * keep
    xhat = (y.astype(np.float64) - mean[None, :, None, None]) * invstd[None, :, None, None]
    ref = np.concatenate([dy.sum(axis=(0, 2, 3)), (dy * xhat).sum(axis=(0, 2, 3))])
    mass = np.concatenate([np.abs(dy).sum(axis=(0, 2, 3)), np.abs(dy * xhat).sum(axis=(0, 2, 3))])
    dev = lambda a: ops.to_nhwc(torch.from_numpy(a).cuda())
    vec = lambda a: torch.from_numpy(a).cuda()
    sums = ops.bn_bwd_reduce(dev(dz), dev(z) if mask == "z" else None, dev(y), vec(mean), vec(invstd),
                             mask_scale=vec(scale) if mask == "recomputed" else None,
                             mask_shift=vec(shift) if mask == "recomputed" else None)
    got = sums[:2 * c].cpu().numpy()
    err = np.abs(got - ref)
    print("\nbn_bwd_reduce C=%d %s mask=%s: worst error / bound %.3f" % (c, hw, mask, float((err / (12 * U32 * mass + 1e-300)).max())))
    assert np.all(err <= 12 * U32 * mass)

"""GPU: the criterion kernels (csrc/losses.hip: fused focal loss, RegL1, stage-2 match / loss / d rois) against the
float64 evaluation of the oracle (oracle/ops.py) on the same seeded host inputs (tests/helpers.py), at the shapes and
edges where a fused kernel goes wrong: the grid-stride loop past 2048 blocks, saturated logits, gt just below 1,
N_pos == 0 at size, atomics on shared pixels, masked slots, interleaved images, ties and empty images.

Tolerances are never read off the kernel:
 - derived (RegL1, where only sums round): |got - ref| <= (n + 3) u sum|term|, u = 2^-24, n = terms meeting in the
   element;
 - measured (focal, stage 2: libm and cancellation): 4x the error of the same oracle code evaluated in float32 on the
   CPU against float64, with a floor of 2u max|ref|; focal gradients per class of p = sigmoid(x).
Loss tolerances are further capped by those of test_losses_vs_reference_goldens (focal 1e-4 + 1e-4|ref|, RegL1 1e-5 +
1e-3|ref|).  Each test prints its float32 figures and the kernel's error (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import U32, focal_inputs, regl1_inputs, stage2_inputs

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def measured_tol(err32, ref):
    return max(4.0 * float(err32), 2.0 * U32 * float(np.abs(ref).max(initial=0.0)))


# --------------------------------------------------------------------------------------------------------------------
# focal loss
# --------------------------------------------------------------------------------------------------------------------
def _focal_oracle(x, gt, dtype):
    from oracle import ops as oo
    xt = torch.from_numpy(x).to(dtype).requires_grad_()
    loss = oo.hm_loss_from_logits(xt, torch.from_numpy(gt).to(dtype))
    (0.5 * loss).backward()
    return float(loss), xt.grad.numpy().astype(np.float64)


@functools.lru_cache(maxsize=2)
def _focal_case(shape, with_pos):
    x, gt = focal_inputs(shape, seed=sum(shape) + 7 * with_pos, with_pos=with_pos)
    l64, g64 = _focal_oracle(x, gt, torch.float64)
    l32, g32 = _focal_oracle(x, gt, torch.float32)
    p = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    classes = {"p<1e-3": p < 1e-3, "1e-3<=p<=0.99": (p >= 1e-3) & (p <= 0.99), "p>0.99": p > 0.99}
    return x, gt, l64, l32, g64, g32, p, classes


FOCAL_CASES = [((1, 1, 1, 1), True), ((3, 7, 37, 41), True), ((2, 10, 128, 128), True), ((8, 10, 256, 256), True),
               ((8, 10, 256, 256), False)]


@pytest.mark.parametrize("gt_layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("shape,with_pos", FOCAL_CASES)
def test_focal_loss_fwd_bwd_vs_fp64(shape, with_pos, gt_layout):
    """rr_focal_loss_fwd/bwd through RF.focal_loss_hm_from_logits, backward driven by (0.5 * loss).backward().
    Measured float32 figures (CPU): loss error 1.4e-7 at (1,1,1,1), 2.4e-5 to 2.6e-5 on losses near 11.8, 6.5 on the
    N_pos == 0 loss of 2.45e6; at bench size the gradient error is 5.7e-13 for p < 1e-3, 2.8e-7 for 1e-3 <= p <= 0.99
    (max|ref| 0.56) and 5.8e-7 for p > 0.99 (max|ref| 0.53)."""
    from rrnet_amd import functional as RF
    x, gt, l64, l32, g64, g32, p, classes = _focal_case(shape, with_pos)
    assert (gt == 1).any() == with_pos
    lg = torch.from_numpy(x).cuda().contiguous(memory_format=CL).requires_grad_()
    gd = torch.from_numpy(gt).cuda()
    gd = gd.contiguous(memory_format=CL) if gt_layout == "nhwc" else gd.contiguous()
    loss = RF.focal_loss_hm_from_logits(lg, gd)
    (0.5 * loss).backward()
    got_l = float(loss)
    got_g = _np(lg.grad)
    tol_l = min(measured_tol(abs(l32 - l64), np.array([l64])), 1e-4 + 1e-4 * abs(l64))
    print("\nfocal %s pos=%s gt=%s: loss fp64 %.9g  fp32 err %.3g  kernel err %.3g  tol %.3g"
          % (shape, with_pos, gt_layout, l64, abs(l32 - l64), abs(got_l - l64), tol_l))
    assert abs(got_l - l64) <= tol_l
    # saturated / clamped logits: the clamp passes no gradient, in fp64 as in the kernel
    clamped = g64 == 0.0
    assert np.all(got_g[clamped] == 0.0), int((got_g[clamped] != 0).sum())
    for name, sel in classes.items():
        if not sel.any():
            continue
        err32 = np.abs(g32[sel] - g64[sel]).max()
        tol = measured_tol(err32, g64[sel])
        err = np.abs(got_g[sel] - g64[sel]).max()
        print("  grad %-14s n=%-8d max|ref| %.3g  fp32 err %.3g  kernel err %.3g  tol %.3g"
              % (name, int(sel.sum()), np.abs(g64[sel]).max(), err32, err, tol))
        assert err <= tol, (name, err, tol)


# --------------------------------------------------------------------------------------------------------------------
# RegL1
# --------------------------------------------------------------------------------------------------------------------
REGL1_CASES = {"b1": dict(batch=1, height=32, width=40, slots=24), "b8": dict(batch=8, height=64, width=64, slots=64),
               "b8_all_masked": dict(batch=8, height=64, width=64, slots=64, all_masked=True),
               "b8_m0": dict(batch=8, height=16, width=24, slots=0)}


@pytest.mark.parametrize("case", list(REGL1_CASES))
def test_regl1_fwd_bwd_vs_fp64(case):
    """rr_regl1_fwd/bwd through RF.reg_l1_loss against oracle.reg_l1_loss in fp64 (autograd for the gradient).
    Derived bound: the loss sums n = B*M*C terms |p*m - t*m| / (sum m + 1e-4); a gradient element sums one term
    coef * sign * m per valid slot on that pixel (n of them, coef = 1 / (sum m + 1e-4)).  Elements with no term, masked
    slots and pred == target slots included, must be exactly 0."""
    from oracle import ops as oo
    from rrnet_amd import functional as RF
    kw = REGL1_CASES[case]
    pred, mask, ind, target = regl1_inputs(seed=31, **kw)
    b, c, h, w = pred.shape
    m = ind.shape[1]
    p64 = torch.from_numpy(pred).double().requires_grad_()
    ref = oo.reg_l1_loss(p64, torch.from_numpy(mask).double(), torch.from_numpy(ind).double(),
                         torch.from_numpy(target).double())
    ref.backward()
    ref_l, ref_g = float(ref), p64.grad.numpy()
    pd = torch.from_numpy(pred).cuda().contiguous(memory_format=CL).requires_grad_()
    loss = RF.reg_l1_loss(pd, torch.from_numpy(mask).cuda(), torch.from_numpy(ind).cuda(), torch.from_numpy(target).cuda())
    loss.backward()
    got_l, got_g = float(loss), _np(pd.grad)
    # loss: all terms are >= 0, so sum|term| is the loss itself
    tol_l = min((b * m * c + 3) * U32 * abs(ref_l), 1e-5 + 1e-3 * abs(ref_l))
    # gradient: count the nonzero terms per element
    nterm = np.zeros((b, c, h * w))
    coef = 1.0 / (float(mask.astype(np.float64).sum()) * c + 1e-4)
    for bi in range(b):
        for s in range(m):
            if mask[bi, s, 0] == 0:
                continue
            pix = int(ind[bi, s, 0])
            d = pred[bi, :, pix // w, pix % w].astype(np.float64) - target[bi, s].astype(np.float64)
            nterm[bi, d != 0, pix] += 1
    nterm = nterm.reshape(b, c, h, w)
    tol_g = (nterm + 3) * U32 * nterm * coef
    err_g = np.abs(got_g - ref_g)
    print("\nregl1 %s: loss %.9g  kernel err %.3g  tol %.3g | grad max|ref| %.3g  kernel err %.3g  max terms %d"
          % (case, ref_l, abs(got_l - ref_l), tol_l, np.abs(ref_g).max(initial=0), err_g.max(initial=0),
             nterm.max(initial=0)))
    assert abs(got_l - ref_l) <= tol_l
    assert np.all(got_g[nterm == 0] == 0.0)
    assert np.all(err_g <= tol_g), float((err_g - tol_g).max())
    if m:
        assert nterm.max() >= (3 if case != "b8_all_masked" else 0)


# --------------------------------------------------------------------------------------------------------------------
# stage 2
# --------------------------------------------------------------------------------------------------------------------
def stage2_oracle(reg, rois, gt, scale):
    """The per-image loop of oracle.ops.criterion (rrnet_operator.py:63-84, oracle/ops.py:292-306), restated on
    tensors of any dtype; gt [B,G,>=4] already xyxy."""
    from oracle import ops as oo
    bs = gt.shape[0]
    loss = 0
    for b in range(bs):
        flag = rois[:, 0] == b
        bbox = rois[flag][:, 1:]
        g = gt[b]
        iou = oo.box_iou(bbox * scale, g[:, :4])
        max_iou, max_idx = torch.max(iou, dim=1)
        pos = max_iou > 0.5
        if pos.sum() == 0:
            pos = torch.zeros_like(max_iou).bool()
            pos[0] = True
            factor = 0
        else:
            factor = 1
        tgt = oo.generate_bbox_target(bbox[pos, :] * scale, g[max_idx[pos], :4])
        loss = loss + F.smooth_l1_loss(reg[flag][pos], tgt) * factor / bs
    return loss


def _stage2_eval(rois, reg, gt, scale, dtype):
    r = torch.from_numpy(rois).to(dtype).requires_grad_()
    g = torch.from_numpy(reg).to(dtype).requires_grad_()
    loss = stage2_oracle(g, r, torch.from_numpy(gt).to(dtype), scale)
    loss.backward()
    return float(loss), g.grad.numpy().astype(np.float64), r.grad.numpy().astype(np.float64)


@functools.lru_cache(maxsize=1)
def _stage2_case(scale):
    rois, reg, gt = stage2_inputs(seed=int(scale) + 40, scale=scale)
    return (rois, reg, gt), _stage2_eval(rois, reg, gt, scale, torch.float64), _stage2_eval(rois, reg, gt, scale, torch.float32)


@pytest.mark.parametrize("rois_grad", [False, True])
@pytest.mark.parametrize("scale", [4.0, 1.0])
def test_stage2_loss_vs_fp64(scale, rois_grad):
    """rr_stage2_loss (match, loss, d reg, d rois) through RF.stage2_reg_loss: B = 8 images of 300 interleaved RoIs,
    G = 100 with zero rows and duplicated gt boxes, one image without a positive, one with only positives.
    Measured float32 figures (CPU): loss 1.6e-9 (scale 4) and 3.2e-8 (scale 1), d reg 4.8e-10 and 4.1e-10, d rois
    4.5e-11 to 1.7e-10."""
    from rrnet_amd import functional as RF
    (rois, reg, gt), (l64, dreg64, droi64), (l32, dreg32, droi32) = _stage2_case(scale)
    regd = torch.from_numpy(reg).cuda().requires_grad_()
    roid = torch.from_numpy(rois).cuda()
    if rois_grad:
        roid.requires_grad_()
    loss = RF.stage2_reg_loss(regd, roid, torch.from_numpy(gt).cuda(), scale)
    loss.backward()
    got_l = float(loss)
    tol_l = min(measured_tol(abs(l32 - l64), np.array([l64])), 1e-5 + 1e-3 * abs(l64))
    tol_r = measured_tol(np.abs(dreg32 - dreg64).max(), dreg64)
    err_r = np.abs(_np(regd.grad) - dreg64).max()
    print("\nstage2 scale %g rois_grad %s: loss %.9g fp32 err %.3g kernel err %.3g tol %.3g | d reg fp32 err %.3g "
          "kernel err %.3g tol %.3g" % (scale, rois_grad, l64, abs(l32 - l64), abs(got_l - l64), tol_l,
                                        np.abs(dreg32 - dreg64).max(), err_r, tol_r))
    assert abs(got_l - l64) <= tol_l
    assert err_r <= tol_r
    # RoIs of the image without positives and non-positive RoIs get exactly zero
    assert np.all(_np(regd.grad)[np.all(dreg64 == 0, axis=1)] == 0.0)
    if rois_grad:
        got_d = _np(roid.grad)
        tol_d = measured_tol(np.abs(droi32 - droi64).max(), droi64)
        err_d = np.abs(got_d - droi64).max()
        print("  d rois fp32 err %.3g  kernel err %.3g  tol %.3g" % (np.abs(droi32 - droi64).max(), err_d, tol_d))
        assert np.all(got_d[:, 0] == 0.0)
        assert np.all(got_d[np.all(droi64 == 0, axis=1)] == 0.0)
        assert err_d <= tol_d
    else:
        assert roid.grad is None

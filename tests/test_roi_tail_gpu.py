"""GPU: the RoI and head-tail kernels that kernel_audit.py does not patch — RoIAlign backward (csrc/roialign.hip),
global average pooling and its fused BN + residual + ReLU form, the WH-head shift-sum (csrc/elementwise.hip) and the
DCN offset / mask split (csrc/dcn.hip) — against float64 references on seeded host inputs (tests/helpers.py).

Tolerances are never read off the kernel:
 - derived, where only sums round (dyadic RoIAlign set, avgpool, bn_res_relu_avgpool, shift-sum forward):
   |got - ref| <= (n + 3) u sum|term| elementwise, u = 2^-24, n = terms meeting in the element, sum|term| = the fp64
   reference evaluated on absolute values;
 - bit-exact for gathers and copies (shift-sum backward, the offset half of the DCN split);
 - measured (random RoIAlign set, the DCN mask): 4x the error of the same computation in float32 on the CPU against
   float64, with a floor of 2u max|ref|.
"""
import numpy as np
import pytest
import torch

from helpers import ROI_DYADIC_CASES, ROI_DYADIC_MAP, U32, measured_tol, roi_dyadic_case, roi_random_set, roi_tap_counts

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _oracle_roi_bwd(feat_shape, rois, dout, size, scale, sr, dtype):
    """d feat of oracle.ops.roi_align by autograd, in `dtype`.  Identical RoIs are merged first with their output
    gradients summed in `dtype` (the map is linear in dout, so this is the same reference, computed once per RoI)."""
    from oracle import ops as oo
    uniq, inv = np.unique(rois, axis=0, return_inverse=True)
    inv = torch.from_numpy(inv.reshape(-1))
    d = torch.zeros((len(uniq),) + tuple(dout.shape[1:]), dtype=dtype).index_add_(0, inv, dout.to(dtype))
    feat = torch.zeros(feat_shape, dtype=dtype, requires_grad=True)
    out = oo.roi_align(feat, torch.from_numpy(uniq), size, spatial_scale=scale, sampling_ratio=sr)
    out.backward(d)
    return feat.grad.numpy().astype(np.float64)


def _kernel_roi_bwd(feat_shape, rois, dout, size, scale, sr):
    from rrnet_amd import functional as RF
    fd = torch.zeros(feat_shape, dtype=torch.float32).cuda().contiguous(memory_format=CL).requires_grad_()
    out = RF.roi_align(fd, torch.from_numpy(rois).cuda(), size, spatial_scale=scale, sampling_ratio=sr)
    out.backward(dout.cuda().contiguous(memory_format=CL))
    return _np(fd.grad)


@pytest.mark.parametrize("size,sr,scale,ch", ROI_DYADIC_CASES)
def test_roi_align_bwd_dyadic_set_vs_fp64(size, sr, scale, ch):
    """rr_roi_align_bwd on RoIs whose sample positions and weights are exact in fp32 (tests/helpers.py), so only the
    atomic sums round: |got - ref| <= (n + 3) u (S^T |dout|) with n the nonzero taps on each pixel.  Image 2 is never
    touched and RoIs entirely outside the map contribute nothing: both exactly 0."""
    B, H, W = ROI_DYADIC_MAP
    rois = roi_dyadic_case(size, sr, scale, ch)
    rng = np.random.default_rng(ch + size[0])
    dout = torch.from_numpy(rng.standard_normal((len(rois), ch) + size).astype(np.float32))
    shape = (B, ch, H, W)
    ref = _oracle_roi_bwd(shape, rois, dout.double(), size, scale, sr, torch.float64)
    mag = _oracle_roi_bwd(shape, rois, dout.double().abs(), size, scale, sr, torch.float64)
    n = roi_tap_counts(rois, size, scale, sr, B, H, W)[:, None]
    got = _kernel_roi_bwd(shape, rois, dout, size, scale, sr)
    tol = (n + 3) * U32 * mag
    err = np.abs(got - ref)
    print("\nroi bwd dyadic %s sr %d scale %g C %d: max|ref| %.3g  max terms %d  kernel err %.3g  worst err/tol %.3g"
          % (size, sr, scale, ch, np.abs(ref).max(), n.max(), err.max(), (err / np.maximum(tol, 1e-300)).max()))
    assert n.max() >= 500                                       # the race patch
    assert np.all(got[2] == 0.0)
    assert np.all(got[np.broadcast_to(n == 0, got.shape)] == 0.0)
    assert np.all(err <= tol), float((err - tol).max())
    outside = rois[-502:-500]                                   # the two RoIs beyond the map
    got_out = _kernel_roi_bwd(shape, outside, dout[-502:-500], size, scale, sr)
    assert np.all(got_out == 0.0)


def _random_set():
    """helpers.roi_random_set (44 RoIs) at 256 channels and a batch of 3."""
    return roi_random_set(), (3, 256, 70, 90)


@pytest.mark.parametrize("sr", [-1, 2])
@pytest.mark.parametrize("size", [(3, 3), (7, 7), (2, 5)])
def test_roi_align_bwd_random_set_vs_fp64(size, sr):
    """rr_roi_align_bwd on arbitrary RoIs at 256 channels against fp64 autograd through oracle.roi_align; measured
    tolerance (the oracle's own backward in fp32).  Measured float32 figures (CPU): 5.3e-7 to 7.8e-7 at (3,3) and
    (2,5) bins (max|ref| ~6), 2.6e-6 and 3.3e-6 at (7,7) (max|ref| ~14).  With FMA-contracted sample positions the
    kernel was off by 2.2e-5 at (7,7) (tolerance 1.0e-5 / 1.3e-5); unrounded-as-the-oracle positions give 4.1e-6 / 5.7e-6."""
    rois, shape = _random_set()
    rng = np.random.default_rng(size[0] * 10 + size[1] + sr)
    dout = torch.from_numpy(rng.standard_normal((len(rois), shape[1]) + size).astype(np.float32))
    ref = _oracle_roi_bwd(shape, rois, dout, size, 1.0, sr, torch.float64)
    r32 = _oracle_roi_bwd(shape, rois, dout, size, 1.0, sr, torch.float32)
    got = _kernel_roi_bwd(shape, rois, dout, size, 1.0, sr)
    err32 = np.abs(r32 - ref).max()
    tol = measured_tol(err32, ref)
    err = np.abs(got - ref).max()
    print("\nroi bwd random %s sr %d: max|ref| %.3g  fp32 err %.3g  kernel err %.3g  tol %.3g"
          % (size, sr, np.abs(ref).max(), err32, err, tol))
    assert np.all(got[2] == 0.0)
    assert err <= tol


# --------------------------------------------------------------------------------------------------------------------
# global average pooling (stage-2 head)
# --------------------------------------------------------------------------------------------------------------------
def _nhwc(gen, r, c, h, w):
    """float32 [r, c, h, w] with NHWC memory, drawn on the host."""
    return torch.randn((r, h, w, c), generator=gen).permute(0, 3, 1, 2)


@pytest.mark.parametrize("hw", [(3, 3), (7, 7)])
@pytest.mark.parametrize("rows", [1, 9000])
def test_avgpool_fwd_bwd_vs_fp64(rows, hw):
    """rr_avgpool_fwd: n = HW terms x / HW per output; rr_avgpool_bwd: one term dout / HW per element."""
    from rrnet_amd import ops
    gen = torch.Generator().manual_seed(rows + hw[0])
    c, (h, w) = 256, hw
    x = _nhwc(gen, rows, c, h, w)
    got = _np(ops.avgpool_fwd(x.cuda()))
    x64 = x.double()
    ref = x64.mean((2, 3), keepdim=True).numpy()
    mag = x64.abs().mean((2, 3), keepdim=True).numpy()
    err = np.abs(got - ref)
    tol = (h * w + 3) * U32 * mag
    print("\navgpool fwd R %d HW %d: kernel err %.3g  worst err/tol %.3g" % (rows, h * w, err.max(), (err / tol).max()))
    assert np.all(err <= tol)
    dout = _nhwc(gen, rows, c, 1, 1)
    gotd = _np(ops.avgpool_bwd(dout.cuda(), (rows, c, h, w)))
    refd = (dout.double() / (h * w)).expand(rows, c, h, w).numpy()
    errd = np.abs(gotd - refd)
    assert np.all(errd <= 4 * U32 * np.abs(refd)), errd.max()


@pytest.mark.parametrize("hw", [(3, 3), (7, 7)])
@pytest.mark.parametrize("rows", [1, 9000])
def test_bn_res_relu_avgpool_vs_fp64(rows, hw):
    """rr_bn_res_relu_avgpool against fp64 mean(relu(y*scale + shift + res)): n = 3 HW terms (y*scale, shift, res
    per position), sum|term| = mean(|y*scale| + |shift| + |res|)."""
    from rrnet_amd import ops
    gen = torch.Generator().manual_seed(7 * rows + hw[0])
    c, (h, w) = 256, hw
    y, res = _nhwc(gen, rows, c, h, w), _nhwc(gen, rows, c, h, w)
    scale = 1.0 + 0.3 * torch.randn(c, generator=gen)
    shift = 0.3 * torch.randn(c, generator=gen)
    got = _np(ops.bn_res_relu_avgpool(y.cuda(), scale.cuda(), shift.cuda(), res.cuda()))
    y64, r64 = y.double(), res.double()
    s64, b64 = scale.double().view(1, c, 1, 1), shift.double().view(1, c, 1, 1)
    ref = torch.relu(y64 * s64 + b64 + r64).mean((2, 3), keepdim=True).numpy()
    mag = ((y64 * s64).abs() + b64.abs() + r64.abs()).mean((2, 3), keepdim=True).numpy()
    err = np.abs(got - ref)
    tol = (3 * h * w + 3) * U32 * mag
    print("\nbn_res_relu_avgpool R %d HW %d: kernel err %.3g  worst err/tol %.3g"
          % (rows, h * w, err.max(), (err / tol).max()))
    assert np.all(err <= tol)


# --------------------------------------------------------------------------------------------------------------------
# WH head shift-sum
# --------------------------------------------------------------------------------------------------------------------
def _shift_sum64(t, bw, bh, k):
    """fp64 restatement of the two k-tap sums: t [N,H,W,ct] -> out [N,H,W,2] (W sum, H sum), the same sums of |term|,
    and the number of terms per output."""
    n, hh, ww, _ = t.shape
    half = k // 2
    out = np.zeros((n, hh, ww, 2))
    mag = np.zeros((n, hh, ww, 2))
    cnt = np.zeros((n, hh, ww, 2))
    out[..., 0], out[..., 1] = bw, bh
    mag[..., 0], mag[..., 1] = abs(bw), abs(bh)
    cnt[:] = 1
    for s in range(k):
        d = s - half
        # W sum: t[h, w + d, k + s]
        lo, hi = max(0, -d), min(ww, ww - d)
        if lo < hi:
            v = t[:, :, lo + d:hi + d, k + s]
            out[:, :, lo:hi, 0] += v
            mag[:, :, lo:hi, 0] += np.abs(v)
            cnt[:, :, lo:hi, 0] += 1
        # H sum: t[h + d, w, s]
        lo, hi = max(0, -d), min(hh, hh - d)
        if lo < hi:
            v = t[:, lo + d:hi + d, :, s]
            out[:, lo:hi, :, 1] += v
            mag[:, lo:hi, :, 1] += np.abs(v)
            cnt[:, lo:hi, :, 1] += 1
    return out, mag, cnt


def _shift_sum_bwd64(dout, k, ct):
    """dout [N,H,W,2] -> dt [N,H,W,ct]: dt[h,w,r] = dout_H[h-(r-half), w], dt[h,w,k+s] = dout_W[h, w-(s-half)], 0 else."""
    n, hh, ww, _ = dout.shape
    half = k // 2
    dt = np.zeros((n, hh, ww, ct), dout.dtype)
    for s in range(k):
        d = s - half
        lo, hi = max(0, d), min(hh, hh + d)          # h - d in [0, H)
        if lo < hi:
            dt[:, lo:hi, :, s] = dout[:, lo - d:hi - d, :, 1]
        lo, hi = max(0, d), min(ww, ww + d)
        if lo < hi:
            dt[:, :, lo:hi, k + s] = dout[:, :, lo - d:hi - d, 0]
    return dt


@pytest.mark.parametrize("hw", [(1, 1), (5, 40), (40, 5), (128, 160)])
@pytest.mark.parametrize("k,pad", [(3, 0), (3, 2), (17, 0), (17, 2)])
def test_wh_shift_sum_fwd_bwd_vs_fp64(k, pad, hw):
    """rr_wh_shift_sum_fwd within (n + 3) u sum|term| (n = bias + in-range taps); rr_wh_shift_sum_bwd, a pure gather,
    bit for bit, its padding channels (ct > 2k) exactly 0.  The padding channels of the input hold noise, which the
    forward must not read."""
    from rrnet_amd import ops
    rng = np.random.default_rng(k * 100 + pad * 10 + hw[0])
    n, (h, w), ct = 2, hw, 2 * k + pad
    t = rng.standard_normal((n, h, w, ct)).astype(np.float32)
    bw, bh = np.float32(rng.standard_normal()), np.float32(rng.standard_normal())
    td = torch.from_numpy(t).cuda().permute(0, 3, 1, 2)
    got = ops.wh_shift_sum_fwd(td, torch.tensor([bw]).cuda(), torch.tensor([bh]).cuda(), k)
    got = got.permute(0, 2, 3, 1).cpu().numpy().astype(np.float64)
    ref, mag, cnt = _shift_sum64(t.astype(np.float64), float(bw), float(bh), k)
    err = np.abs(got - ref)
    tol = (cnt + 3) * U32 * mag
    print("\nshift-sum k %d ct %d %s: fwd kernel err %.3g  worst err/tol %.3g" % (k, ct, hw, err.max(), (err / tol).max()))
    assert np.all(err <= tol)
    dout = rng.standard_normal((n, h, w, 2)).astype(np.float32)
    gotd = ops.wh_shift_sum_bwd(torch.from_numpy(dout).cuda().permute(0, 3, 1, 2), k, ct)
    gotd = gotd.permute(0, 2, 3, 1).cpu().numpy()
    refd = _shift_sum_bwd64(dout.astype(np.float64), k, ct).astype(np.float32)
    assert np.all(gotd[..., 2 * k:] == 0.0)
    assert np.array_equal(gotd.view(np.uint32), refd.view(np.uint32))


# --------------------------------------------------------------------------------------------------------------------
# DCN offset / mask split
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dg", [1, 2])
def test_dcn_split_fwd_bwd_vs_fp64(dg):
    """RF.dcn_offset_mask (rr_dcn_split_fwd/bwd), 3x3 kernel: the offset half is a copy both ways (bit-exact); the mask
    against the fp64 sigmoid, its gradient against fp64 dmask * s * (1 - s) on the saved fp32 mask (measured).
    Measured float32 figures (CPU): mask 8.5e-8, mask gradient 6.5e-8 (dg 1) and 6.8e-8 (dg 2)."""
    from rrnet_amd import functional as RF
    rng = np.random.default_rng(50 + dg)
    t = dg * 9
    n, p, q = 2, 13, 17
    om = rng.normal(0.0, 3.0, (n, 3 * t, p, q))
    om[rng.random(om.shape) < 0.02] = 30.0
    om[rng.random(om.shape) < 0.02] = -30.0
    om = om.astype(np.float32)
    omd = torch.from_numpy(om).cuda().contiguous(memory_format=CL).requires_grad_()
    offset, mask = RF.dcn_offset_mask(omd)
    assert np.array_equal(offset.detach().cpu().numpy(), om[:, :2 * t])
    s64 = 1.0 / (1.0 + np.exp(-om[:, 2 * t:].astype(np.float64)))
    s32 = torch.sigmoid(torch.from_numpy(om[:, 2 * t:])).numpy().astype(np.float64)
    got_m = _np(mask)
    tol_m = measured_tol(np.abs(s32 - s64).max(), s64)
    print("\ndcn split dg %d: mask fp32 err %.3g kernel err %.3g tol %.3g"
          % (dg, np.abs(s32 - s64).max(), np.abs(got_m - s64).max(), tol_m))
    assert np.abs(got_m - s64).max() <= tol_m
    go = rng.standard_normal((n, 2 * t, p, q)).astype(np.float32)
    gm = rng.standard_normal((n, t, p, q)).astype(np.float32)
    ((offset * torch.from_numpy(go).cuda()).sum() + (mask * torch.from_numpy(gm).cuda()).sum()).backward()
    dom = omd.grad.cpu().numpy()
    assert np.array_equal(dom[:, :2 * t], go)
    s = got_m.astype(np.float32)
    ref = gm.astype(np.float64) * s.astype(np.float64) * (1.0 - s.astype(np.float64))
    r32 = (torch.from_numpy(gm) * torch.from_numpy(s) * (1.0 - torch.from_numpy(s))).numpy().astype(np.float64)
    tol = measured_tol(np.abs(r32 - ref).max(), ref)
    err = np.abs(dom[:, 2 * t:].astype(np.float64) - ref).max()
    print("  dmask fp32 err %.3g  kernel err %.3g  tol %.3g" % (np.abs(r32 - ref).max(), err, tol))
    assert err <= tol

"""GPU: the three forward kernels behind rr_roi_align_fwd (csrc/roialign.hip) — the whole-footprint 3x3 kernel, the
separable kernel for up to 8x8 bins and the generic per-sample kernel — against oracle.ops.roi_align in float64, on
every route: per RoI the footprint / separable walk (F) or per-sample taps (P), restated by helpers.roi_forward_route;
tests/test_host_logic.py holds the RoI sets to at least 5 RoIs in every (kernel, branch) cell under either sampling mode.

Tolerances are never read off the kernel:
 - derived on the dyadic and boundary RoIs (helpers.ROI_FWD_CASES), whose sample positions, bilinear weights, weight
   products and 1 / count are exact in float32, so that only the sum over taps rounds:
   |got - ref| <= (n + 3) u sum|term| elementwise, u = 2^-24, n = 4 gh gw the taps of the bin's definition (the walk
   adds at most (gh + 1)(gw + 1) < n terms), sum|term| = the float64 oracle on |feat|;
 - measured on arbitrary RoIs (helpers.roi_random_set), where positions and weights round as well: 4x the error of the
   float32 oracle against float64, floor 2u max|ref| (helpers.measured_tol);
 - bit-exact where only the processing order or the entry point differs.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import (ROI_DYADIC_MAP, ROI_FWD_CASES, ROI_FWD_OUTSIDE, ROI_RANDOM_MAP, ROI_RANDOM_SIZES, U32, measured_tol,
                     roi_forward_route, roi_fwd_case, roi_random_set, roi_sample_grid)
from test_split_model_gpu import _Calls

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=4)
def _features(batch, ch, height, width):
    """Seeded N(0,1) float32 features, NHWC on the host -> logical [batch, ch, height, width] over that memory."""
    rng = np.random.default_rng(1000 * ch + height)
    return torch.from_numpy(rng.standard_normal((batch, height, width, ch)).astype(np.float32)).permute(0, 3, 1, 2)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _oracle(feat, rois, size, scale, sr, dtype):
    from oracle import ops as oo
    return oo.roi_align(feat.to(dtype), torch.from_numpy(rois), size, spatial_scale=scale, sampling_ratio=sr).numpy() \
        .astype(np.float64)


@pytest.mark.parametrize("size,sr,scale,ch", ROI_FWD_CASES)
def test_roi_align_fwd_dyadic_set_vs_fp64(size, sr, scale, ch):
    """rr_roi_align_fwd on RoIs whose sample positions and weights are exact in fp32 (tests/helpers.py), limit samples
    exactly on -1 / H / W and 1/16 beyond included, so only the sum over taps rounds: |got - ref| <= (n + 3) u
    (S |feat|), n = 4 gh gw.  The fixed-sampling cases (n = 16) are the sharp end: there the bound is a few ulps of
    sum|term|, while 32 x 32 adaptive samples leave a bound of 4099 u.  RoIs entirely outside the map give exactly 0.
    Measured (profiles/roi_fwd_fp64_ratios.txt): the float32 oracle on the CPU and the kernels both stay within 0.2 of
    the bound."""
    from rrnet_amd import ops
    B, H, W = ROI_DYADIC_MAP
    rois = roi_fwd_case(size, sr, scale, ch)
    feat = _features(B, ch, H, W)
    ref = _oracle(feat, rois, size, scale, sr, torch.float64)
    mag = _oracle(feat.abs(), rois, size, scale, sr, torch.float64)
    n = np.array([4 * roi_sample_grid(r, size, scale, sr, np.float32)[2] for r in rois], np.float64)
    with _Calls() as calls:
        out = ops.roi_align_fwd(feat.cuda(), torch.from_numpy(rois).cuda(), size, scale, sr)
    assert calls.n == {"rr_roi_align_fwd": 1}, calls.n
    assert tuple(out.shape) == (len(rois), ch) + size
    got = _np(out)
    tol = (n[:, None, None, None] + 3) * U32 * mag
    err = np.abs(got - ref)
    ratio = (err / np.maximum(tol, 1e-300)).max((1, 2, 3))
    cells = np.array(["%s-%s" % roi_forward_route(r, size, scale, sr, ch) for r in rois])
    print("\nroi fwd dyadic %s sr %d scale %g C %d: max|ref| %.3g  kernel err %.3g  worst err/tol %s"
          % (size, sr, scale, ch, np.abs(ref).max(), err.max(),
             "  ".join("%s (%d) %.3g" % (c, (cells == c).sum(), ratio[cells == c].max()) for c in sorted(set(cells)))))
    assert np.all(got[list(ROI_FWD_OUTSIDE)] == 0.0)
    assert np.all(err <= tol), float((err - tol).max())


def _random_refs(size, sr, ch):
    """(fp64 reference, error of the fp32 oracle) of the random set: the yardstick comes from the oracle alone."""
    B, H, W = ROI_RANDOM_MAP
    rois, feat = roi_random_set(large=True), _features(B, ch, H, W)
    ref = _oracle(feat, rois, size, 1.0, sr, torch.float64)
    return ref, float(np.abs(_oracle(feat, rois, size, 1.0, sr, torch.float32) - ref).max())


@pytest.mark.parametrize("sr", [-1, 2])
@pytest.mark.parametrize("size,ch", [(s, 256) for s in ROI_RANDOM_SIZES] + [((3, 3), 260)])
def test_roi_align_fwd_random_set_vs_fp64(size, ch, sr):
    """rr_roi_align_fwd on arbitrary RoIs from 0.3 to 127 pixels a side, partly beyond the map (at least 10 take
    per-sample taps at (3,3), at least 5 at (7,7)); measured tolerance (the oracle's own forward in fp32).  Measured
    float32 figures (CPU): 2.8e-7 to 5.2e-7 (max|ref| 3.0 to 3.8); the kernels: 2.9e-7 to 4.7e-7.  With start + p * bin
    contracted into an FMA the separable kernel was off by 2.2e-5 / 2.1e-5 at (7,7) and 1.7e-6 / 1.1e-5 at (2,5)
    (tolerances 1.4e-6 to 1.8e-6); at 3 bins p * bin is exact and the 3x3 kernel never differed."""
    from rrnet_amd import ops
    B, H, W = ROI_RANDOM_MAP
    rois = roi_random_set(large=True)
    ref, err32 = _random_refs(size, sr, ch)
    out = ops.roi_align_fwd(_features(B, ch, H, W).cuda(), torch.from_numpy(rois).cuda(), size, 1.0, sr)
    tol = measured_tol(err32, ref)
    err = np.abs(_np(out) - ref).max((1, 2, 3))
    cells = np.array(["%s-%s" % roi_forward_route(r, size, 1.0, sr, ch) for r in rois])
    print("\nroi fwd random %s sr %d C %d: max|ref| %.3g  fp32 err %.3g  kernel err %.3g  tol %.3g  (%s)"
          % (size, sr, ch, np.abs(ref).max(), err32, err.max(), tol,
             "  ".join("%s (%d) %.3g" % (c, (cells == c).sum(), err[cells == c].max()) for c in sorted(set(cells)))))
    assert err.max() <= tol


@pytest.mark.parametrize("r,ch", [(1, 8), (3, 8), (4, 8), (29, 8), (33, 8), (37, 8), (37, 260)])
def test_roi_align_fwd_order_is_a_pure_permutation(r, ch):
    """The 3x3 kernel's `order` table and its XCD block remap only change which workgroup takes which RoI: 1 to 10
    workgroups of 4 RoIs (the remap with and without a remainder of 8), under no table, the spatial order of two frames
    and a random permutation, give the same bits."""
    from rrnet_amd import ops
    B, H, W = ROI_DYADIC_MAP
    rois = roi_fwd_case(*ROI_FWD_CASES[0])[:r]
    rois = rois[np.argsort(rois[:, 0], kind="stable")]                            # packed per frame
    frame_off = np.array([0, (rois[:, 0] == 0).sum(), r], np.int32)
    feat, rd = _features(B, ch, H, W).cuda(), torch.from_numpy(rois).cuda()
    plain = ops.roi_align_fwd(feat, rd, (3, 3))
    spatial = ops.roi_spatial_order(rd, torch.from_numpy(frame_off).cuda())
    perm = torch.from_numpy(np.random.default_rng(r + ch).permutation(r).astype(np.int32)).cuda()
    assert sorted(spatial.tolist()) == list(range(r))
    assert roi_forward_route(rois[0], (3, 3), 1.0, -1, ch)[0] == "3x3"
    for order in (spatial, perm):
        assert order.dtype == torch.int32 and torch.equal(ops.roi_align_fwd(feat, rd, (3, 3), order=order), plain)


def test_roi_align_fwd_entry_points_agree():
    """RF.roi_align (the autograd entry, models/rrnet.py:51) hands out ops.roi_align_fwd's bits; no RoIs: an empty
    [0, C, 3, 3] tensor and no launch (an empty grid would be a launch error)."""
    from rrnet_amd import functional as RF, ops
    B, H, W = ROI_DYADIC_MAP
    feat, rois = _features(B, 8, H, W).cuda(), torch.from_numpy(roi_fwd_case(*ROI_FWD_CASES[0])).cuda()
    assert torch.equal(RF.roi_align(feat, rois, (3, 3)), ops.roi_align_fwd(feat, rois, (3, 3)))
    none = ops.roi_align_fwd(feat, rois[:0], (3, 3))
    torch.cuda.synchronize()
    assert tuple(none.shape) == (0, 8, 3, 3) and none.dtype == torch.float32

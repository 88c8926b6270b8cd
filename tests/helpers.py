"""Shared by the parity tests and by tools/gen_goldens.py: deterministic, platform-stable
weights (numpy PCG64, not torch's RNG) for any reference-keyed state_dict, so fixtures need
to store only inputs and expected outputs."""
import zlib

import numpy as np
import torch


def det_fill(shapes, seed=219):
    """shapes: {key: shape tuple} -> {key: float32 tensor}.  He-style conv weights, BN affine near
    (1, 0), running stats (0, 1), hm-style biases small.  Each key draws from its own stream."""
    out = {}
    for key in sorted(shapes):
        shape = tuple(shapes[key])
        rng = np.random.default_rng([seed, zlib.crc32(key.encode())])
        leaf = key.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            out[key] = torch.zeros((), dtype=torch.long)
        elif leaf == "running_mean":
            out[key] = torch.zeros(shape)
        elif leaf == "running_var":
            out[key] = torch.ones(shape)
        elif len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            out[key] = torch.from_numpy((rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)).astype(np.float32))
        elif leaf == "weight":                       # BN gamma
            out[key] = torch.from_numpy((1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32))
        else:                                        # BN beta / conv bias
            out[key] = torch.from_numpy((0.1 * rng.standard_normal(shape)).astype(np.float32))
    return out


def shapes_of(state_dict):
    return {k: tuple(v.shape) for k, v in state_dict.items()}


def synth_annos(rng, n, img_h, img_w, min_wh=5.0, max_wh=60.0):
    """[n,8] VisDrone-style rows x,y,w,h,score,cls(1..10),trunc,occl."""
    w = np.exp(rng.uniform(np.log(min_wh), np.log(max_wh), n))
    h = np.exp(rng.uniform(np.log(min_wh), np.log(max_wh), n))
    x = rng.uniform(0, img_w - w)
    y = rng.uniform(0, img_h - h)
    cls = rng.integers(1, 11, n)
    a = np.stack([x, y, w, h, np.ones(n), cls, np.zeros(n), np.zeros(n)], 1).astype(np.float32)
    return a


def host_synth_batch(batch_size, height, width, boxes_per_image=100, seed=219, rank=0):
    """The synthetic batch recipe with the targets built by the ORACLE's host pipeline (oracle/targets.py), all on
    the CPU: what the parity tests feed to the oracle and (moved to the device) to the HIP path."""
    from oracle.targets import host_batch
    from rrnet_amd.datasets.synthetic import synth_frames
    return host_batch(*synth_frames(batch_size, height, width, boxes_per_image, seed, rank))


# ------------------------------------------------------------------------------------------------------------------
# Analytic pins for RoIAlign (torchvision.ops.roi_align is third-party and absent: models/rrnet.py:51).  Bilinear
# interpolation reproduces a map f(x, y) = a*x + b*y + c exactly, so the published definition (legacy coordinates,
# adaptive ceil(size / bins) sampling grid, RoI size clamped to >= 1, samples outside [-1, H] x [-1, W] contribute
# zero but still count, coordinates clamped into the map) can be evaluated in closed form WITHOUT any bilinear
# weights or indices: each bin = sum over its valid samples of f(clip(x), clip(y)) / (gh * gw).
# ------------------------------------------------------------------------------------------------------------------
def linear_map(n, ch, height, width, seed=0):
    """feat[b, k, y, x] = a[b,k]*x + b_[b,k]*y + c[b,k]  (float32 tensor [n,ch,H,W]) and the float64 coefficients."""
    rng = np.random.default_rng(seed)
    a, b, c = (rng.uniform(-1, 1, (n, ch)) for _ in range(3))
    ys, xs = np.mgrid[0:height, 0:width].astype(np.float64)
    f = a[:, :, None, None] * xs + b[:, :, None, None] * ys + c[:, :, None, None]
    return torch.from_numpy(f.astype(np.float32)), (a, b, c)


def roi_align_on_linear_map(rois, coef, height, width, out_size, sampling_ratio=-1):
    """Closed-form RoIAlign of the map of `linear_map` -> float64 [K, ch, ph, pw]."""
    a, b, c = coef
    ph, pw = out_size
    rois = np.asarray(rois, np.float64)
    out = np.zeros((rois.shape[0], a.shape[1], ph, pw))
    for r, (bi, x1, y1, x2, y2) in enumerate(rois):
        bi = int(bi)
        rw, rh = max(x2 - x1, 1.0), max(y2 - y1, 1.0)
        gh = sampling_ratio if sampling_ratio > 0 else int(np.ceil(rh / ph))
        gw = sampling_ratio if sampling_ratio > 0 else int(np.ceil(rw / pw))
        for i in range(ph):
            ys = y1 + i * rh / ph + (np.arange(gh) + 0.5) * (rh / ph) / gh
            for j in range(pw):
                xs = x1 + j * rw / pw + (np.arange(gw) + 0.5) * (rw / pw) / gw
                yy, xx = np.meshgrid(ys, xs, indexing="ij")
                ok = (yy >= -1.0) & (yy <= height) & (xx >= -1.0) & (xx <= width)
                yc, xc = np.clip(yy, 0, height - 1), np.clip(xx, 0, width - 1)
                val = a[bi][:, None, None] * xc + b[bi][:, None, None] * yc + c[bi][:, None, None]
                out[r, :, i, j] = (val * ok).sum((1, 2)) / (gh * gw)
    return out


ROI_PIN_CASES = np.array([
    [0, 2.3, 1.2, 9.7, 8.1],          # interior, fractional
    [1, 0.0, 0.0, 23.0, 19.0],        # the whole map
    [0, 4.0, 5.0, 13.0, 11.0],        # integer corners
    [1, 10.2, 11.9, 10.9, 12.3],      # smaller than one pixel: the size clamp (>= 1) decides the bins
    [0, 7.0, 3.0, 7.0, 3.0],          # zero size
    [0, -3.0, -2.5, 4.0, 3.0],        # partly beyond the top-left: samples < -1 are cut, [-1, 0) clamps to 0
    [1, 18.0, 15.0, 30.0, 28.0],      # beyond the bottom-right: samples > W / > H are cut, (W-1, W] clamps
    [0, -9.0, -9.0, -2.0, -2.0],      # entirely outside: all zero
    [1, 5.5, 5.5, 17.0, 6.0],         # flat: height clamp, wide bins
    [0, 0.5, 0.5, 22.5, 18.5],        # many samples per bin (adaptive grid 8 x 6)
], np.float32)


# ------------------------------------------------------------------------------------------------------------------
# Seeded host-side inputs for the fp64 kernel checks (tests/test_criterion_gpu.py, tests/test_roi_tail_gpu.py,
# tests/test_train_gpu.py).  Each generator states what it promises; tests/test_host_logic.py checks the promises.
# ------------------------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24                                     # unit roundoff of float32
FOCAL_CLAMP_LOGIT = float(np.log(1e-4 / (1 - 1e-4)))  # sigmoid(x) == 1e-4 at x = -9.21024 (and 1 - 1e-4 at +9.21024)
FOCAL_BAND = 5e-3                                    # no logit lies within this of +-FOCAL_CLAMP_LOGIT
STAGE2_IOU_BAND = 1e-4                               # no fp64 IoU lies within this of 0.5


def focal_inputs(shape, seed, with_pos=True):
    """(logits, gt) float32 NCHW arrays of `shape` for the fused focal loss.  Logits ~ N(-2, 4^2) with +-30 and +-100
    sprinkled in (saturated: the clamp passes no gradient); values inside the clamp band are moved out of it, where the
    fp32 and the fp64 clamp masks may legitimately disagree.  gt mixes exact 1.0 peaks (only if `with_pos`), exact 0,
    np.nextafter(1, 0) (a negative with weight (1-g)^4 ~ 1e-29) and Gaussian-like values in (0, 1)."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    x = rng.normal(-2.0, 4.0, n)
    sat = rng.random(n) < 0.02
    x[sat] = rng.choice([-100.0, -30.0, 30.0, 100.0], int(sat.sum()))
    x = x.astype(np.float32).astype(np.float64)
    near = np.abs(np.abs(x) - abs(FOCAL_CLAMP_LOGIT)) < FOCAL_BAND
    side = np.where(np.abs(x) < abs(FOCAL_CLAMP_LOGIT), -1.0, 1.0)
    x[near] = np.sign(x[near]) * (abs(FOCAL_CLAMP_LOGIT) + side[near] * 4 * FOCAL_BAND)
    u = rng.random(n)
    gt = np.exp(-rng.exponential(1.5, n))                          # (0, 1]
    gt = np.where(gt >= 1.0, 0.5, gt)
    gt[u < 0.4] = 0.0
    gt[(u >= 0.4) & (u < 0.45)] = np.nextafter(np.float32(1), np.float32(0))
    if with_pos:
        gt[(u >= 0.45) & (u < 0.5)] = 1.0
        gt[0] = 1.0
    return x.astype(np.float32).reshape(shape), gt.astype(np.float32).reshape(shape)


def regl1_inputs(batch, height, width, seed, channels=2, slots=24, all_masked=False):
    """(pred [B,C,H,W], mask [B,M,1], ind [B,M,1], target [B,M,C]) float32, M = the longest per-image slot list with
    the shorter ones zero-padded (ind 0, mask 0), as collate_ctnet pads them.  Every image holds two valid slots on one
    pixel and three on another (the backward's atomic scatter), valid slots with target == pred exactly (sign 0),
    masked slots whose ind is a valid object's pixel or H*W-1.  `all_masked` zeroes the whole mask; slots=0 gives M=0."""
    rng = np.random.default_rng(seed)
    hw = height * width
    pred = rng.normal(0.0, 2.0, (batch, channels, height, width)).astype(np.float32)
    if slots == 0:
        return (pred, np.zeros((batch, 0, 1), np.float32), np.zeros((batch, 0, 1), np.float32),
                np.zeros((batch, 0, channels), np.float32))
    counts = [slots] + [int(rng.integers(slots // 2, slots + 1)) for _ in range(batch - 1)]
    mask = np.zeros((batch, slots, 1), np.float32)
    ind = np.zeros((batch, slots, 1), np.float32)
    target = np.zeros((batch, slots, channels), np.float32)
    for b, cnt in enumerate(counts):
        nvalid = cnt - 3
        pix = rng.choice(hw, nvalid, replace=False)
        pix[1] = pix[0]                                  # two objects on one pixel
        pix[3] = pix[4] = pix[2]                         # three on another
        ind[b, :nvalid, 0] = pix
        mask[b, :nvalid, 0] = 1.0
        ind[b, nvalid:cnt, 0] = [pix[5], pix[0], hw - 1]  # masked slots pointing at real pixels
        flat = pred[b].reshape(channels, hw)
        target[b, :cnt] = (rng.normal(0.0, 2.0, (cnt, channels))).astype(np.float32)
        target[b, 6, :] = flat[:, int(ind[b, 6, 0])]      # pred == target on both channels
        target[b, 7, 0] = flat[0, int(ind[b, 7, 0])]      # ... and on one channel
        target[b, 1, 1] = flat[1, int(ind[b, 1, 0])]      # ... on a shared pixel
    if all_masked:
        mask[:] = 0.0
    return pred, mask, ind, target


def _iou64(a, b):
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = np.maximum(a[:, None, :2], b[None, :, :2])
    rb = np.minimum(a[:, None, 2:], b[None, :, 2:])
    wh = np.clip(rb - lt, 0, None)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area_a[:, None] + area_b[None, :] - inter)


def stage2_iou_margins(rois, gt, scale):
    """Per RoI: (distance of the nearest fp64 IoU to 0.5, gap between the best IoU and the best IoU of a gt box that
    differs from the first maximising box, inf when none).  rois [R,5] feature coords, gt [B,G,>=4] xyxy."""
    rois = np.asarray(rois, np.float64)
    gt = np.asarray(gt, np.float64)
    d05 = np.empty(len(rois))
    gap = np.empty(len(rois))
    for r, row in enumerate(rois):
        g = gt[int(row[0]), :, :4]
        iou = _iou64(row[None, 1:5] * scale, g)[0]
        d05[r] = np.abs(iou - 0.5).min()
        best = int(np.argmax(iou))
        other = np.any(g != g[best], axis=1)
        gap[r] = iou[best] - iou[other].max() if other.any() else np.inf
    return d05, gap


def stage2_inputs(seed, batch=8, per_image=300, n_gt=100, scale=4.0, img=512.0, nopos_image=3, allpos_image=5):
    """(rois [R,5] feature coords, reg [R,4], gt [B,G,8] xyxy image coords) float32.  Rows of gt past each image's
    object count are zero; gt rows 1 and 6, 7 repeat rows 0 and 5 exactly.  RoIs are jittered gt boxes and random boxes,
    all of positive area inside the image, shuffled so that images interleave; image `nopos_image` has only RoIs far
    smaller than any gt box (no positive), every RoI of `allpos_image` is positive.  No fp64 IoU lies within
    STAGE2_IOU_BAND of 0.5, and a positive RoI's best IoU leads the best IoU of any differing gt box by more than the
    band (fp32 and fp64 pick the same target)."""
    rng = np.random.default_rng(seed)
    gt = np.zeros((batch, n_gt, 8), np.float32)
    for b in range(batch):
        cnt = int(rng.integers(n_gt // 3, n_gt - 5))
        wh = np.exp(rng.uniform(np.log(12), np.log(120), (cnt, 2)))
        xy = rng.uniform(0, img - wh)
        gt[b, :cnt, :4] = np.concatenate([xy, xy + wh], 1)
        gt[b, :cnt, 4] = 1.0
        gt[b, :cnt, 5] = rng.integers(1, 11, cnt)
        gt[b, 1] = gt[b, 0]
        gt[b, 6] = gt[b, 7] = gt[b, 5]

    def draw(b, kind):
        g = gt[b, :, :4].astype(np.float64)
        live = np.flatnonzero(g[:, 2] > 0)
        if kind == "tiny":
            wh = rng.uniform(1.0, 3.0, 2)
            xy = rng.uniform(0, img - wh)
            return np.concatenate([xy, xy + wh])
        if kind == "random":
            wh = np.exp(rng.uniform(np.log(4), np.log(150), 2))
            xy = rng.uniform(0, img - wh)
            return np.concatenate([xy, xy + wh])
        box = g[rng.choice(live)]
        size = np.tile(box[2:] - box[:2], 2)
        sigma = 0.03 if kind == "tight" else 0.15
        out = box + rng.normal(0, sigma, 4) * size
        out[:2] = np.clip(out[:2], 0, img - 2)
        out[2:] = np.clip(np.maximum(out[2:], out[:2] + 1.0), 1, img)
        return out

    rows = []
    for b in range(batch):
        for _ in range(per_image):
            kind = ("tiny" if b == nopos_image else "tight" if b == allpos_image
                    else rng.choice(["jitter", "jitter", "random"]))
            while True:
                box = (draw(b, kind) / scale).astype(np.float32)
                row = np.concatenate([[b], box]).astype(np.float32)
                d05, gap = stage2_iou_margins(row[None], gt, scale)
                best = stage2_best_iou(row, gt, scale)
                if d05[0] <= STAGE2_IOU_BAND or (gap[0] <= STAGE2_IOU_BAND and best > 0.5):
                    continue
                if b == allpos_image and not best > 0.5:
                    continue
                break
            rows.append(row)
    rois = np.stack(rows)[rng.permutation(len(rows))]
    reg = rng.normal(0.0, 1.0, (len(rois), 4)).astype(np.float32)
    return rois, reg, gt


def stage2_best_iou(row, gt, scale):
    g = np.asarray(gt, np.float64)[int(row[0]), :, :4]
    return float(_iou64(np.asarray(row, np.float64)[None, 1:5] * scale, g).max())


# RoIAlign backward: a RoI set on which every sample position and bilinear weight is exact in float32.  RoI corners are
# multiples of 1/8 (in feature-map units, i.e. after spatial_scale) and the bin sizes are dyadic with ceil(bin) a power
# of two, so bin / samples, the positions, 1 - frac and the weight products carry few bits; samples per bin is a power
# of two, so weight / count is exact too.  The sum over taps is then the only rounding, in any order, with or without
# FMA contraction.
ROI_DYADIC_BINS = (1.75, 3.5, 15.5, 31.5)             # adaptive grid: 2, 4, 16, 32 samples (32 takes the > 16 path)
ROI_DYADIC_BIN_P = (0.4, 0.4, 0.15, 0.05)
ROI_DYADIC_BINS_SR2 = (0.625, 1.75, 2.5, 3.5, 5.25, 15.5)


def roi_dyadic_set(seed, out_size, sampling_ratio, spatial_scale, height, width, n=40, race=500):
    """rois [K,5] float32 (input coordinates: feature units / spatial_scale) on images 0 and 1 of a batch of 3 (image 2
    is never touched): n random dyadic RoIs, partly outside the map, two entirely outside it, and `race` identical RoIs
    over one ~6x6 patch of image 1 (the backward's atomics race on its pixels; race=0: none, any number of bins)."""
    rng = np.random.default_rng(seed)
    ph, pw = out_size
    rows = []
    for _ in range(n):
        if sampling_ratio > 0:
            by, bx = rng.choice(ROI_DYADIC_BINS_SR2, 2)
        else:
            by, bx = rng.choice(ROI_DYADIC_BINS, 2, p=ROI_DYADIC_BIN_P)
        y1 = rng.integers(-24, 8 * height) / 8.0
        x1 = rng.integers(-24, 8 * width) / 8.0
        rows.append([rng.integers(0, 2), x1, y1, x1 + pw * bx, y1 + ph * by])
    rows.append([0, -40.0, -40.0, -40.0 + pw * 1.75, -40.0 + ph * 1.75])           # every sample < -1
    rows.append([1, width + 2.0, 1.0, width + 2.0 + pw * 1.75, 1.0 + ph * 1.75])     # every sample > W
    if race:                                             # the patch holds at most 7 bins per axis
        ry = max(b for b in (0.875, 1.0, 1.75, 2.0) if ph * b <= 6.25)
        rx = max(b for b in (0.875, 1.0, 1.75, 2.0) if pw * b <= 6.25)
        rows += [[1, 5.0, 3.0, 5.0 + pw * rx, 3.0 + ph * ry]] * race
    rois = np.array(rows, np.float64)
    rois[:, 1:] /= spatial_scale
    return rois.astype(np.float32)


# (out_size, sampling_ratio, spatial_scale, channels) of tests/test_roi_tail_gpu.py: every bin shape meets both sampling
# modes, both scales and all three channel counts (6 is not a multiple of 4)
ROI_DYADIC_CASES = [((3, 3), -1, 1.0, 256), ((3, 3), 2, 1.0, 12), ((3, 3), -1, 0.25, 6), ((3, 3), 2, 0.25, 256),
                    ((7, 7), -1, 1.0, 12), ((7, 7), 2, 1.0, 6), ((7, 7), -1, 0.25, 256), ((7, 7), 2, 0.25, 12),
                    ((2, 5), -1, 1.0, 6), ((2, 5), 2, 1.0, 256), ((2, 5), -1, 0.25, 12), ((2, 5), 2, 0.25, 6)]
ROI_DYADIC_MAP = (3, 30, 36)                          # batch, height, width


def roi_dyadic_case(size, sr, scale, ch, race=500):
    """The dyadic RoI set of one ROI_DYADIC_CASES entry."""
    _, h, w = ROI_DYADIC_MAP
    return roi_dyadic_set(seed=100 * size[0] + 10 * size[1] + ch + (sr > 0), out_size=size, sampling_ratio=sr,
                          spatial_scale=scale, height=h, width=w, race=race)


def roi_sample_grid(roi, out_size, spatial_scale, sampling_ratio, dtype):
    """oracle.ops.roi_align's sample positions of one RoI, evaluated in `dtype` (np.float32 reproduces the oracle's
    rounding step by step) -> (ys [ph, gh], xs [pw, gw], gh * gw)."""
    f = dtype
    ph, pw = out_size
    x1, y1, x2, y2 = (f(f(roi[i]) * f(spatial_scale)) for i in range(1, 5))
    rw, rh = f(max(f(x2 - x1), f(1))), f(max(f(y2 - y1), f(1)))
    bh, bw = f(rh / f(ph)), f(rw / f(pw))
    gh = sampling_ratio if sampling_ratio > 0 else int(np.ceil(rh / ph))
    gw = sampling_ratio if sampling_ratio > 0 else int(np.ceil(rw / pw))
    ys = np.array([[f(y1 + f(i) * bh + f(f(iy) + f(0.5)) * bh / f(gh)) for iy in range(gh)] for i in range(ph)], dtype)
    xs = np.array([[f(x1 + f(j) * bw + f(f(ix) + f(0.5)) * bw / f(gw)) for ix in range(gw)] for j in range(pw)], dtype)
    return ys, xs, gh * gw


def bilinear_weights64(y, x, height, width):
    """oracle.ops._bilinear_weights in float64 arithmetic."""
    if y < -1.0 or y > height or x < -1.0 or x > width:
        return False, None, None
    y, x = max(float(y), 0.0), max(float(x), 0.0)
    y_low, x_low = int(y), int(x)
    if y_low >= height - 1:
        y_high = y_low = height - 1
        y = float(y_low)
    else:
        y_high = y_low + 1
    if x_low >= width - 1:
        x_high = x_low = width - 1
        x = float(x_low)
    else:
        x_high = x_low + 1
    ly, lx = y - y_low, x - x_low
    hy, hx = 1.0 - ly, 1.0 - lx
    return True, (y_low * width + x_low, y_low * width + x_high, y_high * width + x_low, y_high * width + x_high), \
        (hy * hx, hy * lx, ly * hx, ly * lx)


def roi_tap_counts(rois, out_size, spatial_scale, sampling_ratio, batch, height, width):
    """Number of nonzero bilinear taps (sample x corner, over all RoIs and bins) that land on each pixel
    [batch, height, width]: the number of terms the RoIAlign backward adds into each gradient element."""
    from oracle.ops import _bilinear_weights
    uniq, mult = np.unique(np.asarray(rois, np.float32), axis=0, return_counts=True)
    cnt = np.zeros(batch * height * width)
    for roi, k in zip(uniq, mult):
        ys, xs, _ = roi_sample_grid(roi, out_size, spatial_scale, sampling_ratio, np.float32)
        base = int(roi[0]) * height * width
        for y in ys.ravel():
            for x in xs.ravel():
                ok, idx, w = _bilinear_weights(y, x, height, width)
                if ok:
                    for q in range(4):
                        if w[q] != 0:
                            cnt[base + idx[q]] += k
    return cnt.reshape(batch, height, width)


# RoIAlign forward (tests/test_roi_fwd_gpu.py): the dyadic sets above without the race patch (identical RoIs add nothing
# to a forward), more cases for the routes of rr_roi_align_fwd that the twelve do not reach, and RoIs whose limit
# samples lie exactly on the inclusive limits -1 and H / W of the inside test.
ROI_FWD_CASES = ROI_DYADIC_CASES + [
    ((3, 3), -1, 1.0, 260),                           # 3x3 kernel, second channel pass with one live lane
    ((7, 7), 2, 0.25, 260),                           # separable kernel, same
    ((8, 8), -1, 1.0, 4),                             # the most bins the separable kernel takes, one lane
    ((9, 9), -1, 1.0, 8),                             # generic kernel at a multiple of 4 channels
    ((1, 9), 2, 0.25, 8),                             # generic, fixed sampling
    ((3, 3), -1, 1.0, 4)]                             # 3x3, one lane
ROI_FWD_OUTSIDE = (40, 41)                            # rows of roi_fwd_case entirely outside the map


def roi_boundary_set(out_size, spatial_scale, height, width):
    """rois [8,5] float32 with bins of 1.75 on both axes (2 samples per bin and axis under either sampling mode, 0.875
    apart, the first 0.4375 inside the RoI): the first sample row exactly -1, the last exactly H, the same in x, and
    after each its twin moved 1/16 outward, whose limit sample the inside test cuts.  Every coordinate is a multiple
    of 1/16: positions, weights and their products are exact in float32."""
    ph, pw = out_size
    top, left = -1.4375, -1.4375
    bottom, right = height - 1.75 * ph + 0.4375, width - 1.75 * pw + 0.4375
    rows = []
    for k, (x1, y1, dx, dy) in enumerate([(4.0, top, 0, -1), (6.5, bottom, 0, 1), (left, 3.0, -1, 0), (right, 5.5, 1, 0)]):
        for out in (0.0, 0.0625):
            x, y = x1 + dx * out, y1 + dy * out
            rows.append([k % 2, x, y, x + 1.75 * pw, y + 1.75 * ph])
    rois = np.array(rows, np.float64)
    rois[:, 1:] /= spatial_scale
    return rois.astype(np.float32)


def roi_fwd_case(size, sr, scale, ch):
    """The RoIs of one ROI_FWD_CASES entry: the dyadic set of that entry (rows ROI_FWD_OUTSIDE beyond the map), then
    roi_boundary_set."""
    _, h, w = ROI_DYADIC_MAP
    return np.concatenate([roi_dyadic_case(size, sr, scale, ch, race=0), roi_boundary_set(size, scale, h, w)])


def roi_forward_route(roi, out_size, spatial_scale, sampling_ratio, channels):
    """(kernel, branch) that rr_roi_align_fwd (csrc/roialign.hip) takes for one RoI, restated in float32: kernel "3x3",
    "sep" or "generic"; branch "F" (footprint / separable walk) or "P" (per-sample taps; the generic kernel has no
    other)."""
    f = np.float32
    ph, pw = out_size
    if channels % 4 == 0 and (ph, pw) == (3, 3):
        kernel = "3x3"
    elif channels % 4 == 0 and ph <= 8 and pw <= 8:      # SEP_MAXBINS
        kernel = "sep"
    else:
        return "generic", "P"
    x1, y1, x2, y2 = (f(f(roi[i]) * f(spatial_scale)) for i in range(1, 5))
    rw, rh = f(max(f(x2 - x1), f(1))), f(max(f(y2 - y1), f(1)))
    bh, bw = f(rh / f(ph)), f(rw / f(pw))
    gh = sampling_ratio if sampling_ratio > 0 else int(np.ceil(bh))
    gw = sampling_ratio if sampling_ratio > 0 else int(np.ceil(bw))
    walk = gh <= 16 and gw <= 16 and bh <= f(gh) and bw <= f(gw)      # SEP_MAXG
    return kernel, "F" if walk else "P"


ROI_RANDOM_SIZES = ((3, 3), (7, 7), (2, 5), (9, 9))
ROI_RANDOM_MAP = (3, 70, 90)                          # batch, height, width


def roi_random_set(large=False):
    """rois [44,5] float32 on images 0 and 1 of a batch of 3: the recipe of
    test_roi_align_large_and_random_rois_vs_oracle (tests/test_model_gpu.py): random RoIs from 0.3 to 30 pixels, partly
    outside, four large / border / outside ones.  large=True appends twelve RoIs of 50 to 127 pixels a side, partly
    beyond the map: sides above 48 take per-sample taps at (3,3) bins under adaptive sampling, sides above 112 at (7,7).
    For every size of ROI_RANDOM_SIZES and both sampling modes float32 and float64 agree on the sampling grid and on
    every sample's inside test, and no sample lies within 1e-3 of -1, H or W (tests/test_host_logic.py)."""
    rng = np.random.default_rng(14)
    n = 40
    xy = rng.uniform(-6, 80, (n, 2)).astype(np.float32)
    wh = np.exp(rng.uniform(np.log(0.3), np.log(30), (n, 2))).astype(np.float32)
    rois = np.concatenate([rng.integers(0, 2, (n, 1)).astype(np.float32), xy, xy + wh], 1)
    rois = np.concatenate([rois, np.array([[0, 1.0, 2.0, 88.0, 68.0], [1, -10, -10, 100, 80], [1, 3, 60, 70, 69.5],
                                           [0, 95, 10, 99, 20]], np.float32)])
    if large:
        rois = np.concatenate([rois, np.array([
            [0, -20.3, -20.6, 100.2, 95.1], [1, 40.3, -61.7, 75.9, 58.8], [0, -33.4, 20.2, 93.1, 49.7],
            [1, -15.2, 5.3, 110.4, 12.9], [0, 60.7, -25.3, 66.1, 101.2], [1, -40.6, 30.4, 80.3, 75.2],
            [0, 10.4, -50.2, 22.7, 72.3], [1, 20.6, 10.3, 95.4, 40.7], [0, -12.7, 35.2, 50.6, 78.9],
            [1, 55.3, -8.4, 70.2, 66.3], [0, 5.8, 15.6, 84.3, 22.1], [1, 30.2, 42.7, 97.6, 93.4]], np.float32)])
    return rois


def measured_tol(err32, ref):
    """Where only the rounding order differs: 4x the error of the same computation in float32 on the CPU against
    float64, with a floor of 2u max|ref|."""
    return max(4.0 * float(err32), 2.0 * U32 * float(np.abs(ref).max(initial=0.0)))


def adam_grads(rng, scales, zero_frac=0.05):
    """One step's synthetic gradient: per-element magnitude `scales` times N(0,1), with exact zeros."""
    g = scales * rng.standard_normal(scales.shape)
    g[rng.random(scales.shape) < zero_frac] = 0.0
    return g.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------
# SyncBN: training-mode BatchNorm over the CONCATENATION of per-rank shards, evaluated in float64 on the host
# (tests/test_syncbn_gpu.py, tests/test_dp_gpu.py; tests/test_host_logic.py holds it against torch's own batch_norm).
# ------------------------------------------------------------------------------------------------------------------
def _chan64(t):
    return torch.as_tensor(t).detach().cpu().double().view(1, -1, 1, 1)


def syncbn_ref64(ys, gamma, beta, eps, momentum=0.1, running_mean=None, running_var=None, dzs=None, masks=None):
    """ys: per-rank pre-BN tensors [n_i,C,H_i,W_i] (any float dtype, read as float64); gamma / beta [C].
    -> dict of float64 tensors:
      count (float: samples per channel over all shards), local_sums[i] = [sum y | sum y^2] of shard i ([2C]: what a rank
      puts into the exchange buffer in front of its count), sums (their total), mean, var (biased), invstd, scale
      (gamma * invstd), shift (beta - mean * scale), out[i] = y_i * scale + shift, and — given running_mean /
      running_var — their momentum update with the unbiased variance var * count / (count - 1).
    With dzs (per-rank gradients w.r.t. out[i]; masks[i], if given, multiplies dz_i: the ReLU mask):
      d[i] (the masked gradient), local_bwd[i] = [sum d | sum d * xhat] of shard i ([2C]: dbeta and dgamma a rank
      accumulates BEFORE the exchange), bwd_sums (their total = the full-batch dbeta | dgamma), and
      dx[i] = gamma * invstd * (d_i - sum d / count - xhat_i * sum(d * xhat) / count)."""
    ys = [torch.as_tensor(y).detach().cpu().double() for y in ys]
    c = ys[0].shape[1]
    g64, b64 = _chan64(gamma), _chan64(beta)
    count = float(sum(y.numel() // c for y in ys))
    local = [torch.cat([y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))]) for y in ys]
    sums = torch.stack(local).sum(0)
    mean = sums[:c] / count
    var = (sums[c:] / count - mean * mean).clamp(min=0.0)
    # (the two-pass variance: the one-pass form above is what the kernels evaluate, in float64 both agree to ~1e-16 |y|^2)
    var2 = sum(((y - mean.view(1, -1, 1, 1)) ** 2).sum((0, 2, 3)) for y in ys) / count
    invstd = 1.0 / torch.sqrt(var2 + eps)
    scale = g64.view(-1) * invstd
    shift = b64.view(-1) - mean * scale
    r = dict(count=count, local_sums=local, sums=sums, mean=mean, var=var2, var_one_pass=var, invstd=invstd, scale=scale,
             shift=shift, out=[y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) for y in ys])
    if running_mean is not None:
        unbiased = var2 * count / (count - 1.0) if count > 1 else var2
        r["running_mean"] = (1.0 - momentum) * torch.as_tensor(running_mean).detach().cpu().double() + momentum * mean
        r["running_var"] = (1.0 - momentum) * torch.as_tensor(running_var).detach().cpu().double() + momentum * unbiased
    if dzs is not None:
        ds = [torch.as_tensor(dz).detach().cpu().double() for dz in dzs]
        if masks is not None:
            ds = [d * torch.as_tensor(m).detach().cpu().double() for d, m in zip(ds, masks)]
        xh = [(y - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1) for y in ys]
        lb = [torch.cat([d.sum((0, 2, 3)), (d * x).sum((0, 2, 3))]) for d, x in zip(ds, xh)]
        bs = torch.stack(lb).sum(0)
        sdy, sdx = (bs[:c] / count).view(1, -1, 1, 1), (bs[c:] / count).view(1, -1, 1, 1)
        a = scale.view(1, -1, 1, 1)
        r.update(d=ds, xhat=xh, local_bwd=lb, bwd_sums=bs, dx=[a * (d - sdy - x * sdx) for d, x in zip(ds, xh)])
    return r


# ------------------------------------------------------------------------------------------------------------------
# fp32 convolutions against float64 (tests/test_conv_fp64_gpu.py; tests/test_host_logic.py checks the promises made here).
# The yardstick for "what a correct fp32 kernel may err by" is a MODEL written from the definition of the operation: the
# products of one output, rounded to float32 and added one after the other in float32 (seq32_error).  A correct kernel's
# chains are never longer than that one (the matrix instruction adds 2 products per step, tiles split the reduction,
# split-K shortens it further), so its error should not exceed the model's by more than a small factor, CONV_MARGIN.
# ------------------------------------------------------------------------------------------------------------------
CONV_SAMPLES = 4096          # sampled outputs per tensor (seeded)
CONV_MARGIN_CAP = 8          # a case that needs more than this is a finding, not a reason to raise the margin
CONV_MARGIN = 8              # = the cap: the grid has not been measured on an MI355X yet.  Rule for lowering it: the largest ratio
                             # tests/test_conv_fp64_gpu.py prints, rounded up to a power of two, not below 2 (CPU float32 conv2d: 1.8)


def conv_ref64(x, w, bias, stride, pad, relu, gy=None):
    """F.conv2d on the CPU in float64 (+ autograd) -> (y, dx, dw) float64 tensors; dx = dw = None without gy.
    x [N,C,H,W], w [K,C,R,S], bias [K] | None, pad (pad_h, pad_w), gy [N,K,P,Q]: the gradient w.r.t. the (post-ReLU)
    output.  With relu the gradient mask comes from the float64 y."""
    import torch.nn.functional as F
    x64 = torch.as_tensor(x).detach().cpu().double().clone().requires_grad_(gy is not None)
    w64 = torch.as_tensor(w).detach().cpu().double().clone().requires_grad_(gy is not None)
    b64 = None if bias is None else torch.as_tensor(bias).detach().cpu().double()
    y = F.conv2d(x64, w64, b64, stride=stride, padding=tuple(pad))
    if relu:
        y = F.relu(y)
    if gy is None:
        return y.detach(), None, None
    y.backward(torch.as_tensor(gy).detach().cpu().double())
    return y.detach(), x64.grad, w64.grad


def conv_bias_clear_of_zero(y_nobias, bias, band=1e-3, step=2.5e-3):
    """bias [K] float32 moved, channel by channel and in steps of `step`, until no element of y_nobias[:, k] + bias[k] lies
    within `band` of 0 (y_nobias: float64 [N,K,P,Q], the convolution without bias) -> float32 array."""
    y = np.asarray(y_nobias, np.float64)
    b = np.asarray(bias, np.float32).copy()
    for k in range(len(b)):
        col = y[:, k].ravel()
        for _ in range(1000):
            if np.abs(col + np.float64(b[k])).min() > 2 * band:
                break
            b[k] = np.float32(b[k] + step)
        else:
            raise AssertionError("no bias found for channel %d" % k)
    return b


def conv_sample_positions(shape, seed, count=CONV_SAMPLES, keep=None):
    """`count` seeded positions of a tensor of `shape` -> tuple of index arrays (with repeats where the tensor is small).
    keep: boolean array of `shape`; only positions where it is True are drawn."""
    rng = np.random.default_rng(seed)
    if keep is None:
        flat = rng.integers(0, int(np.prod(shape)), count)
    else:
        flat = rng.choice(np.flatnonzero(np.asarray(keep).ravel()), count)
    return np.unravel_index(flat, shape)


def _np64(t):
    return t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


def conv_terms(kind, idx, x, w, gy, stride, pad, bias=None, base=None, chunk=1 << 23):
    """The products that make up the sampled outputs `idx` of one convolution pass, gathered from the (zero-padded)
    operands: yields float64 arrays [s, n] that together cover idx in order (chunks of about `chunk` elements).
      kind "fprop": idx = (n, k, p, q) into y;  terms x[n, c, p*st-ph+r, q*st-pw+s] * w[k, c, r, s] over (c, r, s), then bias[k]
      kind "dgrad": idx = (n, c, h, w) into dx; terms gy[n, k, p, q] * w[k, c, r, s] over (k, r, s) with p*st-ph+r == h, after base[idx]
      kind "wgrad": idx = (k, c, r, s) into dw; terms gy[n, k, p, q] * x[n, c, p*st-ph+r, q*st-pw+s] over (n, p, q), after base[idx]
    Taps in the padding appear as exact zeros (adding one changes no float32 sum).  The output size of "wgrad" is gy's (an
    output larger than the symmetric one = more padding at the far edge).  base: the tensor an accumulating call adds into."""
    st, (ph, pw) = stride, pad
    x, w = (None if x is None else _np64(x)), (w if w is None or isinstance(w, tuple) else _np64(w))     # wgrad: w or (R, S)
    gy = None if gy is None else _np64(gy)
    nidx = len(idx[0])
    if kind == "fprop":
        n_all, c_all, h, wd = x.shape
        r, s = w.shape[2:]
        p_all, q_all = (h + 2 * ph - r) // st + 1, (wd + 2 * pw - s) // st + 1
        xp = np.pad(x, ((0, 0), (0, 0), (ph, ph), (pw, pw))) if (ph or pw) else x
        per = c_all * r * s + 1
    elif kind == "dgrad":
        k_all, p_all, q_all = gy.shape[1:]
        r, s = w.shape[2:]
        per = k_all * r * s + 1
    else:
        n_all, c_all, h, wd = x.shape
        _, k_all, p_all, q_all = gy.shape
        r, s = w if isinstance(w, tuple) else w.shape[2:]
        far_h = max(0, (p_all - 1) * st + r - (h + ph))
        far_w = max(0, (q_all - 1) * st + s - (wd + pw))
        xp = np.pad(x, ((0, 0), (0, 0), (ph, far_h), (pw, far_w)))
        per = n_all * p_all * q_all + 1
    step = max(1, chunk // per)
    base = None if base is None else _np64(base)
    N = None
    for lo in range(0, nidx, step):
        i0, i1, i2, i3 = (np.asarray(a[lo:lo + step]) for a in idx)
        m = len(i0)
        if kind == "fprop":
            rows = i2[:, N] * st + np.arange(r)
            cols = i3[:, N] * st + np.arange(s)
            patch = xp[i0[:, N, N, N], np.arange(c_all)[N, :, N, N], rows[:, N, :, N], cols[:, N, N, :]]
            t = (patch * w[i1]).reshape(m, -1)
            tail = np.zeros(m) if bias is None else _np64(bias)[i1]
            yield np.concatenate([t, tail[:, N]], 1)
        elif kind == "dgrad":
            pn = i2[:, N] + ph - np.arange(r)
            qn = i3[:, N] + pw - np.arange(s)
            vh = (pn % st == 0) & (pn // st >= 0) & (pn // st < p_all)
            vw = (qn % st == 0) & (qn // st >= 0) & (qn // st < q_all)
            pi, qi = np.clip(pn // st, 0, p_all - 1), np.clip(qn // st, 0, q_all - 1)
            patch = gy[i0[:, N, N, N], np.arange(k_all)[N, :, N, N], pi[:, N, :, N], qi[:, N, N, :]]
            patch = np.where(vh[:, N, :, N] & vw[:, N, N, :], patch, 0.0)
            t = (patch * w[:, i1].transpose(1, 0, 2, 3)).reshape(m, -1)
            head = np.zeros(m) if base is None else base[i0, i1, i2, i3]
            yield np.concatenate([head[:, N], t], 1)
        else:
            rows = i2[:, N] + st * np.arange(p_all)
            cols = i3[:, N] + st * np.arange(q_all)
            patch = xp[np.arange(n_all)[N, :, N, N], i1[:, N, N, N], rows[:, N, :, N], cols[:, N, N, :]]
            t = (patch * gy[:, i0].transpose(1, 0, 2, 3)).reshape(m, -1)
            head = np.zeros(m) if base is None else base[i0, i1, i2, i3]
            yield np.concatenate([head[:, N], t], 1)


def _seq32(terms):
    terms = np.asarray(terms, np.float64)
    ref = terms.sum(1)
    seq = np.cumsum(terms.astype(np.float32), axis=1, dtype=np.float32)[:, -1].astype(np.float64)
    return ref, seq


def seq32_error(terms):
    """terms [S, n] float64: the products of S outputs.  -> (max-abs, RMS) over the S outputs of the error, against the
    float64 sum, of a chained float32 sum of the float32-rounded products in plain loop order."""
    ref, seq = _seq32(terms)
    err = seq - ref
    return float(np.abs(err).max()), float(np.sqrt(np.mean(err * err)))


def conv_yardstick(chunks, relu=False, head=None):
    """seq32_error over the chunks conv_terms yields -> (ref [S] float64 sums, max_seq, rms_seq).  relu: both the chained
    sum and the float64 sum pass through max(., 0) first (an output the ReLU zeroes carries no error).  head [S]: a second
    triple follows, for the same terms with their first column (an accumulating call's starting value) replaced by head."""
    out = [([], []), ([], [])]
    lo = 0
    for t in chunks:
        for slot in range(1 if head is None else 2):
            if slot == 1:
                t = np.array(t, np.float64)
                t[:, 0] = np.asarray(head, np.float64)[lo:lo + len(t)]
            ref, seq = _seq32(t)
            if relu:
                ref, seq = np.maximum(ref, 0.0), np.maximum(seq, 0.0)
            out[slot][0].append(ref)
            out[slot][1].append(seq - ref)
        lo += len(t)
    res = []
    for refs, errs in out[:1 if head is None else 2]:
        ref, err = np.concatenate(refs), np.concatenate(errs)
        res += [ref, float(np.abs(err).max()), float(np.sqrt(np.mean(err * err)))]
    return tuple(res)


def conv_error_ratios(got_s, ref_s, max_seq, rms_seq, got_all=None, ref_all=None):
    """-> (max-abs error at the samples / max_seq, RMS error at the samples / rms_seq, RMS error over the whole tensor /
    rms_seq or None).  A zero yardstick (exact operands) asks for a zero error: the ratio is then 0 or inf."""
    def ratio(e, bound):
        return 0.0 if e == 0.0 else (float("inf") if bound == 0.0 else e / bound)
    es = np.asarray(got_s, np.float64) - np.asarray(ref_s, np.float64)
    out = [ratio(float(np.abs(es).max()), max_seq), ratio(float(np.sqrt(np.mean(es * es))), rms_seq), None]
    if got_all is not None:
        ea = np.asarray(got_all, np.float64) - np.asarray(ref_all, np.float64)
        out[2] = ratio(float(np.sqrt(np.mean(ea * ea))), rms_seq)
    return tuple(out)


def conv_accepts(ratios, margin=None):
    """The acceptance rule: every ratio of conv_error_ratios is finite and <= margin."""
    margin = CONV_MARGIN if margin is None else margin
    return all(r is None or (np.isfinite(r) and r <= margin) for r in ratios)


def round_sig_bits(a, bits):
    """float64 array rounded (to nearest) to `bits` significant bits."""
    m, e = np.frexp(np.asarray(a, np.float64))
    return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e)


def conv_tap_counts(size, out, r, stride, pad):
    """1-D closed forms of an all-ones convolution: (taps of each output position that fall inside the input [out],
    (output, tap) pairs that reach each input position [size], outputs whose tap t falls inside the input [r])."""
    pos = np.arange(out)[:, None] * stride - pad + np.arange(r)[None, :]
    inside = (pos >= 0) & (pos < size)
    reach = np.zeros(size, np.int64)
    np.add.at(reach, pos[inside], 1)
    return inside.sum(1), reach, inside.sum(0)


# ---- which host route a shape takes: a restatement of the dispatch rules of rrnet_amd/csrc/conv_plan.h, conv.hip ----
# Written from the host code as it stood BEFORE conv_plan.h existed (the two fprop_impl of conv.hip and conv_bf16.hip), and
# kept by hand: tests/test_host_logic.py holds the library's plan (rr_conv_fprop_plan) against it field by field.
_BM, _BK = 128, 32                                  # rr_plan::BM, rr_plan::BK
_SMALL_TILES, _MID_TILES = 16, 48                   # rr_plan::small_tiles() / mid_tiles()
MATH_F32, MATH_BF16, MATH_F16X3 = 0, 1, 2           # the arithmetic argument of rr_conv_fprop_plan
# the fields rr_conv_fprop_plan writes, in its order (include/rrnet_hip.h); after: 0 none, 1 rr_bn_reduce_slab, 2 rr_bn_bwd_reduce, 3 column statistics
CONV_PLAN_FIELDS = ("rows", "scalar", "bn", "blocks", "ks", "pos_major", "xcd_n", "fused", "after", "zero_dst", "zero_slab")


def _cdiv(a, b):
    return -(-a // b)


def pick_ksplit_mirror(blocks, nk):
    """rr_plan::pick_ksplit in float32 arithmetic, the 0.95 hysteresis included (RR_CONV_SPLITK unset)."""
    f = np.float32
    if blocks >= 256 or nk < 16:
        return 1
    best, best_t = 1, f(0)
    ks = 1
    while ks <= 8 and ks <= nk // 8:
        n = (blocks * ks + 255) // 256
        per = f(f(f((nk + ks - 1) // ks) + f(3)) + (f(1) if ks > 1 else f(0)))
        t = f(f(f(n // 2) * f(f(f(2) * per) / f(0.87))) + f(f(n % 2) * f(per / f(0.75))))
        if best_t == 0 or t < f(best_t * f(0.95)):
            best, best_t = ks, t
        ks += 1
    return best


def _fprop_route(n, c, h, w, k, r, s, stride, ph, pw, bias, relu, want_stats, math=MATH_F32, strided=False, link=None,
                 accumulate=False, out_hw=None):
    """rr_plan::fprop_plan restated -> {"labels": set, every name of CONV_PLAN_FIELDS: int}, or None where the arithmetic `math`
    refuses the call.  link: None | "bn" | "relu_bias" (whose backward sums the launch carries); strided: the destination is one
    parity class of a larger map, its grid given by out_hw (16-bit kernels only).  Needs h + 2*ph >= r and w + 2*pw >= s (the
    library divides like C, towards zero)."""
    b16, two_gib = math != MATH_F32, 1 << 31
    if b16 and (c % 4 != 0 or r * s > 64):
        return None                                  # the 16-bit kernels have no scalar gather: refused, not rerouted
    if strided and not b16:
        return None
    p, q = out_hw or ((h + 2 * ph - r) // stride + 1, (w + 2 * pw - s) // stride + 1)
    m = n * p * q
    if p <= 0 or q <= 0 or m >= two_gib:
        return None
    if b16 and (n * h * w * c * 4 >= two_gib or k * r * s * c * 4 >= two_gib or m * k * 4 >= two_gib or (strided and (link or want_stats))):
        return None
    if not b16 and n * h * w * c >= 1 << 40:
        return None
    plan = dict.fromkeys(CONV_PLAN_FIELDS, 0)
    if (not b16 and r == 1 and s == 1 and stride == 1 and ph == 0 and pw == 0 and c in (128, 256) and 48 < k <= 64 and not want_stats
            and link is None and not accumulate and m >= 64 * 1024 and m * c * 4 < two_gib):
        return dict(plan, rows=1, labels={"rows"})
    scalar = not b16 and (c % 4 != 0 or r * s > 64)
    bn = 128 if k > 64 else ((64 if not scalar else 128) if k > 32 else 32)
    if bn == 128 and not scalar and _cdiv(m, _BM) * _cdiv(k, 128) <= _SMALL_TILES:
        bn = 32
    elif bn == 128 and not scalar and _cdiv(m, _BM) * _cdiv(k, 128) <= _MID_TILES:
        bn = 64
    blocks = _cdiv(m, _BM) * _cdiv(k, bn)
    nk = _cdiv(r * s * c, _BK) if scalar else _cdiv(c, _BK) * r * s
    ks = pick_ksplit_mirror(blocks, nk) if (not bias and not relu and k % 4 == 0 and k <= 1024) else 1
    if link == "relu_bias" or strided:
        ks = 1
    labels = {"bn%d" % bn}
    if scalar:
        labels.add("scalar")
    if b16:
        nt, mt = _cdiv(k, bn), _cdiv(m, _BM)
        plan["xcd_n"] = int(nt > 1 and 8 % nt == 0 and mt % (8 // nt) == 0)
    elif (not scalar and not want_stats and link is None and (ph > 0 or pw > 0) and r * s > 1 and p * q <= 16 and n >= 16 * _BM and bn >= 64
            and n * h * w * c * 4 < two_gib and k * r * s * c * 4 < two_gib):
        labels.add("pos_major")
        ks, blocks = 1, p * q * _cdiv(n, _BM) * _cdiv(k, bn)
    if ks > 1:
        labels.add("ksplit>1+stats" if want_stats else "ksplit>1")
    tiles_full = m % _BM == 0 and m * k * 4 < two_gib
    if link == "relu_bias" and not tiles_full:
        return None                                  # the masked store has no fallback pass
    fused = link is not None and ks == 1 and tiles_full
    colstats = ks > 1 and want_stats and link is None
    plan.update(scalar=int(scalar), bn=bn, blocks=blocks, ks=ks, pos_major=int("pos_major" in labels), fused=int(fused),
                after=((1 if fused else 2) if link is not None else (3 if colstats else 0)),
                zero_dst=int(ks > 1 and not accumulate), zero_slab=int(colstats), labels=labels)
    return plan


def conv_routes(n, c, h, w, k, r, s, stride, pad, bias, relu, want_stats, out_h=0, out_w=0):
    """The host route of each pass of one convolution: {"fprop", "dgrad", "wgrad", "dgrad_via_fprop"} -> set of labels.
    A pure-Python mirror of the C rules in rrnet_amd/csrc (the fp32 arithmetic):
      fprop  rr_plan::fprop_plan (conv_plan.h: the rows shortcut, scalar / tile width with small_tiles / mid_tiles, split-K
             with pick_ksplit, pos_major) and launch_igemm (conv.hip):
             rows | bn128 / bn64 / bn32, scalar, pos_major, ksplit>1 (no statistics) / ksplit>1+stats (zero-fill + colstats_kernel)
      dgrad  rr_conv_dgrad (conv.hip) with rr_plan::parity_classes: bn*, scalar, parity4 (stride 2, all four classes have
             taps), parity_live<4 (classes without taps get no workgroups), ksplit>1
      wgrad  rr_conv_wgrad (conv.hip) with rr_plan::pixel_splits: pipe3 / pipe1 (the pipelined 128x128 kernels), 128x128 /
             128x32 / 32x128 / 32x32 (the generic tiles), a_scalar (k % 4 != 0), b_scalar (c % 4 != 0), splits>1; out_h / out_w as there
      dgrad_via_fprop  rr_conv_dgrad_s1 (conv.hip: dgrad_s1, rr_dgrad_s1_geom) = the fprop rules on (dy, flipped filter); empty
             where ops.conv_dgrad cannot take that route (stride > 1, channel counts not multiples of 4, more than 64 taps)."""
    ph, pw = pad
    routes = {"fprop": _fprop_route(n, c, h, w, k, r, s, stride, ph, pw, bias, relu, want_stats)["labels"]}
    p, q = (h + 2 * ph - r) // stride + 1, (w + 2 * pw - s) // stride + 1
    routes["dgrad"] = _dgrad_route(n, c, h, w, k, r, s, stride, ph, pw)["labels"]
    routes["wgrad"] = _wgrad_route(n, c, h, w, k, r, s, stride, ph, pw, out_h, out_w)["labels"]
    via = set()
    if stride == 1 and k % 4 == 0 and c % 4 == 0 and r * s <= 64 and ph < r and pw < s:
        via = _fprop_route(n, k, p, q, c, r, s, 1, r - 1 - ph, s - 1 - pw, False, False, False)["labels"]
    routes["dgrad_via_fprop"] = via
    return routes


# ---- the gradient passes: restatements of the host code of rr_conv_dgrad / rr_conv_wgrad (conv.hip), dgrad_s2_impl / wgrad_impl
# (conv_bf16.hip) and rr_conv16_dgrad_s2 / rr_conv16_wgrad / launch_igemm (conv16.hip) as they stood BEFORE the gradient plans of
# conv_plan.h existed, kept by hand: tests/test_host_logic.py holds the library's plans (rr_conv_grad_plan) against them field by
# field.  Each returns the plan's fields (and the labels the grid-coverage tests use), or None where the entry point refuses.
GRAD_DGRAD, GRAD_DGRAD_S2, GRAD_WGRAD = 0, 1, 2     # the pass argument of rr_conv_grad_plan
FAM_CONV16 = 3                                      # its family argument: a MATH_*, or the kernels of conv16.hip
CONV_GRAD_PLAN_INTS = 44                            # RR_CONV_GRAD_PLAN_INTS
CONV_GRAD_FIELDS = {                                # what rr_conv_grad_plan writes, in its order (include/rrnet_hip.h)
    GRAD_DGRAD: ("scalar", "bn", "blocks", "gy", "parity", "parity_order", "ks", "zero_dst"),
    GRAD_DGRAD_S2: ("p", "q", "zero_dst", "n_launch"),          # then 10 values per launch: dgrad_s2_mirror's "launches"
    GRAD_WGRAD: ("P", "Q", "M", "bm", "bn", "a_scalar", "b_scalar", "pipe", "mt", "nt", "tiles", "splits", "per_split", "grid", "lds"),
}


def refused_call(entry, ints, null=()):
    """Calls entry point `entry` of include/rrnet_hip.h the way tests/golden/conv_grad_refusals.json records a refused call: `ints`
    are its non-pointer arguments in order; every pointer is a dummy host buffer, except those whose position among the pointer
    arguments is in `null`; the stream is null.  -> (return code, rr_last_error).  For calls that are refused before any launch."""
    import ctypes
    from rrnet_amd import _C
    f = _C.fn(entry)
    dummy, values, args, nptr = ctypes.create_string_buffer(256), iter(ints), [], 0
    for j, t in enumerate(f.argtypes):
        if t is not ctypes.c_void_p:
            args.append(next(values))
        elif j == len(f.argtypes) - 1:
            args.append(None)                                # hipStream_t
        else:
            args.append(None if nptr in null else ctypes.addressof(dummy))
            nptr += 1
    rc = f(*args)
    return rc, _C.lib().rr_last_error().decode()


def _dgrad_route(n, c, h, w, k, r, s, stride, ph, pw, accumulate=False):
    """rr_conv_dgrad (conv.hip) with rr_plan::parity_classes restated -> {"labels": set, every name of CONV_GRAD_FIELDS[GRAD_DGRAD]}."""
    if min(n, h, w, c, k, r, s, stride) <= 0 or n * h * w >= 1 << 31:
        return None
    m = n * h * w
    scalar = k % 4 != 0 or c % 4 != 0 or r * s > 64 or stride > 2
    bn = 128 if c > 64 else ((64 if not scalar else 128) if c > 32 else 32)
    if bn == 128 and not scalar and stride == 1 and _cdiv(m, _BM) * _cdiv(c, 128) <= _SMALL_TILES:
        bn = 32
    elif bn == 128 and not scalar and stride == 1 and _cdiv(m, _BM) * _cdiv(c, 128) <= _MID_TILES:
        bn = 64
    blocks, gy = _cdiv(m, _BM) * _cdiv(c, bn), 1
    nk = _cdiv(r * s * k, _BK) if scalar else _cdiv(k, _BK) * r * s
    d = {"bn%d" % bn}
    if scalar:
        d.add("scalar")
    parity = stride == 2 and not scalar
    order, live = 0, 4
    if parity:
        taps = []
        for cl in range(4):
            r0, s0 = ((cl >> 1) + ph) & 1, ((cl & 1) + pw) & 1
            taps.append(((r - r0 + 1) // 2 if r0 < r else 0) * ((s - s0 + 1) // 2 if s0 < s else 0))
        ord_ = [0, 1, 2, 3]                          # the host's exchange sort: classes by falling tap count
        for i in range(4):
            for j in range(i + 1, 4):
                if taps[ord_[j]] > taps[ord_[i]]:
                    ord_[i], ord_[j] = ord_[j], ord_[i]
        order = ord_[0] | ord_[1] << 2 | ord_[2] << 4 | ord_[3] << 6
        taps = [taps[o] for o in ord_]
        while live > 1 and taps[live - 1] == 0:
            live -= 1
        gy = live
        d.add("parity4" if live == 4 else "parity_live<4")
        blocks = _cdiv(n * ((h + 1) // 2) * ((w + 1) // 2), _BM) * _cdiv(c, bn)
        nk = _cdiv(k, _BK) * ((r + 1) // 2) * ((s + 1) // 2)
    ks = 1 if parity else pick_ksplit_mirror(blocks * gy, nk)
    if ks > 1:
        d.add("ksplit>1")
    return dict(labels=d, scalar=int(scalar), bn=bn, blocks=blocks, gy=gy, parity=int(parity), parity_order=order, ks=ks,
                zero_dst=int(((parity and live < 4) or ks > 1) and not accumulate))


def _pixel_splits(tiles, chunks, slots, min_chunks):
    """rr_plan::pixel_splits restated -> (splits, K-steps per split)."""
    splits = slots // tiles if tiles < slots else 1
    splits = max(1, min(splits, _cdiv(chunks, min_chunks)))
    per = _cdiv(chunks, splits)
    return _cdiv(chunks, per), per


def _wgrad_route(n, c, h, w, k, r, s, stride, ph, pw, out_h=0, out_w=0):
    """rr_conv_wgrad (conv.hip) restated -> {"labels": set, every name of CONV_GRAD_FIELDS[GRAD_WGRAD]}."""
    if min(n, h, w, c, k, r, s, stride) <= 0:
        return None
    p, q = (h + 2 * ph - r) // stride + 1, (w + 2 * pw - s) // stride + 1
    pp, qq = (out_h if out_h > 0 else p), (out_w if out_w > 0 else q)
    mw = n * pp * qq
    if not 0 < mw < 1 << 31:
        return None
    bmw, bnw = (128 if k > 32 else 32), (128 if c > 32 else 32)
    mt, nt = _cdiv(k, bmw), _cdiv(c, bnw)
    tiles = mt * nt * r * s
    chunks = _cdiv(mw, _BK)
    a_s, b_s = k % 4 != 0, c % 4 != 0
    pipe_ok = (bmw == 128 and bnw == 128 and not a_s and not b_s and mw * k * 4 < (1 << 31) and n * h * w * c * 4 < (1 << 31))
    wmode = 0 if not pipe_ok else (3 if qq % _BK == 0 else 1)
    slots = 768 if wmode == 3 else 512
    splits, per = _pixel_splits(tiles, chunks, slots, 8)
    g = {"pipe3"} if wmode == 3 else ({"pipe1"} if wmode == 1 else {"%dx%d" % (bmw, bnw)})
    if a_s:
        g.add("a_scalar")
    if b_s:
        g.add("b_scalar")
    if splits > 1:
        g.add("splits>1")
    return dict(labels=g, P=pp, Q=qq, M=mw, bm=bmw, bn=bnw, a_scalar=int(a_s), b_scalar=int(b_s), pipe=wmode, mt=mt, nt=nt, tiles=tiles,
                splits=splits, per_split=per, grid=tiles * splits, lds=4 * (1 if wmode == 3 else 2) * (_BK * bmw + _BK * bnw))


CONV_ROUTE_LABELS = {
    "fprop": {"rows", "pos_major", "bn128", "bn64", "bn32", "scalar", "ksplit>1", "ksplit>1+stats"},
    "dgrad": {"scalar", "parity4", "parity_live<4", "bn128", "bn64", "bn32", "ksplit>1"},
    "wgrad": {"pipe3", "pipe1", "128x128", "128x32", "32x128", "32x32", "a_scalar", "b_scalar", "splits>1"},
}

# (N, C, H, W, K, R, S, stride, pad_h, pad_w, bias, relu, want_stats values, passes: f = fprop, d = dgrad, w = wgrad)
CONV64_GRID = [
    (1, 256, 16, 16, 256, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),     # fprop bn32 split-K (+ stats); dgrad split-K
    (1, 384, 32, 32, 384, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),     # bn64 mid tiles, split-K
    (2, 256, 64, 64, 256, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),     # bn128 pipelined, split-K (128 tiles); wgrad pipe3
    (1, 256, 66, 70, 256, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),     # ragged M tile; wgrad pipe1
    (1, 64, 128, 128, 256, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),    # bn128 with a full first wave: NO split, fused statistics
    (1, 64, 9, 13, 128, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),       # ragged M and N, small
    (2, 128, 15, 17, 256, 1, 1, 2, 0, 0, False, False, (False, True), "fdw"),     # dgrad parity_live<4
    (2, 16, 7, 9, 24, 3, 3, 2, 1, 1, False, False, (False, True), "fdw"),         # dgrad parity4, odd H and W; wgrad 32x32
    (1, 30, 11, 9, 50, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),        # c % 4 != 0: scalar fprop; wgrad 128x32 b_scalar
    (1, 40, 9, 11, 18, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),        # k % 4 != 0: scalar dgrad; wgrad 32x128 a_scalar
    (1, 34, 9, 7, 38, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),         # both: wgrad's generic 128x128 tile, a_ and b_scalar
    (1, 6, 10, 10, 10, 3, 3, 3, 1, 1, False, False, (False, True), "fdw"),        # stride 3: scalar dgrad
    (2, 3, 30, 34, 128, 7, 7, 2, 3, 3, False, False, (False, True), "fdw"),       # stem: 49 taps on 3 channels (scalar gather)
    (1, 256, 20, 12, 1, 17, 1, 1, 8, 0, True, False, (False, True), "fdw"),       # HCov, bias
    (1, 256, 10, 10, 256, 3, 3, 1, 1, 1, True, True, (False, True), "fdw"),       # bias + ReLU keep split-K off
    (2048, 64, 3, 3, 64, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),      # pos_major (without statistics)
    # the row-streaming 1x1 kernel (M = 65536, no statistics).  Forward only: that route exists in the forward pass alone,
    # the gradients of this shape take the bn64 / pipelined routes the cases above hold, and a sampled weight-gradient
    # yardstick here is 4096 chains of 65536 products
    (1, 256, 256, 256, 64, 1, 1, 1, 0, 0, False, False, (False,), "f"),
]
# the weight gradient with the out_h / out_w override (one more output row and column than symmetric padding gives)
CONV64_ASYM_WGRAD = (1, 64, 12, 12, 64, 3, 3, 1, 1, 1, 13, 13)


def conv_grid_routes():
    """{pass: set of labels} over CONV64_GRID (every want_stats value a case runs with) and CONV64_ASYM_WGRAD."""
    seen = {"fprop": set(), "dgrad": set(), "wgrad": set()}
    for cfg in CONV64_GRID:
        n, c, h, w, k, r, s, st, ph, pw, bias, relu, stats, passes = cfg
        for ws in stats:
            rt = conv_routes(n, c, h, w, k, r, s, st, (ph, pw), bias, relu, ws)
            for key, ch in (("fprop", "f"), ("dgrad", "d"), ("wgrad", "w")):
                if ch in passes:
                    seen[key] |= rt[key]
    n, c, h, w, k, r, s, st, ph, pw, oh, ow = CONV64_ASYM_WGRAD
    seen["wgrad"] |= conv_routes(n, c, h, w, k, r, s, st, (ph, pw), False, False, False, oh, ow)["wgrad"]
    return seen


# ---- how a deformable convolution launches: a restatement of the host code of rrnet_amd/csrc/dcn.hip -------------------------------
# Written from dcn.hip as it stood BEFORE csrc/dcn_plan.h existed — fill_args, dcn_fwd_win and the two rr_dcn_fwd* tails,
# dcn_wgrad_win / dcn_wgrad_plain, dcn_dgrad_impl, function by function — and kept by hand: tests/test_host_logic.py holds the
# library's plans (rr_dcn_plan) against it field by field.
DCN_FWD, DCN_WGRAD, DCN_DGRAD = 0, 1, 2                                    # the pass argument of rr_dcn_plan
DCN_HAS_WPACK, DCN_HAS_DYB, DCN_DYB_READY, DCN_ACCUMULATE = 1, 2, 4, 8     # its flags
_DCN_HEAD = ("window", "margin", "WH", "WW", "tiles_y", "tiles_x", "grid", "lds")
DCN_PLAN_FIELDS = {DCN_FWD: _DCN_HEAD + ("wbn", "bn", "pack"),
                   DCN_WGRAD: _DCN_HEAD + ("dy_dma", "ktiles", "per_split", "splits", "dma_window", "mt", "nt", "chunks_per_split"),
                   DCN_DGRAD: _DCN_HEAD + ("zero_dx", "dy_image", "convert_dy", "dma_sweep", "goff_at")}
DCN_PLAN_INTS = 16                                                          # RR_DCN_PLAN_INTS: 8 shared + up to 8 of the pass
# what each entry point of a pass hands its plan: (bf16, flags)
DCN_ENTRY_FLAGS = {
    DCN_FWD: {"rr_dcn_fwd": (0, 0), "rr_dcn_fwd_bf16": (1, 0), "rr_dcn_fwd_bf16_packed": (1, DCN_HAS_WPACK)},
    DCN_WGRAD: {"rr_dcn_wgrad": (0, 0), "rr_dcn_wgrad_bf16": (1, 0), "rr_dcn_wgrad_bf16_img": (1, DCN_HAS_DYB | DCN_DYB_READY)},
    DCN_DGRAD: {"rr_dcn_dgrad": (0, 0), "rr_dcn_dgrad_bf16": (1, 0), "rr_dcn_dgrad_bf16_ws": (1, DCN_HAS_DYB),
                "rr_dcn_dgrad_bf16_img": (1, DCN_HAS_DYB | DCN_DYB_READY),
                "rr_dcn_dgrad_bf16_packed": (1, DCN_HAS_WPACK | DCN_HAS_DYB),
                "rr_dcn_dgrad_bf16_packed+img": (1, DCN_HAS_WPACK | DCN_HAS_DYB | DCN_DYB_READY),
                "rr_dcn_dgrad_bf16_packed+acc": (1, DCN_HAS_WPACK | DCN_HAS_DYB | DCN_ACCUMULATE),
                "rr_dcn_dgrad_bf16_packed+img+acc": (1, DCN_HAS_WPACK | DCN_HAS_DYB | DCN_DYB_READY | DCN_ACCUMULATE)},
}
DCN_ROUTE_LABELS = {      # per pass: (fp32 operands, bf16 operands)
    DCN_FWD: ({"window256", "window256:k>384", "window128", "gather128", "gather32", "margin_shrunk"},
              {"window256+packed", "window256+packed:k>384", "window128", "gather128", "gather32", "margin_shrunk"}),
    DCN_WGRAD: ({"window_f32", "gather", "refused"}, {"window_bf16", "window_dy_dma", "gather", "refused"}),
    DCN_DGRAD: ({"window_f32", "gather", "refused"}, {"window_bf16_convert", "window_bf16_image", "window_dma", "gather", "refused"}),
}


def _c_div(a, b):
    """a / b as C divides ints (towards zero), b > 0."""
    return a // b if a >= 0 else -((-a) // b)


def dcn_plan_mirror(pas, bf16, geo, margin, flags=0):
    """What the entry points of dcn.hip did with geo = (n, c, h, w, k, r, s, stride, pad_h, pad_w, dilation, groups) at window margin
    `margin` (RR_DCN_WINDOW) -> {every name of DCN_PLAN_FIELDS[pas]: int, "labels": set}, or None where the call was refused."""
    n, c, h, w, k, r, s, stride, ph, pw, dil, dg = geo
    two_gib, budget = 1 << 31, 160 * 1024 - 512
    # fill_args
    if min(n, h, w, c, k, r, s, stride, dil, dg) <= 0 or c % 4 or c % dg or (dg != 1 and (c // dg) % 32):
        return None
    p, q = _c_div(h + 2 * ph - (dil * (r - 1) + 1), stride) + 1, _c_div(w + 2 * pw - (dil * (s - 1) + 1), stride) + 1
    m_out = n * p * q
    if p <= 0 or q <= 0 or m_out >= two_gib:
        return None
    plan = dict.fromkeys(DCN_PLAN_FIELDS[pas], 0)
    labels = set()
    cpg = c // dg
    wpack, dyb, ready = bool(flags & DCN_HAS_WPACK), bool(flags & DCN_HAS_DYB), bool(flags & DCN_DYB_READY)

    def window(rw):
        return 8 + (r - 1) * dil + 2 * rw + 1, 16 + (s - 1) * dil + 2 * rw + 1

    def take_window(rw, lds):
        wh, ww = window(rw)
        plan.update(window=1, margin=rw, WH=wh, WW=ww, tiles_y=_cdiv(p, 8), tiles_x=_cdiv(q, 16), lds=lds)

    if pas == DCN_FWD:
        wbn, bn = (256 if (k % 256 == 0 or k > 384) else 128), (128 if k > 32 else 32)
        plan.update(wbn=wbn, bn=bn)
        if margin > 0 and stride == 1 and k > 32 and c % 32 == 0 and h * w < (1 << 30):            # dcn_fwd_win
            for rw in range(margin, 0, -1):
                wh, ww = window(rw)
                lds = wh * ww * 32 * 4 + 128 * r * s * 4 * 8 + 2 * 2 * (128 * 40 + wbn * 40)
                if wh * ww <= 14 * 32 and lds <= budget:
                    take_window(rw, lds)
                    plan["grid"] = n * plan["tiles_y"] * plan["tiles_x"] * _cdiv(k, wbn)
                    # rr_dcn_fwd_bf16_packed hands the workspace on only under these limits; the window launch packs at 256 columns
                    plan["pack"] = int(wbn == 256 and bool(bf16) and wpack and c % 32 == 0 and k * r * s * c * 2 < two_gib)
                    labels.add(("window%d" % wbn) + ("+packed" if plan["pack"] else "") + (":k>384" if wbn == 256 and k % 256 else ""))
                    if rw < margin:
                        labels.add("margin_shrunk")
                    return dict(plan, labels=labels)
        plan["grid"] = _cdiv(m_out, 128) * _cdiv(k, bn)                                               # the tails of rr_dcn_fwd / _bf16
        plan["lds"] = 2 * 2 * (128 * 40 + bn * 40) if bf16 else 4 * 2 * (128 * 36 + bn * 36)
        return dict(plan, labels={"gather%d" % bn})

    if pas == DCN_WGRAD:
        if (margin > 0 and stride == 1 and r * s == 9 and c % 32 == 0 and k % 4 == 0 and h < 32768 and w < 32768
                and (dg == 1 or cpg % 32 == 0)):                                                      # dcn_wgrad_win
            dydma = bool(bf16) and dyb and k % 32 == 0 and m_out * k * 2 < two_gib and n * h * w * c * 4 < two_gib
            for rw in range(margin, 0, -1):
                wh, ww = window(rw)
                lds = 4 * (wh * ww * 32 + 128 * r * s * 4) + 2 * ((256 + r * s * 32) * 72)
                if dydma:
                    lds = lds - 2 * ((256 + r * s * 32) * 72) + 2 * (8 * 6 * 512 + r * s * 64 * 32)
                if lds <= budget:
                    take_window(rw, lds)
                    ntiles = n * plan["tiles_y"] * plan["tiles_x"]
                    ktiles = _cdiv(k, 256)
                    per_split = (c // 32) * ktiles
                    splits = _cdiv(256, per_split)
                    if splits > 8:
                        splits = splits // 8 * 8
                    splits = min(splits, ntiles)
                    plan.update(dy_dma=int(dydma), ktiles=ktiles, per_split=per_split, splits=splits, grid=splits * per_split,
                                dma_window=int(n * h * w * c * 4 < two_gib))
                    return dict(plan, labels={"window_dy_dma" if dydma else ("window_bf16" if bf16 else "window_f32")})
        if k % 4 or (dg != 1 and cpg % 128):                                                          # dcn_wgrad_plain
            return None
        mt, nt = _cdiv(k, 128), _cdiv(c, 128)
        tiles, chunks = mt * nt * r * s, _cdiv(m_out, 32)
        splits = 512 // tiles if tiles < 512 else 1
        splits = max(1, min(splits, _cdiv(chunks, 8)))
        per = _cdiv(chunks, splits)
        splits = _cdiv(chunks, per)
        plan.update(mt=mt, nt=nt, splits=splits, chunks_per_split=per, grid=tiles * splits, lds=4 * 2 * (32 * 128 + 32 * 128))
        return dict(plan, labels={"gather"})

    # dcn_dgrad_impl
    if k % 4 or n * h * w >= two_gib:
        return None
    plan["zero_dx"] = int(not flags & DCN_ACCUMULATE)
    if margin > 0 and stride == 1 and c % 32 == 0 and h < 32768 and w < 32768 and (dg == 1 or cpg % 32 == 0):
        for rw in range(margin, 0, -1):
            wh, ww = window(rw)
            npx = wh * ww
            opa = max(128 * 40 + r * s * 32 * 40, 2 * 128 * 32 + r * s * 32 * 32)
            lds = 4 * (((npx * 33 + 3) & ~3) + 128 * r * s * 7 + npx * 32) + 2 * opa
            if lds <= budget:
                break
        if r * s == 9 and lds <= budget:
            take_window(rw, lds)
            plan["grid"] = n * plan["tiles_y"] * plan["tiles_x"]
            if not bf16:
                return dict(plan, labels={"window_f32"})
            plan["dy_image"] = int(dyb)                        # (k % 4 == 0 here: what is not ready is converted)
            plan["convert_dy"] = int(dyb and not ready)
            if (dyb and wpack and k % 32 == 0 and m_out * k * 2 < two_gib and n * h * w * c * 4 < two_gib and npx <= 368
                    and lds + npx * 4 + 16 <= budget and npx * 33 * 4 >= (128 * 32 + 2 * r * s * 32 * 32) * 2):
                plan.update(dma_sweep=1, goff_at=lds, lds=lds + ((npx * 4 + 15) & ~15))
                return dict(plan, labels={"window_dma"})
            return dict(plan, labels={"window_bf16_image" if (dyb and ready) else ("window_bf16_convert" if dyb else "window_bf16_fp32dy")})
    if dg != 1 and cpg % 128:
        return None
    plan.update(grid=_cdiv(m_out, 128), lds=4 * (2 * (128 * 36 + 32 * 128) + 128 * 8 + 128 * 4 + 128 * 3))
    return dict(plan, labels={"gather"})


# ------------------------------------------------------------------------------------------------------------------
# The bf16 and f16x3 convolutions of csrc/conv_bf16.hip against float64 (tests/test_conv_lowp_fp64_gpu.py; the promises made
# here are checked by tests/test_host_logic.py).  The contract defines each operand's IMAGE — bf16: the value rounded to nearest
# even; f16x3: hi + lo, two fp16 values after the power-of-two scale of the tensor's maximum (oracle/split.py) — and which products
# of image parts a term consists of.  The reference multiplies those images in float64; the yardstick chains the same products (all
# exact in float32) in float32.  Only fp32 accumulation separates a correct kernel from that reference, so conv_accepts is unchanged.
# ------------------------------------------------------------------------------------------------------------------
CONV16_MARGIN = 2            # by the rule of CONV_MARGIN: the largest ratio of profiles/conv_lowp_fp64_ratios.txt (an MI355X run of
                             # tests/test_conv_lowp_fp64_gpu.py) is 1.32 — bf16, weight gradient under the dynamic-range input; f16x3 stays
                             # below 0.35 — rounded up to a power of two, not below 2
LOWP_PAIRS = {MATH_BF16: ((0, 0),), MATH_F16X3: ((0, 0), (0, 1), (1, 0))}     # (part of the first operand, part of the second) per term
LOWP_NAMES = {MATH_BF16: "bf16", MATH_F16X3: "f16x3"}


def _np32(t):
    return t.detach().cpu().float().numpy() if torch.is_tensor(t) else np.asarray(t, np.float32)


def lowp_image(math, t, bits=None):
    """The image of operand t (float32 tensor / array) under arithmetic `math` -> (parts: tuple of float64 arrays, scale float64);
    t is modelled as sum(parts) / scale.  bf16: one part, scale 1.  f16x3: (hi, lo) of oracle.split.split under the scale of
    oracle.split.scale_of(bits), bits = the bit pattern of max|t| unless given (the word the entry point is handed)."""
    a = _np32(t)
    if math == MATH_BF16:
        return (bf16_exact(a).astype(np.float64),), np.float64(1.0)
    from oracle import split as osp
    sc = osp.scale_of(osp.absmax_bits(a) if bits is None else bits)
    hi, lo = osp.split(a, sc)
    return (hi.astype(np.float64), lo.astype(np.float64)), np.float64(sc)


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def lowp_fprop_ref64(math, xi, wi, bias, stride, pad, relu):
    """y float64 from the images xi, wi (lowp_image): the terms of LOWP_PAIRS, each conv_ref64, over the two scales; + bias, ReLU.
    f16x3: exactly oracle.split.conv2d."""
    (xp, sx), (wp, sw) = xi, wi
    y = None
    for i, j in LOWP_PAIRS[math]:
        t = conv_ref64(_t64(xp[i]), _t64(wp[j]), None, stride, pad, False)[0]
        y = t if y is None else y + t
    y = y / (sx * sw)
    if bias is not None:
        y = y + torch.as_tensor(bias).detach().cpu().double().view(1, -1, 1, 1)
    return torch.relu(y) if relu else y


def lowp_grads_ref64(math, xi, wi, gi, stride, pad, far=(0, 0), pairs=None):
    """(dx, dw) float64 from the images of x, w and gy: dx = sum over LOWP_PAIRS of dgrad(gy part, w part) / (s_gy s_w),
    dw = sum of wgrad(x part, gy part) / (s_x s_gy), each through conv_ref64's autograd.  far: rows / columns of zero padding
    added to x at the far edge (the weight gradient's out_h / out_w override)."""
    import torch.nn.functional as F
    (xp, sx), (wp, sw), (gp, sg) = xi, wi, gi
    if pairs is None:                                      # one backward serves dgrad(gy_g, w_b) and wgrad(x_a, gy_g)
        pairs, calls = LOWP_PAIRS[math], ([(0, 0, 0)] if math == MATH_BF16 else [(0, 0, 0), (1, 1, 0), (0, 0, 1)])
    else:
        calls = [(a, b, g) for a in range(len(xp)) for b in range(len(wp)) for g in range(len(gp))]
    dx = dw = 0.0
    done_dx, done_dw = set(), set()
    for a, b, g in calls:
        if ((g, b) not in pairs or (g, b) in done_dx) and ((a, g) not in pairs or (a, g) in done_dw):
            continue
        x64 = _t64(xp[a])
        if far != (0, 0):
            x64 = F.pad(x64, (0, far[1], 0, far[0]))
        _, tdx, tdw = conv_ref64(x64, _t64(wp[b]), None, stride, pad, False, _t64(gp[g]))
        if (g, b) in pairs and (g, b) not in done_dx:
            dx, _ = dx + tdx, done_dx.add((g, b))
        if (a, g) in pairs and (a, g) not in done_dw:
            dw, _ = dw + tdw, done_dw.add((a, g))
    assert done_dx == set(pairs) and done_dw == set(pairs)
    if far != (0, 0):
        dx = dx[:, :, :dx.shape[2] - far[0], :dx.shape[3] - far[1]]
    return dx / (sg * sw), dw / (sx * sg)


def lowp_terms(math, kind, idx, first, second, stride, pad, rs=None, bias=None, base=None, pairs=None):
    """conv_terms over the image products: the chunks hold, side by side, the products of every pair of LOWP_PAIRS (a term of f16x3
    is three separate products), over the two scales; bias / base appear once.  first, second: the images in the order of the
    products — fprop (x, w), dgrad (gy, w), wgrad (x, gy; rs = (R, S))."""
    (ap, sa), (bp, sb) = first, second
    div = sa * sb
    gens = []
    for n_, (i, j) in enumerate(LOWP_PAIRS[math] if pairs is None else pairs):
        extra = {}
        if n_ == 0 and bias is not None:
            extra["bias"] = _np64(bias) * div
        if n_ == 0 and base is not None:
            extra["base"] = _np64(base) * div
        if kind == "fprop":
            gens.append(conv_terms(kind, idx, ap[i], bp[j], None, stride, pad, **extra))
        elif kind == "dgrad":
            gens.append(conv_terms(kind, idx, None, bp[j], ap[i], stride, pad, **extra))
        else:
            gens.append(conv_terms(kind, idx, ap[i], tuple(rs), bp[j], stride, pad, **extra))
    for chunks in zip(*gens):
        yield np.concatenate(chunks, 1) / div


def _parity_launches(h, w, r, s, ph, pw):
    """rr_plan::parity_classes restated -> ([(class, Rc, Sc, lead_h, lead_w, Hc, Wc, taps of the classes before it)] of the classes
    that launch, any_empty)."""
    out, any_empty, before = [], False, 0
    for cl in range(4):
        a, b = cl >> 1, cl & 1
        r0, s0 = (a + ph) & 1, (b + pw) & 1
        rc, sc = ((r - r0 + 1) // 2 if r0 < r else 0), ((s - s0 + 1) // 2 if s0 < s else 0)
        hc, wc = (h - a + 1) // 2, (w - b + 1) // 2
        if hc > 0 and wc > 0 and rc * sc == 0:
            any_empty = True
        if rc * sc > 0 and hc > 0 and wc > 0:
            out.append((cl, rc, sc, rc - 1 - (a + ph - r0) // 2, sc - 1 - (b + pw - s0) // 2, hc, wc, before))
        before += rc * sc
    return out, any_empty


def conv16hip_tile(m, dc):
    """launch_igemm of csrc/conv16.hip restated -> (output channels per tile, workgroups, dynamic LDS bytes)."""
    if dc % 256 == 0:
        return 256, _cdiv(m, 256) * (dc // 256), 2 * (256 * 128 + 256 * 128)
    return 128, _cdiv(m, 256) * (dc // 128), 128 * 1024


def dgrad_s2_mirror(family, n, c, h, w, k, r, s, ph, pw, accumulate=False):
    """dgrad_s2_impl (conv_bf16.hip: family MATH_BF16 / MATH_F16X3) and rr_conv16_dgrad_s2 (conv16.hip: FAM_CONV16) restated ->
    {p, q, zero_dst, n_launch, "launches": [(ph, pw, Rc, Sc, lead_h, lead_w, Hc, Wc, taps before, workgroups)]}, or None where the
    entry point refuses.  Workgroups: launch_igemm's of conv16.hip; 0 for the two arithmetics whose launches _fprop_route states.
    Needs h + 2*ph >= r and w + 2*pw >= s (the library divides like C, towards zero)."""
    if family == FAM_CONV16:
        if min(n, h, w) <= 0 or ph < 0 or pw < 0 or k % 64 != 0 or c % 128 != 0 or r * s > 16:
            return None
    elif min(n, h, w, c, k, r, s) <= 0 or c % 4 != 0 or k % 4 != 0 or r * s > 64 or ph < 0 or pw < 0:
        return None
    p, q = (h + 2 * ph - r) // 2 + 1, (w + 2 * pw - s) // 2 + 1
    if p <= 0 or q <= 0 or (family == FAM_CONV16 and n * p * q * k * 2 >= 1 << 31):
        return None
    if not _s2_pads_ok(r, s, ph, pw):
        return None
    launches, any_empty = _parity_launches(h, w, r, s, ph, pw)
    rows = [(cl >> 1, cl & 1, rc, sc, lh, lw, hc, wc, before, conv16hip_tile(n * hc * wc, c)[1] if family == FAM_CONV16 else 0)
            for cl, rc, sc, lh, lw, hc, wc, before in launches]
    return dict(p=p, q=q, zero_dst=int(any_empty and not accumulate), n_launch=len(rows), launches=rows)


def _s2_pads_ok(r, s, ph, pw):
    """the refusal loop of the two stride-2 hosts: every class that has taps needs non-negative leading pads"""
    for cl in range(4):
        a, b = cl >> 1, cl & 1
        r0, s0 = (a + ph) & 1, (b + pw) & 1
        rc, sc = ((r - r0 + 1) // 2 if r0 < r else 0), ((s - s0 + 1) // 2 if s0 < s else 0)
        if rc * sc > 0 and (rc - 1 - (a + ph - r0) // 2 < 0 or sc - 1 - (b + pw - s0) // 2 < 0):
            return False
    return True


def conv16_fprop_labels(math, n, c, h, w, k, r, s, stride, ph, pw, bias, relu, want_stats):
    """(labels, plan) of one rr_conv_fprop_bf16 / _f16x3 call: _fprop_route's, and what the kernel does differently at this shape."""
    plan = _fprop_route(n, c, h, w, k, r, s, stride, ph, pw, bias, relu, want_stats, math)
    lab, bn = set(plan["labels"]), plan["bn"]
    p, q = (h + 2 * ph - r) // stride + 1, (w + 2 * pw - s) // stride + 1
    lab.add("xcd_n" if plan["xcd_n"] else ("xcd_off,tiles>1" if _cdiv(k, bn) > 1 else "one column tile"))
    lab |= {name for name, on in (("ragged M", n * p * q % _BM), ("ragged filter tile", k % bn), ("partial K-step", c % _BK),
                                  ("C%8: image refused", c % 8), ("bias+relu", bias and relu), ("stride 2", stride == 2),
                                  ("fused stats", want_stats and plan["ks"] == 1)) if on}
    if c % 8 == 0 and (math == MATH_BF16 or bn == 128):
        lab.add("image@bn%d" % bn)                   # the ready-made filter image (bf16 w_bf16 / f16x3 w_split) is read
    return lab, plan


def conv16_dgrad_labels(math, n, c, h, w, k, r, s, stride, ph, pw, link=None):
    """Labels of the data gradient of this convolution on the 16-bit kernels: stride 1 one forward launch on (dy, flipped filter)
    ("s1 ..."), stride 2 one strided launch per live parity class ("s2 ...")."""
    p, q = (h + 2 * ph - r) // stride + 1, (w + 2 * pw - s) // stride + 1
    if stride == 1:
        plan = _fprop_route(n, k, p, q, c, r, s, 1, r - 1 - ph, s - 1 - pw, False, False, False, math, link=link)
        if link is None:
            return {"s1 " + name for name in plan["labels"]}
        how = "fused" if plan["fused"] else "reduce pass"
        return {"link %s bn%d %s" % (link, plan["bn"], how)}
    launches, any_empty = _parity_launches(h, w, r, s, ph, pw)
    lab = {"s2 any_empty"} if any_empty else set()
    for _, rc, sc, lh, lw, hc, wc, _ in launches:
        plan = _fprop_route(n, k, p, q, c, rc, sc, 1, lh, lw, False, False, False, math, strided=True, out_hw=(hc, wc))
        lab.add("s2 bn%d" % plan["bn"])
    return lab


def conv16_wgrad_labels(math, n, c, h, w, k, r, s, stride, ph, pw, out_hw=None):
    """wgrad_impl of csrc/conv_bf16.hip restated (rr_plan::pixel_splits over 1024 workgroup slots, 512 for the split kernel,
    never fewer than 16 K-steps per split) -> labels."""
    return wgrad16_mirror(math, n, c, h, w, k, r, s, stride, ph, pw, out_hw)["labels"]


def wgrad16_mirror(family, n, c, h, w, k, r, s, stride, ph, pw, out_hw=None):
    """wgrad_impl of csrc/conv_bf16.hip (family MATH_BF16 / MATH_F16X3) and rr_conv16_wgrad of csrc/conv16.hip (FAM_CONV16, which
    has no output override) restated -> {"labels": set, every name of CONV_GRAD_FIELDS[GRAD_WGRAD]}, or None where the entry point
    refuses.  Needs h + 2*ph >= r and w + 2*pw >= s."""
    two_gib = 1 << 31
    if family == FAM_CONV16:
        if min(n, h, w) <= 0 or k % 128 != 0 or c % 128 != 0 or r * s > 64 or stride not in (1, 2):
            return None
        p, q = (h + 2 * ph - r) // stride + 1, (w + 2 * pw - s) // stride + 1
        m = n * p * q
        if p <= 0 or q <= 0 or m * k * 2 >= two_gib or n * h * w * c * 2 >= two_gib:
            return None
        nt_w = 256 if c % 256 == 0 else 128
        mt, nt = _cdiv(k, 256), c // nt_w
        tiles = mt * nt * r * s
        splits, per = _pixel_splits(tiles, _cdiv(m, 32), 512, 32)
        lab = {"splits>1" if splits > 1 else "one split", "c tile %d" % nt_w}
        return dict(labels={"wgrad " + name for name in lab}, P=p, Q=q, M=m, bm=256, bn=nt_w, a_scalar=0, b_scalar=0, pipe=0, mt=mt, nt=nt,
                    tiles=tiles, splits=splits, per_split=per, grid=tiles * splits, lds=4 * (8 * 2048 + (nt_w // 32) * 2048))
    if min(n, h, w, c, k, r, s, stride) <= 0 or c % 4 != 0 or k % 4 != 0:
        return None
    p, q = out_hw or ((h + 2 * ph - r) // stride + 1, (w + 2 * pw - s) // stride + 1)
    m = n * p * q
    if not 0 < m < two_gib or m * k * 4 >= two_gib or n * h * w * c * 4 >= two_gib:
        return None
    mt, nt = _cdiv(k, 128), _cdiv(c, 128)
    tiles, chunks, slots = mt * nt * r * s, _cdiv(m, _BK), (512 if family == MATH_F16X3 else 1024)
    splits = max(1, min(slots // tiles if tiles < slots else 1, _cdiv(chunks, 16)))
    per = _cdiv(chunks, splits)
    splits = _cdiv(chunks, per)
    lab = {"splits>1" if splits > 1 else "one split"}
    lab |= {name for name, on in (("ragged K tile", k % 128), ("ragged C tile", c % 128), ("M%32", m % _BK), ("stride 2", stride == 2),
                                  ("out override", out_hw is not None)) if on}
    return dict(labels={"wgrad " + name for name in lab}, P=p, Q=q, M=m, bm=128, bn=128, a_scalar=0, b_scalar=0, pipe=0, mt=mt, nt=nt,
                tiles=tiles, splits=splits, per_split=per, grid=tiles * splits, lds=2 * 4 * 4 * (32 * 32 + 32) * (2 if family == MATH_F16X3 else 1))


# (N, C, H, W, K, R, S, stride, pad_h, pad_w, bias, relu, want_stats values, passes) as CONV64_GRID; every case at the smallest
# size that still takes its route (test_conv16_grid_reaches_every_route names the route of each from the mirror)
CONV16_GRID = [
    (1, 128, 16, 16, 128, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),    # bn32, split-K 4, xcd_n; statistics in the colstats pass
    (1, 64, 9, 13, 128, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),      # bn32, ragged M, split-K 2, xcd_n off on 4 column tiles
    (1, 64, 24, 24, 64, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),      # bn64, split-K 2
    (1, 128, 32, 32, 384, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),    # bn64 by the mid-tile rule, 6 column tiles, split-K 4
    (1, 64, 64, 64, 256, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),     # bn128, xcd_n, split-K 2; the f16x3 filter image
    (1, 32, 80, 80, 132, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),     # bn128, ragged filter tile, no split: fused statistics
    (2, 48, 8, 8, 24, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),        # partial K-step, C % 8 == 0
    (1, 44, 12, 12, 40, 3, 3, 1, 1, 1, False, False, (False, True), "fdw"),      # partial K-step, C % 8 != 0: the filter image is refused
    (1, 256, 20, 12, 1, 17, 1, 1, 8, 0, True, False, (False, True), "f"),        # HCov with bias: bn32, one live column (K % 4 != 0: forward only)
    (1, 256, 10, 10, 256, 3, 3, 1, 1, 1, True, True, (False, True), "fdw"),      # bias + ReLU keep split-K off
    (2, 64, 15, 17, 128, 3, 3, 2, 1, 1, False, False, (False, True), "fdw"),     # stride-2 forward on an odd map; dgrad bn64 strided
    (1, 160, 64, 64, 32, 3, 3, 1, 1, 1, False, False, (), "d"),                  # stride-1 dgrad at bn128 without split-K: the accumulate epilogue
    (2, 256, 79, 81, 16, 3, 3, 2, 1, 1, False, False, (), "dw"),                # stride-2 dgrad: four classes of different sizes, bn128 strided
    (2, 64, 15, 17, 32, 3, 3, 2, 1, 1, False, False, (), "d"),                   # ... bn64 strided
    (1, 32, 9, 7, 16, 3, 3, 2, 1, 1, False, False, (), "dw"),                    # ... bn32 strided
    (2, 128, 15, 17, 64, 1, 1, 2, 0, 0, False, False, (), "d"),                  # ... 1x1: three empty classes (memset; accumulate must not clear dx)
    (1, 64, 12, 12, 64, 3, 3, 2, 0, 0, False, False, (), "d"),                   # ... no padding
]
CONV16_ASYM_WGRAD = (1, 64, 12, 12, 64, 3, 3, 1, 1, 1, 13, 13)                    # the out_h / out_w override, as CONV64_ASYM_WGRAD
# stride-1 data gradients that carry their producer's backward sums: (dx shape (n, c, h, w), k of dy, link, mask source) at 3x3 pad 1.
# mask source of a "bn" link: "affine" (y * scale + shift > 0, recomputed), "z" (the producer's output), None (no ReLU)
CONV16_LINKS = [
    ((2, 64, 16, 16), 32, "bn", "affine"),          # LINK_BN fused at bn64
    ((2, 256, 16, 16), 32, "bn", "z"),              # LINK_BN fused at bn32
    ((2, 64, 16, 16), 64, "relu_bias", "z"),        # LINK_RELU_BIAS at bn64 (the plan keeps split-K off)
    ((1, 32, 16, 16), 64, "relu_bias", "z"),        # LINK_RELU_BIAS at bn32
    ((2, 64, 16, 16), 64, "bn", None),              # split-K: not fused, the sums come from the reduce pass behind the launch
]
_COMMON16 = {"bn128", "bn64", "bn32", "ksplit>1", "ksplit>1+stats", "xcd_n", "xcd_off,tiles>1", "ragged M", "ragged filter tile",
             "partial K-step", "C%8: image refused", "image@bn128", "bias+relu", "stride 2", "fused stats",
             "s1 bn128", "s1 bn64", "s1 bn32", "s1 ksplit>1", "s2 bn128", "s2 bn64", "s2 bn32", "s2 any_empty",
             "link bn bn64 fused", "link bn bn32 fused", "link relu_bias bn64 fused", "link relu_bias bn32 fused", "link bn bn64 reduce pass",
             "wgrad splits>1", "wgrad one split", "wgrad ragged K tile", "wgrad ragged C tile", "wgrad M%32", "wgrad stride 2",
             "wgrad out override"}
CONV16_ROUTE_LABELS = {MATH_BF16: _COMMON16 | {"image@bn64", "image@bn32"}, MATH_F16X3: set(_COMMON16)}


def conv16_case_labels(math, cfg, want_stats=False):
    """{"fprop" | "dgrad" | "wgrad": labels} of the passes one CONV16_GRID case runs."""
    geo, (bias, relu, _, passes) = cfg[:10], cfg[10:]
    out = {}
    if "f" in passes:
        out["fprop"] = conv16_fprop_labels(math, *geo, bias, relu, want_stats)[0]
    if "d" in passes:
        out["dgrad"] = conv16_dgrad_labels(math, *geo)
    if "w" in passes:
        out["wgrad"] = conv16_wgrad_labels(math, *geo)
    return out


def conv16_grid_labels(math):
    """Every label CONV16_GRID, CONV16_LINKS and CONV16_ASYM_WGRAD reach under arithmetic `math`."""
    seen = set()
    for cfg in CONV16_GRID:
        for ws in cfg[12] or (False,):
            for lab in conv16_case_labels(math, cfg, ws).values():
                seen |= lab
    for (n, c, h, w), k, link, _ in CONV16_LINKS:
        seen |= conv16_dgrad_labels(math, n, c, h, w, k, 3, 3, 1, 1, 1, link=link)
    seen |= conv16_wgrad_labels(math, *CONV16_ASYM_WGRAD[:10], out_hw=CONV16_ASYM_WGRAD[10:])
    return seen


# ------------------------------------------------------------------------------------------------------------------
# The deformable convolutions of csrc/dcn.hip against float64 (tests/test_dcn_fp64_gpu.py; the promises made here are checked by
# tests/test_host_logic.py).  Reference: oracle/dcn.py evaluated in float64 on the float32 inputs, the sample position formed by ONE
# float32 addition as the kernels do (pos_fp32).  Yardstick: the same definition in float32 with every reduction chained in plain
# loop order, minus the float64 result.  Acceptance: conv_accepts, margin DCN_MARGIN, plus two allowances restated from reference
# quantities only — the fixed-point window of the data gradient (dcn_fixed_point_allowance) and bf16 column ties (dcn_tie_*).
# ------------------------------------------------------------------------------------------------------------------
DCN_MARGIN = 4                   # by the rule of CONV_MARGIN: the largest ratio of profiles/dcn_fp64_ratios.txt (an MI355X run of
                                 # tests/test_dcn_fp64_gpu.py) is 2.07 — the 32-wide L2-gather forward, fp32, max-abs at the samples; every
                                 # other tensor stays below 1.8 — rounded up to a power of two, not below 2
DCN_TIE_BAND = 8 * U32           # a float32 blend errs by at most 7 roundings (taken up to 8) x 2^-24 x sum |w_e x_e| |mask|
DCN_TIE_MAX = 10                 # outputs with more near-tie terms are left out (2^10 subsets are searched)
DCN_TIE_LEFT_OUT = 0.01          # at most this share of a tensor may be left out
DCN_TIE_CLEAN = 1.0 / 3.0        # at least this share of a tensor's sampled outputs has no near-tie term
DCN_BLOCK = (8, 16)              # the output-pixel block of the window kernels
DCN_FX_UNIT_LOG2 = -29           # one fixed-point unit <= bound * 2^-29 (dcn.hip: bound scaled into [2^29, 2^30))
DCN_EDGE_CLASSES = ("gauss", "border", "exact", "beyond", "far", "pile", "operands")


def bf16_rne64(a):
    """float64 array -> the nearest bf16 value (ties to even) as float64, straight from the float64 bit pattern (normal range)."""
    b = np.ascontiguousarray(a, np.float64).view(np.int64)
    b = (b + ((b >> 45) & 1) + ((1 << 44) - 1)) & ~np.int64((1 << 45) - 1)
    return b.view(np.float64)


def dcn_out_hw(h, w, r, s, stride, ph, pw, dil):
    return (h + 2 * ph - (dil * (r - 1) + 1)) // stride + 1, (w + 2 * pw - (dil * (s - 1) + 1)) // stride + 1


def dcn_ref64(x, offset, mask, w, bias, stride, pad, dil, dg, gy=None, base_dx=None, bf16=False):
    """oracle/dcn.py in float64 on the float32 inputs, pos_fp32=True -> {"out", "cols", and with gy: "dx", "doffset", "dmask", "dw",
    "db"} as float64 numpy arrays.  bf16: the oracle's _ContractBf16 (columns, W and dY rounded to bf16 straight from float64).
    base_dx: what an accumulating data gradient adds into."""
    from oracle import dcn as odcn
    ins = [None if t is None else torch.as_tensor(t).detach().cpu().double().clone().requires_grad_(gy is not None)
           for t in (x, offset, mask, w, bias)]
    k, _, r, s = ins[3].shape
    with torch.no_grad():
        cols = odcn.dcn_columns(ins[0], ins[1], ins[2], r, s, stride, pad, dil, dg, pos_fp32=True)
    out = odcn.dcn_v2_conv(*ins, stride, pad, dil, dg, bf16=bf16, pos_fp32=True)
    res = {"out": out.detach().numpy(), "cols": cols.numpy()}
    if gy is not None:
        out.backward(torch.as_tensor(gy).detach().cpu().double())
        for name, t in zip(("dx", "doffset", "dmask", "dw", "db"), ins):
            res[name] = None if t is None else t.grad.numpy()
        if base_dx is not None:
            res["dx"] = res["dx"] + _np64(base_dx)
    return res


def dcn_geometry(offset, h, w, r, s, stride, pad, dil, dg, dtype=np.float64, fault=None):
    """The sampling geometry of every (n, group, tap, p, q): position = ONE float32 add of the integer grid position and the offset,
    everything after it in `dtype`.  -> dict of arrays [n, dg, T, P, Q] (h, w, inside, lh, lw) and [4, n, dg, T, P, Q] per corner
    e = 2 * (row + 1) + (col + 1): hy, wx (image coordinates), idx (clamped flat pixel), valid, wgt, dwh, dww (d wgt / d h, d w)."""
    off = _np32(offset)
    n, _, p, q = off.shape
    t = r * s
    off = off.reshape(n, dg, t, 2, p, q)
    if fault == "swap_hw":
        off = off[:, :, :, ::-1]
    if fault == "group0":
        off = np.broadcast_to(off[:, :1], off.shape)
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    ti, tj = np.divmod(np.arange(t), s)
    bh = (np.arange(p)[None, :] * stride - ph + ti[:, None] * dil).astype(np.float32)
    bw = (np.arange(q)[None, :] * stride - pw + tj[:, None] * dil).astype(np.float32)
    hp = (bh[None, None, :, :, None] + off[:, :, :, 0]).astype(np.float32).astype(dtype)
    wp = (bw[None, None, :, None, :] + off[:, :, :, 1]).astype(np.float32).astype(dtype)
    if fault == "nonstrict":
        inside = (hp >= -1) & (wp >= -1) & (hp <= h) & (wp <= w)
    else:
        inside = (hp > -1) & (wp > -1) & (hp < h) & (wp < w)
    hf, wf = np.floor(hp), np.floor(wp)
    lh, lw = hp - hf, wp - wf
    one = dtype(1)
    hh, hw = one - lh, one - lw
    h0, w0 = np.clip(hf, -2, h + 1).astype(np.int64), np.clip(wf, -2, w + 1).astype(np.int64)
    hy, wx = np.stack([h0, h0, h0 + 1, h0 + 1]), np.stack([w0, w0 + 1, w0, w0 + 1])
    valid = inside[None] & (hy >= 0) & (hy <= h - 1) & (wx >= 0) & (wx <= w - 1)
    return {"h": hp, "w": wp, "inside": inside, "lh": lh, "lw": lw, "hy": hy, "wx": wx, "valid": valid,
            "idx": np.clip(hy, 0, h - 1) * w + np.clip(wx, 0, w - 1),
            "wgt": np.stack([hh * hw, hh * lw, lh * hw, lh * lw]), "dwh": np.stack([-hw, -lw, hw, lw]),
            "dww": np.stack([-hh, hh, -lh, lh]), "base_h": bh, "base_w": bw}


def dcn_window(r, s, dil, margin):
    """(WH, WW) of the LDS window at margin `margin` (dcn_plan_mirror's window())."""
    return 8 + (r - 1) * dil + 2 * margin + 1, 16 + (s - 1) * dil + 2 * margin + 1


def dcn_in_window(geo, r, s, pad, dil, margin):
    """[4, n, dg, T, P, Q]: whether corner e lies in the LDS window of its output pixel's 8x16 block (stride 1; window pixel (0, 0)
    is image pixel (y0 - pad_h - margin, x0 - pad_w - margin), as dcn.hip places it)."""
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    p, q = geo["inside"].shape[-2:]
    wh, ww = dcn_window(r, s, dil, margin)
    wy0 = (np.arange(p) // DCN_BLOCK[0] * DCN_BLOCK[0] - ph - margin)[:, None]
    wx0 = (np.arange(q) // DCN_BLOCK[1] * DCN_BLOCK[1] - pw - margin)[None, :]
    ly, lx = geo["hy"] - wy0, geo["wx"] - wx0
    return (ly >= 0) & (ly < wh) & (lx >= 0) & (lx < ww)


def _dcn_blocks(p, q):
    by, bx = _cdiv(p, DCN_BLOCK[0]), _cdiv(q, DCN_BLOCK[1])
    return by * bx, (np.arange(p)[:, None] // DCN_BLOCK[0]) * bx + np.arange(q)[None, :] // DCN_BLOCK[1]


DCN_FAULTS = ("clamp", "nonstrict", "swap_hw", "group0", "beyond_margin", "tap_mask", "skip_chunk", "doffset_nomask",
              "cols_unrounded", "round_before_mask", "dy_unrounded", "base_ignored", "fx_unit20")


def dcn_model(x, offset, mask, w, bias, stride, pad, dil, dg, gy=None, base_dx=None, base_dw=None, dtype=np.float64, bf16=False,
              fault=None, margin=3, dcol=None, blocks=False):
    """The definition of the modulated deformable convolution and of its gradients written out in numpy, corner by corner, in `dtype`
    (float64: equal to dcn_ref64, which tests/test_host_logic.py checks; float32: the float32 evaluation the modelled faults are
    applied to).  fault: one of DCN_FAULTS.  dcol: a given column gradient [n, c, T, P, Q] (rr_dcn_col2im) instead of dY . W.
    blocks: also "dx_blocks" [n, dg, blocks, H*W, cpg], d input summed per 8x16 output block.  -> dict of arrays."""
    dt = dtype
    xa, mk, wa = (_np32(t).astype(dt) for t in (x, mask, w))
    n, c, h, wd = xa.shape
    k, _, r, s = wa.shape
    t, cpg = r * s, c // dg
    geo = dcn_geometry(offset, h, wd, r, s, stride, pad, dil, dg, dt, fault)
    p, q = geo["inside"].shape[-2:]
    mk = mk.reshape(n, dg, t, p, q)
    if fault == "tap_mask":
        mk = mk.copy()
        mk[:, :, t // 2] = 1
    valid = geo["valid"]
    if fault == "beyond_margin":
        valid = valid & dcn_in_window(geo, r, s, pad, dil, margin)
    read = np.broadcast_to(geo["inside"][None], valid.shape) if fault == "clamp" else valid
    xg = xa.reshape(n, dg, cpg, h * wd)
    xs = np.stack([np.take_along_axis(xg, geo["idx"][e].reshape(n, dg, 1, -1), axis=3).reshape(n, dg, cpg, t, p, q)
                   * read[e][:, :, None].astype(dt) for e in range(4)])
    wgt = geo["wgt"][:, :, :, None]
    sample = (wgt * xs).sum(0, dtype=dt)
    col = sample * mk[:, :, None]
    rq = (lambda a: a) if not bf16 else (bf16_rne64 if dt == np.float64 else bf16_exact)
    colq = col if fault == "cols_unrounded" else (rq(sample) * mk[:, :, None] if fault == "round_before_mask" and bf16 else rq(col))
    w3 = rq(wa).reshape(k, c, t)
    colf = colq.reshape(n, c, t, p, q)
    live = slice(0, c - 32) if fault == "skip_chunk" else slice(None)            # the last 32-channel chunk never runs
    out = np.einsum("nctpq,kct->nkpq", colf[:, live], w3[:, live], optimize=True)
    if bias is not None:
        out = out + _np32(bias).astype(dt).reshape(1, -1, 1, 1)
    res = {"geo": geo, "xs": xs, "sample": sample, "col": col.reshape(n, c, t, p, q), "colq": colf, "w3": w3, "out": out, "mask": mk,
           "absblend": (np.abs(wgt * xs).sum(0) * np.abs(mk[:, :, None])).reshape(n, c, t, p, q)}
    if gy is None and dcol is None:
        return res
    if dcol is None:
        ga = _np32(gy).astype(dt)
        gq = ga if fault == "dy_unrounded" else rq(ga)
        dcol = np.einsum("nkpq,kct->nctpq", gq, w3, optimize=True)
        dw = np.einsum("nkpq,nctpq->kct", gq, colf, optimize=True)
        if fault == "skip_chunk":
            dcol[:, c - 32:] = 0
            dw[:, c - 32:] = 0
        if base_dw is not None and fault != "base_ignored":
            dw = dw + _np32(base_dw).astype(dt).reshape(k, c, t)
        res.update(gyq=gq, dw=dw.reshape(k, c, r, s), db=ga.sum((0, 2, 3)))
    else:
        dcol = np.asarray(dcol).astype(dt)
    dcg = dcol.reshape(n, dg, cpg, t, p, q)
    dsm = dcg * mk[:, :, None]
    dsrc = dcg if fault == "doffset_nomask" else dsm
    gh = (geo["dwh"][:, :, :, None] * xs).sum(0, dtype=dt)
    gw = (geo["dww"][:, :, :, None] * xs).sum(0, dtype=dt)
    res.update(dcol=dcol, dmask=(dcg * sample).sum(2, dtype=dt).reshape(n, dg * t, p, q),
               doffset=np.stack([(dsrc * gh).sum(2, dtype=dt), (dsrc * gw).sum(2, dtype=dt)], 3).reshape(n, 2 * dg * t, p, q))
    nb, blk = _dcn_blocks(p, q)
    unit = None
    if fault == "fx_unit20":
        unit = _dcn_fx_units(geo, dcol, mk, h * wd, -20)[0]                       # [n, dg, cpg, nb]
    part = np.zeros((n, dg, nb if blocks else 1, h * wd, cpg), dt)
    bsel = np.broadcast_to(blk if blocks else np.zeros_like(blk), (t, p, q)).ravel()
    for e in range(4):
        ce = dsm * (geo["wgt"][e] * valid[e])[:, :, None].astype(dt)               # [n, dg, cpg, T, P, Q]
        if unit is not None:
            u = unit[:, :, :, blk][:, :, :, None]                                  # [n, dg, cpg, 1, P, Q]
            ce = np.where(u > 0, np.round(ce / np.where(u > 0, u, 1)) * u, ce).astype(dt)
        for i in range(n):
            for g in range(dg):
                np.add.at(part[i, g], (bsel, geo["idx"][e][i, g].ravel()), ce[i, g].reshape(cpg, -1).T)
    dx = part.sum(2, dtype=dt).transpose(0, 1, 3, 2).reshape(n, c, h, wd)
    if base_dx is not None and fault != "base_ignored":
        dx = dx + _np32(base_dx).astype(dt)
    res["dx"] = dx
    if blocks:
        res["dx_blocks"] = part
    return res


def _dcn_fx_units(geo, dcol, mk, npix, unit_log2=DCN_FX_UNIT_LOG2):
    """The fixed-point contract of the window data gradient from reference quantities: per (n, group, 8x16 output block) the hit count
    of every image pixel (valid corners of the block's samples that land on it) and its maximum, the block's largest |dcol| per
    channel and largest |mask| -> (unit [n, dg, cpg, blocks] = maxhits * max|dcol| * max|mask| * 2^unit_log2, hits [n, dg, blocks, npix])."""
    n, dg, t, p, q = geo["inside"].shape
    c = dcol.shape[1]
    nb, blk = _dcn_blocks(p, q)
    hits = np.zeros((n, dg, nb, npix))
    for e in range(4):
        nn, gg, tt, pp, qq = np.nonzero(geo["valid"][e])
        np.add.at(hits, (nn, gg, blk[pp, qq], geo["idx"][e][nn, gg, tt, pp, qq]), 1)
    maxhits = np.maximum(hits.max(3), 1)
    ad, am = np.abs(dcol).max(2), np.abs(mk).reshape(n, dg * t, p, q).max(1)
    maxd, maxm = np.zeros((n, c, nb)), np.zeros((n, nb))
    for b in range(nb):
        maxd[:, :, b], maxm[:, b] = ad[:, :, blk == b].max(-1), am[:, blk == b].max(-1)
    unit = maxhits[:, :, None] * maxd.reshape(n, dg, c // dg, nb) * maxm[:, None, None] * 2.0 ** unit_log2
    return unit, hits


def dcn_fixed_point_allowance(m64, base_dx=None):
    """What the window data-gradient routes may add to a d-input element's error, from the float64 model m64 (dcn_model(..., blocks=
    True)) alone: every contribution is rounded to nearest in its block's unit (half a unit each, hits x half a unit per block that
    reaches the element) and each block's sum joins the element with one float32 add (2^-24 of the running magnitude, taken as the
    sum of the blocks' |partial sums| and |base|).  -> (allowance [n, c, h, w], its fixed-point part alone)."""
    geo, part = m64["geo"], m64["dx_blocks"]
    n, dg, nb, npix, cpg = part.shape
    unit, hits = _dcn_fx_units(geo, m64["dcol"], m64["mask"], npix)
    fx = 0.5 * np.einsum("ngbx,ngcb->ngcx", hits, unit)
    mag = np.abs(part).sum(2).transpose(0, 1, 3, 2)                                # [n, dg, cpg, npix]
    shape = m64["dx"].shape
    if base_dx is not None:
        mag = mag + np.abs(_np64(base_dx)).reshape(mag.shape)
    reach = (hits > 0).sum(2)[:, :, None]
    return (fx + U32 * reach * mag).reshape(shape), fx.reshape(shape)


def dcn_tie_info(m64):
    """Near-tie columns of the float64 bf16 model m64: a float32 blend errs by at most DCN_TIE_BAND x sum |w_e x_e| |mask|, so a kernel's
    column may round to the other bf16 neighbour where the float64 column lies within that band of the rounding boundary.
    -> (near [n, c, T, P, Q] bool, alternative rounding - chosen rounding, float64)."""
    col = m64["col"]
    qv = bf16_rne64(col)
    step = np.where(np.abs(col) > np.abs(qv), 1, -1).astype(np.int64) << 45
    alt = np.where(qv == 0, qv, (qv.view(np.int64) + step).view(np.float64))
    near = (qv != 0) & (np.abs(col - 0.5 * (qv + alt)) < DCN_TIE_BAND * m64["absblend"])
    return near, alt - qv


def dcn_tie_counts(kind, near, k):
    """Near-tie terms per output of `kind`: "out" [n, k, P, Q] (the (c, tap) terms of a pixel), "dw" [k, c, T] (the (n, p, q) terms)."""
    if kind == "out":
        cnt = near.sum((1, 2))
        return np.broadcast_to(cnt[:, None], (cnt.shape[0], k) + cnt.shape[1:])
    cnt = near.sum((0, 3, 4))
    return np.broadcast_to(cnt[None], (k,) + cnt.shape)


def dcn_tie_deltas(kind, idx, near, alt_minus, other):
    """delta_i = other operand x (alternative rounding - chosen rounding) of the near-tie terms of the sampled outputs idx, zero-padded
    -> [S, DCN_TIE_MAX] (samples must hold at most DCN_TIE_MAX such terms).  other: w3 [k, c, T] for "out", dY's image [n, k, P, Q]
    for "dw" (idx = (k, c, tap))."""
    if kind == "out":
        i0, i1, i2, i3 = idx
        nr = near[i0, :, :, i2, i3].reshape(len(i0), -1)
        dl = (alt_minus[i0, :, :, i2, i3] * other[i1]).reshape(len(i0), -1)
    else:
        i0, i1, i2 = idx
        nr = near[:, i1, i2].transpose(1, 0, 2, 3).reshape(len(i0), -1)
        dl = (alt_minus[:, i1, i2] * other[:, i0]).transpose(1, 0, 2, 3).reshape(len(i0), -1)
    assert nr.sum(1).max() <= DCN_TIE_MAX
    order = np.argsort(~nr, axis=1, kind="stable")[:, :DCN_TIE_MAX]
    return np.take_along_axis(np.where(nr, dl, 0.0), order, 1)


def dcn_tie_adjust(err, deltas):
    """err [S] = got - ref; deltas [S, t] -> err - sum over the subset of deltas that leaves the smallest |.| (all 2^t are tried)."""
    tmax = deltas.shape[1]
    combos = ((np.arange(1 << tmax)[:, None] >> np.arange(tmax)) & 1).astype(np.float64)
    cand = np.asarray(err, np.float64)[:, None] - deltas @ combos.T
    return cand[np.arange(len(cand)), np.abs(cand).argmin(1)]


def _chain32(terms):
    return np.cumsum(np.asarray(terms).astype(np.float32), axis=1, dtype=np.float32)[:, -1].astype(np.float64)


def dcn_chain_dcol(gy, w3):
    """dcol [n, c, T, P, Q] = sum over k of dY x W chained in float32 in plain loop order (float32 array)."""
    gy, w3 = np.asarray(gy, np.float64).astype(np.float32), np.asarray(w3, np.float64).astype(np.float32)
    acc = np.zeros((gy.shape[0],) + w3.shape[1:] + gy.shape[2:], np.float32)
    for k in range(w3.shape[0]):
        acc += gy[:, k, None, None] * w3[k][None, :, :, None, None]
    return acc


def dcn_terms(kind, idx, y, chunk=1 << 24):
    """The float32 terms of the sampled outputs idx of one tensor, in plain loop order: yields float64 arrays [s, terms] covering idx in
    order.  y: the yardstick's operands — "col" [n, c, T, P, Q] (the float32 oracle's columns, or the bf16 images), "w3" [k, c, T],
    "gy" [n, k, P, Q], "bias", "dcol" (dcn_chain_dcol), "m32" (dcn_model in float32: geometry, corner values, mask), "base_dx",
    "base_dw".
      "out"     idx (n, k, p, q): col x W over (c, tap), then bias
      "dw"      idx (k, c, tap): base, then dY x col over (n, p, q)
      "dmask"   idx (n, g T + tap, p, q): dcol x wgt_e x x_e over (c, corner)
      "doffset" idx (n, g 2T + 2 tap + {0, 1}, p, q): dcol x mask x d wgt_e x x_e over (c, corner)
      "dx"      idx (n, c, y, x): base, then dcol x mask x wgt_e over the (tap, p, q, corner) whose corner is that pixel"""
    N = None
    if kind == "out":
        i0, i1, i2, i3 = idx
        t = (y["col"][i0, :, :, i2, i3] * y["w3"][i1]).reshape(len(i0), -1)
        tail = np.zeros(len(i0)) if y.get("bias") is None else _np64(y["bias"])[i1]
        yield np.concatenate([t, tail[:, N]], 1)
        return
    if kind == "dw":
        i0, i1, i2 = idx
        t = (y["col"][:, i1, i2] * y["gy"][:, i0]).transpose(1, 0, 2, 3).reshape(len(i0), -1)
        head = np.zeros(len(i0)) if y.get("base_dw") is None else _np64(y["base_dw"]).reshape(y["w3"].shape)[i0, i1, i2]
        yield np.concatenate([head[:, N], t], 1)
        return
    m = y["m32"]
    geo, xs, mk = m["geo"], m["xs"], m["mask"]
    n, dg, cpg, t_all, p, q = xs.shape[1:]
    dcg = y["dcol"].reshape(n, dg, cpg, t_all, p, q).astype(np.float64)
    if kind in ("dmask", "doffset"):
        i0, ch, i2, i3 = idx
        if kind == "dmask":
            g, tap = np.divmod(ch, t_all)
            fac = geo["wgt"][:, i0, g, tap, i2, i3].astype(np.float64)                                  # [4, S]
        else:
            g, rest = np.divmod(ch, 2 * t_all)
            tap, hw = np.divmod(rest, 2)
            fac = np.where(hw == 0, geo["dwh"][:, i0, g, tap, i2, i3], geo["dww"][:, i0, g, tap, i2, i3]).astype(np.float64)
            fac = fac * mk[i0, g, tap, i2, i3].astype(np.float64)
        xv = xs[:, i0, g, :, tap, i2, i3].astype(np.float64)                                            # [S, 4, cpg]
        yield (dcg[i0, g, :, tap, i2, i3][:, N] * fac.T[:, :, N] * xv).transpose(0, 2, 1).reshape(len(i0), -1)
        return
    # dx: per (n, group) the valid corners sorted by the pixel they land on
    i0, i1, i2, i3 = idx
    wd = m["wd"]
    g, cl = np.divmod(i1, cpg)
    pix = i2 * wd + i3
    cw = (geo["wgt"] * geo["valid"]).astype(np.float64) * mk[N].astype(np.float64)                     # [4, n, dg, T, P, Q]
    base = None if y.get("base_dx") is None else _np64(y["base_dx"])
    lists = {}
    for key in set(zip(i0.tolist(), g.tolist())):
        tgt = np.where(geo["valid"][:, key[0], key[1]], geo["idx"][:, key[0], key[1]], -1).transpose(1, 2, 3, 0).ravel()
        order = np.argsort(tgt, kind="stable")
        lists[key] = (order, np.searchsorted(tgt[order], np.arange(m["npix"] + 1)))
    step = max(1, chunk // max(1, 4 * t_all * p * q))
    for lo in range(0, len(i0), step):
        sl = slice(lo, lo + step)
        rows, width = [], 1
        for a, b, c_, px in zip(i0[sl], g[sl], cl[sl], pix[sl]):
            order, start = lists[int(a), int(b)]
            ent = order[start[px]:start[px + 1]]                                  # entries (tap, p, q, corner) flattened
            e = ent % 4
            tpq = ent // 4
            rows.append(dcg[a, b, c_].ravel()[tpq] * cw[:, a, b].transpose(1, 2, 3, 0).ravel()[ent] if len(ent) else np.zeros(0))
            width = max(width, len(ent))
        out = np.zeros((len(rows), width + 1))
        for j, row in enumerate(rows):
            out[j, 1:1 + len(row)] = row
        if base is not None:
            out[:, 0] = base[i0[sl], i1[sl], i2[sl], i3[sl]]
        yield out


def dcn_yardstick(kind, idx, y, ref_s):
    """The chained float32 evaluation of the sampled outputs minus the float64 reference at them -> (max-abs, RMS)."""
    seq = np.concatenate([_chain32(t) for t in dcn_terms(kind, idx, y)])
    err = seq - np.asarray(ref_s, np.float64)
    return float(np.abs(err).max()), float(np.sqrt(np.mean(err * err)))


def dcn_error_ratios(got, ref, idx, yard, allow=None, deltas=None, keep=None, slack=None):
    """conv_error_ratios for one DCN tensor: got, ref whole tensors (float64 arrays), idx the sampled positions, yard = (max_seq,
    rms_seq).  allow: per-element allowance subtracted from |error| (the fixed-point window); deltas [S, t]: the bf16 near-tie terms of
    the samples (dcn_tie_adjust); keep / slack: whole-tensor mask of outputs that are not left out / their sum of |delta|.
    -> (ratios, share): share = the largest part the allowance takes of a sample's bound margin x max_seq + allowance."""
    err = np.asarray(got, np.float64) - np.asarray(ref, np.float64)
    es = err[idx]
    if deltas is not None:
        es = dcn_tie_adjust(es, deltas)
    share = 0.0
    if allow is not None:
        al = allow[idx]
        share = float((al / (DCN_MARGIN * yard[0] + al + 1e-300)).max())
        es = np.sign(es) * np.maximum(np.abs(es) - al, 0.0)
        err = np.sign(err) * np.maximum(np.abs(err) - allow, 0.0)
    if slack is not None:
        err = np.sign(err) * np.maximum(np.abs(err) - slack, 0.0)
    if keep is not None:
        err = err[keep]
    zero = np.zeros_like
    return conv_error_ratios(es, zero(es), yard[0], yard[1], err, zero(err)), share


# ---- edge inputs (seeded); tests/test_host_logic.py asserts from the float64 geometry that each holds what it claims ----
def dcn_edge_inputs(cls, geo, seed, margin=3):
    """Seeded float32 inputs (x, offset, mask, w, bias, gy) of edge class cls (DCN_EDGE_CLASSES) for geometry
    geo = (n, c, h, w, k, r, s, stride, pad_h, pad_w, dilation, groups).  margin: the LDS window margin the plan reports ("beyond")."""
    n, c, h, w, k, r, s, stride, ph, pw, dil, dg = geo
    p, q = dcn_out_hw(h, w, r, s, stride, ph, pw, dil)
    t = r * s
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    x = torch.randn(n, c, h, w, generator=g)
    off = (torch.randn(n, dg, t, 2, p, q, generator=g) * 1.5).numpy()
    mask = torch.sigmoid(torch.randn(n, dg * t, p, q, generator=g))
    wt = torch.randn(k, c, r, s, generator=g) / float(np.sqrt(c * t))
    bias = torch.randn(k, generator=g)
    gy = torch.randn(n, k, p, q, generator=g)
    ti, tj = np.divmod(np.arange(t), s)
    bh = np.broadcast_to((np.arange(p)[None, :] * stride - ph + ti[:, None] * dil)[None, None, :, :, None], (n, dg, t, p, q)).astype(np.float32)
    bw = np.broadcast_to((np.arange(q)[None, :] * stride - pw + tj[:, None] * dil)[None, None, :, None, :], (n, dg, t, p, q)).astype(np.float32)
    base = (bh, bw)
    size = (h, w)

    def place(axis, sel, target):
        """offset such that float32(base + offset) == target where that is representable; elsewhere the sample keeps its offset."""
        o = (np.asarray(target, np.float32) - base[axis]).astype(np.float32)
        ok = sel & ((base[axis] + o).astype(np.float32) == np.asarray(target, np.float32))
        off[:, :, :, axis][ok] = o[ok]
        return ok

    if cls == "border":
        pp, qq = np.arange(p)[:, None], np.arange(q)[None, :]
        for axis, first, last in ((0, pp == 0, pp == p - 1), (1, qq == 0, qq == q - 1)):
            u = rng.uniform(0.1, 0.9, (n, dg, t, p, q)).astype(np.float32)
            off[:, :, :, axis] = np.where(first, (u - 1) - base[axis], np.where(last, (size[axis] - 1 + u) - base[axis], off[:, :, :, axis]))
    elif cls == "exact":
        for axis in (0, 1):
            kind = rng.integers(0, 10, (n, dg, t, p, q))                                  # 8, 9: the sample keeps its Gaussian offset
            off[:, :, :, axis][kind == 0] = 0.0
            place(axis, kind == 1, np.clip(base[axis] + rng.integers(-2, 3, kind.shape), 0, size[axis] - 1))
            place(axis, kind == 2, np.float32(-1))
            place(axis, kind == 3, np.float32(size[axis]))
            place(axis, (kind == 4) | (kind == 5), np.nextafter(np.float32(-1), np.float32(0)))    # representable next to few grid positions
            place(axis, (kind == 6) | (kind == 7), np.nextafter(np.float32(size[axis]), np.float32(0)))
    elif cls == "beyond":
        way = rng.integers(0, 8, (n, dg, t, p, q))                                       # 0..3: up, down, left, right; others stay
        dist = rng.uniform(margin + 1, margin + 6, way.shape).astype(np.float32)
        off[:, :, :, 0] = np.where(way == 0, -dist, np.where(way == 1, dist, off[:, :, :, 0]))
        off[:, :, :, 1] = np.where(way == 2, -dist, np.where(way == 3, dist, off[:, :, :, 1]))
    elif cls == "far":
        pick = rng.integers(0, 240, (n, dg, t, p, q))                                    # 5 % of the samples: 12 of 240
        vals = np.array([1e4, -1e4, 3e9, -3e9, 1e30, -1e30], np.float32)
        for j in range(12):
            off[:, :, :, j % 2][pick == j] = vals[j // 2]
    elif cls == "pile":
        off[:, :, :, 0] = np.float32(0.43 * h - 0.2) - bh
        off[:, :, :, 1] = np.float32(0.57 * w - 0.4) - bw
        mask = torch.rand(n, dg * t, p, q, generator=g) * 0.5 + 0.5
        wt = (torch.rand(k, c, r, s, generator=g) + 0.5) / float(c * t)
        gy = torch.rand(n, k, p, q, generator=g) + 0.5
    elif cls == "operands":
        mask = torch.randn(n, dg * t, p, q, generator=g) * 1.2
        mask[torch.rand(mask.shape, generator=g) < 0.1] = 0.0
        x = x * torch.exp2(torch.randint(-12, 13, (1, c, 1, 1), generator=g).float())
        gy = gy * torch.exp2(torch.randint(-12, 13, (1, k, 1, 1), generator=g).float())
    else:
        assert cls == "gauss", cls
    return x, torch.from_numpy(off.reshape(n, 2 * dg * t, p, q).astype(np.float32)), mask, wt, bias, gy


# ---- the grid: the smallest shapes that still split.  name -> (n, c, h, w, k, r, s, stride, pad_h, pad_w, dilation, groups) ----
DCN64_GRID = {
    "k36":       (2, 32, 17, 20, 36, 3, 3, 1, 1, 1, 1, 1),      # ragged 8x16 blocks (3 x 2), a partial 32-filter slab: window kernels, no DMA
    "k64":       (2, 64, 9, 17, 64, 3, 3, 1, 1, 1, 1, 1),       # 2 x 2 ragged blocks, two channel chunks: dY by DMA, the DMA sweep
    "k12":       (1, 32, 9, 17, 12, 3, 3, 1, 1, 1, 1, 1),       # K <= 32: the 32-wide gather forward
    "k256":      (1, 32, 9, 17, 256, 3, 3, 1, 1, 1, 1, 1),      # one 256-filter tile
    "k260":      (1, 32, 9, 17, 260, 3, 3, 1, 1, 1, 1, 1),      # two 256-filter tiles in the weight gradient, 128-wide forward window
    "k388":      (1, 32, 9, 17, 388, 3, 3, 1, 1, 1, 1, 1),      # K > 384: the 256-wide forward window with a ragged second tile
    "stride2":   (2, 32, 17, 19, 36, 3, 3, 2, 1, 1, 1, 1),      # stride 2: the L2-gather kernels in every pass
    "c8":        (1, 8, 9, 17, 36, 3, 3, 1, 1, 1, 1, 1),        # C % 32 != 0: gather kernels at stride 1
    "dil2":      (1, 32, 12, 20, 64, 3, 3, 1, 2, 2, 2, 1),      # dilation 2: the window fits only with a smaller margin
    "dil3g2":    (1, 256, 14, 14, 32, 3, 3, 1, 3, 3, 3, 2),     # dilation 3, two groups of 128: the gather data gradient
    "5x5":       (1, 64, 11, 9, 64, 5, 5, 1, 2, 2, 1, 1),       # 5x5: forward on the window, gradients on the gather kernels
    "g2":        (1, 64, 10, 18, 48, 3, 3, 1, 1, 1, 1, 2),      # two groups of 32 channels
    "g4":        (1, 128, 9, 17, 32, 3, 3, 1, 1, 1, 1, 4),      # four groups of 32 channels
    "edge":      (1, 32, 18, 24, 64, 3, 3, 1, 1, 1, 1, 1),      # 3 x 2 blocks; tall and wide enough that, from a block on one image border,
                                                                # corners beyond the window margin still lie inside the image in all four directions
}
DCN64_EDGE_CASES = ("edge", "stride2")
DCN64_BF16_PASSES = {"dil3g2": (DCN_DGRAD,)}  # 2304 terms per output leave fewer than a third of them without a near-tie column: the shape is
                                              # there for its data gradient (no tie handling), its bf16 forward / weight gradient are not run        # one window route and one gather route per pass: every edge class runs on both


def dcn64_entries(shape, margin=3):
    """What tests/test_dcn_fp64_gpu.py calls for the grid shape named `shape`: [(pass, entry point of DCN_ENTRY_FLAGS, bf16, flags, labels
    the plan mirror gives)]; entries whose plan refuses the shape are left out (the refusals have their own test)."""
    out, geo = [], DCN64_GRID[shape]
    for pas in (DCN_FWD, DCN_WGRAD, DCN_DGRAD):
        for name, (bf, flags) in DCN_ENTRY_FLAGS[pas].items():
            if bf and pas not in DCN64_BF16_PASSES.get(shape, (DCN_FWD, DCN_WGRAD, DCN_DGRAD)):
                continue
            plan = dcn_plan_mirror(pas, bf, geo, margin, flags)
            if plan is not None:
                out.append((pas, name, bf, flags, plan["labels"]))
    return out


class DcnCase:
    """One (grid shape, edge class, operand precision): inputs, float64 reference, yardsticks and the acceptance rule of every tensor.
    Built on the CPU only; check(tensor, got, ...) -> (ratios, allowance share, accepted)."""

    def __init__(self, geo, cls, bf16, seed=0, margin=3, accumulate=False, samples=CONV_SAMPLES):
        n, c, h, w, k, r, s, stride, ph, pw, dil, dg = geo
        self.geo, self.cls, self.bf16, self.margin = geo, cls, bf16, margin
        seed = seed + zlib.crc32(repr((geo, cls)).encode()) % 100000
        self.inputs = x, off, mask, wt, bias, gy = dcn_edge_inputs(cls, geo, seed, margin)
        gen = torch.Generator().manual_seed(seed + 1)
        self.base_dw = torch.randn(k, c, r, s, generator=gen) * 0.1
        self.base_dx = torch.randn(n, c, h, w, generator=gen) * float(gy.abs().mean()) if accumulate else None
        args = (x, off, mask, wt, bias, stride, (ph, pw), dil, dg)
        self.m64 = dcn_model(*args, gy=gy, base_dx=self.base_dx, base_dw=self.base_dw, bf16=bf16, blocks=True)
        self.m32 = dcn_model(*args, gy=gy, dtype=np.float32)
        self.m32["wd"], self.m32["npix"] = w, h * w
        self.ref = dcn_ref64(*args, gy=gy, base_dx=self.base_dx, bf16=bf16)
        self.ref["dw"] = (self.ref["dw"] + _np64(self.base_dw)).reshape(k, c, r * s)
        if bf16:
            ycol, yw, ygy = self.m64["colq"], self.m64["w3"], self.m64["gyq"]
            self.near, self.alt_minus = dcn_tie_info(self.m64)
        else:
            from oracle import dcn as odcn
            ycol = odcn.dcn_columns(x, off, mask, r, s, stride, (ph, pw), dil, dg, pos_fp32=True).numpy().astype(np.float64)
            yw, ygy = _np64(wt).reshape(k, c, r * s), _np64(gy)
        self.y = {"col": ycol, "w3": yw, "gy": ygy, "bias": bias, "dcol": dcn_chain_dcol(ygy, yw), "m32": self.m32,
                  "base_dx": self.base_dx, "base_dw": self.base_dw}
        self.samples, self._yard, self._tie = samples, {}, {}
        self.allow, self.allow_fx = dcn_fixed_point_allowance(self.m64, self.base_dx)

    def tie(self, tensor):
        """bf16 "out" / "dw": (keep mask over the tensor, near-tie counts)."""
        if tensor not in self._tie:
            cnt = dcn_tie_counts(tensor, self.near, self.geo[4])
            self._tie[tensor] = (cnt <= DCN_TIE_MAX, cnt)
        return self._tie[tensor]

    def yard(self, tensor):
        if tensor not in self._yard:
            ref = self.ref[tensor]
            keep = self.tie(tensor)[0] if (self.bf16 and tensor in ("out", "dw")) else None
            idx = conv_sample_positions(ref.shape, zlib.crc32(tensor.encode()) % 1000, self.samples, keep)
            if tensor == "cols":
                err = self.y["col"][idx] - ref[idx] if not self.bf16 else np.zeros(1)
                yd = (float(np.abs(err).max()), float(np.sqrt(np.mean(err * err))))
            else:
                yd = dcn_yardstick(tensor, idx, self.y, ref[idx])
            self._yard[tensor] = (idx, yd)
        return self._yard[tensor]

    def check(self, tensor, got, window=False, ties=True):
        """got: the kernel's tensor in the reference's layout (dw as [k, c, T]).  window: a window data-gradient route (the fixed-point
        allowance applies to dx).  ties: bf16 columns are rounded by the kernel (False where the test hands over rounded columns)."""
        idx, yd = self.yard(tensor)
        ref = self.ref[tensor]
        kw = {}
        if tensor == "dx" and window:
            kw["allow"] = self.allow
        if self.bf16 and ties and tensor in ("out", "dw"):
            keep, _ = self.tie(tensor)
            other = self.m64["w3"] if tensor == "out" else self.m64["gyq"]
            kw["deltas"] = dcn_tie_deltas(tensor, idx, self.near, self.alt_minus, other)
            ad = np.abs(self.alt_minus) * self.near
            if tensor == "out":
                kw["slack"] = np.einsum("nctpq,kct->nkpq", ad, np.abs(other), optimize=True)
            else:
                kw["slack"] = np.einsum("nkpq,nctpq->kct", np.abs(other), ad, optimize=True)
            kw["keep"] = keep
        ratios, share = dcn_error_ratios(_np64(got).reshape(ref.shape), ref, idx, yd, **kw)
        return ratios, share, conv_accepts(ratios, DCN_MARGIN)


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm forward / ReLU-mask agreement (tests/test_bn_forward_gpu.py; tests/test_bn_mask_host.py checks the builder).
# ------------------------------------------------------------------------------------------------------------------
def bf16_exact(a):
    """float32 array -> the same values rounded to bfloat16 (nearest even), as float32."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def bf16_half_ulp(v):
    """Half a bfloat16 ulp at magnitude v (float64 array, normal range): the most a round-to-nearest conversion of a value of
    that magnitude can move it.  bfloat16 keeps 8 significant bits, its ulp at v is 2^(floor(log2 v) - 7)."""
    v = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(v)) - 8.0)


def bn_mask_edge_inputs(seed, c, pixels, bf16=False):
    """Inputs that sit ON the ReLU edge of y * sc + sh: per channel sc ~ N(1, 0.3), sh ~ N(0, 0.5) (float32), y0 = fl32(-sh / sc),
    every element y0 stepped by k in [-3, 3] float32 ulps.  The exact value y * sc + sh is then a few ulps of sh: a 48-bit product
    plus a 24-bit addend of like exponent, representable in float64, so `exact` below IS exact and `mask = exact > 0` leaves no
    element out.  A mul + add that rounds the product first (fl(fl(y * sc) + sh)) gets the sign wrong on a few per cent of such a
    set (muladd32_mask; measured 6.4 % at seed 7, c 64, pixels 4096); one explicit fma never does.
    bf16: y holds bfloat16 values (y0 rounded to bfloat16, steps of bfloat16 ulps) so that it can live as a bf16 image only; sh is
    then re-centred to fl32(-y0 * sc), which puts the k = 0 elements on the rounding residue of that product (the others lie
    2^-8 |sh| away from the edge).
    -> dict: y, dz [pixels, c] float32 (dz: magnitude in [0.5, 1.5], random sign), sc, sh [c] float32, exact [pixels, c]
    float64, mask [pixels, c] bool."""
    rng = np.random.default_rng(seed)
    sc = rng.normal(1.0, 0.3, c).astype(np.float32)
    sh = rng.normal(0.0, 0.5, c).astype(np.float32)
    sc[np.abs(sc) < 0.05] = 0.05                       # (a scale next to zero would send y0 towards overflow)
    sh[sh == 0.0] = 0.25
    y0 = (-sh.astype(np.float64) / sc.astype(np.float64)).astype(np.float32)
    ulp = 1
    if bf16:
        y0 = bf16_exact(y0)
        sh = (-(y0.astype(np.float64) * sc.astype(np.float64))).astype(np.float32)
        ulp = 1 << 16
    k = rng.integers(-3, 4, (pixels, c))
    bits = np.broadcast_to(y0.view(np.int32)[None, :], (pixels, c)).astype(np.int64)
    bits = bits + k * ulp * np.sign(y0).astype(np.int64)[None, :]       # the integer view moves the MAGNITUDE: k ulps of value
    y = bits.astype(np.int32).view(np.float32)
    if bf16:
        assert np.array_equal(bf16_exact(y), y)
    dz = (rng.uniform(0.5, 1.5, (pixels, c)) * rng.choice([-1.0, 1.0], (pixels, c))).astype(np.float32)
    exact = y.astype(np.float64) * sc.astype(np.float64)[None, :] + sh.astype(np.float64)[None, :]
    return dict(y=y, dz=dz, sc=sc, sh=sh, exact=exact, mask=exact > 0.0, k=k)


def muladd32_mask(y, sc, sh):
    """The sign a float32 multiply followed by a float32 add gives (the product rounded on its own): what a kernel that lost its
    explicit fma and was compiled without contraction would compute."""
    return ((y * sc[None, :]).astype(np.float32) + sh[None, :]).astype(np.float32) > 0.0


def nhwc_from_rows(a, n=1):
    """[pixels, c] array -> torch tensor of logical shape [n, c, 1, pixels / n] over the same NHWC memory."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    p, c = t.shape
    return t.view(n, 1, p // n, c).permute(0, 3, 1, 2)


def bn_apply_ref64(y, scale, shift, residual=None, relu=False):
    """relu?(y * scale + shift [+ residual]) in float64 on [pixels, c] arrays, and the sum of the magnitudes the float32 bound is
    taken of: |y * scale| + |shift| + |residual|."""
    ys = y.astype(np.float64) * scale.astype(np.float64)[None, :]
    v = ys + shift.astype(np.float64)[None, :]
    mag = np.abs(ys) + np.abs(shift.astype(np.float64))[None, :]
    if residual is not None:
        v = v + residual.astype(np.float64)
        mag = mag + np.abs(residual.astype(np.float64))
    return (np.maximum(v, 0.0) if relu else v), mag


# ------------------------------------------------------------------------------------------------------------------
# hourglass up path (tests/test_fanin_upsample_gpu.py)
# ------------------------------------------------------------------------------------------------------------------
def upsample_add_ref64(up1, low):
    """up1 + F.interpolate(F.interpolate(low, scale_factor=2), size=up1's, mode="bilinear", align_corners=True) in float64
    (NCHW tensors), as backbones/hourglass.py's up path composes it."""
    import torch.nn.functional as F
    up = F.interpolate(low.double(), scale_factor=2)
    return up1.double() + F.interpolate(up, size=tuple(up1.shape[2:]), mode="bilinear", align_corners=True)


def bf16_crafted_vector(seed=5, normals=1000):
    """float32 values on which a float32 -> bfloat16 conversion can go wrong (bit patterns noted; 0x7f in the low half word below
    the tie, 0x80 00 the tie, 0x80 01 above it): ties with an even and an odd kept mantissa, one float32 ulp either side of each,
    +-0, +-Inf, NaN, the largest finite float32 (rounds to Inf), the largest value that stays finite, and random normals.
    float32 subnormals are left out.  The length is a multiple of 4."""
    pat = [0x3f808000, 0x3f818000,              # ties: kept mantissa even (rounds down), odd (rounds up)
           0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001,
           0xbf808000, 0xbf818000, 0xbf807fff, 0xbf818001,
           0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001,
           0x7f7fffff, 0xff7fffff, 0x7f7f7fff, 0x7f7f8000,      # max finite -> Inf; just below the last tie stays finite; the tie -> Inf
           0x00800000, 0x80800000, 0x3f800000, 0x3f7fffff, 0x3fffffff, 0x477fe000]
    v = np.array(pat, dtype=np.uint32).view(np.float32)
    r = np.random.default_rng(seed).normal(0.0, 1.0, normals).astype(np.float32)
    out = np.concatenate([v, r, r * np.float32(1e-20), r * np.float32(1e20)])
    keep = (np.abs(out) >= np.float32(2.0 ** -126)) | (out == 0) | ~np.isfinite(out)
    out = out[keep]
    return np.ascontiguousarray(out[:len(out) // 4 * 4])

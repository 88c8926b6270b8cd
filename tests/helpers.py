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
    over one ~6x6 patch of image 1 (the backward's atomics race on its pixels)."""
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


def roi_dyadic_case(size, sr, scale, ch):
    """The dyadic RoI set of one ROI_DYADIC_CASES entry."""
    _, h, w = ROI_DYADIC_MAP
    return roi_dyadic_set(seed=100 * size[0] + 10 * size[1] + ch + (sr > 0), out_size=size, sampling_ratio=sr,
                          spatial_scale=scale, height=h, width=w)


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

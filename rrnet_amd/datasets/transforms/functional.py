"""Host restatements of the reference's datasets/transforms/functional.py that the data layer needs: the two
test-time helpers the operators call (flip evaluation, operators/centernet_operator.py:259-262) and the pixel /
annotation steps of the training chain (resize, to_tensor, mask_ignore, crop, normalize).  These are the *host path*:
the CPU loader runs them, and the device kernel rr_augment_frames (csrc/augment.hip) is checked against them bit for bit.
Target generation (gaussian splat + regression targets, functional.py:177-262 of the reference) is the device kernel
rr_ctnet_targets, reached through rrnet_amd.datasets.synthetic.collate_ctnet_device / the ToHeatmap transform."""
import numpy as np
import torch

PRECISION_BITS = 32 - 8 - 2          # PIL's fixed-point coefficient precision for 8-bit channels (Resample.c)


def flip_img(data):
    """datasets/transforms/functional.py:13-19: horizontal flip of a [C,H,W] image tensor."""
    return data.flip(dims=(2,))


def flip_annos(data, w):
    """datasets/transforms/functional.py:22-29: x -> w - x - width for xywh rows (in place, like the reference)."""
    data[:, 0] = w - data[:, 0] - data[:, 2]
    return data


def img_to_tensor(data):
    """functional.py:32-38 (torchvision's to_tensor for an 8-bit RGB image): PIL image or uint8 HWC array ->
    float32 [3,H,W] = uint8.float().div(255)."""
    arr = torch.from_numpy(np.array(data, dtype=np.uint8, copy=True))
    return arr.permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def annos_to_tensor(data):
    """functional.py:41-56: annotation rows (integer array, or the raw text lines) -> float32 tensor."""
    if len(data) and isinstance(data[0], str):
        data = [[int(x) for x in d.strip().split(',')] for d in data]
    return torch.tensor(np.asarray(data)).float()


def resize_annos(anno, scale_factor):
    """functional.py:81: `anno[:, :4] = anno[:, :4] * scale_factor` written back into the INTEGER annotation array, so
    the scaled coordinates are truncated toward zero (517 * 1.15 -> 594).  In place, like the reference."""
    anno[:, :4] = anno[:, :4] * scale_factor
    return anno


def scaled_size(height, width, scale_factor):
    """functional.py:77."""
    return int(height * scale_factor), int(width * scale_factor)


def resize(data, scale_factor):
    """functional.py:72-82 without the road map: (PIL image, integer annotations[, ...]) -> PIL bilinear resize to
    (int(h*s), int(w*s)) and the truncated annotations."""
    from PIL import Image
    img, anno = data[0], data[1]
    out_h, out_w = scaled_size(img.size[1], img.size[0], scale_factor)
    img = img.resize((out_w, out_h), Image.BILINEAR)
    return (img, resize_annos(anno, scale_factor)) + tuple(data[2:])


def crop_tensor(data, crop_coor):
    """functional.py:104-111."""
    return data[:, int(crop_coor[1]):int(crop_coor[3]), int(crop_coor[0]):int(crop_coor[2])]


def crop_annos(data, crop_coor, h, w):
    """functional.py:114-132: xywh rows relative to the crop origin, clipped to the crop (in place)."""
    crop_coor_tensor = torch.tensor(crop_coor).float().unsqueeze(0)
    data[:, 2:4] = data[:, :2] + data[:, 2:4]
    data[:, :4] -= crop_coor_tensor[:, :2].repeat(1, 2)
    data[data[:, 0] < 0, 0] = 0
    data[data[:, 1] < 0, 1] = 0
    data[data[:, 2] > w, 2] = w
    data[data[:, 3] > h, 3] = h
    data[:, 2] = data[:, 2] - data[:, 0]
    data[:, 3] = data[:, 3] - data[:, 1]
    return data


def normalize(data, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """functional.py:135-143 (torchvision's normalize): (x - mean) / std per channel in the tensor's dtype."""
    mean = torch.tensor(mean, dtype=data.dtype).view(-1, 1, 1)
    std = torch.tensor(std, dtype=data.dtype).view(-1, 1, 1)
    return (data - mean) / std


def ignore_rects(annos, height, width, ignore_cls=0):
    """The half-open slices `int(y):int(y+h), int(x):int(x+w)` of functional.py:305-307, resolved against a frame of
    height x width the way Python resolves a slice (clipped; an empty slice stays empty) -> int32 [k,4] rows
    (y0, y1, x0, x1).  This is what the device kernel receives."""
    rows = []
    for x, y, w, h in np.asarray(annos)[np.asarray(annos)[:, 5] == ignore_cls, :4].tolist():
        y0, y1, _ = slice(int(y), int(y + h)).indices(height)
        x0, x1, _ = slice(int(x), int(x + w)).indices(width)
        rows.append((y0, max(y1, y0), x0, max(x1, x0)))
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def mask_ignore(data, mean=(0.485, 0.456, 0.406), ignore_cls=0):
    """functional.py:290-313 without the road map: fill the ignore regions with `mean` (in place) and drop their rows.
    The reference selects the kept rows with `data[1][1 - ign_idx, :]`; torch refuses `1 - <bool tensor>` today, and
    on the uint8 masks it was written for the expression is the mask's negation, so it is restated as `~ign_idx`."""
    mean = torch.tensor(mean).unsqueeze(1).unsqueeze(1)
    img = data[0]
    ign_idx = data[1][:, 5] == ignore_cls
    for ign_bbox in data[1][ign_idx, :4]:
        x, y, w, h = ign_bbox[:4]
        img[:, int(y):int(y + h), int(x):int(x + w)] = mean
    return (img, data[1][~ign_idx, :]) + tuple(data[2:])


def pil_bilinear_taps(in_size, out_size):
    """The coefficients of one pass of PIL's `Image.resize(..., BILINEAR)` for 8-bit channels (Resample.c:
    precompute_coeffs + normalize_coeffs_8bpc) for out_size >= in_size, as int32 [out_size, 3] rows
    (first tap, k0, k1): output i = clip8((src[first]*k0 + src[first+1]*k1 + (1 << 21)) >> 22).  Weights are computed in
    double, normalised, and converted as (int)(k * (1 << 22) + 0.5); an up-scale has at most two non-zero taps per
    output coordinate.  Equal sizes give the identity table (PIL skips the pass)."""
    if out_size < in_size:
        raise ValueError("pil_bilinear_taps: %d -> %d shrinks; only scale factors >= 1 have two taps" % (in_size, out_size))
    one = 1 << PRECISION_BITS
    tab = np.zeros((out_size, 3), dtype=np.int32)
    if out_size == in_size:
        tab[:, 0] = np.arange(out_size)
        tab[:, 1] = one
        return tab
    scale = float(in_size) / out_size
    support = 1.0                                   # bilinear support * max(scale, 1)
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)
    xmax = np.minimum(np.trunc(center + support + 0.5), in_size).astype(np.int64) - xmin
    ksize = 3
    k = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    for x in range(ksize):
        arg = np.abs((x + xmin).astype(np.float64) - center + 0.5)
        w = np.where((arg < 1.0) & (x < xmax), 1.0 - arg, 0.0)
        k[:, x] = w
        ww = ww + w
    k = np.where(ww[:, None] != 0.0, k / np.where(ww == 0.0, 1.0, ww)[:, None], k)
    ki = np.trunc(0.5 + k * one).astype(np.int64)
    nz = ki != 0
    first = np.argmax(nz, axis=1)
    last = ksize - 1 - np.argmax(nz[:, ::-1], axis=1)
    if not nz.any(axis=1).all() or (last - first > 1).any():
        raise ValueError("pil_bilinear_taps: %d -> %d needs more than two taps" % (in_size, out_size))
    rows = np.arange(out_size)
    tab[:, 0] = xmin + first
    tab[:, 1] = ki[rows, first]
    tab[:, 2] = np.where(last > first, ki[rows, np.minimum(first + 1, ksize - 1)], 0)
    return tab


def resize_u8_taps(img, out_h, out_w):
    """PIL's two separable 8-bit passes restated with the tap tables: uint8 [H,W,C] -> uint8 [out_h,out_w,C].  The
    horizontal pass comes first and rounds to uint8; the vertical pass follows.  Checker for the tables (the host
    path itself calls PIL)."""
    img = np.asarray(img, dtype=np.int64)
    half = 1 << (PRECISION_BITS - 1)
    for axis, out in ((1, out_w), (0, out_h)):
        n = img.shape[axis]
        t = pil_bilinear_taps(n, out).astype(np.int64)
        a = np.take(img, t[:, 0], axis=axis)
        b = np.take(img, np.minimum(t[:, 0] + 1, n - 1), axis=axis)
        shape = [1, 1, 1]
        shape[axis] = out
        acc = a * t[:, 1].reshape(shape) + b * t[:, 2].reshape(shape) + half
        img = np.clip(acc >> PRECISION_BITS, 0, 255)
    return img.astype(np.uint8)

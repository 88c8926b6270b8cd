"""Host restatements of the reference's datasets/transforms/functional.py that the data layer needs: the two
test-time helpers the operators call (flip evaluation, operators/centernet_operator.py:259-262) and the pixel /
annotation steps of the training chain (resize, to_tensor, mask_ignore, fill_duck, crop, normalize).  These are the
*host path*: the CPU loader runs them, and the device kernels rr_augment_frames (csrc/augment.hip) and
rr_augment_frames_pasted (csrc/augment_paste.hip) are checked against them: bit for bit, except for the pixels FillDuck
pastes, which are held to a derived bound (see apply_paste_plan).
Target generation (gaussian splat + regression targets, functional.py:177-262 of the reference) is the device kernel
rr_ctnet_targets, reached through rrnet_amd.datasets.synthetic.collate_ctnet_device / the ToHeatmap transform."""
import math

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


def nearest_resize(a, out_h, out_w):
    """cv2.resize(..., interpolation=cv2.INTER_NEAREST) of functional.py:79 restated for a [H,W(,C)] array: source
    index sx = min(floor(dx * in/out), in-1) per axis, in double, with in/out formed the way cv2 forms it (the inverse
    of the double out/in).  cv2 is not installed where this was written, so the restatement is unpinned."""
    a = np.asarray(a)
    ys = np.minimum(np.floor(np.arange(out_h, dtype=np.float64) * (1.0 / (float(out_h) / a.shape[0]))), a.shape[0] - 1)
    xs = np.minimum(np.floor(np.arange(out_w, dtype=np.float64) * (1.0 / (float(out_w) / a.shape[1]))), a.shape[1] - 1)
    return a[ys.astype(np.int64)][:, xs.astype(np.int64)]


def roadmap_to_tensor(data):
    """functional.py:59-69 for a one-channel map: uint8 [H,W] -> float32 / 255; None stays None."""
    if data is None:
        return None
    return torch.from_numpy(np.array(data, dtype=np.uint8, copy=True)).float() / 255


def resize(data, scale_factor):
    """functional.py:72-82: (PIL image, integer annotations[, road map, ...]) -> PIL bilinear resize to
    (int(h*s), int(w*s)), the truncated annotations and the road map (uint8 [H,W] or None) resized nearest-neighbour."""
    from PIL import Image
    img, anno = data[0], data[1]
    out_h, out_w = scaled_size(img.size[1], img.size[0], scale_factor)
    img = img.resize((out_w, out_h), Image.BILINEAR)
    rest = tuple(data[2:])
    if rest and rest[0] is not None:
        rest = (nearest_resize(rest[0], out_h, out_w),) + rest[1:]
    return (img, resize_annos(anno, scale_factor)) + rest


def color_jitter(image, brightness, contrast, saturation):
    """functional.py:159-174 with the three factors as arguments (the reference draws them here; ColorJitter.__call__
    and the loader's sampler draw them): PIL's ImageEnhance.Brightness, Contrast and Color, in this order, on the uint8
    PIL image.  rr_jitter_gray_mean and the jittered tap reads of rr_augment_frames_jitter equal it bit for bit."""
    from PIL import ImageEnhance
    im = ImageEnhance.Brightness(image).enhance(brightness)
    im = ImageEnhance.Contrast(im).enhance(contrast)
    return ImageEnhance.Color(im).enhance(saturation)


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
    """functional.py:290-313: fill the ignore regions with `mean` (in place), zero the road map there (a tensor as
    third element, :308-309) and drop their rows.
    The reference selects the kept rows with `data[1][1 - ign_idx, :]`; torch refuses `1 - <bool tensor>` today, and
    on the uint8 masks it was written for the expression is the mask's negation, so it is restated as `~ign_idx`."""
    mean = torch.tensor(mean).unsqueeze(1).unsqueeze(1)
    img = data[0]
    ign_idx = data[1][:, 5] == ignore_cls
    for ign_bbox in data[1][ign_idx, :4]:
        x, y, w, h = ign_bbox[:4]
        img[:, int(y):int(y + h), int(x):int(x + w)] = mean
        if len(data) > 2 and data[2] is not None:
            data[2][int(y):int(y + h), int(x):int(x + w)] = 0
    return (img, data[1][~ign_idx, :]) + tuple(data[2:])


PASTE_WORDS = 12         # RR_PASTE_WORDS: int32 words of one row of a paste table


class TorchRand:
    """fill_duck's random source as the reference draws it: the global torch generator, so that under
    torch.manual_seed(s) the draws equal the reference's."""

    @staticmethod
    def integers(low, high, size):
        return torch.randint(low=low, high=high, size=(size,))


class GeneratorRand:
    """The same draws from a numpy Generator (the loader's sampler keys one per sample and attempt)."""

    def __init__(self, rng):
        self.rng = rng

    def integers(self, low, high, size):
        return torch.from_numpy(self.rng.integers(low, high, size=size, dtype=np.int64))


class PastePlan:
    """What fill_duck decided, without a pixel touched.
      pastes      int32 [k,12] rows (src_y, src_x, src_h, src_w, dst_y, dst_x, out_h, out_w, bits(rheight), bits(rwidth),
                  0, 0) in execution order; rheight = float32(src_h-1)/float32(out_h-1) (0 where out_h == 1), the scale
                  torch's align_corners=True kernel forms; rectangles are resolved slices inside the frame;
      new_annos   float32 [m,8] rows to append to the annotations (empty after an abort);
      aborted_at  -1, or the number of pastes executed before the reference's `except` returned the image as pasted so
                  far with the original annotations (== len(pastes));
      depth       the longest chain of pastes in which each reads pixels an earlier one wrote (0 without pastes)."""
    __slots__ = ("pastes", "new_annos", "aborted_at", "depth")

    def __init__(self):
        self.pastes = np.zeros((0, PASTE_WORDS), np.int32)
        self.new_annos = torch.zeros(0, 8)
        self.aborted_at, self.depth = -1, 0

    def key(self):
        return (self.pastes.tobytes(), self.new_annos.numpy().tobytes(), self.aborted_at, self.depth)


class _PasteAbort(Exception):
    pass


def interpolate_size(in_size, scale_factor):
    """The output size F.interpolate(..., scale_factor=f) gives one axis: the double product, truncated."""
    return int(math.floor(float(in_size) * float(scale_factor)))


def _plan_paste(rows, frame_h, frame_w, ys, xs, factor, paste_coor):
    """One `crop -> F.interpolate(scale_factor=float(factor)) -> slice assignment` of functional.py:438-452 / :486-501
    with Python's slice semantics and torch's failures but no pixels: appends the table row and leaves the clamped
    paste origin in `paste_coor` (float32 [2] = x, y, modified in place like the reference's) -> (obj_h, obj_w)."""
    y0, y1, _ = ys.indices(frame_h)
    x0, x1, _ = xs.indices(frame_w)
    sh, sw = max(y1 - y0, 0), max(x1 - x0, 0)
    if sh == 0 or sw == 0:
        raise _PasteAbort("empty crop: F.interpolate refuses it")
    obj_h, obj_w = interpolate_size(sh, factor), interpolate_size(sw, factor)
    if obj_h <= 0 or obj_w <= 0:
        raise _PasteAbort("empty output: F.interpolate refuses it")
    paste_coor[0] -= obj_w / 2
    paste_coor[1] -= obj_h / 2
    paste_coor[0] = paste_coor[0].clamp(min=1, max=frame_w - obj_w - 1)
    paste_coor[1] = paste_coor[1].clamp(min=1, max=frame_h - obj_h - 1)
    dy0, dy1, _ = slice(int(paste_coor[1]), int(paste_coor[1] + obj_h)).indices(frame_h)
    dx0, dx1, _ = slice(int(paste_coor[0]), int(paste_coor[0] + obj_w)).indices(frame_w)
    ly, lx = max(dy1 - dy0, 0), max(dx1 - dx0, 0)
    # the assignment broadcasts a size-1 axis of the object (onto an empty slice too) and raises on any other mismatch
    if not ((ly == obj_h or obj_h == 1) and (lx == obj_w or obj_w == 1)):
        raise _PasteAbort("destination slice and object differ in shape")
    if (ly, lx) == (obj_h, obj_w):
        rh = np.float32(sh - 1) / np.float32(obj_h - 1) if obj_h > 1 else np.float32(0)
        rw = np.float32(sw - 1) / np.float32(obj_w - 1) if obj_w > 1 else np.float32(0)
        rows.append((y0, x0, sh, sw, dy0, dx0, obj_h, obj_w, int(np.float32(rh).view(np.int32)),
                     int(np.float32(rw).view(np.int32)), 0, 0))
    elif ly and lx:
        raise _PasteAbort("broadcast paste")              # a 1-pixel object spread over a longer slice: cannot occur
    return obj_h, obj_w


def paste_depth(pastes, frame_h, frame_w):
    """The longest read-after-write chain of a paste table (per-pixel bookkeeping, so overwritten pixels do not count)."""
    if len(pastes) == 0:
        return 0
    level = np.zeros((frame_h, frame_w), np.int32)
    for sy, sx, sh, sw, dy, dx, oh, ow in np.asarray(pastes)[:, :8].tolist():
        level[dy:dy + oh, dx:dx + ow] = 1 + int(level[sy:sy + sh, sx:sx + sw].max())
    return int(level.max())


def fill_duck_decide(annos, roadmap, cls_list, factor, frame_h, frame_w, rand=TorchRand):
    """The reference's fill_duck (functional.py:356-523) with all pixel work removed -> PastePlan.  annos: the float
    [n,8] rows after MaskIgnore (not modified); roadmap: float [H,W].  Every number that reaches an annotation or a
    rectangle is computed by the reference's own torch expressions, in its order; the three draws (paste points, normal
    samples, relation samples) come from `rand.integers(low, high, size)` in the reference's order.  Whatever makes the
    reference raise ends the plan (`aborted_at`): its bare `except` returns the image as pasted so far with the
    original annotations."""
    from rrnet_amd.utils.metrics.metrics import bbox_iou
    plan, rows, new_annos = PastePlan(), [], []
    try:
        # I. Get valid area.
        valid_idx = roadmap.reshape(-1)
        idx = torch.nonzero(valid_idx).view(-1)
        if idx.size(0) == 0:
            return plan
        xs = idx % roadmap.size(1)
        ys = idx // roadmap.size(1)
        coor = torch.stack((xs, ys), dim=1)
        annos_cls = annos[:, 5]

        # II. Scale factor for depth.
        people_bbox = annos[annos_cls == 1, :4]
        if people_bbox.size(0) != 0:
            people_diag = people_bbox[:, 2:4].pow(2).sum(dim=1).sqrt()
            max_diag, max_idx = torch.topk(people_diag, k=min(3, people_diag.size(0)))
            min_diag, min_idx = torch.topk(people_diag, k=1, largest=False)
            y_diff = people_bbox[max_idx, 1] - people_bbox[min_idx, 1]
            scale_factor = ((max_diag - min_diag) / (y_diff.abs() + 1e-5)).mean()
        else:
            scale_factor = 1

        # III. Relation class.
        people_select_annos = annos[annos_cls == 2, :]
        relation_flag = torch.zeros_like(annos_cls).byte()
        people_idx = vechile_idx = None
        if people_select_annos.size(0) != 0:
            iou = bbox_iou(people_select_annos[:, :4], annos[:, :4], x1y1x2y2=False)
            if iou.size(1) > 2:
                max_v, max_i = torch.topk(iou, dim=1, k=2)
                max_i = max_i[max_v[:, 1] > 0, :]
                people_idx, vechile_idx = max_i[:, 0], max_i[:, 1]
                relation_flag[people_idx] = 1
                relation_flag[vechile_idx] = 1

        # IV. Aug N.
        cls = torch.as_tensor(cls_list).view(1, -1).repeat(annos.size(0), 1)
        normal_flag = (cls == annos_cls.unsqueeze(1).repeat(1, cls.size(1)).long()).sum(dim=1) > 0
        normal_flag = normal_flag * (1 - relation_flag)
        total_n = max(int(factor * valid_idx.sum()), 5)
        relation_n = relation_flag.float().sum() / 2
        normal_n = normal_flag.float().sum()
        if relation_n + normal_n == 0:
            return plan
        r_n = int(relation_n / (relation_n + normal_n) * total_n)
        n_n = total_n - r_n

        # V. Fill image.
        paste_coors = coor[rand.integers(0, coor.size(0), total_n)]
        if n_n != 0:
            normal_annos = annos[normal_flag.bool(), :]          # the reference indexes with the uint8 mask itself
            if normal_annos.size(0) == 0:
                raise _PasteAbort("torch.randint(0, 0)")
            sample_annos = normal_annos[rand.integers(0, normal_annos.size(0), n_n)]
            for i, anno in enumerate(sample_annos):
                paste_coor = paste_coors[i].float()
                anno_ct_y = anno[1] + anno[3] / 2
                diff = (anno_ct_y - paste_coor[1]).abs() * scale_factor
                anno_diag = (anno[2].pow(2) + anno[3].pow(2)).sqrt()
                if anno_ct_y > paste_coor[1]:
                    f = 1 - diff / anno_diag
                else:
                    f = 1 + diff / anno_diag
                f = f.clamp(min=0.5, max=2)
                obj_h, obj_w = _plan_paste(rows, frame_h, frame_w, slice(int(anno[1]), int(anno[1] + anno[3])),
                                           slice(int(anno[0]), int(anno[0] + anno[2])), f, paste_coor)
                new_annos.append(torch.tensor([[int(paste_coor[0]), int(paste_coor[1]), int(obj_w), int(obj_h),
                                                anno[4], anno[5], anno[6], anno[7]]]))
        if r_n != 0:
            people_annos = annos[people_idx, :]
            vechile_annos = annos[vechile_idx, :]
            if people_annos.size(0) == 0:
                raise _PasteAbort("torch.randint(0, 0)")
            sample_idx = rand.integers(0, people_annos.size(0), r_n)
            sample_people_annos = people_annos[sample_idx]
            sample_vechile_annos = vechile_annos[sample_idx]
            sample_people_annos[:, 2:4] += sample_people_annos[:, 0:2]
            sample_vechile_annos[:, 2:4] += sample_vechile_annos[:, 0:2]
            for i in range(r_n):
                paste_coor = paste_coors[i + n_n].float()
                people_anno = sample_people_annos[i]
                vechile_anno = sample_vechile_annos[i]
                min_x = int(min(people_anno[0], vechile_anno[0]))
                min_y = int(min(people_anno[1], vechile_anno[1]))
                max_x = int(max(people_anno[2], vechile_anno[2]))
                max_y = int(max(people_anno[3], vechile_anno[3]))
                anno_ct_y = (min_y + max_y) / 2
                diff = (anno_ct_y - paste_coor[1]).abs() * scale_factor
                anno_diag = math.sqrt((max_x - min_x) ** 2 + (max_y - min_y) ** 2)
                if anno_ct_y > paste_coor[1]:
                    f = 1 - diff / anno_diag
                else:
                    f = 1 + diff / anno_diag
                f = f.clamp(min=0.5, max=2)
                _plan_paste(rows, frame_h, frame_w, slice(min_y, max_y), slice(min_x, max_x), f, paste_coor)
                x_bias = min_x - paste_coor[0]
                y_bias = min_y - paste_coor[1]
                for new in (people_anno, vechile_anno):
                    new[2:4] -= new[0:2]
                    new[2:4] *= f
                    new[0] -= x_bias
                    new[1] -= y_bias
                    new_annos.append(new.unsqueeze(0).floor())
        plan.new_annos = torch.cat(new_annos)
    except Exception:                                             # the reference's bare `except`
        plan.aborted_at = len(rows)
    plan.pastes = np.asarray(rows, dtype=np.int32).reshape(-1, PASTE_WORDS)
    plan.depth = paste_depth(plan.pastes, frame_h, frame_w)
    return plan


def apply_paste_plan(img, plan):
    """The host pixel path of a plan on a float [3,H,W] frame, in place: per paste crop, F.interpolate(..., mode=
    'bilinear', align_corners=True) to (out_h, out_w) — with align_corners the kernel's scale is (in-1)/(out-1)
    whatever scale factor asked for that size — then slice assignment, in order.  torch's CPU kernel and the device
    kernel agree in every source index and differ by float32 rounding in the blend, so pasted pixels are held to
    E(depth) = depth * 9 * 2**-25 / min(std) + 2 * 2**-23 after Normalize instead of bit equality."""
    for sy, sx, sh, sw, dy, dx, oh, ow in plan.pastes[:, :8].tolist():
        obj = torch.nn.functional.interpolate(img[:, sy:sy + sh, sx:sx + sw].unsqueeze(0), size=(oh, ow),
                                              mode='bilinear', align_corners=True)[0]
        img[:, dy:dy + oh, dx:dx + ow] = obj
    return img


def fill_duck(data, cls_list, factor, rand=None):
    """functional.py:356-523 as decide + apply: (img [3,H,W], annos [n,8], roadmap [H,W]) -> (img, annos); the image is
    pasted into in place, like the reference's."""
    img, annos, roadmap = data
    plan = fill_duck_decide(annos, roadmap, cls_list, factor, img.size(1), img.size(2), rand or TorchRand)
    apply_paste_plan(img, plan)
    if plan.new_annos.size(0):
        annos = torch.cat((annos, plan.new_annos))
    return img, annos


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

"""Transform classes of the reference's datasets/transforms/transforms.py: the training chain of
configs/rrnet_config.py:40-49 (MultiScale, ToTensor, MaskIgnore, FillDuck, HorizontalFlip, RandomCrop, Normalize,
ToHeatmap) and ColorJitter (which no reference config uses), with the reference's constructor and call signatures, on
host tensors.  A sample is the tuple
(image, annotations[, road map, ...]); the road map (uint8 [H,W] or None, third element when the dataset loads one) is
resized by MultiScale, made a tensor by ToTensor, masked by MaskIgnore and consumed by FillDuck.  Two-element samples
pass through every class as before.

These classes are the host path.  DeviceAugmentLoader (rrnet_amd/datasets/augment.py) reads the chain's parameters
from the instances in `cfg.Train.transforms` and lowers everything that touches pixels to rr_augment_frames and
rr_augment_frames_pasted."""
import random

import numpy as np
import torch
from torch.nn.functional import interpolate, pad

from . import functional as F
from .functional import flip_annos, flip_img  # noqa: F401


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, data):
        for t in self.transforms:
            data = t(data)
        return data


class ToHeatmap:
    """datasets/transforms/transforms.py ToHeatmap: (img [3,H,W], annos [n,>=6]) -> (img, annos, hm, wh, ind, offset,
    reg_mask).  The targets are built by rr_ctnet_targets on the current device and returned as CPU tensors in the
    reference's shapes (a per-sample transform runs in the loader, before collation)."""

    def __init__(self, scale_factor=4, cls_num=10):
        self.scale_factor = scale_factor
        self.cls_num = cls_num

    def __call__(self, data):
        from rrnet_amd.datasets.synthetic import collate_ctnet_device
        img, annos = data[0], data[1]
        _, hm, wh, ind, off, mask = collate_ctnet_device([annos.float()], img.size(1), img.size(2), self.scale_factor,
                                                         self.cls_num)
        return (img, annos, hm[0].cpu().contiguous(), wh[0].cpu(), ind[0].cpu(), off[0].cpu(), mask[0].cpu())


class Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, data):
        img = data[0]
        mean = torch.tensor(self.mean, dtype=img.dtype).view(-1, 1, 1)
        std = torch.tensor(self.std, dtype=img.dtype).view(-1, 1, 1)
        return ((img - mean) / std,) + tuple(data[1:])


class MultiScale:
    """transforms.py:145-151: (PIL image, integer annotations[, ...]) resized by a factor drawn from `scale`."""

    def __init__(self, scale=(0.5, 0.75, 1, 1.25, 1.5)):
        self.scale = scale

    def __call__(self, data):
        rand_idx = random.randint(0, len(self.scale) - 1)
        return F.resize(data, self.scale[rand_idx])


class ToTensor:
    """transforms.py:27-29: PIL image -> float32 [3,H,W] in [0,1], annotations -> float32 tensor, road map (when the
    sample carries one) -> float32 [H,W] / 255 or None."""

    def __call__(self, data):
        out = F.img_to_tensor(data[0]), F.annos_to_tensor(data[1])
        return out + (F.roadmap_to_tensor(data[2]),) if len(data) > 2 else out


class ColorJitter:
    """transforms.py:120-130: brightness, contrast and saturation factors drawn with random.uniform (in this order,
    functional.py:168-170) from [max(1 - x, 0), 1 + x], applied to the PIL image by PIL's ImageEnhance."""

    def __init__(self, brightness=0.5, contrast=0.5, saturation=0.5):
        self.brightness = [max(1 - brightness, 0), 1 + brightness]
        self.contrast = [max(1 - contrast, 0), 1 + contrast]
        self.saturation = [max(1 - saturation, 0), 1 + saturation]

    def __call__(self, data):
        from PIL import Image
        assert isinstance(data[0], Image.Image)
        b, c, s = (random.uniform(*r) for r in (self.brightness, self.contrast, self.saturation))
        return (F.color_jitter(data[0], b, c, s),) + tuple(data[1:])


class MaskIgnore:
    """transforms.py:133-142: ignore regions (class `ignore_idx`) are filled with `mean` and their rows dropped."""

    def __init__(self, mean=(0.485, 0.456, 0.406), ignore_idx=0):
        self.mean = mean
        self.ignore_idx = ignore_idx

    def __call__(self, data):
        assert isinstance(data[0], torch.Tensor) and isinstance(data[1], torch.Tensor)
        return F.mask_ignore(data, self.mean, self.ignore_idx)


class FillDuck:
    """transforms.py:173-179, the paper's adaptive resampling: copies objects of `cls_list`, rescales them by a depth
    heuristic and pastes them onto road pixels.  (img, annos, road map) -> (img, annos); without a road map (None, or
    a two-element sample) the data comes back unchanged, as in the reference, whose `except` swallows the failure."""

    def __init__(self, cls_list=(1, 2, 3, 7, 8, 10), factor=0.00005):
        self.cls_list = torch.tensor(cls_list).unsqueeze(0)
        self.factor = factor

    def __call__(self, data):
        if len(data) < 3 or data[2] is None:
            return data[0], data[1]
        return F.fill_duck(data[:3], self.cls_list, self.factor)


class HorizontalFlip:
    """transforms.py:14-24: flips when random.random() <= p."""

    def __init__(self, p=0.5):
        self.p = p

    def __call__(self, data):
        assert isinstance(data[0], torch.Tensor)
        if random.random() > self.p:
            return data
        w = data[0].size(2)
        return (F.flip_img(data[0]), F.flip_annos(data[1], w)) + tuple(data[2:])


class _ReferenceRandom:
    """The random sources RandomCrop uses in the reference: random.random() and numpy's global integer draw."""

    @staticmethod
    def random():
        return random.random()

    @staticmethod
    def integers(low, high):
        return int(np.random.randint(low, high))


class RandomCrop:
    """transforms.py:42-117.  The decision logic works on annotations alone (`decide`), so that the loader's sampler
    can run it without pixels; `__call__` is the reference's per-sample transform on a host tensor.

    Restated lines: `1 - <bool tensor>` (transforms.py:78) is the mask's negation on the uint8 masks it was written
    for and is refused by torch today, so it reads `~mask`.  A zero-area box gives 0/0 in bbox_iou(..., overlap=True);
    NaN fails `> keep_iou` and the box is dropped, as in the reference."""

    def __init__(self, size, keep_iou=0.5):
        self.h, self.w = size
        self.keep_iou = keep_iou

    def _coor(self, h, w, rand):
        rx, ry = rand.random() * (w - self.w), rand.random() * (h - self.h)
        return int(rx), int(ry), int(rx) + self.w, int(ry) + self.h

    def generate_coor(self, img):
        h, w = img.size()[-2:]
        return self._coor(h, w, _ReferenceRandom)

    def remove_bbox_outside(self, annos, xywh):
        from rrnet_amd.utils.metrics.metrics import bbox_iou
        _, overlap = bbox_iou(annos, xywh, x1y1x2y2=False, overlap=True)
        keep_flag = overlap[:, 0] > self.keep_iou
        return annos[keep_flag, :].view(-1, 8)

    def _place(self, annos_wo_large, h, w, crop_coordinate, rand):
        """transforms.py:92-110 for a padded frame of h x w -> (crop_coordinate, cropped annotations)."""
        annos = self.remove_bbox_outside(annos_wo_large,
                                         torch.tensor([[crop_coordinate[0], crop_coordinate[1], self.w, self.h]]))
        if annos.size(0) == 0:
            include_bbox = annos_wo_large[rand.integers(0, annos_wo_large.size(0)), :]
            x1, y1 = int(include_bbox[0]), int(include_bbox[1])
            x2, y2 = int(include_bbox[0] + include_bbox[2]), int(include_bbox[1] + include_bbox[3])
            min_x1, max_x1 = sorted([min(x1, w - self.w), max(0, int(x2 - self.w))])
            min_y1, max_y1 = sorted([min(y1, h - self.h), max(0, int(y2 - self.h))])
            x1 = rand.integers(min_x1, max_x1) if min_x1 != max_x1 else min_x1
            y1 = rand.integers(min_y1, max_y1) if min_y1 != max_y1 else min_y1
            crop_coordinate = (int(x1), int(y1), int(x1) + self.w, int(y1) + self.h)
            annos = self.remove_bbox_outside(annos_wo_large, torch.tensor([[x1, y1, self.w, self.h]]))
        return crop_coordinate, F.crop_annos(annos, crop_coordinate, self.h, self.w)

    def decide(self, annos, h, w, rand=_ReferenceRandom):
        """The annotation half of one pass of transforms.py:64-110 for an (unpadded) frame of h x w:
        -> (crop_coordinate, annotations) with the origin in the padded frame, or None where no box fits the crop
        (the reference's rescale branch, transforms.py:81-90).  The input is not modified."""
        if (self.w, self.h) == (w, h) or (self.w > w and self.h > h):
            return (0, 0, self.w, self.h), annos
        h, w = max(h, self.h), max(w, self.w)
        crop_coordinate = self._coor(h, w, rand)
        annos = annos.clone()
        remove_large_flag = ~(((annos[:, 2] > self.w) | (annos[:, 3] > self.h)))
        annos_wo_large = annos[remove_large_flag, :]
        if annos_wo_large.size(0) == 0:
            return None
        return self._place(annos_wo_large, h, w, crop_coordinate, rand)

    def __call__(self, data):
        assert isinstance(data[0], torch.Tensor)
        assert isinstance(data[1], torch.Tensor)
        rest = tuple(data[2:])
        for _ in range(50):
            img = data[0]
            h, w = img.size()[-2:]
            if (self.w, self.h) == (w, h):
                return data
            if self.w > w or self.h > h:
                img = pad(img, [0, max(self.w - w, 0), 0, max(self.h - h, 0)])
                if self.w > w and self.h > h:
                    return (img, data[1]) + rest
            decision = self.decide(data[1], h, w)
            if decision is None:
                # Means that current scale size is invalid (transforms.py:81-90; h and w stay those of the frame
                # before the rescale, as in the reference).
                h, w = img.size()[-2:]
                scale_factor = self.w / min(h, w)
                img = interpolate(img.unsqueeze(0), scale_factor=scale_factor, mode='bilinear',
                                  align_corners=True).squeeze(0)
                annos_wo_large = data[1].clone()
                annos_wo_large[:, :4] = annos_wo_large[:, :4] * scale_factor
                decision = self._place(annos_wo_large, h, w, self.generate_coor(img), _ReferenceRandom)
            crop_coordinate, cropped_annos = decision
            cropped_img = F.crop_tensor(img, crop_coordinate)
            if cropped_img.size(1) == self.h and cropped_img.size(2) == self.w:
                return (cropped_img, cropped_annos) + rest
        print("Fake image")
        return (torch.randn(3, self.h, self.w), torch.tensor([[0., 0, 1, 1, 1, 1, 1, 1]])) + rest

"""modules/anchor.py of the reference: the anchor boxes of a RetinaNet pyramid, on the host in numpy (float64 arithmetic,
one rounding to float32 at the end, as there), cached per image size.

Per pyramid level p (stride 2^p unless given): 9 base boxes centred on the origin, aspect ratios (0.5, 1, 2) major, scales
(1, 2^(1/3), 2^(2/3)) minor, each of area (size * scale)^2, shifted to the centre (i + 0.5) * stride of every cell of the
ceil(image / 2^p) map, cells row-major, the 9 boxes of a cell adjacent.  Rows are (x1, y1, x2, y2)."""
import numpy as np
import torch
import torch.nn as nn


def generate_anchors(base_size=16, ratios=None, scales=None):
    ratios = np.array([0.5, 1, 2]) if ratios is None else np.asarray(ratios)
    scales = np.array([2 ** 0, 2 ** (1.0 / 3.0), 2 ** (2.0 / 3.0)]) if scales is None else np.asarray(scales)
    ratio_of = np.repeat(ratios, len(scales))
    side = base_size * np.tile(scales, len(ratios))
    areas = side * side
    widths = np.sqrt(areas / ratio_of)
    heights = widths * ratio_of
    boxes = np.zeros((len(ratio_of), 4))
    boxes[:, 2] = widths
    boxes[:, 3] = heights
    boxes[:, 0::2] -= (widths * 0.5)[:, None]
    boxes[:, 1::2] -= (heights * 0.5)[:, None]
    return boxes


def shift(shape, stride, anchors):
    cx = (np.arange(0, shape[1]) + 0.5) * stride
    cy = (np.arange(0, shape[0]) + 0.5) * stride
    gx, gy = np.meshgrid(cx, cy)
    centres = np.stack((gx.ravel(), gy.ravel(), gx.ravel(), gy.ravel()), axis=1)
    return (centres[:, None, :] + anchors[None, :, :]).reshape(-1, 4)


class Anchors(nn.Module):
    def __init__(self, pyramid_levels=None, strides=None, sizes=None, ratios=None, scales=None):
        super().__init__()
        self.pyramid_levels = [3, 4, 5] if pyramid_levels is None else pyramid_levels
        self.strides = [2 ** x for x in self.pyramid_levels] if strides is None else strides
        self.sizes = [2 ** (x + 2) for x in self.pyramid_levels] if sizes is None else sizes
        self.ratios = np.array([0.5, 1, 2]) if ratios is None else ratios
        self.scales = np.array([2 ** 0, 2 ** (1.0 / 3.0), 2 ** (2.0 / 3.0)]) if scales is None else scales
        self._cache = {}

    def forward(self, image_shape):
        """image_shape (h, w) -> float32 tensor [anchors, 4], finest level first."""
        key = (int(image_shape[0]), int(image_shape[1]))
        hit = self._cache.get(key)
        if hit is None:
            hw = np.array(key)
            levels = []
            for i, p in enumerate(self.pyramid_levels):
                cells = (hw + 2 ** p - 1) // (2 ** p)
                base = generate_anchors(base_size=self.sizes[i], ratios=self.ratios, scales=self.scales)
                levels.append(shift(cells, self.strides[i], base))
            hit = torch.from_numpy(np.concatenate(levels, axis=0).astype(np.float32))
            self._cache[key] = hit
        return hit.clone()

"""Shared by tests/test_jitter_host.py and tests/test_jitter_gpu.py: a float32 / integer restatement of what PIL's
ImageEnhance.Brightness, Contrast and Color compute (the formulas rr_jitter_gray_mean and the jittered tap reads
implement), the recorded reference cases (tests/golden/jitter.npz, tools/gen_golden_jitter.py), the factor triples and
the frames of the grey-mean batch."""
import functools
import os

import numpy as np

import augment_cases as C
from rrnet_amd.datasets import augment as A

# (brightness, contrast, saturation): identity; the lower and the upper end of the default ranges (the upper one reaches
# all three clip branches); an uneven triple with saturation 0 (grey); contrast 0 (every pixel becomes m); brightness 0
TRIPLES = ((1, 1, 1), (0.5, 0.5, 0.5), (1.5, 1.5, 1.5), (0.73, 1.41, 0), (1, 0, 1), (0, 1, 1))


def gray(rgb):
    """PIL's RGB -> L (Convert.c): (r*19595 + g*38470 + b*7471 + 0x8000) >> 16 on integer [...,3] -> [...]."""
    rgb = np.asarray(rgb).astype(np.int64)
    return (rgb[..., 0] * 19595 + rgb[..., 1] * 38470 + rgb[..., 2] * 7471 + 0x8000) >> 16


def blend(d, v, alpha):
    """Image.blend(degenerate, image, alpha) (Blend.c) in float32: one multiply, one add, clip, truncate."""
    d, v = np.asarray(d).astype(np.int64), np.asarray(v).astype(np.int64)
    prod = (np.float32(alpha) * (v - d).astype(np.float32)).astype(np.float32)
    t = (d.astype(np.float32) + prod).astype(np.float32)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(np.clip(t, 0, 255)))).astype(np.int64)


def brightness(img, b):
    return blend(np.zeros_like(img, dtype=np.int64), img, b)


def gray_sum(img, b):
    """The integer sum of L over the brightness-adjusted frame."""
    return int(gray(brightness(img, b)).sum())


def int_mean(total, n):
    """int(total / n + 0.5) in integers."""
    return (2 * int(total) + int(n)) // (2 * int(n))


def gray_mean(img, b):
    return int_mean(gray_sum(img, b), img.shape[0] * img.shape[1])


def jitter(img, b, c, s):
    """uint8 [h,w,3] -> uint8 [h,w,3]: brightness, contrast with the whole frame's grey mean, colour with each pixel's
    own L."""
    x = brightness(img, b)
    m = int_mean(gray(x).sum(), x.shape[0] * x.shape[1])
    x = blend(np.full_like(x, m), x, c)
    x = blend(gray(x)[..., None].repeat(3, -1), x, s)
    return x.astype(np.uint8)


def pil_jitter(img, b, c, s):
    from PIL import Image
    from rrnet_amd.datasets.transforms import functional as F
    return np.asarray(F.color_jitter(Image.fromarray(img), b, c, s), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(C.GOLDEN, "jitter.npz")))


def random_frame(rng, h, w):
    """Plain noise, a dark frame or a nearly saturated one."""
    kind = int(rng.integers(0, 3))
    lo, hi = ((0, 256), (0, 40), (215, 256))[kind]
    return rng.integers(lo, hi, (h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def mean_batch():
    """The frames of the grey-mean test, packed back to back in this order so that their byte offsets take many residues
    mod 16 -> [(name, uint8 [h,w,3], brightness)]."""
    rng = np.random.default_rng(20260)
    halves = np.zeros((1, 2, 3), np.uint8)
    halves[0, 0], halves[0, 1] = 10, 11                  # L = 10 and 11: the mean is 10.5 exactly -> 11
    noise = lambda h, w: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    frames = [("1x1", noise(1, 1), 0.8),
              ("halves", halves, 1.0),
              ("3x5", noise(3, 5), 1.3),
              ("17x31", noise(17, 31), 0.61),
              ("64x64", noise(64, 64), 1.5),
              ("cut", C.source("demo_cut")[0], 1.17),
              ("257x513", noise(257, 513), 0.93),          # many workgroups and a ragged tail
              ("white", np.full((9, 7, 3), 255, np.uint8), 1.5),
              ("black_by_factor", noise(23, 11), 0.0),
              ("identity", noise(33, 45), 1.0)]
    assert gray(halves).tolist() == [[10, 11]]
    return frames


def whole_item(img, d):
    """What a loader thread hands to pack_batch for a jittered sample: the whole frame."""
    h, w = img.shape[:2]
    taps_rows = (0, 0)
    return d, h, w, (0, 0, h, w) + taps_rows, np.ascontiguousarray(img)


def plain_records(frames):
    """[(name, frame, brightness)] -> pack_batch output for whole frames at scale 1 (the records the reduction reads) and
    the factors [B,3]."""
    items = []
    for _, img, _ in frames:
        d = C.decision(img, np.zeros((0, 8), np.int64), 1, 0, img.shape[:2], "zero")
        items.append(whole_item(img, d))
    factors = np.ones((len(frames), 3), np.float32)
    factors[:, 0] = [f[2] for f in frames]
    return A.pack_batch(items), factors


def jittered_decision(img, annos, factors, scale, flip, crop, origin):
    d = C.decision(img, annos, scale, flip, crop, origin)
    d.jitter = tuple(float(np.float32(f)) for f in factors)
    return d


def item_of(img, d, crop, taps):
    """A jittered sample ships its whole frame; the tap table rows are those of its crop."""
    h, w = img.shape[:2]
    return d, h, w, (0, 0, h, w) + A.source_window(d, h, w, crop[0], crop[1], taps)[4:], np.ascontiguousarray(img)


@functools.lru_cache(maxsize=None)
def host_reference(src_name, factors, scale, flip, crop, origin):
    """The host chain with PIL's ImageEnhance in front -> float32 [h,w,3]."""
    from PIL import Image
    img, annos = C.source(src_name)
    d = jittered_decision(img, annos, factors, scale, flip, crop, origin)
    ref = A.host_chain(Image.fromarray(img), annos, d, C.PARAMS, crop[0], crop[1])
    return ref.permute(1, 2, 0).contiguous().numpy()


def chain(crop, fill_duck=False, amounts=(0.5, 0.5, 0.5)):
    from rrnet_amd.datasets.transforms import (ColorJitter, Compose, FillDuck, HorizontalFlip, MaskIgnore, MultiScale,
                                               Normalize, RandomCrop, ToHeatmap, ToTensor)
    ts = [ColorJitter(*amounts), MultiScale(scale=(1, 1.15, 1.25, 1.35, 1.5)), ToTensor(), MaskIgnore(C.MEAN),
          HorizontalFlip(), RandomCrop(crop), Normalize(C.MEAN, C.STD), ToHeatmap(scale_factor=4)]
    if fill_duck:
        ts.insert(4, FillDuck(factor=2e-4))
    return Compose(ts)

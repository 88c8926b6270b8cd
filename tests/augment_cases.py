"""Shared by tests/test_augment_host.py and tests/test_augment_gpu.py: the case grid of rr_augment_frames, the host
reference of every case (computed once per process and cached), and a numpy restatement of the kernel's index
arithmetic that lets the CPU suite check the packed records without a GPU."""
import functools
import os

import numpy as np
import torch

from rrnet_amd.datasets import augment as A
from rrnet_amd.datasets.transforms import functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEMO_ROOT = os.path.join(GOLDEN, "visdrone_demo")
DEMO_NAME = "0000364_01765_d_0000782"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PARAMS = dict(scales=(1, 1.15, 1.5), flip_p=0.5, crop=None, keep_iou=0.5, mean=MEAN, std=STD, ignore_idx=0,
              ignore_mean=MEAN, scale_factor=4, cls_num=10)

SOURCES = ("noise_97x61", "noise_160x90", "noise_64x200", "demo_cut")     # width x height
SCALES = (1, 1.15, 1.5)
CROPS = ((64, 64), (96, 128), (50, 62))                                   # (h, w): 64x64, 128x96, 62x50 as w x h
ORIGINS = ("zero", "interior", "flush")


@functools.lru_cache(maxsize=None)
def source(name):
    """-> (uint8 [h,w,3], int64 annotations [n,8]).  Ignore regions: one crossing the right edge of the frame (and of
    most crops), one in the middle (crosses interior crop edges), one with zero width (empty after truncation) and one
    near the left edge (it moves under the flip)."""
    if name == "demo_cut":
        img = np.load(os.path.join(GOLDEN, "augment.npz"))["cut"]
    else:
        w, h = (int(v) for v in name.split("_")[1].split("x"))
        img = np.random.default_rng([219, w, h]).integers(0, 256, (h, w, 3), dtype=np.uint8)
    h, w = img.shape[:2]
    annos = np.array([[w // 4, h // 4, 10, 10, 1, 4, 0, 0],
                      [w - 20, h // 3, 40, 15, 0, 0, 0, 0],
                      [w // 2 - 8, h // 2 - 6, 30, 20, 0, 0, 0, 0],
                      [10, 10, 0, 7, 0, 0, 0, 0],
                      [5, 5, 12, 9, 0, 0, 0, 0]], dtype=np.int64)
    return img, annos


def decision(img, annos, scale, flip, crop, origin):
    """A Decision built by hand (the sampler is tested on its own): origin in the scaled, flipped, padded frame."""
    h, w = img.shape[:2]
    d = A.Decision()
    d.index, d.redraws, d.scale, d.flip = 0, 0, scale, bool(flip)
    d.dst_h, d.dst_w = F.scaled_size(h, w, scale)
    ph, pw = max(d.dst_h, crop[0]), max(d.dst_w, crop[1])
    room_y, room_x = ph - crop[0], pw - crop[1]
    interior_x = min((room_x // 2) | 1, room_x)                # odd where there is room: no vector-width luck
    d.crop_y0, d.crop_x0 = {"zero": (0, 0), "interior": (room_y // 3, interior_x), "flush": (room_y, room_x)}[origin]
    a = F.resize_annos(annos.copy(), scale)
    d.rects = F.ignore_rects(a, d.dst_h, d.dst_w, 0)
    d.annos = F.annos_to_tensor(a)
    return d


def item_of(img, d, crop, taps):
    """What a loader thread hands to pack_batch: only the window of the source the crop reads."""
    h, w = img.shape[:2]
    win = A.source_window(d, h, w, crop[0], crop[1], taps)
    y0, x0, wh, ww = win[:4]
    return d, h, w, win, np.ascontiguousarray(img[y0:y0 + wh, x0:x0 + ww])


@functools.lru_cache(maxsize=None)
def host_reference(src_name, scale, flip, crop, origin):
    """The host chain (PIL resize -> to_tensor -> mask_ignore -> flip -> pad/crop -> normalize) -> float32 [h,w,3]."""
    from PIL import Image
    img, annos = source(src_name)
    d = decision(img, annos, scale, flip, crop, origin)
    ref = A.host_chain(Image.fromarray(img), annos, d, PARAMS, crop[0], crop[1])
    return ref.permute(1, 2, 0).contiguous().numpy()


def grid(src_name, crop):
    return [(src_name, s, f, crop, o) for s in SCALES for f in (0, 1) for o in ORIGINS]


MIXED = [("noise_97x61", 1.5, 1, "interior"), ("demo_cut", 1.15, 0, "flush"), ("noise_64x200", 1, 1, "zero"),
         ("noise_160x90", 1.5, 0, "flush"), ("noise_97x61", 1, 0, "zero")]


def packed(cases, taps):
    """cases: [(source, scale, flip, crop, origin)] of ONE crop size -> pack_batch output + the references [B,h,w,3]."""
    items, refs = [], []
    for c in cases:
        img, annos = source(c[0])
        items.append(item_of(img, decision(img, annos, *c[1:]), c[3], taps))
        refs.append(host_reference(*c))
    return A.pack_batch(items), np.stack(refs)


def kernel_model(src, params, rects, rect_off, taps, mean, std, out_h, out_w):
    """The kernel's arithmetic in numpy (same records, same order of decisions, same clamps)."""
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    lut = ((np.arange(256, dtype=np.float32) / np.float32(255))[:, None] - mean[None]) / std[None]
    half = 1 << 21
    out = np.empty((len(params), out_h, out_w, 3), np.float32)
    for b, P in enumerate(params.astype(np.int64)):
        oy, ox = np.mgrid[0:out_h, 0:out_w]
        sy, sxp = P[9] + oy, P[10] + ox
        pad = (sy >= P[6]) | (sxp >= P[7])
        sx = P[7] - 1 - sxp if P[8] else sxp
        ign = np.zeros_like(pad)
        for y0, y1, x0, x1 in rects[rect_off[b]:rect_off[b + 1]]:
            ign |= (sy >= y0) & (sy < y1) & (sx >= x0) & (sx < x1)
        ty = taps[np.clip(P[13] + sy, 0, len(taps) - 1)].astype(np.int64)
        tx = taps[np.clip(P[14] + sx, 0, len(taps) - 1)].astype(np.int64)
        y0, y1 = np.clip(ty[..., 0] - P[2], 0, P[4] - 1), np.clip(ty[..., 0] + 1 - P[2], 0, P[4] - 1)
        x0, x1 = np.clip(tx[..., 0] - P[3], 0, P[5] - 1), np.clip(tx[..., 0] + 1 - P[3], 0, P[5] - 1)
        off = int(P[11] & 0xffffffff) | (int(P[12]) << 32)
        win = src[off:off + P[4] * P[5] * 3].reshape(P[4], P[5], 3).astype(np.int64)
        kx0, kx1, ky0, ky1 = tx[..., 1:2], tx[..., 2:3], ty[..., 1:2], ty[..., 2:3]
        h0 = np.clip((win[y0, x0] * kx0 + win[y0, x1] * kx1 + half) >> 22, 0, 255)
        h1 = np.clip((win[y1, x0] * kx0 + win[y1, x1] * kx1 + half) >> 22, 0, 255)
        v = np.clip((h0 * ky0 + h1 * ky1 + half) >> 22, 0, 255)
        val = lut[v, np.arange(3)[None, None]]
        out[b] = np.where(pad[..., None], lut[0][None, None], np.where(ign[..., None], np.float32(0), val))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def write_dataset(root, splits=("train",), extra=3, size=(200, 150)):
    """A temporary VisDrone-shaped directory: the demo frame plus `extra` seeded JPEGs written by PIL, each with
    boxes and one ignore region, under every split of `splits`."""
    import shutil
    from PIL import Image
    for split in splits:
        os.makedirs(os.path.join(root, split, "images"), exist_ok=True)
        os.makedirs(os.path.join(root, split, "annotations"), exist_ok=True)
        shutil.copy(os.path.join(DEMO_ROOT, "images", DEMO_NAME + ".jpg"), os.path.join(root, split, "images"))
        shutil.copy(os.path.join(DEMO_ROOT, "annotations", DEMO_NAME + ".txt"), os.path.join(root, split, "annotations"))
        for i in range(extra):
            w, h = size[0] + 37 * i, size[1] + 21 * i
            rng = np.random.default_rng([7, i])
            coarse = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
            img = Image.fromarray(coarse).resize((w, h), Image.BICUBIC)
            img.save(os.path.join(root, split, "images", "synth_%02d.jpg" % i), quality=90)
            rows = []
            for _ in range(6):
                bw, bh = int(rng.integers(8, 40)), int(rng.integers(8, 40))
                rows.append((int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh)), bw, bh, 1, int(rng.integers(1, 11)), 0, 0))
            rows.append((w // 3, h // 3, 30, 20, 0, 0, 0, 0))
            rows.append((3, 3, 9, 9, 1, 11, 0, 0))
            with open(os.path.join(root, split, "annotations", "synth_%02d.txt" % i), "w") as f:
                f.write("".join(",".join(str(v) for v in r) + "\n" for r in rows))
    return root

"""Generates tests/golden/augment.npz by IMPORTING THE REFERENCE (build container only; tools/ref_shims.py is the import
recipe).  Data only: a stored uint8 input cut, the decisions, and what the reference's own functions return for them.

Recorded reference functions (the ones that run on this image's torch):
  datasets/transforms/functional.py  resize (:72-82, PIL bilinear + the integer write-back of the annotations),
                                     flip_img, flip_annos (:13-29), crop_tensor, crop_annos (:104-132)
  datasets/transforms/transforms.py  RandomCrop.remove_bbox_outside (:53-58)
  utils/metrics/metrics.py           bbox_iou(..., overlap=True) (:10-48)
torchvision is not installed here, so `to_tensor` / `normalize` are the stand-ins below (uint8.float().div(255) and
sub(mean).div(std), what torchvision 0.3 computes); `mask_ignore` and RandomCrop.__call__ contain `1 - <bool tensor>`,
which today's torch refuses, so they are not recorded — the fill is written out below with the reference's own slice
expression (functional.py:305-307).

The input pixels are stored in the file: a golden comparison must not depend on a JPEG decoder."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

ref_shims.install()

import torch  # noqa: E402
from PIL import Image  # noqa: E402

from datasets.transforms import functional as RF  # noqa: E402  (reference)
from datasets.transforms.transforms import RandomCrop  # noqa: E402  (reference)
from utils.metrics.metrics import bbox_iou  # noqa: E402  (reference)

GOLD = os.path.join(ROOT, "tests", "golden")
DEMO = os.path.join(GOLD, "visdrone_demo")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CUT = (300, 400, 160, 90)               # x, y, w, h of the stored cut of the demo frame
CROP = (96, 128)                        # h, w
# (scale, flip, crop x0, crop y0)
CASES = [(1, 0, 0, 0), (1.15, 1, 17, 3), (1.25, 0, 72, 16), (1.35, 1, 88, 25), (1.5, 0, 112, 39), (1.5, 1, 5, 30)]


def to_tensor(img):
    return torch.from_numpy(np.array(img, dtype=np.uint8)).permute(2, 0, 1).contiguous().float().div(255)


def normalize(t):
    return t.sub(torch.tensor(MEAN).view(3, 1, 1)).div(torch.tensor(STD).view(3, 1, 1))


def main():
    name = sorted(os.listdir(os.path.join(DEMO, "images")))[0][:-4]
    frame = np.array(Image.open(os.path.join(DEMO, "images", name + ".jpg")).convert("RGB"))
    x, y, w, h = CUT
    cut = np.ascontiguousarray(frame[y:y + h, x:x + w])
    rows = [[int(v) for v in l.strip().split(',')[:8]] for l in open(os.path.join(DEMO, "annotations", name + ".txt"))]
    annos = np.array(rows, dtype=np.int64)
    # the boxes that touch the cut, moved to its origin; plus two ignore regions (one crossing the right edge) and a
    # zero-area box, which the demo cut does not have
    a = annos.copy()
    a[:, 0] -= x
    a[:, 1] -= y
    inside = (a[:, 0] + a[:, 2] > 0) & (a[:, 1] + a[:, 3] > 0) & (a[:, 0] < w) & (a[:, 1] < h) & (a[:, 5] != 0)
    a = np.concatenate([a[inside], np.array([[20, 10, 31, 17, 0, 0, 0, 0], [140, 60, 40, 50, 0, 0, 0, 0],
                                             [50, 40, 0, 9, 1, 4, 0, 0]])]).astype(np.int64)
    out = {"cut": cut, "annos": a, "cases": np.array(CASES, dtype=np.float64), "crop": np.array(CROP),
           "mean": np.array(MEAN), "std": np.array(STD)}
    rc = RandomCrop(CROP)
    for i, (s, flip, cx, cy) in enumerate(CASES):
        img, an, _ = RF.resize((Image.fromarray(cut), a.copy(), None), s)
        out["resized_%d" % i] = np.array(img)
        out["resized_annos_%d" % i] = an.copy()
        t, ta = to_tensor(img), torch.tensor(an).float()
        ign = ta[:, 5] == 0
        for bx, by, bw, bh in ta[ign, :4]:
            t[:, int(by):int(by + bh), int(bx):int(bx + bw)] = torch.tensor(MEAN).view(3, 1, 1)
        ta = ta[~ign]
        if flip:
            t, ta = RF.flip_img(t), RF.flip_annos(ta, t.size(2))
        out["flipped_annos_%d" % i] = ta.numpy().copy()
        coor = (cx, cy, cx + CROP[1], cy + CROP[0])
        win = torch.tensor([[cx, cy, CROP[1], CROP[0]]])
        _, ov = bbox_iou(ta, win, x1y1x2y2=False, overlap=True)
        out["overlap_%d" % i] = ov.numpy()
        kept = rc.remove_bbox_outside(ta.clone(), win)
        out["kept_%d" % i] = kept.numpy().copy()
        out["cropped_annos_%d" % i] = RF.crop_annos(kept.clone(), coor, CROP[0], CROP[1]).numpy()
        th, tw = t.shape[-2:]
        t = torch.nn.functional.pad(t, [0, max(CROP[1] - tw, 0), 0, max(CROP[0] - th, 0)])
        out["pixels_%d" % i] = normalize(RF.crop_tensor(t, coor)).numpy()
    path = os.path.join(GOLD, "augment.npz")
    np.savez_compressed(path, **out)
    print("wrote %s %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()

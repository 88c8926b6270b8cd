"""Generates tests/golden/fillduck.npz by IMPORTING THE REFERENCE (build container only; tools/ref_shims.py is the import
recipe).  Data only: per case the stored uint8 input frame, the road map, the annotations, `factor` and the torch seed,
and what the reference's own fill_duck (datasets/transforms/functional.py:356-523) returns for them under
torch.manual_seed(seed): the output annotations and the CHANGED pixels of the float frame as flat indices into
[3,H,W] plus their float32 values (whole output frames are not stored).

Cases (frames of at most 96 x 128):
  base     factor 5e-5, 7 boxes: total_n = 5, single objects and person/vehicle pairs
  dense    factor 2e-3 on the same frame
  nodepth  no class-1 box: the depth scale is the integer 1
  two      two boxes: the relation search is skipped (iou.size(1) > 2 fails)
  noroad   an empty road map: data unchanged
  nocls    no eligible class: data unchanged
  abort    a box almost as large as the frame pasted far below its centre: the resized object does not fit, the
           slice assignment raises, and the reference returns the frame as pasted so far with the ORIGINAL rows
The input pixels are stored in the file: a golden comparison must not depend on a JPEG decoder."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

ref_shims.install()

import torch  # noqa: E402
from PIL import Image  # noqa: E402

from datasets.transforms import functional as RF  # noqa: E402  (reference)

GOLD = os.path.join(ROOT, "tests", "golden")
CLS_LIST = (1, 2, 3, 7, 8, 10)


def frame(h, w, tag):
    rng = np.random.default_rng([219, tag])
    coarse = rng.integers(0, 256, (h // 6 + 1, w // 6 + 1, 3), dtype=np.uint8)
    return np.array(Image.fromarray(coarse).resize((w, h), Image.BICUBIC))


def band(h, w, y0, y1):
    r = np.zeros((h, w), np.uint8)
    r[y0:y1] = 255
    return r


BASE = [[10, 8, 5, 9, 1, 1, 0, 0], [70, 60, 9, 17, 1, 1, 0, 0], [30, 40, 8, 14, 1, 2, 0, 0], [28, 46, 14, 10, 1, 10, 0, 0],
        [90, 20, 20, 12, 1, 4, 0, 0], [50, 70, 12, 9, 1, 3, 0, 0], [100, 50, 1, 6, 1, 7, 0, 0]]

# name -> (h, w, road map, annotations, factor, seed)
CASES = {
    "base": (96, 128, band(96, 128, 48, 96), BASE, 5e-5, 5),
    "dense": (96, 128, band(96, 128, 48, 96), BASE, 2e-3, 5),
    "nodepth": (96, 128, band(96, 128, 40, 90), [r for r in BASE if r[5] != 1], 5e-5, 1),
    "two": (80, 100, band(80, 100, 30, 80), [BASE[2], [28, 46, 14, 10, 1, 10, 0, 0]], 5e-5, 4),
    "noroad": (64, 64, band(64, 64, 0, 0), BASE[:3], 5e-5, 0),
    "nocls": (64, 64, band(64, 64, 20, 60), [[10, 10, 20, 12, 1, 4, 0, 0], [30, 30, 9, 9, 1, 5, 0, 0]], 5e-5, 0),
    "abort": (64, 96, band(64, 96, 2, 64), [[4, 4, 80, 30, 1, 3, 0, 0], [10, 44, 6, 8, 1, 7, 0, 0]], 5e-5, 5),
}


def run(h, w, road, annos, factor, seed):
    img = frame(h, w, h * 1000 + w)
    t = torch.from_numpy(img).permute(2, 0, 1).contiguous().float().div(255)
    before = t.clone()
    a = torch.tensor(annos).float()
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out_img, out_annos = RF.fill_duck((t, a.clone(), torch.from_numpy(road).float() / 255),
                                          torch.tensor(CLS_LIST).unsqueeze(0), factor)
    changed = torch.nonzero((out_img.view(torch.int32) != before.view(torch.int32)).reshape(-1)).view(-1)
    return img, a.numpy(), out_annos.numpy(), changed.numpy().astype(np.int32), out_img.reshape(-1)[changed].numpy()


def main():
    out = {"names": np.array(list(CASES)), "cls_list": np.array(CLS_LIST)}
    for name, (h, w, road, annos, factor, seed) in CASES.items():
        img, a, oa, idx, val = run(h, w, road, annos, factor, seed)
        out.update({name + "_frame": img, name + "_road": road, name + "_annos": a, name + "_factor": np.float64(factor),
                    name + "_seed": np.int64(seed), name + "_out_annos": oa, name + "_idx": idx, name + "_val": val})
        print("%-8s rows %d -> %d, changed %d" % (name, len(a), len(oa), len(idx)))
    path = os.path.join(GOLD, "fillduck.npz")
    np.savez_compressed(path, **out)
    print("wrote %s %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()

"""Generates tests/golden/jitter.npz by IMPORTING THE REFERENCE (build container only; tools/ref_shims.py is the import
recipe).  Data only: the factors and what the reference's own ColorJitter returns for the stored 160x90 demo cut of
tests/golden/augment.npz (the input pixels are not stored a second time).

Recorded reference code: datasets/transforms/transforms.py:120-130 (ColorJitter, which hands its ranges to)
datasets/transforms/functional.py:159-174 (color_jitter: three random.uniform draws, then PIL's ImageEnhance.Brightness,
Contrast and Color).  Each case runs under random.seed(k); the factors are recovered by re-seeding and drawing the same
three uniforms from the transform's own ranges."""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

ref_shims.install()

from PIL import Image  # noqa: E402

from datasets.transforms.transforms import ColorJitter  # noqa: E402  (reference)

GOLD = os.path.join(ROOT, "tests", "golden")
# (seed, brightness, contrast, saturation): the reference's defaults, a wide range whose lower ends clamp at 0 and whose
# factors reach all three clip branches, and a narrow one around the identity
CASES = [(0, 0.5, 0.5, 0.5), (1, 0.5, 0.5, 0.5), (2, 0.5, 0.5, 0.5), (4, 1.5, 1.5, 1.5), (6, 1.5, 1.5, 1.5),
         (5, 0.05, 0.05, 0.05)]


def main():
    cut = np.load(os.path.join(GOLD, "augment.npz"))["cut"]
    assert cut.shape == (90, 160, 3) and cut.dtype == np.uint8
    out = {"cases": np.array(CASES, dtype=np.float64)}
    factors = []
    for i, (seed, b, c, s) in enumerate(CASES):
        t = ColorJitter(b, c, s)
        random.seed(seed)
        img, annos = t((Image.fromarray(cut), None))
        out["out_%d" % i] = np.array(img, dtype=np.uint8)
        random.seed(seed)
        factors.append([random.uniform(*t.brightness), random.uniform(*t.contrast), random.uniform(*t.saturation)])
    out["factors"] = np.array(factors, dtype=np.float64)
    path = os.path.join(GOLD, "jitter.npz")
    np.savez_compressed(path, **out)
    print("wrote %s %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()

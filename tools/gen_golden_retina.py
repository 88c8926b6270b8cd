"""Writes tests/golden/retina.npz: recorded results of the reference's RetinaNet pieces, computed on the CPU.

Needs the reference tree (tools/ref_shims.py makes it importable), so it runs in the build container only; the tests read the
file.  Data only:
  * anchors of `Anchors(sizes=(16, 64, 128))` for four image sizes (the 512x512 table as a SHA-256 of its float32 bytes plus
    its first and last 64 rows: the whole table would be most of a megabyte);
  * the reference's `RetinaNetOperator.criterion` (with `.cuda` patched to the identity) on the inputs of
    tests/retina_cases.py: the inputs and the two losses;
  * `focal_loss` on a small dense table;
  * the `state_dict` key / shape lists of `RetinaNet` with resnet10 and resnet50 (JSON text).

  python tools/gen_golden_retina.py
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "retina.npz")

SIZES = [(64, 64), (72, 56), (40, 104), (512, 512)]
CRITERION_CASES = [("base", (64, 64), 10, 11), ("base", (40, 104), 10, 12), ("duplicate", (64, 64), 10, 13),
                   ("base", (72, 56), 1, 14)]


def main():
    import retina_cases as rc                  # before the reference is put in front of sys.path
    from tools import ref_shims
    ref_shims.install()
    torch.Tensor.cuda = lambda self, *a, **k: self
    from modules.anchor import Anchors
    from modules.loss.focalloss import FocalLoss
    from modules.loss.functional import focal_loss
    from operators.retinanet_operator import RetinaNetOperator
    from models.retinanet import RetinaNet

    out = {}
    maker = Anchors(sizes=(16, 64, 128))
    for h, w in SIZES:
        a = maker((h, w)).numpy()
        assert a.dtype == np.float32
        if a.nbytes > 100000:
            out["anchors_%dx%d_sha256" % (h, w)] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
            out["anchors_%dx%d_rows" % (h, w)] = np.array(a.shape[0])
            out["anchors_%dx%d_head" % (h, w)] = a[:64]
            out["anchors_%dx%d_tail" % (h, w)] = a[-64:]
        else:
            out["anchors_%dx%d" % (h, w)] = a

    for i, (kind, size, classes, seed) in enumerate(CRITERION_CASES):
        op = object.__new__(RetinaNetOperator)
        op.anchor_maker = maker
        op.anchors, op.anchors_widths, op.anchors_heights, op.anchors_ctr_x, op.anchors_ctr_y = op.make_anchor(size)
        op.focal_loss = FocalLoss()
        annos = rc.criterion_batch(kind, classes)
        loc, logits = rc.criterion_preds(annos.shape[0], op.anchors.shape[0], classes, seed)
        with torch.no_grad():
            cls_loss, loc_loss = op.criterion((torch.from_numpy(loc), torch.from_numpy(logits)),
                                              torch.from_numpy(annos).clone())
        key = "crit%d_" % i
        out[key + "annos"], out[key + "loc"], out[key + "logits"] = annos, loc, logits
        out[key + "size"] = np.array(size)
        out[key + "losses"] = np.array([float(cls_loss), float(loc_loss)], dtype=np.float64)

    g = np.random.default_rng(5)
    x = (g.standard_normal((50, 10)) * 3).astype(np.float32)
    x[0, :3] = (40.0, -40.0, 0.0)
    t = (g.random((50, 10)) < 0.1).astype(np.float32)
    out["focal_x"], out["focal_t"] = x, t
    out["focal_loss"] = np.array(float(focal_loss(torch.from_numpy(x), torch.from_numpy(t))), dtype=np.float64)

    # the reference's configs/retinanet_config.py does not import (it names transforms its datasets/transforms lacks):
    # the model reads four keys only
    from types import SimpleNamespace as NS
    for name in ("resnet10", "resnet50"):
        cfg = NS(num_classes=10, Model=NS(num_anchors=9, backbone=name), Train=NS(pretrained=False))
        keys = [[k, list(v.shape)] for k, v in RetinaNet(cfg).state_dict().items()]
        out["state_keys_" + name] = np.array(json.dumps(keys))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

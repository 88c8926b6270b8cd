"""Anchor statistics: k-means over the box sizes of a VisDrone split, on the device (ext.kmeans.kmeans.lloyd).

  python tools/kmeans_anchors.py --data-root ./data/DronesDET [--split train] [--k 3] [--restarts 8] [--seed 219]
                                 [--out anchors.json]

Reads <data-root>/<split>/annotations/*.txt with datasets.drones_det.parse_annotations — no image is opened — and drops
class 0 (the ignored regions MaskIgnore removes; class 11 is dropped by the parser).  Three clusterings, in the order the
reference's scripts/kmeans.py prints them:
  1. annotation column 3 alone (the reference's `all_h` list, printed first),
  2. annotation column 2 alone (its `all_w` list, printed second),
  3. both columns jointly (M = 2; not in the reference).
The annotation columns are x, y, w, h: column 2 is the WIDTH and column 3 the HEIGHT.  The reference's script has the two
names the wrong way round (it appends column 3 to `all_w` and column 2 to `all_h`, then prints `h_results` first); its
order of output is kept here and each block is labelled with what the column really is.  Centres are printed ascending
with their counts, the inertia and the iteration count.

Without a dataset under --data-root it clusters the boxes of datasets.synthetic.synth_annotations, so the command runs
anywhere a device is."""
import argparse
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IGNORE_CLS = 0


def gather_sizes(root, split="train"):
    """float32 [n,2] = annotation columns 2 and 3 (width, height) of every box of <root>/<split>/annotations/*.txt, files
    in name order, classes 0 and 11 left out."""
    from rrnet_amd.datasets.drones_det import parse_annotations
    files = sorted(glob.glob(os.path.join(root, split, "annotations", "*.txt")))
    rows = [parse_annotations(f) for f in files]
    rows = [r[r[:, 5] != IGNORE_CLS][:, 2:4] for r in rows]
    if not rows:
        return np.zeros((0, 2), dtype=np.float32)
    return np.concatenate(rows, 0).astype(np.float32)


def synthetic_sizes(n=20000, seed=219):
    from rrnet_amd.datasets.synthetic import synth_annotations
    return np.round(synth_annotations(np.random.default_rng(seed), n, 765, 1360)[:, 2:4]).astype(np.float32)


def cluster(X, k, restarts, seed):
    """lloyd with `restarts` Forgy draws after np.random.seed(seed) -> dict with the centres sorted ascending (by their
    first column) and the counts in the same order."""
    from rrnet_amd.ext.kmeans.kmeans import lloyd
    np.random.seed(seed)
    _, centres, info = lloyd(X, k, restarts=restarts, return_info=True)
    order = np.lexsort(centres.T[::-1])
    return {"centres": centres[order].tolist(), "counts": info["counts"][order].tolist(), "inertia": info["inertia"],
            "iters": info["iters"], "converged": info["converged"], "restart": info["restart"]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data-root", default="./data/DronesDET")
    ap.add_argument("--split", default="train")
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--restarts", type=int, default=8)
    ap.add_argument("--seed", type=int, default=219)
    ap.add_argument("--out", default=None, help="write the three results as JSON")
    args = ap.parse_args(argv)
    sizes = gather_sizes(args.data_root, args.split)
    source = os.path.join(args.data_root, args.split)
    if sizes.shape[0] == 0:
        sizes, source = synthetic_sizes(seed=args.seed), "synthetic boxes (no annotations under %s)" % source
    print("%d boxes from %s" % (sizes.shape[0], source))
    report = {"source": source, "boxes": int(sizes.shape[0]), "k": args.k, "restarts": args.restarts, "seed": args.seed}
    for key, title, X in (("column3_height", "annotation column 3 (height; the reference's `all_h`)", sizes[:, 1:2]),
                          ("column2_width", "annotation column 2 (width; the reference's `all_w`)", sizes[:, 0:1]),
                          ("joint_width_height", "columns 2 and 3 jointly (width, height)", sizes)):
        res = report[key] = cluster(np.ascontiguousarray(X), args.k, args.restarts, args.seed)
        print("%s: %d iterations, inertia %.6g%s" % (title, res["iters"], res["inertia"],
                                                     "" if res["converged"] else " (NOT converged)"))
        for c, n in zip(res["centres"], res["counts"]):
            print("   %s  %8d boxes" % ("  ".join("%9.4f" % v for v in c), n))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")
    return report


if __name__ == "__main__":
    main()

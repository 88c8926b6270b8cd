"""Inputs shared by the device-evaluator tests: synthetic frames (detections x,y,w,h,score,cls and VisDrone annotation
rows), globally distinct scores, result / annotation text files in save_result's format."""
import numpy as np
import torch

GRID_D = (0, 1, 63, 64, 65, 130, 500)
GRID_G = (0, 1, 63, 64, 65, 130)


def frame(rng, n_det, n_gt, gt_classes=(1, 2, 3, 4, 5, 6, 7, 9), det_classes=(0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11),
          n_ignore=0, integer=True, extent=300):
    """One image.  Ground truth of classes 1..7 and 9 (8 and 10 never: detections of 8 and 10 meet no ground truth, 9
    only where a detection copies one); about two thirds of the detections are jittered copies of a ground truth with
    its class, the rest random boxes of any class 0..11.  Scores are left at 0: see distinct_scores."""
    gt = np.zeros((n_gt, 8), np.float32)
    if n_gt:
        gt[:, 0:2] = rng.integers(0, extent, (n_gt, 2))
        gt[:, 2:4] = rng.integers(4, 60, (n_gt, 2))
        gt[:, 4] = 1
        gt[:, 5] = rng.choice(gt_classes, n_gt)
        ign = rng.permutation(n_gt)[:min(n_ignore, n_gt)]
        gt[ign, 2:4] = rng.integers(40, 120, (len(ign), 2))
        gt[ign, 4:6] = 0
    det = np.zeros((n_det, 6), np.float32)
    if n_det:
        det[:, 0:2] = rng.integers(0, extent, (n_det, 2))
        det[:, 2:4] = rng.integers(0, 60, (n_det, 2))          # width or height 0 happens: integer snapping does that
        det[:, 5] = rng.choice(det_classes, n_det)
        if n_gt:
            src = rng.integers(0, n_gt, n_det)
            copy = rng.random(n_det) < 0.67
            jit = rng.integers(-3, 4, (n_det, 4))
            det[copy, 0:4] = (gt[src, 0:4] + jit)[copy]
            det[copy, 2:4] = np.maximum(det[copy, 2:4], 0)
            det[copy, 5] = np.where(gt[src[copy], 5] > 0, gt[src[copy], 5], 3)
        if not integer:
            det[:, 0:4] += rng.random((n_det, 4)).astype(np.float32)
    return det, gt


def distinct_scores(rng, dets):
    """Writes a permutation of k/10000 into column 4 of every frame: distinct inside a frame and across frames."""
    total = sum(d.shape[0] for d in dets)
    assert total < 10000
    vals = (rng.permutation(9999)[:total] + 1).astype(np.float64) / 10000.0
    at = 0
    for d in dets:
        d[:, 4] = vals[at:at + d.shape[0]].astype(np.float32)
        at += d.shape[0]
    allv = np.concatenate([d[:, 4] for d in dets]) if dets else np.zeros(0, np.float32)
    assert np.unique(allv).size == allv.size, "scores must be pairwise distinct"
    return dets


def grid_frames(seed=7):
    """The (D, G) size grid, one frame per pair; every third frame with ground truth holds ignored regions."""
    rng = np.random.default_rng(seed)
    dets, gts = [], []
    for i, nd in enumerate(GRID_D):
        for j, ng in enumerate(GRID_G):
            d, g = frame(rng, nd, ng, n_ignore=(3 if (i + j) % 3 == 0 else 0), integer=(i + j) % 4 != 1)
            dets.append(d), gts.append(g)
    return distinct_scores(rng, dets), gts


def tensors(arrays):
    return [torch.from_numpy(a.copy()) for a in arrays]


def write_files(pred_dir, gt_dir, dets, gts):
    """save_result's line format for the detections, integer VisDrone rows for the annotations."""
    for i, (d, g) in enumerate(zip(dets, gts)):
        with open(pred_dir / ("img%02d.txt" % i), "w") as f:
            for r in d:
                f.write('%f,%f,%f,%f,%.4f,%d,-1,-1\n' % (r[0], r[1], r[2], r[3], r[4], int(r[5])))
        with open(gt_dir / ("img%02d.txt" % i), "w") as f:
            for r in g:
                f.write(','.join('%d' % int(v) for v in r) + '\n')


def split_sum_box():
    """(x, w) as six-decimal texts whose float32 values give an x + w' (w' = the width after the float32 corner round
    trip of the Soft-NMS step) that truncates to different integers in float32 and in float64."""
    rng = np.random.default_rng(11)
    for _ in range(20000):           # x below 1 carries bits far under the grid of x + w near 100: w' gets rounded
        n = int(rng.integers(60, 120))
        xs = "%.6f" % rng.random()
        ws = "%.6f" % (n - float(xs))
        x, w = np.float32(float(xs)), np.float32(float(ws))
        w2 = np.float32(np.float32(x + w) - x)
        if int(np.float32(x + w2)) != int(np.float64(x) + np.float64(w2)):
            return xs, ws
    raise AssertionError("no such pair found")

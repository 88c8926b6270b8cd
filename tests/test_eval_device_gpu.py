"""The device evaluator (rr_eval_match / rr_eval_ap behind evaluate_arrays, evaluate_results, auto_evaluate_results and
sweep_evaluate_results with device=...) against the host evaluator: true-positive flags, the lists they land in and the
counts equal exactly; AP and AR within the tolerance tests/test_metrics.py holds the host evaluator to."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import eval_cases as E
from rrnet_amd.utils.metrics import metrics as M

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-6


def _dev():
    return torch.device("cuda", 0)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _same_detail(got, ref, confs=True):
    assert len(got["flags"]) == len(ref["flags"])
    for c in range(len(ref["flags"])):
        assert got["flags"][c].shape == ref["flags"][c].shape, ("class", c + 1, got["flags"][c].shape, ref["flags"][c].shape)
        assert torch.equal(got["flags"][c], ref["flags"][c]), ("flags of class", c + 1)
        if confs:
            assert torch.equal(got["confs"][c], ref["confs"][c]), ("confidences of class", c + 1)
    assert torch.equal(got["target_count"], ref["target_count"])
    assert torch.equal(got["in_img_count"], ref["in_img_count"])


def _close(ap, rc, ap_ref, rc_ref):
    print("ap", ap.tolist(), "ref", ap_ref.tolist(), "rc", float(rc), "ref", float(rc_ref))
    np.testing.assert_allclose(ap.numpy(), ap_ref.numpy(), rtol=RTOL, atol=ATOL, equal_nan=True)
    np.testing.assert_allclose(float(rc), float(rc_ref), rtol=RTOL, atol=ATOL, equal_nan=True)


def _both(dets, gts, thresholds=M.THRESHOLDS, confs=True, **kw):
    """evaluate_arrays on the device and on the host, compared; -> the device result."""
    ap, rc, detail = M.evaluate_arrays(E.tensors(dets), E.tensors(gts), thresholds, device=_dev(), **kw)
    ap_ref, rc_ref, ref = M.evaluate_arrays(E.tensors(dets), E.tensors(gts), thresholds, device=None, **kw)
    _same_detail(detail, ref, confs)
    _close(ap, rc, ap_ref, rc_ref)
    return ap, rc, detail


def test_golden_cases_in_one_launch(golden_dir):
    z = np.load(os.path.join(golden_dir, "metrics.npz"))
    preds = [torch.from_numpy(z["c%d/pred" % i]) for i in range(4)]
    targets = [torch.from_numpy(z["c%d/target" % i]) for i in range(4)]
    ap, rc, detail = M.evaluate_arrays(preds, targets, device=_dev())
    for c in range(10):
        np.testing.assert_array_equal(detail["flags"][c].numpy(), z["all/flags%d" % c])
        np.testing.assert_array_equal(detail["confs"][c].numpy(), z["all/confs%d" % c])
    np.testing.assert_array_equal(detail["target_count"].numpy(), z["c3/target_count"])
    np.testing.assert_array_equal(detail["in_img_count"].numpy(), z["c3/in_img_count"])
    np.testing.assert_allclose(ap.numpy(), z["all/ap"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(float(rc), float(z["all/rc"]), rtol=RTOL, atol=ATOL)


@pytest.fixture(scope="module")
def grid():
    return E.grid_frames()


@pytest.mark.parametrize("thresholds", [M.THRESHOLDS, M.THRESHOLDS[5:6]], ids=["T10", "T1"])
def test_size_grid(grid, thresholds):
    """Every (D, G) of the grid in one launch: empty frames, one row, one below / at / above the wave width, several
    strides of it; detections of classes 0 and 11, of classes without ground truth (8, 10), ground truth without
    detections (G > 0 with D = 0)."""
    dets, gts = grid
    assert len(dets) == len(E.GRID_D) * len(E.GRID_G)
    _, _, detail = _both(dets, gts, thresholds)
    assert sum(f.shape[0] for f in detail["flags"]) > 1000 and float(sum(f.sum() for f in detail["flags"])) > 100
    assert detail["flags"][7].shape[0] == 0 and detail["flags"][9].shape[0] == 0      # classes 8 and 10: dropped


def test_rows_past_max_det_num_are_cut():
    rng = np.random.default_rng(3)
    frames = [E.frame(rng, 130, 130, n_ignore=2), E.frame(rng, 65, 130), E.frame(rng, 130, 64, n_ignore=1)]
    dets = E.distinct_scores(rng, [f[0] for f in frames])
    _both(dets, [f[1] for f in frames], max_det_num=100)


def test_largest_frame_the_kernel_takes():
    """2048 ground truths in one frame (the LDS limit), nearly all of two classes: lanes stride over a class's list
    several times and positions beyond 64 must win ties correctly; next to it an empty and a small frame."""
    from rrnet_amd import ops
    rng = np.random.default_rng(13)
    big = E.frame(rng, 200, ops.EVAL_MAX_GT, gt_classes=(1, 1, 1, 2, 2, 7), n_ignore=4, extent=900)
    frames = [E.frame(rng, 0, 0), big, E.frame(rng, 65, 63)]
    dets = E.distinct_scores(rng, [f[0] for f in frames])
    _, _, detail = _both(dets, [f[1] for f in frames], max_det_num=ops.EVAL_MAX_GT)
    assert detail["target_count"][0] > 700 and float(detail["flags"][0].sum()) > 100


def test_ap_kernel_on_long_lists():
    """rr_eval_ap alone against calculate_ap_rc: lists of 0, 1 and around one and several chunks of the backward walk
    (1024 rows), a class without ground truth that still has rows, one whose list is empty."""
    from rrnet_amd import ops
    dev = _dev()
    rng = np.random.default_rng(17)
    sizes = [0, 1, 1023, 1024, 1025, 3000, 5000, 2049, 7, 0]
    tc = torch.tensor([5, 1, 700, 2000, 300, 1500, 0, 2100, 3, 0], dtype=torch.float32)
    ic = torch.tensor([2, 1, 40, 90, 33, 70, 0, 55, 3, 0], dtype=torch.float32)
    for t_n, thresholds in ((10, M.THRESHOLDS), (1, M.THRESHOLDS[:1])):
        flags, confs, words = [], [], []
        for n in sizes:
            f = (rng.random((n, t_n)) < np.linspace(0.5, 0.05, t_n)).astype(np.float32)
            flags.append(torch.from_numpy(f))
            confs.append(torch.from_numpy(np.sort(rng.permutation(100000)[:n].astype(np.float32) / 100000.0)[::-1].copy()))
            words.append((f.astype(np.int64) << np.arange(t_n)).sum(axis=1).astype(np.int32))
        ap_ref, rc_ref = M.calculate_ap_rc(flags, confs, tc, ic)
        seg_off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
        ap, rc = ops.eval_ap(torch.from_numpy(np.concatenate(words)).to(dev), seg_off, tc.to(torch.int32).to(dev),
                             ic.to(torch.int32).to(dev), t_n)
        _close(ap.cpu(), rc.cpu(), ap_ref, rc_ref)


def _det(rows):
    return np.asarray(rows, np.float32).reshape(-1, 6)


def _gt(rows):
    return np.asarray([[x, y, w, h, 1 if c else 0, c, 0, 0] for x, y, w, h, c in rows], np.float32).reshape(-1, 8)


def test_boundary_arithmetic():
    """Integer boxes that land on a threshold, ties between ground truths, per-threshold bookkeeping, the 0.5 overlap
    rule at equality and on zero areas."""
    dets = [
        _det([[0, 0, 10, 10, .99, 1]]),                                    # IoU 100/200 = 0.5
        _det([[0, 0, 30, 10, .98, 1]]),                                    # 300/400 = 0.75
        _det([[0, 0, 30, 10, .97, 1]]),                                    # 300/500 = 0.6
        _det([[100, 100, 10, 10, .96, 2], [100, 100, 10, 10, .95, 2], [100, 100, 10, 10, .94, 2]]),
        _det([[0, 0, 60, 10, .93, 4], [0, 0, 90, 10, .92, 4], [0, 0, 63, 8, .91, 4]]),
        _det([[200, 200, 20, 10, .90, 5], [0, 0, 20, 10, .89, 5], [0, 0, 20, 10, .88, 6]]),
        _det([[50, 50, 0, 10, .87, 1], [50, 50, 10, 10, .86, 1]]),         # zero-area detection, no ignored region
        _det([[50, 50, 0, 10, .85, 1], [50, 50, 10, 10, .84, 1]]),         # ... with one
        _det([[10, 10, 20, 20, .83, 1], [300, 300, 5, 5, .82, 2]]),        # only ignored regions in the frame
    ]
    gts = [
        _gt([[0, 0, 10, 20, 1]]),
        _gt([[0, 0, 40, 10, 1]]),
        _gt([[0, 0, 50, 10, 1]]),
        _gt([[100, 100, 10, 20, 2], [100, 90, 10, 20, 2]]),                # both at IoU 0.5 with every detection
        _gt([[0, 0, 100, 10, 4], [0, 0, 90, 8, 4]]),                       # det 2 prefers A where det 1 left it free
        _gt([[200, 200, 20, 10, 5], [210, 200, 50, 50, 0], [0, 0, 20, 10, 6]]),   # class 5 exactly half ignored
        _gt([[50, 50, 10, 10, 1], [70, 70, 0, 10, 1]]),                    # zero-area ground truth stays
        _gt([[50, 50, 10, 10, 1], [70, 70, 0, 10, 1], [400, 400, 30, 30, 0]]),    # ... and leaves with a region around
        _gt([[0, 0, 50, 50, 0], [100, 100, 50, 50, 0]]),
    ]
    ap, rc, detail = _both(dets, gts)
    flags = detail["flags"]
    thr = M.THRESHOLDS
    # class 1 (frames 0, 1, 2, 6, 7): what bbox_iou's own fp32 quotient clears, nothing else
    for row, iou in ((0, np.float32(100) / np.float32(200)), (1, np.float32(300) / np.float32(400)),
                     (2, np.float32(300) / np.float32(500))):
        want = ((torch.tensor(float(iou)) - thr) >= 0).float()
        assert torch.equal(flags[0][row], want), (row, flags[0][row], want)
    assert flags[0][0].sum() == 1 and flags[0][1].sum() >= 5
    # class 2: two detections take the two ground truths at 0.5, the third finds none
    assert flags[1][:, 0].tolist() == [1, 1, 0] and float(flags[1][:, 1:].sum()) == 0
    # class 4: the third detection is a false positive where B is taken and a true positive where it is free
    assert flags[3].shape[0] == 3 and 0 < float(flags[3][2].sum()) < float(flags[3][1].sum())
    assert flags[3][2, 0] == 0
    # class 5: its only ground truth left with the region, so its detections are not even counted
    assert flags[4].shape[0] == 0 and detail["target_count"][4] == 0
    assert flags[5].shape[0] == 1 and detail["target_count"][5] == 1
    # class 1 counts: frames 0, 1, 2 one each; frame 6 two (the zero-area one stays), frame 7 one (it left)
    assert detail["target_count"][0] == 6 and detail["in_img_count"][0] == 5
    # class 1 detections: 3 + 2 in frame 6 (zero-area detection kept without a region) + 1 in frame 7
    assert flags[0].shape[0] == 6


def test_all_ignored_or_empty_gives_nan():
    dets = [_det([[10, 10, 20, 20, .5, 1]]), _det([])]
    gts = [_gt([[0, 0, 50, 50, 0]]), _gt([])]
    ap, rc, _ = _both(dets, gts)
    assert torch.isnan(ap).all() and torch.isnan(rc)


def test_ties_are_stable():
    """Equal scores keep row order within a frame and (frame, row) order within a class: the device result on tied
    scores equals the host result after the ties are replaced by strictly decreasing values in that order."""
    rng = np.random.default_rng(5)
    frames = [E.frame(rng, nd, ng, n_ignore=ni) for nd, ng, ni in ((90, 40, 0), (130, 70, 2), (64, 30, 0), (200, 66, 1))]
    dets, gts = [f[0] for f in frames], [f[1] for f in frames]
    for d in dets:
        d[:, 4] = rng.choice(np.asarray([.9, .7, .5, .3, .1], np.float32), d.shape[0])
    ordered = [d[np.argsort(-d[:, 4], kind="stable")] for d in dets]       # the order the device path is defined to use
    allv = np.concatenate([d[:, 4] for d in ordered])
    rank = np.empty(allv.size, np.int64)
    rank[np.argsort(-allv, kind="stable")] = np.arange(allv.size)         # (frame, row) order among equal scores
    fresh, at = [], 0
    for d in ordered:
        d = d.copy()
        d[:, 4] = ((allv.size - rank[at:at + d.shape[0]]) / (2.0 * allv.size)).astype(np.float32)
        at += d.shape[0]
        fresh.append(d)
    assert np.unique(np.concatenate([d[:, 4] for d in fresh])).size == allv.size
    ap, rc, detail = M.evaluate_arrays(E.tensors(dets), E.tensors(gts), device=_dev())
    ap_ref, rc_ref, ref = M.evaluate_arrays(E.tensors(fresh), E.tensors(gts), device=None)
    _same_detail(detail, ref, confs=False)
    _close(ap, rc, ap_ref, rc_ref)
    assert float(sum(f.sum() for f in detail["flags"])) > 50


CT, SNMS = (0.05, 0.2), (0.02, 0.1)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Twelve small result / annotation files, non-integer boxes, distinct scores; file 0 also holds a box whose x + w
    truncates differently in float32 and in float64."""
    root = tmp_path_factory.mktemp("eval")
    pd_dir, gt_dir = root / "pred", root / "gt"
    pd_dir.mkdir(), gt_dir.mkdir()
    rng = np.random.default_rng(9)
    frames = [E.frame(rng, int(rng.integers(20, 79)), int(rng.integers(5, 40)), n_ignore=(2 if i % 3 == 0 else 0),
                      det_classes=(1, 2, 3, 4, 5, 6, 7, 8, 10), integer=False) for i in range(12)]
    dets = E.distinct_scores(rng, [f[0] for f in frames])
    E.write_files(pd_dir, gt_dir, dets, [f[1] for f in frames])
    xs, ws = E.split_sum_box()
    x, w = np.float32(float(xs)), np.float32(float(ws))
    w2 = np.float32(np.float32(x + w) - x)
    assert int(np.float32(x + w2)) != int(np.float64(x) + np.float64(w2))
    with open(pd_dir / "img00.txt", "a") as f:
        f.write("%s,700.250000,%s,30.500000,1.0000,1,-1,-1\n" % (xs, ws))
    return str(pd_dir), str(gt_dir), (xs, ws)


@pytest.fixture(scope="module")
def host_pairs(files):
    return {(ct, sn): _quiet(M.auto_evaluate_results, files[0], files[1], ct, sn) for ct in CT for sn in SNMS}


def test_sweep_equals_host_pairs(files, host_pairs):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        got = M.sweep_evaluate_results(files[0], files[1], CT, SNMS, device=_dev())
    assert got.shape == (2, 2, 11) and got.dtype == np.float32
    assert out.getvalue().count("Average Precision  (AP) @[ IoU=0.50:0.95]") == 4
    for i, ct in enumerate(CT):
        for j, sn in enumerate(SNMS):
            ap, rc = host_pairs[(ct, sn)]
            _close(torch.from_numpy(got[i, j, :-1]), torch.tensor(got[i, j, -1]), ap, rc)
    assert 0.0 < got[..., :-1].mean() < 1.0 and not np.array_equal(got[0, 0], got[1, 1])


def test_sweep_rows_equal_host_nms_and_snap(files):
    """Per frame, the rows that enter the matching == ext_nms_batch + _snap + sort + cut of auto_evaluate_results."""
    pred_dir, _, (xs, ws) = files
    dev = _dev()
    preds, _, lens = M._sweep_read(pred_dir, files[1], CT, 500)
    dets, _ = M._pad(preds, dev)
    lens = torch.from_numpy(np.ascontiguousarray(lens)).to(dev)
    names = M._names(pred_dir)
    seen_split = False
    for i, ct in enumerate(CT):
        host_in = []
        for name in names:
            p = M._read(os.path.join(pred_dir, name + ".txt"))
            p = torch.from_numpy(p[p[:, 4] > ct]).float()
            host_in.append(p[torch.sort(p[:, 4], descending=True)[1]])
        for sn in SNMS:
            rows, det_len = M.sweep_nms_rows(dets, lens[i], sn, 500)
            rows, det_len = rows.cpu().numpy(), det_len.cpu().numpy()
            for k, kept in enumerate(M.ext_nms_batch(host_in, sn)):
                want = torch.from_numpy(M._snap(kept.astype(np.float64))).float()
                assert want[:, 4].unique().numel() == want.shape[0], "kept scores must be distinct"
                want = want[torch.sort(want[:, 4], descending=True)[1]][:500].numpy()
                assert det_len[k] == want.shape[0], (ct, sn, names[k])
                assert np.array_equal(rows[k, :det_len[k]].view(np.uint32), want[:, :6].view(np.uint32)), (ct, sn, names[k])
                if names[k] == "img00":
                    hit = want[want[:, 1] == 700.0]
                    assert hit.shape[0] == 1
                    x32 = np.float32(float(xs))
                    w2 = np.float32(np.float32(x32 + np.float32(float(ws))) - x32)
                    assert hit[0, 2] == float(int(np.float64(x32) + np.float64(w2)) - int(x32))
                    assert hit[0, 2] != float(int(np.float32(x32 + w2)) - int(x32))
                    seen_split = True
    assert seen_split


def test_file_drivers_with_device(files, host_pairs):
    pred_dir, gt_dir, _ = files
    ap_ref, rc_ref = _quiet(M.evaluate_results, pred_dir, gt_dir)
    ap, rc = _quiet(M.evaluate_results, pred_dir, gt_dir, device=_dev())
    _close(ap, rc, ap_ref, rc_ref)
    ap, rc = _quiet(M.auto_evaluate_results, pred_dir, gt_dir, CT[0], SNMS[1], device=_dev())
    _close(ap, rc, *host_pairs[(CT[0], SNMS[1])])

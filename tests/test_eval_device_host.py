"""The evaluator's new entry points where no GPU is needed: the `device` keywords default to the host path and leave
its results untouched, the wrappers refuse what the kernels cannot take, and include/rrnet_hip.h declares both kernels
(tests/test_abi.py then checks that the library exports them)."""
import contextlib
import inspect
import io
import os

import numpy as np
import pytest
import torch

from rrnet_amd.utils.metrics import metrics as M


def _golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "metrics.npz"))
    return z, [z["c%d/pred" % i] for i in range(4)], [z["c%d/target" % i] for i in range(4)]


def _host_accumulation(preds, targets):
    flags, confs, tc, ic = M._fresh(11, 10)
    for p, t in zip(preds, targets):
        flags, confs, tc, ic = M.get_tp(torch.from_numpy(p).float()[:500], torch.from_numpy(t).float()[:500], flags, confs,
                                        tc, ic, M.THRESHOLDS, 11)
    return flags, confs, tc, ic, M.calculate_ap_rc(flags, confs, tc, ic)


def test_keywords_default_to_the_host_path():
    for fn in (M.evaluate_arrays, M.evaluate_results, M.auto_evaluate_results, M.sweep_evaluate_results):
        assert inspect.signature(fn).parameters["device"].default is None
    names = list(inspect.signature(M.evaluate_results).parameters)
    assert names == ["pred_dir", "target_dir", "thresholds", "cls_num", "max_det_num", "device"]
    names = list(inspect.signature(M.auto_evaluate_results).parameters)
    assert names == ["pred_dir", "target_dir", "ctnet_min_threshold", "softnms_min_threshold", "thresholds", "cls_num",
                     "max_det_num", "device"]
    names = list(inspect.signature(M.sweep_evaluate_results).parameters)
    assert names == ["pred_dir", "target_dir", "ctnet_min_thresholds", "softnms_min_thresholds", "thresholds", "cls_num",
                     "max_det_num", "device"]


def test_evaluate_arrays_host_is_get_tp_and_calculate_ap_rc(golden_dir):
    z, preds, targets = _golden(golden_dir)
    flags, confs, tc, ic, (ap_ref, rc_ref) = _host_accumulation(preds, targets)
    for kw in ({}, {"device": None}):
        ap, rc, detail = M.evaluate_arrays(preds, targets, **kw)
        assert torch.equal(ap, ap_ref) and torch.equal(rc, rc_ref)
        for c in range(10):
            assert torch.equal(detail["flags"][c], flags[c]) and torch.equal(detail["confs"][c], confs[c])
            np.testing.assert_array_equal(detail["flags"][c].numpy(), z["all/flags%d" % c])
        assert torch.equal(detail["target_count"], tc) and torch.equal(detail["in_img_count"], ic)
    np.testing.assert_allclose(ap_ref.numpy(), z["all/ap"], rtol=1e-5, atol=1e-6)


def test_evaluate_results_default_is_unchanged(golden_dir, tmp_path):
    z, preds, targets = _golden(golden_dir)
    pd_dir, gt_dir = tmp_path / "pred", tmp_path / "gt"
    pd_dir.mkdir(), gt_dir.mkdir()
    for i in range(4):
        with open(pd_dir / ("f%d.txt" % i), "w") as f:
            for r in preds[i]:
                f.write('%f,%f,%f,%f,%.4f,%d,-1,-1\n' % (r[0], r[1], r[2], r[3], r[4], int(r[5])))
        with open(gt_dir / ("f%d.txt" % i), "w") as f:
            for r in targets[i]:
                f.write(','.join('%d' % int(v) for v in r) + '\n')
    snapped, annos = [], []
    for name in M._names(str(pd_dir)):
        snapped.append(M._snap(M._read(os.path.join(str(pd_dir), name + ".txt")).astype(np.float64)))
        annos.append(M._read(os.path.join(str(gt_dir), name + ".txt")))
    ap_ref, rc_ref = _host_accumulation(snapped, annos)[4]
    for kw in ({}, {"device": None}):
        with contextlib.redirect_stdout(io.StringIO()) as out:
            ap, rc = M.evaluate_results(str(pd_dir), str(gt_dir), **kw)
        assert torch.equal(ap, ap_ref) and torch.equal(rc, rc_ref)
        assert out.getvalue().count("Average") == 4 and "Cost Time" in out.getvalue()
    ap, rc, _ = M.evaluate_arrays(snapped, annos)
    assert torch.equal(ap, ap_ref) and torch.equal(rc, rc_ref)


def test_eval_match_refuses_cpu_tensors_and_too_many_ground_truths():
    from rrnet_amd import _C, ops
    lens = torch.zeros(2, dtype=torch.int32)
    thr = M.THRESHOLDS.float()
    with pytest.raises(_C.RRNetHipError, match="no CPU fallback"):
        ops.eval_match(torch.zeros(2, 4, 6), lens, torch.zeros(2, 4, 6), lens, thr)
    with pytest.raises(ValueError, match="2048"):
        ops.eval_match(torch.zeros(2, 4, 6), lens, torch.zeros(2, ops.EVAL_MAX_GT + 1, 6), lens, thr)
    with pytest.raises(ValueError, match="16"):
        ops.eval_match(torch.zeros(2, 4, 6), lens, torch.zeros(2, 4, 6), lens, torch.zeros(17))
    with pytest.raises(_C.RRNetHipError, match="no CPU fallback"):
        ops.eval_ap(torch.zeros(4, dtype=torch.int32), torch.zeros(11, dtype=torch.int32),
                    torch.zeros(10, dtype=torch.int32), torch.zeros(10, dtype=torch.int32), 10)


def test_header_declares_both_entry_points():
    from ctypes import c_int, c_long, c_void_p
    from rrnet_amd import _C, ops
    sigs = _C.header_signatures()
    assert sigs["rr_eval_match"] == (c_int, [c_void_p] * 5 + [c_int] * 5 + [c_void_p] * 4)
    assert sigs["rr_eval_ap"] == (c_int, [c_void_p, c_long] + [c_void_p] * 3 + [c_int] * 2 + [c_void_p] * 4)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rrnet_hip.h")).read()
    assert "#define RR_EVAL_MAX_GT %d\n" % ops.EVAL_MAX_GT in header
    assert "#define RR_EVAL_MAX_THRESHOLDS %d\n" % ops.EVAL_MAX_THRESHOLDS in header
    from rrnet_amd.csrc import build
    assert build.PER_FILE["evalmatch.hip"] == ["-ffp-contract=off"]


@pytest.mark.gpu
def test_sweep_without_device_is_a_loop_of_auto_evaluate_results(tmp_path):
    """Needs the GPU all the same: auto_evaluate_results runs its Soft-NMS there."""
    import eval_cases as E
    pd_dir, gt_dir = tmp_path / "pred", tmp_path / "gt"
    pd_dir.mkdir(), gt_dir.mkdir()
    rng = np.random.default_rng(2)
    frames = [E.frame(rng, 40, 15, det_classes=(1, 2, 3, 4, 5), integer=False) for _ in range(3)]
    E.write_files(pd_dir, gt_dir, E.distinct_scores(rng, [f[0] for f in frames]), [f[1] for f in frames])
    cts, sns = (0.05, 0.3), (0.05,)
    with contextlib.redirect_stdout(io.StringIO()):
        got = M.sweep_evaluate_results(str(pd_dir), str(gt_dir), cts, sns)
        assert got.shape == (2, 1, 11)
        for i, ct in enumerate(cts):
            ap, rc = M.auto_evaluate_results(str(pd_dir), str(gt_dir), ct, sns[0])
            assert np.array_equal(got[i, 0, :-1], ap.numpy()) and got[i, 0, -1] == np.float32(float(rc))

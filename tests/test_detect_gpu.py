"""GPU tests of detection on raw frames (rrnet_amd/inference.py detect_frames; kernels rr_prepare_frames, rr_merge_scales,
rr_sort_frames_by_score in csrc/detect.hip): bit-exact pieces against host compositions of the oracle, and the whole
path on a tiny RRNet against the per-frame evaluation."""
import types
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _normalised(frames_u8):
    """ToTensor -> Normalize on the host, float32 torch: [B,H,W,3] uint8 -> [B,3,H,W]."""
    x = frames_u8.permute(0, 3, 1, 2).float().div(255)
    mean = torch.tensor(MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).view(1, 3, 1, 1)
    return x.sub(mean).div(std).contiguous()


# ---- 1. rr_prepare_frames ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,scales", [((2, 5, 7, 3), (1, 1.1, 1.25, 1.5, 0.7)),
                                          ((2, 37, 53, 3), (1, 1.1, 1.25, 1.5, 0.7)),   # 159 bytes per row: no multiple of 4
                                          ((1, 1, 9, 3), (1.5,))])                      # OH == 1
def test_prepare_frames_bit_identical_to_normalise_then_resize(shape, scales):
    import torch.nn.functional as F
    from rrnet_amd import ops
    rng = np.random.default_rng(7)
    frames = torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8))
    frames[0, 0, 0] = torch.tensor([0, 255, 128], dtype=torch.uint8)
    host = _normalised(frames)
    mean, std = torch.tensor(MEAN).cuda(), torch.tensor(STD).cuda()
    for s in scales:
        got = ops.prepare_frames(frames.cuda(), mean, std, s)
        chain = ops.resize_bilinear_ac(host.cuda(), s)
        ref = F.interpolate(host, scale_factor=s, mode='bilinear', align_corners=True)
        assert tuple(got.shape) == tuple(chain.shape) == tuple(ref.shape), (got.shape, chain.shape, ref.shape)
        assert ops.is_nhwc(got)
        got, chain = got.cpu().numpy(), chain.cpu().numpy()
        diff = int((_u32(got) != _u32(chain)).sum())
        print("prepare_frames %s x%g: %d of %d words differ from the chain, max |got - F.interpolate| %.3g"
              % (shape, s, diff, got.size, float(np.abs(got - ref.numpy()).max())))
        assert diff == 0
        np.testing.assert_allclose(got, ref.numpy(), atol=1e-4, rtol=1e-4)


# ---- 2. / 3. merge, sort, Soft-NMS tail --------------------------------------------------------------------------------

def _stage2_inputs(rng, counts, distinct):
    """counts[f][j] rows of frame f at scale j -> per scale (rois [R,5], reg [R,4], scores [R], clses [R], frame_off
    [B+1]) as numpy float32 / int32; reg[:, 2:] = 0 keeps exp() out (exp(0) * w == w on both sides)."""
    nframes, nscales = len(counts), len(counts[0])
    total = sum(sum(c) for c in counts)
    pool = (rng.permutation(max(total, 1) * 3)[:total] + 1).astype(np.float32) / np.float32(max(total, 1) * 3 + 1)
    used, per_scale = 0, []
    for j in range(nscales):
        rois, off = [], [0]
        for f in range(nframes):
            n = counts[f][j]
            xy = rng.uniform(0, 40, (n, 2)).astype(np.float32)
            wh = rng.uniform(1, 12, (n, 2)).astype(np.float32)
            rois.append(np.concatenate([np.full((n, 1), f, np.float32), xy, xy + wh], 1))
            off.append(off[-1] + n)
        rois = np.concatenate(rois).astype(np.float32)
        r = rois.shape[0]
        reg = rng.normal(0, 0.1, (r, 4)).astype(np.float32)
        reg[:, 2:] = 0
        if distinct:
            scores = pool[used:used + r].copy()
            used += r
        else:
            scores = (np.round(rng.uniform(0, 1, r) * 50) / 50).astype(np.float32)       # ties within and across scales
        clses = rng.integers(0, 10, r).astype(np.float32)
        per_scale.append((rois, reg, scores, clses, np.asarray(off, np.int32)))
    return per_scale


def _host_rows(per_scale, scales, f, filt):
    """generate_bbox rows of frame f, filtered, / float32(s), concatenated in scale order (float32 on the host)."""
    from oracle import ops as oops
    rows = []
    for (rois, reg, scores, clses, _), s in zip(per_scale, scales):
        outs = (None, None, None, torch.from_numpy(reg), torch.from_numpy(rois), torch.from_numpy(scores),
                torch.from_numpy(clses))
        pred = oops.generate_bbox(outs, f, 4)[1].numpy().astype(np.float32).reshape(-1, 6)
        if filt:
            pred = pred[pred[:, 4] > np.float32(0.01)]
        pred = pred.copy()
        pred[:, :4] = pred[:, :4] / np.float32(s)
        rows.append(pred)
    return np.concatenate(rows).astype(np.float32)


def _device_merge(per_scale, scales, nframes, k, filt):
    from rrnet_amd import ops
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    merged, count = ops.merge_buffers(nframes, k, torch.device("cuda"))
    for (rois, reg, scores, clses, off), s in zip(per_scale, scales):
        ops.merge_scales(T(rois), T(reg), T(scores), T(clses), T(off), s, merged, count, scale=4,
                         score_thr=0.01 if filt else None)
    return merged, count


def _check_merge_and_sort(per_scale, scales, nframes, k, filt):
    from rrnet_amd import ops
    merged, count = _device_merge(per_scale, scales, nframes, k, filt)
    ordered = ops.sort_frames_by_score(merged, count)
    off = ops.seg_prefix(count)
    packed = ops.sort_frames_by_score(merged, count, out_off=off)
    as_xyxy = ops.sort_frames_by_score(merged, count, xyxy=True)
    merged, count, ordered = merged.cpu().numpy(), count.cpu().numpy(), ordered.cpu().numpy()
    off, packed, as_xyxy = off.cpu().numpy(), packed.cpu().numpy(), as_xyxy.cpu().numpy()
    for f in range(nframes):
        cat = _host_rows(per_scale, scales, f, filt)
        n = cat.shape[0]
        assert count[f] == n, (f, count[f], n)
        assert off[f + 1] - off[f] == n
        np.testing.assert_array_equal(_u32(merged[f, :n]), _u32(cat))
        exp = cat[np.argsort(-cat[:, 4], kind='stable')]
        np.testing.assert_array_equal(_u32(ordered[f, :n]), _u32(exp))
        np.testing.assert_array_equal(_u32(packed[off[f]:off[f + 1]]), _u32(exp))
        xyxy = exp.copy()
        xyxy[:, 2] = exp[:, 0] + exp[:, 2]
        xyxy[:, 3] = exp[:, 1] + exp[:, 3]
        np.testing.assert_array_equal(_u32(as_xyxy[f, :n]), _u32(xyxy))
        for pad in (merged[f, n:, 5], ordered[f, n:, 5], as_xyxy[f, n:, 5]):      # padding: no class of 1..10
            assert np.all((pad < 1) | (pad > 10))


SMALL_SCALES = (1, 1.25, 1.5)


def _small_counts(rng):
    sizes = [0, 1, 63, 64, 65, 70, 257]
    counts = [[int(sizes[i]) for i in rng.integers(0, len(sizes), 3)] for _ in range(3)]
    counts[0] = [257, 65, 64]              # more than one block of 256, a full wave and one past it
    counts[1] = [0, 0, 0]                  # a frame without rows
    counts[2][1] = 0                       # a scale that contributes nothing to a frame with rows
    counts[2][2] = max(counts[2][2], 63)
    return counts


@pytest.mark.parametrize("filt", [True, False])
def test_merge_and_sort_bit_exact_small(filt):
    rng = np.random.default_rng(21)
    counts = _small_counts(rng)
    per_scale = _stage2_inputs(rng, counts, distinct=False)
    _check_merge_and_sort(per_scale, SMALL_SCALES, 3, 3 * 257, filt)


def test_merge_and_sort_bit_exact_workload_size():
    """2 frames x 6 scales x 1500 rows: 9000 rows per frame, 16384 keys in LDS (the configuration's size)."""
    rng = np.random.default_rng(22)
    scales = (1, 1.1, 1.2, 1.3, 1.4, 1.5)
    per_scale = _stage2_inputs(rng, [[1500] * 6, [1500] * 6], distinct=False)
    _check_merge_and_sort(per_scale, scales, 2, 9000, False)


def test_merge_and_sort_frame_of_16384_rows_and_the_limit():
    from rrnet_amd import ops
    rng = np.random.default_rng(23)
    per_scale = _stage2_inputs(rng, [[4096] * 4], distinct=False)
    _check_merge_and_sort(per_scale, (1, 1.1, 1.25, 1.5), 1, 16384, False)
    with pytest.raises(ValueError, match="16384"):
        ops.merge_buffers(1, 16385, torch.device("cuda"))
    with pytest.raises(ValueError, match="16384"):
        ops.sort_frames_by_score(torch.zeros((1, 16385, 6), device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))


def test_nms_tail_bit_exact_vs_oracle_composition():
    """merge -> sort -> per-class Soft-NMS -> sort on the device equals cat, divide, stable sort, oracle.nms.ext_nms,
    stable sort on the host, bit for bit (pairwise distinct scores)."""
    from oracle import nms as onms
    from rrnet_amd import inference
    rng = np.random.default_rng(24)
    counts = _small_counts(rng)
    per_scale = _stage2_inputs(rng, counts, distinct=True)
    merged, count = _device_merge(per_scale, SMALL_SCALES, 3, 3 * 257, True)
    boxes, frame_off = inference.finish_frames(merged, count, True, 10)
    boxes, fo = boxes.cpu().numpy(), frame_off.cpu().numpy()
    assert fo[0] == 0 and fo[-1] == boxes.shape[0]
    for f in range(3):
        cat = _host_rows(per_scale, SMALL_SCALES, f, True)
        ref = cat[np.argsort(-cat[:, 4], kind='stable')]
        ref = onms.ext_nms(ref).reshape(-1, 6)
        ref = ref[np.argsort(-ref[:, 4], kind='stable')]
        got = boxes[fo[f]:fo[f + 1]]
        assert got.shape == ref.shape, (f, got.shape, ref.shape)
        np.testing.assert_array_equal(_u32(got), _u32(ref))
    # without nms the tail is the first sort alone
    merged, count = _device_merge(per_scale, SMALL_SCALES, 3, 3 * 257, False)
    boxes, frame_off = inference.finish_frames(merged, count, False, 10)
    boxes, fo = boxes.cpu().numpy(), frame_off.cpu().numpy()
    for f in range(3):
        cat = _host_rows(per_scale, SMALL_SCALES, f, False)
        np.testing.assert_array_equal(_u32(boxes[fo[f]:fo[f + 1]]), _u32(cat[np.argsort(-cat[:, 4], kind='stable')]))


# ---- 4. end to end on the tiny RRNet -----------------------------------------------------------------------------------

def _cfg(bf16=False):
    model = SimpleNamespace(num_stacks=2, backbone="hourglass_tiny", nms_type_for_stage1="nms",
                            nms_per_class_for_stage1=True)
    if bf16:
        model.bf16 = True
    return SimpleNamespace(num_classes=10, Model=model, Train=SimpleNamespace(scale_factor=4),
                           Val=SimpleNamespace(scales=[1, 1.25, 1.5], auto_test=False))


@pytest.fixture(scope="module")
def tiny():
    """Weights and running statistics by test_multi_scale_evaluate_images_vs_oracle's recipe; two 256x256 frames."""
    from oracle import model as om
    from rrnet_amd.models.rrnet import RRNet
    from tests.helpers import det_fill
    model = RRNet(_cfg())
    sd = det_fill({k: tuple(v.shape) for k, v in model.state_dict().items()}, 80)
    for i in range(2):
        sd["hm.detect_layer.%d.1.bias" % i].fill_(-2.19)
        sd["wh.detect_H_layer.%d.0.conv.bias" % i].fill_(3.0)
        sd["wh.detect_W_layer.%d.0.conv.bias" % i].fill_(3.0)
    sd["head_detector.regressor.weight"] = sd["head_detector.regressor.weight"] * 0.05
    rng = np.random.default_rng(3)
    frames = torch.from_numpy(rng.integers(0, 256, (2, 256, 256, 3), dtype=np.uint8))
    om.BN_MOMENTUM = 1.0
    try:
        with torch.no_grad():
            pc = om.Params(sd, training=True)
            om.stage1(pc, om.hourglass_net(pc, _normalised(frames[:1])))
    finally:
        om.BN_MOMENTUM = 0.1
    model.load_state_dict(sd)
    return model.cuda().to(memory_format=torch.channels_last).eval(), sd, frames


def _well_formed(boxes, frame_off, nframes):
    fo = frame_off.cpu().numpy()
    rows = boxes.cpu().numpy()
    assert fo.shape == (nframes + 1,) and fo[0] == 0 and fo[-1] == rows.shape[0]
    assert np.all(np.diff(fo) >= 0)
    assert rows.shape[1] == 6 and np.all(np.isfinite(rows))
    for f in range(nframes):
        assert np.all(np.diff(rows[fo[f]:fo[f + 1], 4]) <= 0)
    assert np.all((rows[:, 5] >= 1) & (rows[:, 5] <= 10))
    return rows, fo


def test_detect_frames_matches_per_frame_evaluation(tiny):
    from rrnet_amd import inference
    from rrnet_amd.operators.rrnet_operator import RRNetOperator
    model, _, frames = tiny
    cfg = _cfg()
    boxes, frame_off = inference.detect_frames(model, frames.cuda(), cfg.Val.scales, MEAN, STD, nms=True)
    rows, fo = _well_formed(boxes, frame_off, 2)
    ns = SimpleNamespace(cfg=cfg, model=model)
    ns.generate_bbox = types.MethodType(RRNetOperator.generate_bbox, ns)
    ns._ext_nms = RRNetOperator._ext_nms
    ns._ext_nms_device = RRNetOperator._ext_nms_device
    host = _normalised(frames)
    for f in range(2):
        with torch.no_grad():
            ref = RRNetOperator.evaluate_images(ns, host[f:f + 1].cuda()).numpy()
        got = rows[fo[f]:fo[f + 1]]
        used = np.zeros(got.shape[0], bool)
        hits = 0
        for i in range(ref.shape[0]):
            lo, hi = max(0, i - 40), min(got.shape[0], i + 41)
            cand = np.where(~used[lo:hi] & (np.abs(got[lo:hi, 4] - ref[i, 4]) < 1e-4) & (got[lo:hi, 5] == ref[i, 5]) &
                            np.all(np.abs(got[lo:hi, :4] - ref[i, :4]) < 5e-2 + 1e-3 * np.abs(ref[i, :4]), axis=1))[0]
            if cand.size:
                used[lo + cand[0]] = True
                hits += 1
        print("frame %d: %d rows against %d per-frame rows, %d matched" % (f, got.shape[0], ref.shape[0], hits))
        assert ref.shape[0] > 0
        assert abs(got.shape[0] - ref.shape[0]) <= max(2, ref.shape[0] // 200), (got.shape, ref.shape)
        assert hits >= 0.98 * ref.shape[0], (hits, ref.shape[0])


def test_detect_frames_raw_and_bf16_are_well_formed(tiny):
    from rrnet_amd import inference
    from rrnet_amd.models.rrnet import RRNet
    model, sd, frames = tiny
    boxes, frame_off = inference.detect_frames(model, frames.cuda(), [1, 1.25, 1.5], MEAN, STD, nms=False)
    rows, fo = _well_formed(boxes, frame_off, 2)
    assert np.all(np.diff(fo) <= 3 * 1500) and fo[-1] > 0
    m16 = RRNet(_cfg(bf16=True))
    m16.load_state_dict(sd)
    m16 = m16.cuda().to(memory_format=torch.channels_last).eval()
    boxes, frame_off = inference.detect_frames(m16, frames.cuda(), [1, 1.25, 1.5], MEAN, STD, nms=True)
    rows, fo = _well_formed(boxes, frame_off, 2)
    assert fo[-1] > 0

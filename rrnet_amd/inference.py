"""Batched inference post-process: heat-map decode -> stage-1 NMS -> RoIAlign -> re-regression head ->
stage-2 boxes -> score filter -> per-class gaussian Soft-NMS -> per-frame score order.

This is what `RRNet.forward` (after the backbone and stage-1 heads, models/rrnet.py:30-54) followed by the
single-scale body of `RRNetOperator.evaluation_process` (operators/rrnet_operator.py:262-279: generate_bbox,
`score > 0.01`, sort, `_ext_nms`, sort) computes for ONE frame with Python loops over classes and a D2H copy
per class — here for a whole batch of frames with one launch per stage and two host reads per batch (the RoI
count that sizes the head's tensors, and the final box count).

Ordering note: decode emits rows score-descending, grouping / hard NMS are stable, so inside every
(frame, class) segment the stage-2 boxes already are in the order the reference's global
`torch.sort(score, descending=True)` + `pred_bbox[:, 5] == cls` selection hands to `soft_nms`
(ties: torch.sort leaves them unspecified; here they keep decode order).

`detect_frames` / `Detector` are the entry point from raw frames: the multi-scale evaluation body
(operators/rrnet_operator.py:256-279) for a batch of equal-size uint8 frames.  `detect_frames_centernet` /
`CenterNetFrameDetector` are the same for CenterNet (operators/centernet_operator.py:262-285: every scale once flipped
and once plain, both in one model pass).  `detect_frames_retinanet` / `RetinaNetFrameDetector` are RetinaNet's single-scale
evaluation body (operators/retinanet_operator.py:243-255): decode, score sort, the reference's hard NMS.
`plan_tiles` / `detect_tiled_retinanet` / `finish_tiles` are tiled inference for RetinaNet: overlapping tiles of the
training size cut out of frames of any sizes, detected as one batch of equal-size images (no counterpart in the reference)."""
import os

import torch

from rrnet_amd import ops
from rrnet_amd.ext.nms.nms_wrapper import soft_nms_segments
from rrnet_amd.models.rrnet import stage1_proposals


# RoIAlign processing order: per-frame spatial sort (rr_roi_spatial_order).  Off by default since round 3: with eight
# footprint pixels in flight per wave the kernel runs as fast in decode order (2.66-2.73 ms against 2.62-2.87 ms sorted, per
# 128 frames at config 5) and the sort is a launch of its own (0.05 ms).  Module constant; no switch.
ROI_SPATIAL_ORDER = False


@torch.no_grad()
def refine_frames(hm, wh, offset, feat, head_detector, k=1500, num_classes=10, scale_factor=4, score_thr=0.01,
                  nms_type='nms', relu_feat=True):
    """hm [B,C,H,W] logits, wh / offset [B,2,H,W], feat [B,256,H,W] (pre-ReLU backbone output unless
    relu_feat=False), head_detector = FasterRCNNDetector in eval mode.
    -> boxes [n,6] = x,y,w,h,score,cls+1 (image coordinates, frames back to back, each score-descending),
       frame_off int32 [B+1] (device).  Raises ZeroDivisionError where the reference's soft_nms would."""
    b = hm.shape[0]
    rois, scores, clses, row_off = stage1_proposals(hm, wh, offset, k, num_classes, nms_type, True, want_offsets=True)
    feat = ops.to_nhwc(feat)
    if relu_feat:
        feat = ops.relu_fwd(feat)
    # RoIs of a frame in spatial order (overlapping footprints back to back on one XCD: shared rows come from L2)
    order = ops.roi_spatial_order(rois, row_off[::num_classes].contiguous()) if ROI_SPATIAL_ORDER else None
    roi_feat = ops.roi_align_fwd(feat, rois, (3, 3), order=order)
    reg = head_detector(roi_feat)                                   # [R,4]
    boxes6, seg_len = ops.refine_boxes(rois, reg, scores, clses, row_off, scale_factor, score_thr)
    n_out, err = soft_nms_segments(boxes6, row_off, k, sigma=0.5, Nt=0.7, threshold=0.1, method=2, seg_len=seg_len,
                                   check=False)
    out6, frame_off = ops.finalize_frames(boxes6, row_off, n_out, b, num_classes, k)
    fo = frame_off.cpu()                                            # one sync: final counts (+ error flag)
    if int(err.item()) != 0:
        raise ZeroDivisionError("float division")
    return out6[:int(fo[-1])], frame_off


def _frame_ranges(bxyxy, b):
    """Row range of every frame in the model's packed RoI list (column 0 = frame index, ascending) -> int32 [b+1]."""
    ids = torch.arange(b + 1, dtype=torch.float32, device=bxyxy.device)
    return torch.searchsorted(bxyxy[:, 0].contiguous(), ids).to(torch.int32)


def _vec3(v, device):
    if torch.is_tensor(v):
        return v.to(device=device, dtype=torch.float32).contiguous()
    return torch.tensor([float(x) for x in v], dtype=torch.float32, device=device)


def _check_frames(what, frames_u8):
    """The frame-tensor checks of the detect_frames* entry points; `what` is the caller's name in the messages."""
    if not torch.is_tensor(frames_u8) or frames_u8.dtype != torch.uint8:
        raise TypeError("%s: frames must be a uint8 tensor [B,H,W,3], got %s"
                        % (what, frames_u8.dtype if torch.is_tensor(frames_u8) else type(frames_u8).__name__))
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError("%s: frames must be [B,H,W,3], got %s" % (what, tuple(frames_u8.shape)))


def _soft_nms_by_class(merged, count, num_classes):
    """`_ext_nms` up to the Soft-NMS itself on merged [B,K,6] xywh rows, count int32 [B]: stable score sort into xyxy rows
    (x2 = x + w as the kernel forms it), stable grouping by class (the padding rows, class -1, are dropped there), per-class
    gaussian Soft-NMS (sigma 0.5, Nt 0.7, threshold 0.1).  -> (rows [B*K,6], seg_off, n_out, err), all on the device."""
    ordered = ops.sort_frames_by_score(merged, count, xyxy=True)
    grouped, seg_off, seg_len = ops.group_by_class(ordered, num_classes, cls_base=1)
    rows = grouped.view(-1, 6)
    n_out, err = soft_nms_segments(rows, seg_off, merged.shape[1], sigma=0.5, Nt=0.7, threshold=0.1, method=2,
                                   seg_len=seg_len, check=False)
    return rows, seg_off, n_out, err


def _hard_nms_tail(rows, count, counts, nms_thresh):
    """RetinaNet's tail on rows [B,K,6], count int32 [B] (counts: its host copy, not all zero): stable score sort,
    rr_nms_frames ("+1" IoU, suppression at IoU > nms_thresh), rr_pack_frames.  -> (boxes [n,6], frame_off int32 [B+1]).
    One host read: the final offsets."""
    most = int(counts.max())
    cand_off = ops.seg_prefix(count)
    ordered = ops.sort_frames_by_score(rows, count, out_off=cand_off)
    keep, kept = ops.nms_frames(ordered, cand_off, most, nms_thresh)
    out6, frame_off = ops.pack_frames(ordered, cand_off, keep, kept, most, out_rows=int(counts.sum()))
    fo = frame_off.cpu()                                            # host read: the final offsets
    return out6[:int(fo[-1])], frame_off


@torch.no_grad()
def detect_frames(model, frames_u8, scales, mean, std, *, nms, k=1500, score_thr=0.01, scale_factor=4, num_classes=10,
                  timer=None):
    """Multi-scale detection (operators/rrnet_operator.py:256-279) on B equal-size frames.
    frames_u8 uint8 [B,H,W,3] on the device (RGB as PIL decodes it), model = RRNet in eval mode, scales = the list of
    cfg.Val.scales, mean / std = Normalize's, nms = `not cfg.Val.auto_test`.
    -> boxes [n,6] = x,y,w,h,score,cls+1 (frames back to back, each score-descending), frame_off int32 [B+1]; both on
    the device.  Per frame: every scale's generate_bbox rows (filtered by `score > score_thr` when nms), divided by the
    scale, concatenated in scale order, stably sorted by score; with nms, per-class gaussian Soft-NMS (sigma 0.5, Nt 0.7,
    threshold 0.1) and a second stable sort.  Host reads: the model's RoI count per scale and the final counts.
    Raises ValueError when len(scales)*k exceeds the LDS sort's 16384 rows, ZeroDivisionError where soft_nms would.
    timer (optional): called as timer(stage) with 'prepare' / 'model' / 'post' after the launches of each stage."""
    _check_frames("detect_frames", frames_u8)
    scales = list(scales)
    rows_per_frame = len(scales) * int(k)
    if rows_per_frame > ops.DETECT_MAX_ROWS or rows_per_frame <= 0:
        raise ValueError("detect_frames: %d scales x %d boxes = %d rows per frame (limit %d)"
                         % (len(scales), k, rows_per_frame, ops.DETECT_MAX_ROWS))
    from rrnet_amd import _C
    _C.require_cuda(frames_u8)
    tick = timer if timer is not None else (lambda stage: None)
    dev = frames_u8.device
    frames_u8 = frames_u8.contiguous()
    b = frames_u8.shape[0]
    mean, std = _vec3(mean, dev), _vec3(std, dev)
    merged, count = ops.merge_buffers(b, rows_per_frame, dev)
    for s in scales:
        x = ops.prepare_frames(frames_u8, mean, std, s)
        tick('prepare')
        _, _, _, reg, bxyxy, scores, clses = model(x, k=k)
        tick('model')
        ops.merge_scales(bxyxy, reg, scores, clses.float(), _frame_ranges(bxyxy, b), s, merged, count,
                         scale=scale_factor, score_thr=score_thr if nms else None)
        tick('post')
    out = finish_frames(merged, count, nms, num_classes)
    tick('post')
    return out


@torch.no_grad()
def finish_frames(merged, count, nms, num_classes=10):
    """The cross-scale tail of detect_frames on the merged rows (ops.merge_buffers / ops.merge_scales): merged [B,K,6]
    xywh rows, count int32 [B] -> (boxes [n,6], frame_off int32 [B+1]).  First stable sort by score; with nms the
    per-class Soft-NMS of `_ext_nms` and the second sort.  One host read (final counts, error flag)."""
    b, rows_per_frame, _ = merged.shape
    if not nms:
        frame_off = ops.seg_prefix(count)
        out6 = ops.sort_frames_by_score(merged, count, out_off=frame_off)
        fo = frame_off.cpu()                                        # the one sync: final counts
        return out6[:int(fo[-1])], frame_off
    rows, seg_off, n_out, err = _soft_nms_by_class(merged, count, num_classes)
    out6, frame_off = ops.finalize_frames(rows, seg_off, n_out, b, num_classes, rows_per_frame)
    frame_off = frame_off.contiguous()
    fo = frame_off.cpu()                                            # the one sync: final counts (+ error flag)
    if int(err.item()) != 0:
        raise ZeroDivisionError("float division")
    return out6[:int(fo[-1])], frame_off


class _LoadedModel:
    """What the three frame detectors share: model_cls(cfg) with a reference-format state dict (a path or a dict, with or
    without `module.` prefixes; checkpoint=None keeps the initial weights) on the device, channels-last, in eval mode;
    mean / std from cfg.Val.transforms."""

    def __init__(self, model_cls, cfg, checkpoint, device):
        from rrnet_amd.datasets.augment import chain_params
        self.cfg = cfg
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        model = model_cls(cfg)
        if checkpoint is not None:
            sd = torch.load(checkpoint, map_location='cpu') if isinstance(checkpoint, (str, os.PathLike)) else checkpoint
            sd = {(key[7:] if key.startswith('module.') else key): v for key, v in sd.items()}
            model.load_state_dict(sd)
        self.model = model.to(self.device).to(memory_format=torch.channels_last).eval()
        p = chain_params(cfg.Val.transforms)
        self.mean, self.std = p["mean"], p["std"]


class Detector(_LoadedModel):
    """RRNet from a reference-format checkpoint, ready for `detect`: builds RRNet(cfg) (stage-1 NMS as
    cfg.Model.nms_type_for_stage1 / nms_per_class_for_stage1 say, bf16 as cfg.Model.bf16 says), loads the state dict
    (checkpoint=None keeps the initial weights) and sets eval mode."""

    def __init__(self, cfg, checkpoint=None, device=None):
        from rrnet_amd.models.rrnet import RRNet
        super().__init__(RRNet, cfg, checkpoint, device)
        self.scale_factor = int(cfg.Train.scale_factor)
        self.num_classes = int(cfg.num_classes)

    def detect(self, frames_u8, scales=None, nms=None, k=1500, timer=None):
        """frames uint8 [B,H,W,3] on the device -> (boxes [n,6], frame_off int32 [B+1]) as detect_frames."""
        scales = self.cfg.Val.scales if scales is None else scales
        nms = (not self.cfg.Val.auto_test) if nms is None else bool(nms)
        return detect_frames(self.model, frames_u8, scales, self.mean, self.std, nms=nms, k=k,
                             scale_factor=self.scale_factor, num_classes=self.num_classes, timer=timer)


@torch.no_grad()
def detect_frames_centernet(model, frames_u8, scales, mean, std, *, nms, flip=True, k=250, score_thr=0.01, scale_factor=4,
                            num_classes=10, timer=None):
    """CenterNet's multi-scale flip evaluation (operators/centernet_operator.py:262-285) on B equal-size frames.
    frames_u8 uint8 [B,H,W,3] on the device, model = CenterNet in eval mode (fp32: CenterNet has no bf16 scope), scales =
    cfg.Val.scales, mean / std = Normalize's, nms = `not cfg.Val.auto_test`, flip=False drops the flipped passes.
    Per scale: one prepare (plain images 0..B-1, mirrored B..2B-1), ONE model pass on the 2B images, one decode of the last
    stack's maps (k rows per image, box_mode 1), one merge.  A frame's rows are concatenated as the reference does: scale
    by scale, flipped before plain, each filtered by `score > score_thr`, the flipped rows un-mirrored, x,y,w,h / scale.
    -> (boxes [n,6], frame_off int32 [B+1]) on the device, frames back to back.
      nms=False: x,y,w,h,score,cls+1, each frame stably sorted by score.
      nms=True: `_ext_nms` (:222-236) after that sort: per-class gaussian Soft-NMS (sigma 0.5, Nt 0.7, threshold 0.1).
        As in the reference the rows stay x1,y1,x2,y2,score,cls+1 (x2 = x + w) in class-ascending order; no second sort.
    Host reads: none per scale; at the end the final counts (with nms also the packed row count and the error flag).
    Raises ValueError when len(scales) * (2 if flip else 1) * k exceeds the LDS sort's 16384 rows, ZeroDivisionError where
    soft_nms would.  timer as in detect_frames."""
    _check_frames("detect_frames_centernet", frames_u8)
    scales = list(scales)
    halves = 2 if flip else 1
    rows_per_frame = len(scales) * halves * int(k)
    if rows_per_frame > ops.DETECT_MAX_ROWS or rows_per_frame <= 0:
        raise ValueError("detect_frames_centernet: %d scales x %d images x %d boxes = %d rows per frame (limit %d)"
                         % (len(scales), halves, k, rows_per_frame, ops.DETECT_MAX_ROWS))
    from rrnet_amd import _C
    _C.require_cuda(frames_u8)
    tick = timer if timer is not None else (lambda stage: None)
    dev = frames_u8.device
    frames_u8 = frames_u8.contiguous()
    b = frames_u8.shape[0]
    mean, std = _vec3(mean, dev), _vec3(std, dev)
    merged, count = ops.merge_buffers(b, rows_per_frame, dev)
    for s in scales:
        x = (ops.prepare_frames_pair if flip else ops.prepare_frames)(frames_u8, mean, std, s)
        tick('prepare')
        hms, whs, regs = model(x)
        tick('model')
        rows = ops.decode_topk(ops.to_nhwc(hms[-1]), ops.to_nhwc(whs[-1]), ops.to_nhwc(regs[-1]), int(k), is_logits=True,
                               box_mode=1, scale=float(scale_factor))
        ops.merge_ctnet(rows, b, x.shape[3], s, merged, count, pair=flip, score_thr=score_thr)
        tick('post')
    out = finish_frames_centernet(merged, count, nms, num_classes)
    tick('post')
    return out


@torch.no_grad()
def finish_frames_centernet(merged, count, nms, num_classes=10):
    """The cross-scale tail of detect_frames_centernet on the merged rows: merged [B,K,6] xywh rows, count int32 [B] ->
    (boxes [n,6], frame_off int32 [B+1]).  Without nms finish_frames' stable sort; with nms `_ext_nms`
    (operators/centernet_operator.py:222-236) behind that sort: per class ascending the gaussian Soft-NMS on x1,y1,x2,y2
    rows, concatenated — the rows stay xyxy and are not sorted again, as in the reference."""
    if not nms:
        return finish_frames(merged, count, False, num_classes)
    rows, seg_off, n_out, err = _soft_nms_by_class(merged, count, num_classes)
    _, _, _, out6, out_off = ops.pack_segments(rows, seg_off, n_out, num_classes, want_rois=False, want_rows=True,
                                               want_offsets=True)   # its host read: the packed row count
    frame_off = out_off[::num_classes].contiguous()
    if int(err.item()) != 0:
        raise ZeroDivisionError("float division")
    return out6, frame_off


class CenterNetFrameDetector(_LoadedModel):
    """CenterNet from a reference-format checkpoint, ready for `detect`: the counterpart of Detector.  Builds CenterNet(cfg),
    loads the state dict (with or without `module.` prefixes; checkpoint=None keeps the initial weights), sets eval mode
    and channels-last; mean / std come from cfg.Val.transforms.  fp32 only."""

    def __init__(self, cfg, checkpoint=None, device=None):
        from rrnet_amd.models.centernet import CenterNet
        super().__init__(CenterNet, cfg, checkpoint, device)
        self.scale_factor = int(cfg.Train.scale_factor)
        self.num_classes = int(cfg.num_classes)

    def detect(self, frames_u8, scales=None, nms=None, flip=True, k=250, timer=None):
        """frames uint8 [B,H,W,3] on the device -> (boxes [n,6], frame_off int32 [B+1]) as detect_frames_centernet."""
        scales = self.cfg.Val.scales if scales is None else scales
        nms = (not self.cfg.Val.auto_test) if nms is None else bool(nms)
        return detect_frames_centernet(self.model, frames_u8, scales, self.mean, self.std, nms=nms, flip=flip, k=k,
                                       scale_factor=self.scale_factor, num_classes=self.num_classes, timer=timer)


RETINA_MAX_CANDIDATES = ops.DETECT_MAX_ROWS     # candidates of one frame the batched score sort holds


@torch.no_grad()
def detect_frames_retinanet(model, frames_u8, mean, std, anchors, *, score_thr=0.1, nms_thresh=0.3, timer=None):
    """RetinaNet's evaluation body (operators/retinanet_operator.py:243-255, with RetinaNetOperator's two deviations: the
    kept indices select the rows, and every image of the batch is evaluated) on B equal-size frames.
    frames_u8 uint8 [B,H,W,3] on the device, model = RetinaNet in eval mode (fp32), mean / std = Normalize's (the validation
    chain is ToTensor, Normalize: no resize), anchors [A,4] xyxy on the device for this frame size.
    One prepare at the frames' own size, one model pass, rr_retina_decode_frames (at most 16384 rows per frame), the stable
    score sort, rr_nms_frames ("+1" IoU, suppression at IoU > nms_thresh) and the pack.
    -> (boxes [n,6] = x,y,w,h,prob,cls+1, frames back to back, each score-descending; frame_off int32 [B+1]), both on the
    device: per frame the rows RetinaNetOperator.evaluate_images returns.  Host reads: the candidate counts and the final
    offsets.  Raises ValueError when a frame has more than 16384 candidates (evaluate_images' refusal), before the sort.
    timer as in detect_frames."""
    _check_frames("detect_frames_retinanet", frames_u8)
    from rrnet_amd import _C
    _C.require_cuda(frames_u8)
    tick = timer if timer is not None else (lambda stage: None)
    dev = frames_u8.device
    frames_u8 = frames_u8.contiguous()
    b = frames_u8.shape[0]
    mean, std = _vec3(mean, dev), _vec3(std, dev)
    x = ops.prepare_frames(frames_u8, mean, std, 1)
    tick('prepare')
    loc_pre, cls_pre = model(x)
    tick('model')
    a = cls_pre.shape[1]
    if tuple(anchors.shape) != (a, 4):
        raise ValueError("detect_frames_retinanet: %d predictions per frame against %s anchors" % (a, tuple(anchors.shape)))
    limit = RETINA_MAX_CANDIDATES
    rows, count = ops.retina_decode_frames(cls_pre, loc_pre, anchors, score_thr, k=min(a, limit))
    counts = count.cpu()                                            # host read: the candidate counts
    over = torch.nonzero(counts > limit)
    if over.numel():
        f = int(over[0, 0])
        raise ValueError("detect_frames_retinanet: frame %d has %d candidates above the score threshold; the score sort "
                         "accepts %d per frame" % (f, int(counts[f]), limit))
    if int(counts.max()) == 0:
        out = rows.new_zeros((0, 6)), torch.zeros(b + 1, dtype=torch.int32, device=dev)
    else:
        out = _hard_nms_tail(rows, count, counts, nms_thresh)
    tick('post')
    return out


def _tile_hw(tile):
    if isinstance(tile, (tuple, list)):
        if len(tile) != 2:
            raise ValueError("tile must be N or (H, W), got %r" % (tile,))
        return int(tile[0]), int(tile[1])
    return int(tile), int(tile)


def plan_tiles(h, w, tile, overlap):
    """Origins (y0, x0) of the overlapping tiles that cover an h x w frame, row-major (y outer).  tile = (th, tw) or N,
    0 <= overlap < min(th, tw).  Along an axis of length L with tile size t the step is s = t - overlap; the origins are
    0, s, 2s, ... while origin + t < L, then a last origin L - t (L == t: [0]).  Every tile has the full size and lies
    inside the frame: nothing is padded and no edge tile is smaller, so t > L raises ValueError."""
    th, tw = _tile_hw(tile)
    h, w, overlap = int(h), int(w), int(overlap)
    if th <= 0 or tw <= 0:
        raise ValueError("plan_tiles: tile %dx%d" % (th, tw))
    if not 0 <= overlap < min(th, tw):
        raise ValueError("plan_tiles: overlap %d must be in [0, %d) for a %dx%d tile" % (overlap, min(th, tw), th, tw))
    if th > h or tw > w:
        raise ValueError("plan_tiles: a %dx%d frame is smaller than the %dx%d tile (tiles are neither padded nor shrunk)"
                         % (h, w, th, tw))

    def axis(length, t):
        step, origins, o = t - overlap, [], 0
        while o + t < length:
            origins.append(o)
            o += step
        return origins + [length - t]

    return [(y0, x0) for y0 in axis(h, th) for x0 in axis(w, tw)]


TILE_MAX_ROWS = ops.DETECT_MAX_ROWS             # merged rows of one frame the batched score sort holds


@torch.no_grad()
def finish_tiles(rows, count_in, tiles, sizes, tile, in_size, zoom=1.0, margin=0.0, nms_thresh=0.3):
    """What follows the model in detect_tiled_retinanet: rows [T,k,6] = every tile's candidates (x,y,w,h,prob,cls+1 in the
    model's input coordinates, in_size = (oh, ow)) as rr_retina_decode_frames writes them, count_in int32 [T] its true
    counts; tiles = T host rows (frame, y0, x0) sorted by frame, sizes = (H, W) of every frame, tile = (th, tw).
    rr_merge_tiles (div = float32(zoom), margin as ops.merge_tiles explains it) brings the rows into per-frame blocks in
    frame coordinates; then detect_frames_retinanet's tail: stable score sort, rr_nms_frames, rr_pack_frames.
    -> (boxes [n,6], frame_off int32 [F+1]) on the device.  Host reads: the tile counts, the frame counts, the final
    offsets.  Raises ValueError, before the sort, for a tile with more than k candidates and for a frame with more than
    16384 merged rows."""
    import numpy as np
    t, k, _ = rows.shape
    nframes = len(sizes)
    dev = rows.device
    table, tile_off = ops.check_tiles(tiles, sizes, tile)
    if table.shape[0] != t:
        raise ValueError("finish_tiles: %d tiles in the table, rows of %d" % (table.shape[0], t))
    empty = (rows.new_zeros((0, 6)), torch.zeros(nframes + 1, dtype=torch.int32, device=dev))
    if t == 0 or nframes == 0:
        return empty
    tile_counts = count_in.cpu().numpy().astype(np.int64)           # host read: the tile counts
    over = np.nonzero(tile_counts > k)[0]
    if over.size:
        i = int(over[0])
        raise ValueError("finish_tiles: tile %d (frame %d, origin y %d x %d) has %d candidates above the score threshold; a "
                         "tile's buffer holds %d" % (i, table[i, 0], table[i, 1], table[i, 2], tile_counts[i], k))
    bound = [int(np.clip(tile_counts[tile_off[f]:tile_off[f + 1]], 0, None).sum()) for f in range(nframes)]
    if max(bound) == 0:
        return empty
    limit = TILE_MAX_ROWS

    def refuse_over(per_frame):
        for f, n in enumerate(per_frame):
            if n > limit:
                raise ValueError("finish_tiles: frame %d has %d merged rows from its %d tiles; the score sort accepts %d per "
                                 "frame" % (f, n, int(tile_off[f + 1] - tile_off[f]), limit))

    if not float(margin) > 0:
        refuse_over(bound)                                          # nothing leaves: the sums are the merged counts
    merged, count = ops.merge_buffers(nframes, min(max(bound), limit), dev)
    ops.merge_tiles(rows, count_in, table, sizes, tile, in_size, np.float32(zoom), margin, merged, count)
    counts = count.cpu()                                            # host read: the frame counts
    refuse_over(counts.tolist())
    if int(counts.max()) == 0:
        return empty
    return _hard_nms_tail(merged, count, counts, nms_thresh)


def _tiles_of(frames, tile, overlap):
    """-> (sizes, host table [(frame, y0, x0), ...]) of plan_tiles over every frame, frames in order."""
    sizes = ops._frame_sizes(frames)
    table = []
    for f, (h, w) in enumerate(sizes):
        try:
            table += [(f, y0, x0) for y0, x0 in plan_tiles(h, w, tile, overlap)]
        except ValueError as e:
            raise ValueError("frame %d: %s" % (f, e)) from None
    return sizes, table


def _check_tiled_frames(what, frames):
    tensors = [frames] if torch.is_tensor(frames) else list(frames)
    if not tensors:
        raise ValueError("%s: no frames" % what)
    for fr in tensors:
        if not torch.is_tensor(fr) or fr.dtype != torch.uint8:
            raise TypeError("%s: frames must be uint8 tensors ([B,H,W,3] or a list of [H,W,3]), got %s"
                            % (what, fr.dtype if torch.is_tensor(fr) else type(fr).__name__))
    return tensors


@torch.no_grad()
def detect_tiled_retinanet(model, frames, mean, std, anchors, *, tile, overlap, zoom=1.0, margin=0.0, tile_batch=8,
                           score_thr=0.1, nms_thresh=0.3, timer=None):
    """Tiled inference with RetinaNet (the builder's own feature; the reference has none): every frame is cut into
    overlapping tiles of one size (plan_tiles), each tile is resized by `zoom` and detected on its own, the boxes are moved
    back into the frame and the duplicates the overlap produces are suppressed by the NMS.
    frames: a list of uint8 [H_i,W_i,3] device tensors of ANY sizes, or one uint8 [B,H,W,3] tensor — tiles of one size are
    equal-size images whatever frame they come from, so nothing is padded and no batch is cut short.  tile = N or (th, tw),
    anchors [A,4] for the model's input size (floor(th*zoom), floor(tw*zoom)).
    One rr_prepare_tiles call; model passes over the tiles `tile_batch` at a time (a frame's tiles may straddle two passes);
    rr_retina_decode_frames per pass into slices of one [T,k,6] buffer, k = min(A, 16384); finish_tiles.
    margin (in input pixels, 0 = off): rows within `margin` of a tile side that is not on the frame's border leave — the
    boxes that side has cut.  The neighbouring tile sees such an object whole only if `overlap` is larger than margin / zoom
    plus the object's size: choose overlap accordingly.
    -> (boxes [n,6] = x,y,w,h,prob,cls+1 in frame coordinates, frames back to back, each score-descending; frame_off int32
    [F+1]) on the device, as detect_frames_retinanet.  Host reads: three (finish_tiles).  timer as in detect_frames."""
    import math
    tensors = _check_tiled_frames("detect_tiled_retinanet", frames)
    from rrnet_amd import _C
    _C.require_cuda(*tensors)
    tick = timer if timer is not None else (lambda stage: None)
    dev = tensors[0].device
    th, tw = _tile_hw(tile)
    tile_batch = int(tile_batch)
    if tile_batch < 1:
        raise ValueError("detect_tiled_retinanet: tile_batch %d" % tile_batch)
    if not float(zoom) > 0 or not float(margin) >= 0:
        raise ValueError("detect_tiled_retinanet: zoom %r, margin %r" % (zoom, margin))
    sizes, table = _tiles_of(frames, (th, tw), overlap)
    oh, ow = int(math.floor(th * zoom)), int(math.floor(tw * zoom))
    mean, std = _vec3(mean, dev), _vec3(std, dev)
    x = ops.prepare_tiles(frames, table, (th, tw), zoom, mean, std)
    tick('prepare')
    t = len(table)
    rows = count_in = None
    for i in range(0, t, tile_batch):
        loc_pre, cls_pre = model(x[i:i + tile_batch])
        tick('model')
        if rows is None:
            a = cls_pre.shape[1]
            if tuple(anchors.shape) != (a, 4):
                raise ValueError("detect_tiled_retinanet: %d predictions per %dx%d tile against %s anchors"
                                 % (a, oh, ow, tuple(anchors.shape)))
            k = min(a, TILE_MAX_ROWS)
            rows = torch.zeros((t, k, 6), dtype=torch.float32, device=dev)
            count_in = torch.zeros(t, dtype=torch.int32, device=dev)
        _, c = ops.retina_decode_frames(cls_pre, loc_pre, anchors, score_thr, k=k, rows=rows[i:i + tile_batch])
        count_in[i:i + c.numel()] = c
        tick('post')
    out = finish_tiles(rows, count_in, table, sizes, (th, tw), (oh, ow), zoom, margin, nms_thresh)
    tick('post')
    return out


class RetinaNetFrameDetector(_LoadedModel):
    """RetinaNet from a reference-format checkpoint, ready for `detect`: the counterpart of CenterNetFrameDetector.  Builds
    RetinaNet(cfg), loads the state dict (with or without `module.` prefixes; checkpoint=None keeps the initial weights),
    sets eval mode and channels-last; mean / std come from cfg.Val.transforms; the anchors are Anchors(sizes=(16, 64, 128)),
    cached per frame size on the device.  fp32 only."""

    def __init__(self, cfg, checkpoint=None, device=None):
        from rrnet_amd.models.retinanet import RetinaNet
        from rrnet_amd.modules.anchor import Anchors
        super().__init__(RetinaNet, cfg, checkpoint, device)
        self.anchor_maker = Anchors(sizes=(16, 64, 128))
        self._anchors = {}

    def anchors(self, size):
        key = (int(size[0]), int(size[1]))
        hit = self._anchors.get(key)
        if hit is None:
            hit = self._anchors[key] = self.anchor_maker(key).to(self.device)
        return hit

    def detect(self, frames_u8, score_thr=0.1, nms_thresh=0.3, timer=None):
        """frames uint8 [B,H,W,3] on the device -> (boxes [n,6], frame_off int32 [B+1]) as detect_frames_retinanet."""
        return detect_frames_retinanet(self.model, frames_u8, self.mean, self.std, self.anchors(frames_u8.shape[1:3]),
                                       score_thr=score_thr, nms_thresh=nms_thresh, timer=timer)

    def detect_tiled(self, frames, tile, overlap, zoom=1.0, margin=0.0, tile_batch=8, score_thr=0.1, nms_thresh=0.3,
                     timer=None):
        """frames (a list of uint8 [H_i,W_i,3] device tensors or one [B,H,W,3]) -> (boxes [n,6], frame_off int32 [F+1]) as
        detect_tiled_retinanet; the anchors are those of the model's input size floor(tile * zoom), cached as detect's."""
        import math
        th, tw = _tile_hw(tile)
        anchors = self.anchors((int(math.floor(th * zoom)), int(math.floor(tw * zoom))))
        return detect_tiled_retinanet(self.model, frames, self.mean, self.std, anchors, tile=(th, tw), overlap=overlap,
                                      zoom=zoom, margin=margin, tile_batch=tile_batch, score_thr=score_thr,
                                      nms_thresh=nms_thresh, timer=timer)

    @torch.no_grad()
    def threshold_for_tile_rows(self, frames, tile, overlap, zoom, rows_per_tile, tile_batch=8):
        """threshold_for_rows for the tiled path: model passes over these frames' tiles -> (threshold, the largest number of
        candidates a tile keeps at it).  Not part of the detection path."""
        th, tw = _tile_hw(tile)
        _, table = _tiles_of(frames, (th, tw), overlap)
        x = ops.prepare_tiles(frames, table, (th, tw), zoom, _vec3(self.mean, self.device), _vec3(self.std, self.device))
        best = torch.cat([torch.sigmoid(self.model(x[i:i + tile_batch])[1].float()).amax(dim=2)
                          for i in range(0, len(table), int(tile_batch))])      # [T,A]
        thr, kept = self._pick_threshold(best, rows_per_tile)
        return thr, int(kept.max())

    @staticmethod
    def _pick_threshold(best, rows):
        """best [N,A] = per image the largest class probability of every anchor -> (the smallest threshold at which
        `prob > thr` keeps at most `rows` anchors of any image, the number each image keeps at it)."""
        rows = min(int(rows), best.shape[1] - 1)
        thr = float(best.topk(rows + 1, dim=1).values[:, -1].max())
        return thr, (best > thr).sum(dim=1)

    @torch.no_grad()
    def threshold_for_rows(self, frames_u8, rows_per_frame):
        """A score threshold for models whose scores mean nothing (random weights: every anchor sits near 0.5 and passes
        0.1, which the score sort refuses): one model pass on these frames -> (threshold, candidates per frame at it), the
        threshold being the smallest at which no frame keeps more than rows_per_frame anchors.  For smoke runs and the
        benchmark, not part of the detection path."""
        x = ops.prepare_frames(frames_u8.contiguous(), _vec3(self.mean, self.device), _vec3(self.std, self.device), 1)
        _, cls_pre = self.model(x)
        thr, kept = self._pick_threshold(torch.sigmoid(cls_pre.float()).amax(dim=2), rows_per_frame)   # [B,A]
        return thr, kept.tolist()

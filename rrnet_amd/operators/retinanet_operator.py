"""RetinaNetOperator — operators/retinanet_operator.py:16-265 of the reference on the MI355X path.  Same constructor /
make_anchor / criterion / training_process / transform_bbox / save_result / evaluation_process surface; underneath: the
HIP kernels of librrnet_hip.so (convolutions, max-pool, bilinear upsample-add), the anchor criterion as one autograd node
over rr_retina_assign / rr_retina_loss_* (RF.retina_criterion), the fused flat Adam, rr_retina_decode, the score sort and
rr_nms_sorted.  fp32, one process, one GPU.  With cfg.Val.device_batch >= 1 the evaluation runs batched on raw frames
(rrnet_amd.inference.detect_frames_retinanet); with cfg.Val.tile set beside it, on overlapping tiles
(rrnet_amd.inference.detect_tiled_retinanet).

Deviations from the reference, all in the evaluation (:227-265):
  * the reference indexes `pred_bbox` with what `nms()` returns (:254-255) — `nms()` returns the kept ROWS, not indices, so
    that line raises; here the kept indices select the rows;
  * it evaluates image 0 of every batch only (:248, :257); here every image of the batch is evaluated and written.
and one in the criterion: an annotation class outside [1, num_classes] sets no target bit (the reference would index
column -1 or raise)."""
import os

import numpy as np
import torch
import torch.optim as optim

from rrnet_amd import _C
from rrnet_amd import functional as RF
from rrnet_amd import ops
from rrnet_amd.datasets import make_dataloader
from rrnet_amd.flat import FlatAdam, FlatParams
from rrnet_amd.models.retinanet import RetinaNet
from rrnet_amd.modules.anchor import Anchors
from rrnet_amd.modules.loss.focalloss import FocalLoss
from .base_operator import BaseOperator, guard_options, make_lr_scheduler
from .centernet_operator import _released

NMS_THRESH = 0.3            # :254
SCORE_THRESH = 0.1          # :188
MAX_CANDIDATES = ops.DETECT_MAX_ROWS      # rows of one frame the score sort accepts (rr_nms_sorted takes 64 times as many)


class RetinaNetOperator(BaseOperator):
    def __init__(self, cfg):
        self.cfg = cfg
        if int(getattr(cfg.Distributed, "world_size", 1) or 1) > 1:
            # the two heads' weights are used once per pyramid level, three times per step; FlatParams.mark_ready counts a
            # parameter as finished after its first weight gradient and would launch its bucket's all-reduce while the
            # other two levels are still adding into it
            raise NotImplementedError("RetinaNetOperator: world_size > 1 is not supported: the shared heads' weights receive "
                                      "three gradient contributions per step and the flat buffer's bucketing would "
                                      "all-reduce a bucket after the first")
        model = RetinaNet(cfg).cuda(cfg.Distributed.gpu_id).to(memory_format=torch.channels_last)
        flat = FlatParams(model)
        self.optimizer = FlatAdam(flat, lr=cfg.Train.lr, **guard_options(cfg))
        self.lr_sch = make_lr_scheduler(cfg, self.optimizer)
        self.training_loader, self.validation_loader = make_dataloader(cfg, collate_fn='ctnet')
        super(RetinaNetOperator, self).__init__(cfg=self.cfg, model=model, lr_sch=self.lr_sch, flat=flat)
        self.anchor_maker = Anchors(sizes=(16, 64, 128))
        self._anchor_sets = {}
        self.anchors, self.anchors_widths, self.anchors_heights, self.anchors_ctr_x, self.anchors_ctr_y = \
            self.make_anchor(cfg.Train.crop_size)
        self.focal_loss = FocalLoss()
        self.main_proc_flag = cfg.Distributed.gpu_id == 0

    def make_anchor(self, size):
        """:39-45 -> (anchors [A,4] xyxy on the device, widths, heights, centre x, centre y); cached per image size."""
        key = (int(size[0]), int(size[1]))
        hit = self._anchor_sets.get(key)
        if hit is None:
            anchors = self.anchor_maker(key).cuda()
            widths = anchors[:, 2] - anchors[:, 0]
            heights = anchors[:, 3] - anchors[:, 1]
            hit = (anchors, widths, heights, anchors[:, 0] + 0.5 * widths, anchors[:, 1] + 0.5 * heights)
            self._anchor_sets[key] = hit
        return hit

    def criterion(self, outs, annos):
        """:47-113 -> (cls_loss, loc_loss).  annos [B,M,8] xywh rows, zero rows as padding; not modified (the reference
        turns its argument into xyxy in place, which is why its caller passes a clone)."""
        loc_preds, cls_preds = outs
        if loc_preds.size(1) != self.anchors.size(0):
            raise ValueError("criterion: %d predictions per image against %d anchors" % (loc_preds.size(1), self.anchors.size(0)))
        return RF.retina_criterion(loc_preds, cls_preds, annos, self.anchors, self.cfg.num_classes)

    def train_step(self, step, batch):
        """One iteration of training_process (:128-149) without the logging."""
        imgs, annos = batch[0], batch[1]
        size = (imgs.size(2), imgs.size(3))
        if size != tuple(self.cfg.Train.crop_size):
            self.anchors = self.make_anchor(size)[0]
        self.lr_sch.step()
        self.optimizer.zero_grad()
        outs = self.model(imgs)
        cls_loss, loc_loss = self.criterion(outs, annos)
        loss = cls_loss + loc_loss
        loss.backward()
        self.optimizer.step()
        return _released(outs), _released((loss, cls_loss, loc_loss))

    def training_process(self):
        self.model.train()
        totals = np.zeros(3)
        log_dir = os.path.join('./log', self.cfg.log_prefix)
        full_state = bool(getattr(self.cfg.Train, "full_state", False))
        resume = getattr(self.cfg.Train, "resume", None)
        start_step = self.resume_state(resume, log_dir) if resume else 0
        for step in range(start_step, self.cfg.Train.iter_num):
            batch = self.training_loader.get_batch()
            outs, losses = self.train_step(step, batch)
            totals += np.array([float(l.detach()) for l in losses])
            pi = self.cfg.Train.print_interval
            if self.main_proc_flag:
                if step % pi == pi - 1:
                    print("step %d  loss %.4f cls %.4f loc %.4f  lr %.3g" %
                          ((step,) + tuple(totals / pi) + (self.optimizer.param_groups[0]['lr'],)) + self.guard_report(),
                          flush=True)
                    totals[:] = 0
                ci = self.cfg.Train.checkpoint_interval
                if step % ci == ci - 1 or step == self.cfg.Train.iter_num - 1:
                    os.makedirs(log_dir, exist_ok=True)
                    self.save_ckp(self.model.module, step, log_dir)
                    self.save_ema_ckp(step, log_dir)
                    if full_state:
                        self.save_state(step, log_dir)
        self.close_state()

    def transform_bbox(self, cls_pred, loc_pred):
        """:179-213: cls_pred [A,C] logits and loc_pred [A,4] of one image -> rows (x, y, w, h, prob, cls+1) of the anchors
        with prob > 0.1, in anchor order."""
        rows, count = ops.retina_decode(cls_pred.detach().unsqueeze(0), loc_pred.detach().unsqueeze(0), self.anchors,
                                        SCORE_THRESH)
        return rows[0, :int(count.item())]

    @staticmethod
    def save_result(file_path, pred_bbox):
        """:215-225: truncated integer boxes."""
        rows = torch.clamp(pred_bbox, min=0.).detach().cpu().tolist()
        with open(file_path, 'w') as f:
            f.write(''.join('%d,%d,%d,%d,%.4f,%d,-1,-1\n' % (int(r[0]), int(r[1]), int(r[2]), int(r[3]), float(r[4]), int(r[5]))
                            for r in rows))

    def evaluate_images(self, imgs):
        """Body of evaluation_process (:243-255) for a batch of equal-size images -> one [k,6] tensor of kept rows
        (x, y, w, h, prob, cls+1; score descending) per image: decode, xywh -> xyxy, score sort, hard NMS at 0.3 in the
        gpu_nms convention (legacy +1 IoU, suppression at IoU > thresh)."""
        self.anchors = self.make_anchor((imgs.size(2), imgs.size(3)))[0]
        loc_pre, cls_pre = self.model(imgs)
        rows, count = ops.retina_decode(cls_pre.detach(), loc_pre.detach(), self.anchors, SCORE_THRESH)
        counts = count.cpu().tolist()
        for i, n in enumerate(counts):
            if n > MAX_CANDIDATES:
                raise ValueError("evaluate_images: image %d has %d candidates above the score threshold; the score sort "
                                 "accepts %d per frame" % (i, n, MAX_CANDIDATES))
        return [self._nms_rows(rows[i, :n]) for i, n in enumerate(counts)]

    @staticmethod
    def _nms_rows(rows6):
        n = rows6.size(0)
        if n == 0:
            return rows6
        ordered = ops.sort_rows_by_score(rows6)
        xyxy = ordered.clone()
        xyxy[:, 2:4] += xyxy[:, 0:2]                        # :252-253
        dev = rows6.device
        ws = torch.empty(_C.call("rr_nms_workspace_bytes", n), dtype=torch.uint8, device=dev)
        keep = torch.empty(n, dtype=torch.int32, device=dev)
        num = torch.zeros(1, dtype=torch.int32, device=dev)
        _C.call("rr_nms_sorted", xyxy, n, 6, float(np.float32(NMS_THRESH)), 0, ws, keep, num)
        return ordered[keep[:int(num.item())].long()]

    @staticmethod
    def write_results(result_dir, names, boxes, frame_off):
        """The files save_result writes for the frames of one batch, byte for byte, from one host conversion: boxes [n,6]
        and frame_off [B+1] as detect_frames_retinanet returns them (tensors or arrays), names the B file stems."""
        rows = boxes.detach().cpu().numpy() if torch.is_tensor(boxes) else np.asarray(boxes)
        rows = rows.astype(np.float32, copy=False).reshape(-1, 6)
        rows = np.where(rows < 0, np.float32(0.), rows).tolist()     # torch.clamp(min=0.): -0.0 passes through
        off = frame_off.tolist() if hasattr(frame_off, "tolist") else list(frame_off)
        for i, name in enumerate(names):
            with open(os.path.join(result_dir, name + '.txt'), 'w') as f:
                f.write(''.join('%d,%d,%d,%d,%.4f,%d,-1,-1\n' % (int(r[0]), int(r[1]), int(r[2]), int(r[3]), r[4], int(r[5]))
                                for r in rows[off[i]:off[i + 1]]))

    @staticmethod
    def write_results_device(result_dir, names, boxes, frame_off):
        """write_results from a device tensor: the same files, formatted by rr_text_format (rrnet_amd/textio.py) in one launch
        sequence for the whole batch and written in binary mode; a frame with a row the codec flags goes through the host
        expression."""
        from rrnet_amd import textio
        rows = boxes.detach().to(torch.float32).reshape(-1, 6)
        textio.write_frames([os.path.join(result_dir, name + '.txt') for name in names], rows, frame_off, "retinanet", True)

    def evaluate_batched(self, device_batch, result_dir=None):
        """evaluation_process' loop over SizeBucketedFrames -> detect_frames_retinanet: equal-size raw frames `device_batch`
        at a time, one D2H copy per batch.
        Builder-defined, opt-in (the config modules do not carry the keys): with cfg.Val.tile = N or (H, W) the loop runs
        over OrderedFrames -> detect_tiled_retinanet instead: `device_batch` frames of any sizes per step, cut into
        overlapping tiles; cfg.Val.tile_overlap (default a quarter of the tile), tile_zoom (1.0) and tile_margin (0.0) are
        optional beside it."""
        import math
        from rrnet_amd.datasets.augment import chain_params
        from rrnet_amd.datasets.frames import OrderedFrames, SizeBucketedFrames
        from rrnet_amd import inference
        from rrnet_amd.inference import detect_frames_retinanet
        cfg = self.cfg
        result_dir = getattr(cfg.Val, "result_dir", './results/') if result_dir is None else result_dir
        p = chain_params(cfg.Val.transforms)
        model = getattr(self.model, "module", self.model)
        tile = getattr(cfg.Val, "tile", None)
        if tile:
            th, tw = inference._tile_hw(tile)
            overlap = getattr(cfg.Val, "tile_overlap", None)
            overlap = min(th, tw) // 4 if overlap is None else int(overlap)
            zoom = float(getattr(cfg.Val, "tile_zoom", None) or 1.0)
            margin = float(getattr(cfg.Val, "tile_margin", None) or 0.0)
            anchors = self.make_anchor((int(math.floor(th * zoom)), int(math.floor(tw * zoom))))[0]
            frames = OrderedFrames(self.validation_loader.dataset, device_batch, rank=getattr(cfg.Distributed, "rank", 0),
                                   world_size=max(int(getattr(cfg.Distributed, "world_size", 1)), 1),
                                   num_workers=cfg.Val.num_workers)
            for frame_list, names in frames:
                boxes, frame_off = inference.detect_tiled_retinanet(model, frame_list, p["mean"], p["std"], anchors,
                                                                    tile=(th, tw), overlap=overlap, zoom=zoom, margin=margin,
                                                                    score_thr=SCORE_THRESH, nms_thresh=NMS_THRESH)
                self.write_results(result_dir, names, boxes, frame_off.cpu())
            return
        frames = SizeBucketedFrames(self.validation_loader.dataset, device_batch, rank=getattr(cfg.Distributed, "rank", 0),
                                    world_size=max(int(getattr(cfg.Distributed, "world_size", 1)), 1),
                                    num_workers=cfg.Val.num_workers)
        for frames_u8, names in frames:
            anchors = self.make_anchor(frames_u8.shape[1:3])[0]
            boxes, frame_off = detect_frames_retinanet(model, frames_u8, p["mean"], p["std"], anchors,
                                                       score_thr=SCORE_THRESH, nms_thresh=NMS_THRESH)
            self.write_results(result_dir, names, boxes, frame_off.cpu())

    def evaluation_process(self):
        self.model.eval()
        state_dict = torch.load(self.cfg.Val.model_path, map_location='cpu')
        self.model.module.load_state_dict(state_dict)
        if self.validation_loader is None:
            raise RuntimeError("no validation data: %s/val/images does not exist" % self.cfg.data_root)
        result_dir = getattr(self.cfg.Val, "result_dir", './results/')
        os.makedirs(result_dir, exist_ok=True)
        # builder-defined, opt-in (the config modules do not carry the key): cfg.Val.device_batch = N >= 1 runs the batched
        # path on raw frames; absent or 0 is the per-frame loop below
        device_batch = int(getattr(self.cfg.Val, "device_batch", 0) or 0)
        if device_batch >= 1:
            with torch.no_grad():
                self.evaluate_batched(device_batch, result_dir)
            print('Done !!!')
            return
        step = 0
        with torch.no_grad():
            for data in self.validation_loader:
                step += 1
                imgs, _annos, names = data
                for name, pred in zip(names, self.evaluate_images(imgs.cuda())):
                    self.save_result(os.path.join(result_dir, name + '.txt'), pred)
                if self.main_proc_flag:
                    print('Step : %d / %d' % (step, len(self.validation_loader)))
            print('Done !!!')

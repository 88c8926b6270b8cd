"""RRNetOperator — operators/rrnet_operator.py:22-284 of the reference on the MI355X path.

Same constructor / criterion / training_process / generate_bbox / _ext_nms / save_result /
evaluation_process surface.  What changed underneath:
  * model, losses, decode, NMS, RoIAlign, optimizer are the HIP kernels of librrnet_hip.so;
  * Adam runs fused over one flat buffer and carries the RCCL gradient all-reduce (FlatAdam);
  * the stage-2 loss has no per-image host loop and no `.sum() == 0` synchronisation;
  * `_ext_nms` runs the bit-exact wavefront-parallel Soft-NMS over all classes in one launch.
Out of scope and reduced to stdout: tensorboard / cv2 visualisation (utils/vis)."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.optim as optim

from rrnet_amd import functional as RF
from rrnet_amd import ops
from rrnet_amd.datasets import make_dataloader
from rrnet_amd.ext.nms.nms_wrapper import soft_nms_segments
from rrnet_amd.flat import FlatAdam, FlatParams
from rrnet_amd.models.rrnet import RRNet
from rrnet_amd.modules.loss.focalloss import FocalLossHM
from rrnet_amd.modules.loss.regl1loss import RegL1Loss
from .base_operator import BaseOperator, guard_options, make_lr_scheduler



def _released(v):
    """The same values without the autograd graph (recursively through tuples / lists).  backward() has consumed the graph;
    handing its roots out would keep every node of the step alive until the caller drops them — and with the nodes what they
    attach to their ctx by hand (shared fan-in buffers, bf16 images, parameter references): 20 GiB at the bench configuration
    that a training loop holding `losses` until the next step returns would carry through that step's forward."""
    if torch.is_tensor(v):
        return v.detach()
    if isinstance(v, (tuple, list)):
        return type(v)(_released(x) for x in v)
    return v

class RRNetOperator(BaseOperator):
    def __init__(self, cfg):
        self.cfg = cfg
        model = RRNet(cfg).cuda(cfg.Distributed.gpu_id).to(memory_format=torch.channels_last)
        model = nn.SyncBatchNorm.convert_sync_batchnorm(model)
        flat = FlatParams(model)
        self.optimizer = FlatAdam(flat, lr=cfg.Train.lr, **guard_options(cfg))
        self.lr_sch = make_lr_scheduler(cfg, self.optimizer)
        self.training_loader, self.validation_loader = make_dataloader(cfg, collate_fn='rrnet')
        super(RRNetOperator, self).__init__(cfg=self.cfg, model=model, lr_sch=self.lr_sch, flat=flat)
        self.hm_focal_loss = FocalLossHM()
        self.l1_loss = RegL1Loss()
        self.main_proc_flag = cfg.Distributed.gpu_id == 0

    def criterion(self, outs, targets):
        """rrnet_operator.py:42-84 -> (hm_loss, wh_loss, off_loss, s2_reg_loss)."""
        s1_hms, s1_whs, s1_offsets, s2_reg, bxyxy, scores, _ = outs
        gt_hms, gt_whs, gt_inds, gt_offsets, gt_reg_masks, gt_annos = targets
        ns = self.cfg.Model.num_stacks
        gt_hm_nhwc = ops.to_nhwc(gt_hms)                 # one layout for logits and targets
        hm_loss = wh_loss = off_loss = 0
        for s in range(ns):
            hm_loss = hm_loss + self.hm_focal_loss.from_logits(s1_hms[s], gt_hm_nhwc) / ns
            wh_loss = wh_loss + self.l1_loss(s1_whs[s], gt_reg_masks, gt_inds, gt_whs) / ns
            off_loss = off_loss + self.l1_loss(s1_offsets[s], gt_reg_masks, gt_inds, gt_offsets) / ns
        gt_annos[:, :, 2:4] += gt_annos[:, :, 0:2]       # in place, as the reference (:67)
        s2_reg_loss = RF.stage2_reg_loss(s2_reg, bxyxy, gt_annos, self.cfg.Train.scale_factor)
        return hm_loss, wh_loss, off_loss, s2_reg_loss

    @staticmethod
    def generate_bbox_target(ex_rois, gt_rois):
        """rrnet_operator.py:86-102 (kept for API parity; the fused loss kernel computes the same)."""
        ew = ex_rois[:, 2] - ex_rois[:, 0] + 1.0
        eh = ex_rois[:, 3] - ex_rois[:, 1] + 1.0
        ecx, ecy = ex_rois[:, 0] + 0.5 * ew, ex_rois[:, 1] + 0.5 * eh
        gw = gt_rois[:, 2] - gt_rois[:, 0] + 1.0
        gh = gt_rois[:, 3] - gt_rois[:, 1] + 1.0
        gcx, gcy = gt_rois[:, 0] + 0.5 * gw, gt_rois[:, 1] + 0.5 * gh
        return torch.stack(((gcx - ecx) / ew, (gcy - ecy) / eh, torch.log(gw / ew), torch.log(gh / eh)), dim=1)

    def train_step(self, step, batch):
        """One iteration of training_process (rrnet_operator.py:116-144) without the logging."""
        imgs, annos, gt_hms, gt_whs, gt_inds, gt_offsets, gt_reg_masks, _names = batch
        self.lr_sch.step()
        self.optimizer.zero_grad()
        outs = self.model(imgs)
        targets = gt_hms, gt_whs, gt_inds, gt_offsets, gt_reg_masks, annos
        hm_loss, wh_loss, offset_loss, s2_reg_loss = self.criterion(outs, targets)
        s2_factor = 0 if step < 2000 else 1
        loss = hm_loss + (0.1 * wh_loss) + offset_loss + s2_reg_loss * s2_factor
        loss.backward()
        self.optimizer.step()
        return _released(outs), _released((loss, hm_loss, wh_loss, offset_loss, s2_reg_loss))

    def training_process(self):
        self.model.train()
        totals = np.zeros(5)
        log_dir = os.path.join('./log', self.cfg.log_prefix)
        # builder-defined, opt-in (the config modules do not carry the keys): cfg.Train.full_state = True writes a full
        # training state beside every checkpoint; cfg.Train.resume = 'auto' | <path> continues from one.  The running sums
        # of the print interval are not part of a state: the first report after a resume averages over fewer steps
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
                    lr = self.optimizer.param_groups[0]['lr']
                    print("step %d  loss %.4f hm %.4f wh %.4f off %.4f s2 %.4f  lr %.3g" %
                          ((step,) + tuple(totals / pi) + (lr,)) + self.guard_report(), flush=True)
                    s1_pred_bbox, s2_pred_bbox = self.generate_bbox(outs, batch_idx=0)
                    s2_pred_bbox = self._ext_nms(s2_pred_bbox)
                    totals[:] = 0
                ci = self.cfg.Train.checkpoint_interval
                if step % ci == ci - 1 or step == self.cfg.Train.iter_num - 1:
                    os.makedirs(log_dir, exist_ok=True)
                    self.save_ckp(self.model.module, step, log_dir)
                    self.save_ema_ckp(step, log_dir)
                    if full_state:
                        self.save_state(step, log_dir)
        self.close_state()

    def generate_bbox(self, outs, batch_idx=0):
        """rrnet_operator.py:188-209 -> (stage-1 boxes [n,6] xywh cls=0, stage-2 boxes [n,6] xywh cls+1)."""
        _, _, _, s2_reg, bxyxy, scores, clses = outs
        flag = bxyxy[:, 0] == batch_idx
        reg = s2_reg[flag].detach()
        box = bxyxy[flag, 1:] * self.cfg.Train.scale_factor
        score, cls = scores[flag], clses[flag]
        xy, wh = box[:, 0:2], box[:, 2:4] - box[:, 0:2]
        s1 = torch.cat((xy, wh, score.view(-1, 1), torch.zeros((box.size(0), 1), device=box.device)), dim=1)
        wh1 = wh + 1
        cx = reg[:, 0] * wh1[:, 0] + xy[:, 0] + wh1[:, 0] / 2
        cy = reg[:, 1] * wh1[:, 1] + xy[:, 1] + wh1[:, 1] / 2
        w = reg[:, 2].exp() * wh1[:, 0]
        h = reg[:, 3].exp() * wh1[:, 1]
        s2 = torch.stack((cx - w / 2., cy - h / 2., w, h, score, cls.float() + 1), dim=1)
        return s1, s2

    @staticmethod
    def _ext_nms_device(pred_bbox, per_cls=True):
        """rrnet_operator.py:211-232 on the device: per-class gaussian Soft-NMS (Nt 0.7, threshold 0.1) on xywh boxes,
        all classes in one launch; returns a device tensor."""
        dev = pred_bbox.device if pred_bbox.is_cuda else torch.device("cuda", torch.cuda.current_device())
        b = pred_bbox.detach().to(dev, torch.float32).clone()
        b[:, 2] = b[:, 0] + b[:, 2]
        b[:, 3] = b[:, 1] + b[:, 3]
        n = b.size(0)
        if per_cls:
            # one segment per class id present, like the reference's unique() loop (ids are cls+1, any dataset)
            lo, hi = int(b[:, 5].min()), int(b[:, 5].max())
            nc = hi - lo + 1
            if nc > 1023:
                raise ValueError("_ext_nms: class ids span %d values (limit 1023)" % nc)
            grouped, seg_off, seg_len = ops.group_by_class(b.view(1, n, 6), nc, cls_base=lo)
        else:
            nc = 1
            grouped = b.view(1, n, 6).clone()
            seg_off = torch.tensor([0, n], dtype=torch.int32, device=dev)
            seg_len = None
        rows = grouped.view(-1, 6)
        n_out = soft_nms_segments(rows, seg_off, n, sigma=0.5, Nt=0.7, threshold=0.1, method=2, seg_len=seg_len)
        _, _, _, kept = ops.pack_segments(rows, seg_off, n_out, nc, want_rois=False, want_rows=True)
        kept[:, 2:4] -= kept[:, 0:2]
        return kept

    @staticmethod
    def _ext_nms(pred_bbox, per_cls=True):
        """rrnet_operator.py:211-232 -> CPU tensor, like the reference."""
        if pred_bbox.size(0) == 0:
            return pred_bbox
        return RRNetOperator._ext_nms_device(pred_bbox, per_cls).cpu()

    @staticmethod
    def save_result(file_path, pred_bbox):
        """rrnet_operator.py:234-244 text format."""
        pred_bbox = torch.clamp(pred_bbox, min=0.)
        with open(file_path, 'w') as f:
            for i in range(pred_bbox.size()[0]):
                bbox = pred_bbox[i]
                f.write('%f,%f,%f,%f,%.4f,%d,-1,-1\n' % (float(bbox[0]), float(bbox[1]), float(bbox[2]),
                                                        float(bbox[3]), float(bbox[4]), int(bbox[5])))

    def evaluate_images(self, imgs):
        """Multi-scale inference of rrnet_operator.py:256-276 for one image batch (bs=1) -> boxes [n,6] on the host.
        Everything between the resize and the final result stays on the device: per-scale boxes, the cross-scale
        concatenation, both score sorts (rr_sort_rows_by_score) and the Soft-NMS; one D2H copy at the end."""
        multi_scale_bboxes = []
        for scale in self.cfg.Val.scales:
            img = ops.resize_bilinear_ac(imgs, scale)
            outs = self.model(img)
            _, pred_bbox = self.generate_bbox(outs)
            if not self.cfg.Val.auto_test:
                pred_bbox = pred_bbox[pred_bbox[:, 4] > 0.01]
            pred_bbox = pred_bbox.clone()
            pred_bbox[:, :4] = pred_bbox[:, :4] / scale
            multi_scale_bboxes.append(pred_bbox)
        pred_bbox = torch.cat(multi_scale_bboxes, dim=0)
        if pred_bbox.size(0) == 0:
            return pred_bbox.cpu()
        if pred_bbox.size(0) > 16384:          # beyond the LDS sort (6 scales x 1500 boxes = 9000 in the reference config)
            pred_bbox = pred_bbox[torch.sort(pred_bbox[:, 4], descending=True, stable=True)[1]]
        else:
            pred_bbox = ops.sort_rows_by_score(pred_bbox)
        if not self.cfg.Val.auto_test:
            pred_bbox = self._ext_nms_device(pred_bbox)
        if 0 < pred_bbox.size(0) <= 16384:
            pred_bbox = ops.sort_rows_by_score(pred_bbox)
        elif pred_bbox.size(0) > 16384:
            pred_bbox = pred_bbox[torch.sort(pred_bbox[:, 4], descending=True, stable=True)[1]]
        return pred_bbox.cpu()

    @staticmethod
    def write_results(file_path, rows):
        """The file save_result writes, byte for byte, from a [n,6] tensor or array: one host conversion of the whole
        block instead of six tensor reads per row."""
        rows = rows.detach().cpu().numpy() if torch.is_tensor(rows) else np.asarray(rows)
        rows = rows.astype(np.float32, copy=False).reshape(-1, 6)
        rows = np.where(rows < 0, np.float32(0.), rows)      # torch.clamp(min=0.): -0.0 and NaN pass through
        with open(file_path, 'w') as f:
            f.write(''.join('%f,%f,%f,%f,%.4f,%d,-1,-1\n' % (r[0], r[1], r[2], r[3], r[4], int(r[5])) for r in rows.tolist()))

    @staticmethod
    def write_results_device(file_path, rows):
        """write_results from a device tensor [n,6]: the same file, formatted by rr_text_format (rrnet_amd/textio.py) and
        written in binary mode; a row the codec flags sends the file through the host expression."""
        from rrnet_amd import textio
        rows = rows.detach().to(torch.float32).reshape(-1, 6)
        textio.write_frames([file_path], rows, [0, rows.shape[0]], "rrnet", True)

    def evaluate_batched(self, device_batch, k=1500):
        """evaluation_process' loop over SizeBucketedFrames -> detect_frames: equal-size frames `device_batch` at a time,
        one D2H copy per batch."""
        from rrnet_amd.datasets.augment import chain_params
        from rrnet_amd.datasets.frames import SizeBucketedFrames
        from rrnet_amd.inference import detect_frames
        cfg = self.cfg
        p = chain_params(cfg.Val.transforms)
        model = getattr(self.model, "module", self.model)
        frames = SizeBucketedFrames(self.validation_loader.dataset, device_batch, rank=getattr(cfg.Distributed, "rank", 0),
                                    world_size=max(int(getattr(cfg.Distributed, "world_size", 1)), 1),
                                    num_workers=cfg.Val.num_workers)
        for frames_u8, names in frames:
            boxes, frame_off = detect_frames(model, frames_u8, cfg.Val.scales, p["mean"], p["std"],
                                             nms=not cfg.Val.auto_test, k=k, scale_factor=cfg.Train.scale_factor,
                                             num_classes=cfg.num_classes)
            rows, off = boxes.cpu().numpy(), frame_off.cpu().tolist()
            for i, name in enumerate(names):
                self.write_results(os.path.join(cfg.Val.result_dir, name + '.txt'), rows[off[i]:off[i + 1]])

    def evaluation_process(self):
        self.model.eval()
        state_dict = torch.load(self.cfg.Val.model_path, map_location='cpu')
        self.model.module.load_state_dict(state_dict)
        if self.validation_loader is None:
            raise RuntimeError("no validation data: %s/val/images does not exist" % self.cfg.data_root)
        os.makedirs(self.cfg.Val.result_dir, exist_ok=True)
        # builder-defined, opt-in (the config modules do not carry the key): cfg.Val.device_batch = N >= 1 runs the batched
        # path on raw frames; absent or 0 is the reference's per-frame loop below
        device_batch = int(getattr(self.cfg.Val, "device_batch", 0) or 0)
        if device_batch >= 1:
            from rrnet_amd import ops
            if len(self.cfg.Val.scales) * 1500 > ops.DETECT_MAX_ROWS:
                print("warning: Val.device_batch ignored: %d scales x 1500 boxes exceed the batched sort's %d rows per "
                      "frame; evaluating frame by frame" % (len(self.cfg.Val.scales), ops.DETECT_MAX_ROWS), flush=True)
            else:
                with torch.no_grad():
                    self.evaluate_batched(device_batch)
                print('=> Evaluation Done!')
                return
        with torch.no_grad():
            for step, data in enumerate(self.validation_loader):
                imgs, annos, names = data
                pred_bbox = self.evaluate_images(imgs.cuda())
                self.save_result(os.path.join(self.cfg.Val.result_dir, names[0] + '.txt'), pred_bbox)
            print('=> Evaluation Done!')

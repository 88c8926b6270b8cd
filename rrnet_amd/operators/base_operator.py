"""operators/base_operator.py:11-51 of the reference.  `DistributedDataParallel(model, ...)` is
replaced by RCCLDataParallel: parameters and gradients live in flat HBM buffers
(rrnet_amd.flat), the initial broadcast is one collective and the gradient exchange is a few
large RCCL all-reduces over xGMI issued from the optimizer step."""
import os
import random

import torch
import torch.nn as nn

from rrnet_amd.flat import FlatParams


def broadcast_buffers(module, src=0):
    """All buffers of `module` from rank `src` in one collective: packed into one float64 tensor (exact for float32
    statistics and for the int64 `num_batches_tracked` counters below 2^53), broadcast, unpacked in place."""
    from rrnet_amd import dptrace
    bufs = [b for b in module.buffers() if b.numel() > 0]
    if not bufs:
        return 0
    flat = torch.cat([b.detach().reshape(-1).to(torch.float64) for b in bufs])
    dptrace.record("default", "broadcast", flat.numel(), "buffers")
    torch.distributed.broadcast(flat, src)
    off = 0
    with torch.no_grad():
        for b in bufs:
            n = b.numel()
            b.copy_(flat[off:off + n].view(b.shape).to(b.dtype))
            off += n
    return len(bufs)


def guard_options(cfg):
    """FlatAdam's guard arguments from the opt-in keys cfg.Train.max_grad_norm / skip_nonfinite / ema_decay / ema_warmup
    (builder-defined: the config modules do not carry them, as with full_state).  All absent: an empty dict."""
    opts = {}
    for key in ("max_grad_norm", "skip_nonfinite", "ema_decay", "ema_warmup"):
        v = getattr(cfg.Train, key, None)
        if v is not None:
            opts[key] = v
    return opts


def make_lr_scheduler(cfg, optimizer):
    """cfg.Train.warmup_iters > 0 (opt-in, with warmup_factor and warmup_method) puts the reference's warm-up in front of
    the milestones (utils/warmup_lr.py); otherwise MultiStepLR as the reference's operators build it."""
    warmup_iters = int(getattr(cfg.Train, "warmup_iters", 0) or 0)
    if warmup_iters > 0:
        from rrnet_amd.utils.warmup_lr import WarmupMultiStepLR
        return WarmupMultiStepLR(optimizer, milestones=cfg.Train.lr_milestones, gamma=0.1,
                                 warmup_factor=float(getattr(cfg.Train, "warmup_factor", 1.0 / 3)),
                                 warmup_iters=warmup_iters, warmup_method=getattr(cfg.Train, "warmup_method", "linear"))
    return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=cfg.Train.lr_milestones, gamma=0.1)


class RCCLDataParallel(nn.Module):
    """Keeps DDP's surface used by the reference (`self.model(x)`, `self.model.module`,
    state_dict of `.module`)."""

    def __init__(self, module, flat=None):
        super().__init__()
        self.module = module
        self.flat = flat if flat is not None else FlatParams(module)
        self.flat.broadcast(0)
        # buffers (BN running statistics and counters) start identical on all ranks — rank 0's — through ONE broadcast
        # of a packed fp64 image (490 single-buffer broadcasts in round 2; fp64 holds the int64 counters exactly)
        from rrnet_amd import dptrace
        if dptrace.dp_active():
            broadcast_buffers(module, 0)

    def forward(self, *a, **kw):
        return self.module(*a, **kw)


class BaseOperator(object):
    def __init__(self, cfg, model, lr_sch=None, flat=None):
        self.cfg = cfg
        random.seed(cfg.seed)
        torch.manual_seed(cfg.seed)
        torch.cuda.manual_seed(cfg.seed)
        self.model = RCCLDataParallel(model, flat)
        self.lr_sch = lr_sch

    def criterion(self, outs, labels):
        raise NotImplementedError

    def training_process(self):
        raise NotImplementedError

    def evaluation_process(self):
        raise NotImplementedError

    @staticmethod
    def save_ckp(models, step, path):
        """Same file format as the reference: state_dict of the bare module, reference key names."""
        sd = {k: v.detach().cpu().contiguous() for k, v in models.state_dict().items()}
        torch.save(sd, os.path.join(path, 'ckp-{}.pth'.format(step)))

    # ---- the guarded optimiser step (FlatAdam's max_grad_norm / skip_nonfinite / ema_decay) ----
    def guard_report(self):
        """What the print-interval line gains with a guard active (one small device read), else ''."""
        opt = getattr(self, "optimizer", None)
        if opt is None or not getattr(opt, "guarded", False):
            return ""
        s = opt.guard_stats()
        return "  gnorm %.4g clipped %d skipped %d" % (s["norm"], s["clipped"], s["skipped"])

    def save_ema_ckp(self, step, path):
        """With averaged weights on: `ckp-ema-{step}.pth` beside `ckp-{step}.pth`, the same format (the module's keys), the
        trainable parameters replaced by their averages (FlatAdam.ema_state_dict)."""
        opt = getattr(self, "optimizer", None)
        if opt is None or getattr(opt, "ema", None) is None:
            return
        sd = {k: v.detach().cpu().contiguous() for k, v in opt.ema_state_dict(self.model.module).items()}
        torch.save(sd, os.path.join(path, 'ckp-ema-{}.pth'.format(step)))

    # ---- full-state checkpoints (rrnet_amd/checkpoint.py; opt-in through cfg.Train.full_state / cfg.Train.resume) ----
    _state_writer = None

    def save_state(self, step, log_dir=None):
        """Enqueue a copy of the whole training state after step `step` and return; `state-{step}.pth` appears in
        `log_dir` (default: where save_ckp writes) once the writer's thread is done.  Needs `self.optimizer` (FlatAdam)."""
        from rrnet_amd.checkpoint import StateWriter
        if self._state_writer is None:
            log_dir = log_dir or os.path.join('./log', self.cfg.log_prefix)
            self._state_writer = StateWriter(self.model.module, self.optimizer, log_dir, self.lr_sch,
                                             getattr(self, "training_loader", None),
                                             keep=getattr(self.cfg.Train, "keep_states", 2))
        self._state_writer.save_state(step)

    def load_state(self, path):
        """Load a state file into the live model, optimizer, scheduler and training loader -> the step to continue at."""
        from rrnet_amd.checkpoint import load_state
        return load_state(path, self.model.module, self.optimizer, self.lr_sch, getattr(self, "training_loader", None))

    def resume_state(self, where, log_dir):
        """cfg.Train.resume ('auto' or a path) -> the step training_process starts at."""
        from rrnet_amd.checkpoint import resume
        return resume(where, log_dir, self.model.module, self.optimizer, self.lr_sch, getattr(self, "training_loader", None))

    def close_state(self):
        """Wait for the state file in flight, stop the writer's thread (re-raises what it raised)."""
        writer, self._state_writer = self._state_writer, None
        if writer is not None:
            writer.close()

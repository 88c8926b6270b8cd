"""Train RRNet, CenterNet or RetinaNet on one GPU: the counterpart of tools/detect.py.

  python tools/train.py --config rrnet_config|rrnet_fillduck_config|centernet_config|retinanet_config [--data-root D] [--iters N]
                        [--batch B] [--crop H W] [--backbone NAME] [--bf16] [--full-state] [--resume auto|PATH]
                        [--checkpoint-interval N] [--print-interval N] [--keep-states N] [--color-jitter B C S]
                        [--clip-grad-norm X] [--skip-nonfinite] [--ema DECAY] [--no-ema-warmup] [--warmup ITERS]
                        [--warmup-factor F] [--attention K DIL]

A single process: it sets the config keys and calls the operator's training_process().  Without a dataset under
--data-root the synthetic loader feeds the loop.  `ckp-{step}.pth` (weights, the reference's format) goes to
./log/<log_prefix>/ every --checkpoint-interval steps; --full-state writes `state-{step}.pth` beside each of them
(parameters, Adam moments, scheduler, BatchNorm buffers, step, loader position; rrnet_amd/checkpoint.py) and
--resume continues from one: `auto` takes the newest state of the log directory that loads and verifies.
--color-jitter B C S puts ColorJitter(B, C, S) in front of the config's training chain (the config modules carry none,
as the reference's): brightness, contrast and saturation factors from [max(1 - x, 0), 1 + x], applied on the device.
--clip-grad-norm X clips the gradient's global norm to X, --skip-nonfinite drops a step whose gradient holds a NaN or an Inf,
--ema DECAY keeps averaged weights and writes `ckp-ema-{step}.pth` beside each checkpoint (--no-ema-warmup: the full decay
from the first step); all three are decided on the device inside the optimiser step.  --warmup ITERS puts the
reference's linear learning-rate warm-up (from --warmup-factor F, default 1/3, of the rate) in front of the milestones.
--backbone NAME overrides cfg.Model.backbone (utils/model_tools.get_backbone: the hourglass family for RRNet and CenterNet;
resnet10 / resnet50 / resnet101 and shufflenet_v2_x0_5 / _x1_5 / _x2_0 for RetinaNet).
--attention K DIL (RRNet, CenterNet; fp32) puts a zero-initialised SelfAttentionModule (K x K window at dilation DIL, 64 key
and value channels, padding DIL * (K // 2)) per stack in front of the stage-1 heads: cfg.Model.attention."""
import argparse
import copy
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ("rrnet_config", "rrnet_fillduck_config", "centernet_config", "retinanet_config")


def load_config(name):
    if name not in CONFIGS:
        raise SystemExit("unknown config %r (one of %s)" % (name, ", ".join(CONFIGS)))
    return copy.deepcopy(importlib.import_module("rrnet_amd.configs." + name).Config)


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="rrnet_config")
    ap.add_argument("--data-root")
    ap.add_argument("--iters", type=int)
    ap.add_argument("--batch", type=int)
    ap.add_argument("--crop", type=int, nargs=2, metavar=("H", "W"))
    ap.add_argument("--backbone")
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--full-state", action="store_true")
    ap.add_argument("--resume", metavar="auto|PATH")
    ap.add_argument("--checkpoint-interval", type=int)
    ap.add_argument("--print-interval", type=int)
    ap.add_argument("--keep-states", type=int)
    ap.add_argument("--color-jitter", type=float, nargs=3, metavar=("B", "C", "S"))
    ap.add_argument("--clip-grad-norm", type=float, metavar="X")
    ap.add_argument("--skip-nonfinite", action="store_true")
    ap.add_argument("--ema", type=float, metavar="DECAY")
    ap.add_argument("--no-ema-warmup", action="store_true")
    ap.add_argument("--warmup", type=int, metavar="ITERS")
    ap.add_argument("--warmup-factor", type=float, metavar="F")
    ap.add_argument("--attention", type=int, nargs=2, metavar=("K", "DIL"))
    return ap.parse_args(argv)


def configure(args):
    """The config the arguments describe (a deep copy of the named module's Config)."""
    cfg = load_config(args.config)
    if args.bf16 and args.config.startswith("centernet"):
        raise SystemExit("--bf16: CenterNet runs in fp32 only (the model has no bf16 scope)")
    if args.bf16 and args.config.startswith("retinanet"):
        raise SystemExit("--bf16: RetinaNet runs in fp32 only (the model has no bf16 scope)")
    if args.data_root is not None:
        cfg.data_root = args.data_root
    if args.iters is not None:
        cfg.Train.iter_num = args.iters
    if args.batch is not None:
        cfg.Train.batch_size = args.batch
    if args.crop is not None:
        from rrnet_amd.datasets.transforms import RandomCrop
        cfg.Train.crop_size = tuple(args.crop)
        chain = cfg.Train.transforms.transforms
        for i, t in enumerate(chain):               # the real-data loader takes the crop from the chain, as the reference does
            if isinstance(t, RandomCrop):
                chain[i] = RandomCrop(tuple(args.crop))
    if args.color_jitter is not None:
        from rrnet_amd.datasets.transforms import ColorJitter
        cfg.Train.transforms.transforms.insert(0, ColorJitter(*args.color_jitter))
    if args.backbone is not None:
        if args.backbone.startswith("shufflenet") and not args.config.startswith("retinanet"):
            raise SystemExit("--backbone %s: ShuffleNetV2 is a backbone of RetinaNet (--config retinanet_config)" % args.backbone)
        cfg.Model.backbone = args.backbone
    if args.bf16:
        cfg.Model.bf16 = True
    if args.attention is not None:
        if args.config.startswith("retinanet"):
            raise SystemExit("--attention: the block sits in front of the stage-1 heads of RRNet and CenterNet")
        if args.bf16:
            raise SystemExit("--attention: the window-attention kernels are fp32 (drop --bf16)")
        from rrnet_amd.utils.model_tools import attention_kwargs
        cfg.Model.attention = attention_kwargs(*args.attention)
    if args.checkpoint_interval is not None:
        cfg.Train.checkpoint_interval = args.checkpoint_interval
    if args.print_interval is not None:
        cfg.Train.print_interval = args.print_interval
    if args.keep_states is not None:
        cfg.Train.keep_states = args.keep_states
    if args.full_state:
        cfg.Train.full_state = True
    if args.resume is not None:
        cfg.Train.resume = args.resume
    if args.clip_grad_norm is not None:
        if not args.clip_grad_norm > 0:
            raise SystemExit("--clip-grad-norm: %r is not a positive norm" % args.clip_grad_norm)
        cfg.Train.max_grad_norm = args.clip_grad_norm
    if args.skip_nonfinite:
        cfg.Train.skip_nonfinite = True
    if args.ema is not None:
        if not 0.0 <= args.ema <= 1.0:
            raise SystemExit("--ema: decay %r outside [0, 1]" % args.ema)
        cfg.Train.ema_decay = args.ema
    if args.no_ema_warmup:
        if args.ema is None:
            raise SystemExit("--no-ema-warmup needs --ema DECAY")
        cfg.Train.ema_warmup = False
    if args.warmup is not None:
        cfg.Train.warmup_iters = args.warmup
    if args.warmup_factor is not None:
        if args.warmup is None:
            raise SystemExit("--warmup-factor needs --warmup ITERS")
        cfg.Train.warmup_factor = args.warmup_factor
    cfg.Distributed.gpu_id, cfg.Distributed.rank, cfg.Distributed.world_size = 0, 0, 1
    return cfg


def main(argv=None):
    args = parse(argv)
    cfg = configure(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/train.py needs the GPU (there is no CPU path)")
    torch.cuda.set_device(0)
    if args.config.startswith("centernet"):
        from rrnet_amd.operators.centernet_operator import CenterNetOperator as Operator
    elif args.config.startswith("retinanet"):
        from rrnet_amd.operators.retinanet_operator import RetinaNetOperator as Operator
    else:
        from rrnet_amd.operators.rrnet_operator import RRNetOperator as Operator
    Operator(cfg).training_process()


if __name__ == "__main__":
    main()

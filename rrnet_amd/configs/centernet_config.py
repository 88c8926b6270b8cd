"""`Config` for CenterNet with the keys and values of the reference's configs/centernet_config.py:6-99 (BASELINE
configs[0] plumbing).  As in rrnet_config.py the transform chains are the reference's without FillDuck (see
rrnet_fillduck_config.py for the full chain)."""
from torch.utils.data import DistributedSampler

from rrnet_amd.configs.rrnet_config import IMAGENET_MEAN, IMAGENET_STD, STRIDE, _tree
from rrnet_amd.datasets.transforms import (Compose, HorizontalFlip, MaskIgnore, MultiScale, Normalize, RandomCrop,
                                            ToHeatmap, ToTensor)

Config = _tree({
    "seed": 219, "dataset": 'drones_det', "data_root": './data/DronesDET', "log_prefix": 'CenterNetMS',
    "use_tensorboard": True, "num_classes": 10,
    "Train": {
        "pretrained": True, "batch_size": 4, "num_workers": 4, "sampler": DistributedSampler,
        "lr": 2.5e-4, "momentum": 0.9, "weight_decay": 0.0001, "lr_milestones": [60000, 80000], "iter_num": 100000,
        "crop_size": (512, 512), "mean": IMAGENET_MEAN, "std": IMAGENET_STD, "scale_factor": STRIDE, "with_road": True,
        "transforms": Compose([MultiScale(scale=(1, 1.15, 1.25, 1.35, 1.5)), ToTensor(), MaskIgnore(IMAGENET_MEAN),
                               HorizontalFlip(), RandomCrop((512, 512)), Normalize(IMAGENET_MEAN, IMAGENET_STD),
                               ToHeatmap(scale_factor=STRIDE)]),
        "print_interval": 20, "checkpoint_interval": 15000,
    },
    "Val": {
        "model_path": './log/ckp-99999.pth', "is_eval": True, "auto_test": True, "batch_size": 1, "num_workers": 4,
        "scales": [1, 1.1, 1.2, 1.3, 1.4, 1.5], "sampler": DistributedSampler, "mean": IMAGENET_MEAN,
        "std": IMAGENET_STD, "transforms": Compose([ToTensor(), Normalize(IMAGENET_MEAN, IMAGENET_STD)]), "result_dir": './results/',
    },
    "Model": {"backbone": 'hourglass', "hm_detector": 'centernet_detector', "wh_detector": 'centernet_WH_detector',
              "reg_detector": 'centernet_detector', "num_stacks": 2},
    "Distributed": {"world_size": 1, "gpu_id": -1, "rank": 0, "ngpus_per_node": 1,
                    "dist_url": 'tcp://127.0.0.1:34567'},
})

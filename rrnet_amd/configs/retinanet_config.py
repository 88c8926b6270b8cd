"""`Config` for RetinaNet with the keys and values of the reference's configs/retinanet_config.py:6-93 (the unused NAS
block included), declared as one nested table like the other configs.

Deviation: the reference's training chain is ToTensor, HorizontalFlip, RandomCropNTimes, NormalizeNTimes, MaskIgnoreNTimes
(:36-45: several crops of one frame per sample).  Here it is the single-crop chain ToTensor, MaskIgnore, HorizontalFlip,
RandomCrop, Normalize, ToHeatmap that the device loader serves for the other two models: one crop per frame, the batch
made of `batch_size` frames.  The operator reads `imgs` and `annos` from the batch and ignores the heat-map targets;
`Train.scale_factor` (not a key of the reference's file) is what ToHeatmap and the loaders are given."""
from torch.utils.data import DistributedSampler

from rrnet_amd.configs.rrnet_config import IMAGENET_MEAN, IMAGENET_STD, STRIDE, _tree
from rrnet_amd.datasets.transforms import (Compose, HorizontalFlip, MaskIgnore, Normalize, RandomCrop, ToHeatmap,
                                            ToTensor)

Config = _tree({
    "seed": 219, "dataset": 'drones_det', "data_root": './data/DronesDET', "log_prefix": 'RetinaNet',
    "use_tensorboard": True, "num_classes": 10,
    "Train": {
        "pretrained": True, "batch_size": 2, "num_workers": 1, "sampler": DistributedSampler,
        "lr": 1e-5, "lr_milestones": [60000, 80000], "iter_num": 90000,
        "crop_size": (512, 512), "mean": IMAGENET_MEAN, "std": IMAGENET_STD, "scale_factor": STRIDE,
        "transforms": Compose([ToTensor(), MaskIgnore(IMAGENET_MEAN), HorizontalFlip(), RandomCrop((512, 512)),
                               Normalize(IMAGENET_MEAN, IMAGENET_STD), ToHeatmap(scale_factor=STRIDE)]),
        "print_interval": 20, "checkpoint_interval": 10000,
    },
    "Val": {
        "model_path": './log/model.pth', "batch_size": 2, "num_workers": 4, "sampler": DistributedSampler,
        "mean": IMAGENET_MEAN, "std": IMAGENET_STD,
        "transforms": Compose([ToTensor(), Normalize(IMAGENET_MEAN, IMAGENET_STD)]),
        "result_dir": './results/',          # read by the evaluation (:257); the reference's file does not define it
    },
    "Model": {"backbone": 'resnet50', "fpn": 'fpn', "cls_detector": 'retinanet_detector',
              "loc_detector": 'retinanet_detector', "num_anchors": 9},
    "NAS": {"ss_num": 7, "path_num": 3, "fpn_inplane": [512, 1024, 2048], "fpn_plane": 256,
            "p_seq": [1, 2, 1, 0, 0, 1, 1, 0, 0, 1, 1, 2, 0, 2, 1, 0, 0, 0, 0, 1, 0],
            "l_seq": [0, 0, 0, 1, 0, 0, 2, 2, 0, 2, 1, 0, 0, 3, 1, 3, 2, 5, 6, 1, 5]},
    "Distributed": {"world_size": 1, "gpu_id": -1, "rank": 0, "ngpus_per_node": 1,
                    "dist_url": 'tcp://127.0.0.1:34567'},
})

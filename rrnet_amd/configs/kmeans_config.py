"""`Config` of the anchor statistics with the keys and values of the reference's configs/kmeans_config.py:6-42, declared
as one nested table like the other configs.  tools/kmeans_anchors.py does not walk a loader (it reads the annotation files
directly); the table exists so that the import line of the reference's scripts/kmeans.py resolves."""
from rrnet_amd.configs.rrnet_config import IMAGENET_MEAN, _tree
from rrnet_amd.datasets.transforms import Compose, MaskIgnore, ToTensor

Config = _tree({
    "seed": 219, "dataset": 'drones_det', "data_root": './data/DronesDET',
    "Train": {
        "pretrained": True, "batch_size": 1, "num_workers": 4, "sampler": None,
        "mean": IMAGENET_MEAN, "transforms": Compose([ToTensor(), MaskIgnore(IMAGENET_MEAN)]),
    },
    "Val": {
        "batch_size": 1, "num_workers": 4, "sampler": None,
        "mean": IMAGENET_MEAN, "transforms": Compose([ToTensor(), MaskIgnore(IMAGENET_MEAN)]),
    },
})

"""`Config` for RRNet with the reference's FULL training chain (configs/rrnet_config.py:40-49, `Train.with_road = True`):
MultiScale -> ToTensor -> MaskIgnore -> FillDuck -> HorizontalFlip -> RandomCrop -> Normalize -> ToHeatmap.  Everything
else is a deep copy of rrnet_config.Config, which keeps its chain without FillDuck.  With this chain the real-data loader
opens `<data_root>/train/roadmap/<name>.jpg` next to every image (an image without one is left unpasted), plans the
pastes on the host and runs them on the device in rr_augment_frames_pasted (rrnet_amd/datasets/augment.py)."""
import copy

from rrnet_amd.configs.rrnet_config import IMAGENET_MEAN, IMAGENET_STD, STRIDE
from rrnet_amd.configs.rrnet_config import Config as _Base
from rrnet_amd.datasets.transforms import (Compose, FillDuck, HorizontalFlip, MaskIgnore, MultiScale, Normalize,
                                            RandomCrop, ToHeatmap, ToTensor)

Config = copy.deepcopy(_Base)
Config.Train.with_road = True
Config.Train.transforms = Compose([MultiScale(scale=(1, 1.15, 1.25, 1.35, 1.5)), ToTensor(), MaskIgnore(IMAGENET_MEAN),
                                   FillDuck(), HorizontalFlip(), RandomCrop((512, 512)),
                                   Normalize(IMAGENET_MEAN, IMAGENET_STD), ToHeatmap(scale_factor=STRIDE)])

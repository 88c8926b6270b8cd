"""Data layer of the hot path.  Two sources feed the same `get_batch()` surface:
  * real VisDrone-DET frames (drones_det.py, augment.py): the host decodes the JPEG and decides scale, flip and crop;
    everything that touches pixels runs on the device in rr_augment_frames (rr_augment_frames_pasted where FillDuck
    pastes objects onto road pixels; the _jitter variants of both, behind rr_jitter_gray_mean, where ColorJitter leads
    the chain), the targets in rr_ctnet_targets.  The host restatement of the reference's transforms (transforms/) is
    the CPU path and the checker of the kernels;
  * the synthetic VisDrone-shaped generator (synthetic.py), which make_dataloader returns when `cfg.data_root` holds no
    dataset.
Inference on raw frames has its own feeder (frames.py): decode, group by size, upload uint8."""
from .augment import DeviceAugmentLoader, DeviceValLoader, HostAugmentLoader  # noqa: F401
from .drones_det import DronesDET  # noqa: F401
from .frames import FrameFolder, SizeBucketedFrames, plan_buckets  # noqa: F401
from .synthetic import SyntheticDronesDET, make_dataloader  # noqa: F401

datasets = {'drones_det': DronesDET}

"""rr_augment_frames and the device loader against the host path, bit for bit; one train step and the evaluation entry
point on real (temporary) VisDrone-shaped data."""
import os
import re

import numpy as np
import pytest
import torch

import augment_cases as C
from rrnet_amd.datasets import augment as A

pytestmark = pytest.mark.gpu


def _run_kernel(cases, crop, taps):
    from rrnet_amd import ops
    (src, params, rects, rect_off), refs = C.packed(cases, taps)
    dev = torch.device("cuda", 0)
    out = ops.augment_frames(torch.from_numpy(src.copy()).to(dev), torch.from_numpy(params).to(dev),
                             torch.from_numpy(rects).to(dev) if len(rects) else None,
                             torch.from_numpy(rect_off).to(dev), taps.device(dev),
                             torch.tensor(C.MEAN, device=dev), torch.tensor(C.STD, device=dev), crop[0], crop[1])
    assert out.shape == (len(cases), 3, crop[0], crop[1]) and out.is_contiguous(memory_format=torch.channels_last)
    return out.permute(0, 2, 3, 1).contiguous().cpu(), torch.from_numpy(refs)


@pytest.mark.parametrize("crop", C.CROPS, ids=lambda c: "%dx%d" % (c[1], c[0]))
@pytest.mark.parametrize("src_name", C.SOURCES)
def test_kernel_is_bit_identical_to_the_host_path(src_name, crop):
    """B = 1 over scales x flip x crop origins (0, interior, flush right/bottom) for one source frame and crop size:
    windows that do not start at (0, 0), frames smaller than the crop in one and in both dimensions (padding), ignore
    rectangles crossing the crop edge, empty after truncation, and moving under the flip."""
    taps = A.TapCache()
    for case in C.grid(src_name, crop):
        got, ref = _run_kernel([case], crop, taps)
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), case


@pytest.mark.parametrize("crop", C.CROPS, ids=lambda c: "%dx%d" % (c[1], c[0]))
def test_kernel_mixed_batch_of_five(crop):
    """B = 5 with mixed source sizes, scales, flips and origins in one launch."""
    taps = A.TapCache()
    got, ref = _run_kernel([(n, s, f, crop, o) for n, s, f, o in C.MIXED], crop, taps)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


def _chain(crop):
    from rrnet_amd.datasets.transforms import (Compose, HorizontalFlip, MaskIgnore, MultiScale, Normalize, RandomCrop,
                                               ToHeatmap, ToTensor)
    return Compose([MultiScale(scale=(1, 1.15, 1.25, 1.35, 1.5)), ToTensor(), MaskIgnore(C.MEAN), HorizontalFlip(),
                    RandomCrop(crop), Normalize(C.MEAN, C.STD), ToHeatmap(scale_factor=4)])


@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    return C.write_dataset(str(tmp_path_factory.mktemp("visdrone")), splits=("train", "val"), extra=3)


def test_device_loader_equals_host_loader(data_root):
    """Demo frame + three JPEGs written by PIL, B=2, crop 128x128, four batches, same seed: imgs bit-identical, every
    other tensor equal."""
    from rrnet_amd.datasets.drones_det import DronesDET
    chain = _chain((128, 128))
    ds = DronesDET(data_root, chain, "train")
    assert len(ds) == 4
    p = A.chain_params(chain)
    dev = A.DeviceAugmentLoader(ds, p, 2, seed=5, num_workers=4)
    host = A.HostAugmentLoader(ds, p, 2, seed=5, num_workers=1)
    try:
        for _ in range(4):
            a, b = dev.get_batch(), host.get_batch()
            assert a[7] == b[7]
            assert a[0].shape == (2, 3, 128, 128) and a[0].is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
            for k in range(1, 7):
                assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    finally:
        dev.close()
        host.close()


def _cfg(data_root, tmp_path):
    import copy
    from rrnet_amd.configs.rrnet_config import Config
    cfg = copy.deepcopy(Config)
    cfg.data_root = data_root
    cfg.Train.batch_size, cfg.Train.crop_size, cfg.Train.num_workers = 2, (128, 128), 4
    cfg.Train.transforms = _chain((128, 128))
    cfg.Val.num_workers, cfg.Val.scales = 2, [1, 1.2]
    cfg.Val.result_dir = str(tmp_path / "results")
    cfg.Val.model_path = str(tmp_path / "ckp.pth")
    cfg.Model.backbone = "hourglass_tiny"
    cfg.Distributed.gpu_id, cfg.Distributed.rank, cfg.Distributed.world_size = 0, 0, 1
    return cfg


def test_train_step_and_evaluation_on_real_frames(data_root, tmp_path):
    """make_dataloader finds the directory; one train_step of the tiny hourglass on a loader batch gives finite losses;
    evaluation_process runs to the end on the same frames as `val` and writes one well-formed result file per image."""
    from rrnet_amd.datasets import DeviceAugmentLoader, DeviceValLoader
    from rrnet_amd.operators.rrnet_operator import RRNetOperator
    cfg = _cfg(data_root, tmp_path)
    torch.manual_seed(219)
    op = RRNetOperator(cfg)
    try:
        assert isinstance(op.training_loader, DeviceAugmentLoader) and isinstance(op.validation_loader, DeviceValLoader)
        op.model.train()
        _, losses = op.train_step(0, op.training_loader.get_batch())
        assert all(bool(torch.isfinite(v)) for v in losses), losses
        op.save_ckp(op.model.module, 0, str(tmp_path))
        os.replace(str(tmp_path / "ckp-0.pth"), cfg.Val.model_path)
        op.evaluation_process()
    finally:
        op.training_loader.close()
    names = sorted(f[:-4] for f in os.listdir(os.path.join(data_root, "val", "images")))
    assert sorted(os.listdir(cfg.Val.result_dir)) == [n + ".txt" for n in names] and len(names) == 4
    line = re.compile(r"^\d+\.\d+,\d+\.\d+,\d+\.\d+,\d+\.\d+,\d\.\d{4},\d+,-1,-1$")
    for n in names:
        for l in open(os.path.join(cfg.Val.result_dir, n + ".txt")).read().splitlines():
            assert line.match(l), l


def test_validation_loader_is_totensor_normalize(data_root):
    """The validation chain through the kernel (scale 1, no flip, crop = frame) equals ToTensor -> Normalize on the host."""
    from PIL import Image
    from rrnet_amd.datasets.drones_det import DronesDET
    from rrnet_amd.datasets.transforms import Compose, Normalize, ToTensor
    chain = Compose([ToTensor(), Normalize(C.MEAN, C.STD)])
    ds = DronesDET(data_root, chain, "val")
    seen = 0
    for imgs, annos, names in A.DeviceValLoader(ds, A.chain_params(chain), num_workers=2):
        i = ds.mdf.index(names[0])
        ref, ref_annos, _ = ds[i]
        assert torch.equal(imgs.cpu()[0].contiguous().view(torch.int32), ref.view(torch.int32))
        assert torch.equal(annos[0], ref_annos) and annos.shape[0] == 1
        seen += 1
    assert seen == len(ds) == 4

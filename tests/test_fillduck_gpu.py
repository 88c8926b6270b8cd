"""rr_augment_frames_pasted and the device loader with FillDuck: unpasted pixels bit-identical to rr_augment_frames and to
the host path, pasted pixels within the derived bound E(depth) of the float64 evaluation (2 E against the host chain)."""
import numpy as np
import pytest
import torch

import augment_cases as C
import fillduck_cases as D
from rrnet_amd.datasets import augment as A

pytestmark = pytest.mark.gpu

CROP = (64, 64)


def _run(cases, crop, taps):
    """cases: [(name, scale, flip, origin)] -> (pasted kernel [B,h,w,3], plain kernel [B,h,w,3], decisions, float64
    references, pasted masks)."""
    from rrnet_amd import ops
    items, refs, masks, ds = [], [], [], []
    for name, scale, flip, origin in cases:
        frame, annos, d = D.decision(name, scale, flip, crop, origin)
        items.append(D.item_of(frame, d, crop, taps))
        ref, mask = D.reference_f64(frame, annos, d, crop[0], crop[1])
        refs.append(ref), masks.append(mask), ds.append(d)
    src, params, rects, rect_off = A.pack_batch(items)
    pastes, paste_off, _, _ = A.pack_pastes(ds)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = (t(src.copy()), t(params), t(rects) if len(rects) else None, t(rect_off), taps.device(dev))
    mean, std = torch.tensor(C.MEAN, device=dev), torch.tensor(C.STD, device=dev)
    got = ops.augment_frames_pasted(*args, t(pastes) if len(pastes) else None, t(paste_off), mean, std, crop[0], crop[1])
    plain = ops.augment_frames(*args, mean, std, crop[0], crop[1])
    assert got.shape == (len(cases), 3, crop[0], crop[1]) and got.is_contiguous(memory_format=torch.channels_last)
    return (got.permute(0, 2, 3, 1).contiguous().cpu().numpy(), plain.permute(0, 2, 3, 1).contiguous().cpu().numpy(), ds,
            np.stack(refs), np.stack(masks))


def _check(got, plain, ds, refs, masks, what):
    worst = 0.0
    for k, d in enumerate(ds):
        m = masks[k]
        assert np.array_equal(C.bits(got[k][~m]), C.bits(plain[k][~m])), (what, k, "unpasted pixels")
        # where nothing was pasted the float64 reference differs by Normalize's two float32 roundings alone: the
        # difference (below 1) rounds by 2**-25, divided by min(std); the quotient (below 4) rounds by 2**-23
        assert np.abs(got[k][~m].astype(np.float64) - refs[k][~m]).max(initial=0) <= 2.0 ** -25 / min(C.STD) + 2.0 ** -23
        if m.any():
            err = float(np.abs(got[k].astype(np.float64) - refs[k])[m].max())
            e = D.bound(d.plan.depth)
            print(what, k, "pasted pixels", int(m.sum()), "depth", d.plan.depth, "err", err, "E", e)
            assert err <= e, (what, k, err, e)
            worst = max(worst, err / e)
    return worst


@pytest.mark.parametrize("name", D.PASTED_CASES + ("hand",))
def test_pasted_kernel_on_the_golden_frames(name):
    """B = 1, crop 64x64, scale {1, 1.5} x flip {0, 1} x three crop origins; at least one crop cuts through a pasted
    object and at least one holds a whole one."""
    taps = A.TapCache()
    cut = whole = 0
    for scale in (1, 1.5):
        for flip in (0, 1):
            for origin in C.ORIGINS:
                got, plain, ds, refs, masks = _run([(name, scale, flip, origin)], CROP, taps)
                _check(got, plain, ds, refs, masks, (name, scale, flip, origin))
                d = ds[0]
                for dy, dx, oh, ow in d.plan.pastes[:, 4:8].tolist():
                    box = np.zeros((d.dst_h, d.dst_w), bool)
                    box[dy:dy + oh, dx:dx + ow] = True
                    inside = int(D.to_crop(box, d, CROP[0], CROP[1], False).sum())
                    cut += 0 < inside < oh * ow
                    whole += inside == oh * ow
    assert cut > 0 and whole > 0


def test_pasted_kernel_mixed_batch_of_five():
    """Different frame sizes and scales in one launch, two frames with empty paste lists (they ship windows only), one
    aborted plan, padding in both dimensions."""
    crop = (80, 112)
    cases = [("base", 1.5, 1, "interior"), ("dense", 1, 0, "flush"), ("noroad", 1, 1, "zero"), ("nocls", 1.5, 0, "flush"),
             ("abort", 1, 1, "zero")]
    got, plain, ds, refs, masks = _run(cases, crop, A.TapCache())
    assert [A.n_pastes(d) > 0 for d in ds] == [True, True, False, False, True] and ds[4].plan.aborted_at >= 1
    assert ds[2].dst_h < crop[0] and ds[2].dst_w < crop[1] and ds[4].dst_h < crop[0] and ds[4].dst_w < crop[1]
    _check(got, plain, ds, refs, masks, "mixed")
    assert masks[0].any() and masks[1].any() and masks[4].any() and not masks[2].any() and not masks[3].any()


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    with_road = D.write_roadmaps(C.write_dataset(str(tmp_path_factory.mktemp("visdrone_road")), extra=3))
    return with_road, C.write_dataset(str(tmp_path_factory.mktemp("visdrone_plain")), extra=3)


def _loaders(root, chain, road, seed):
    from rrnet_amd.datasets.drones_det import DronesDET
    ds = DronesDET(root, chain, "train", with_road_map=road)
    assert len(ds) == 4
    p = A.chain_params(chain)
    return A.DeviceAugmentLoader(ds, p, 2, seed=seed, num_workers=4), A.HostAugmentLoader(ds, p, 2, seed=seed, num_workers=1)


def test_device_loader_equals_host_loader_with_pastes(roots):
    """Full chain, B=2, crop 128x128, four batches, same seed: annotations and targets equal, pasted pixels within
    2 E(depth) of the host chain (torch on the CPU), every other pixel bit-identical."""
    dev, host = _loaders(roots[0], D.full_chain((128, 128)), True, D.LOADER_SEED)
    pasted_in_crop = 0
    try:
        for j in range(4):
            a, b = dev.get_batch(), host.get_batch()
            assert a[7] == b[7]
            assert a[0].shape == (2, 3, 128, 128) and a[0].is_contiguous(memory_format=torch.channels_last)
            for k in range(1, 7):
                assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
            x, y = a[0].permute(0, 2, 3, 1).cpu().numpy(), b[0].permute(0, 2, 3, 1).cpu().numpy()
            for k in range(2):
                d = host._decide(*host._where(j * 2 + k))[3]
                assert d.plan is not None
                m = D.to_crop(D.pasted_mask(d.plan, d.dst_h, d.dst_w), d, 128, 128, False)
                assert np.array_equal(C.bits(x[k][~m]), C.bits(y[k][~m])), (j, k)
                if m.any():
                    pasted_in_crop += 1
                    err, e = float(np.abs(x[k].astype(np.float64) - y[k])[m].max()), D.bound(d.plan.depth)
                    print("loader batch", j, k, "pasted pixels", int(m.sum()), "depth", d.plan.depth, "err", err, "2E", 2 * e)
                    assert err <= 2 * e
    finally:
        dev.close()
        host.close()
    assert pasted_in_crop >= 1


def test_loaders_without_a_roadmap_folder_equal_the_chain_without_fillduck(roots):
    dev, host = _loaders(roots[1], D.full_chain((128, 128)), True, 5)
    dev0, host0 = _loaders(roots[1], D.full_chain((128, 128), fill_duck=False), False, 5)
    try:
        for _ in range(2):
            got = [l.get_batch() for l in (dev, host, dev0, host0)]
            for other in got[1:]:
                assert other[7] == got[0][7]
                assert torch.equal(got[0][0].view(torch.int32), other[0].view(torch.int32))
                for k in range(1, 7):
                    assert torch.equal(got[0][k], other[k]), k
    finally:
        for l in (dev, host, dev0, host0):
            l.close()


def test_train_step_under_the_fillduck_config(roots, tmp_path):
    """make_dataloader with rrnet_fillduck_config opens the road maps; one train_step of the tiny hourglass on a loader
    batch with pastes gives finite losses."""
    import copy
    from rrnet_amd.configs.rrnet_fillduck_config import Config
    from rrnet_amd.datasets import DeviceAugmentLoader
    from rrnet_amd.datasets.transforms import FillDuck, RandomCrop
    from rrnet_amd.operators.rrnet_operator import RRNetOperator
    cfg = copy.deepcopy(Config)
    cfg.data_root = roots[0]
    cfg.Train.batch_size, cfg.Train.crop_size, cfg.Train.num_workers = 2, (128, 128), 4
    cfg.Train.transforms.transforms = [RandomCrop((128, 128)) if isinstance(t, RandomCrop) else t
                                       for t in cfg.Train.transforms.transforms]
    assert any(isinstance(t, FillDuck) for t in cfg.Train.transforms.transforms)
    cfg.Val.result_dir, cfg.Val.model_path = str(tmp_path / "results"), str(tmp_path / "ckp.pth")
    cfg.Model.backbone = "hourglass_tiny"
    cfg.Distributed.gpu_id, cfg.Distributed.rank, cfg.Distributed.world_size = 0, 0, 1
    torch.manual_seed(219)
    op = RRNetOperator(cfg)
    try:
        loader = op.training_loader
        assert isinstance(loader, DeviceAugmentLoader) and loader.pasting and loader.dataset.with_road_map
        _, losses = op.train_step(0, loader.get_batch())
        assert all(bool(torch.isfinite(v)) for v in losses), losses
    finally:
        op.training_loader.close()

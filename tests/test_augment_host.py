"""CPU checks of the data layer: the host transforms against the reference's recorded outputs (tests/golden/augment.npz,
tools/gen_golden_augment.py), PIL's resize tables against live PIL, annotation parsing, the sampler, and the records
rr_augment_frames receives (through a numpy restatement of the kernel's index arithmetic)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch
from PIL import Image

import augment_cases as C
from rrnet_amd.datasets import augment as A
from rrnet_amd.datasets.drones_det import DronesDET, parse_annotations
from rrnet_amd.datasets.transforms import (Compose, HorizontalFlip, MaskIgnore, MultiScale, Normalize, RandomCrop,
                                           ToHeatmap, ToTensor)
from rrnet_amd.datasets.transforms import functional as F


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(C.GOLDEN, "augment.npz"))


def test_host_transforms_equal_the_reference(gold):
    """Pixels byte for byte (the float32 bits of the normalised crop), annotations exactly."""
    cut, annos, crop = gold["cut"], gold["annos"], tuple(int(v) for v in gold["crop"])
    mean, std = tuple(gold["mean"]), tuple(gold["std"])
    rc = RandomCrop(crop)
    for i, (s, flip, cx, cy) in enumerate(gold["cases"]):
        s = int(s) if s == int(s) else float(s)
        cx, cy = int(cx), int(cy)
        img, an = F.resize((Image.fromarray(cut), annos.copy()), s)
        assert np.array_equal(np.array(img), gold["resized_%d" % i])
        assert np.array_equal(an, gold["resized_annos_%d" % i])
        t, ta = ToTensor()((img, an))
        t, ta = MaskIgnore(mean)((t, ta))
        if flip:
            t, ta = F.flip_img(t), F.flip_annos(ta, t.size(2))
        assert np.array_equal(ta.numpy(), gold["flipped_annos_%d" % i])
        win = torch.tensor([[cx, cy, crop[1], crop[0]]])
        from rrnet_amd.utils.metrics.metrics import bbox_iou
        _, ov = bbox_iou(ta, win, x1y1x2y2=False, overlap=True)
        assert np.array_equal(ov.numpy(), gold["overlap_%d" % i], equal_nan=True)
        kept = rc.remove_bbox_outside(ta.clone(), win)
        assert np.array_equal(kept.numpy(), gold["kept_%d" % i])
        coor = (cx, cy, cx + crop[1], cy + crop[0])
        assert np.array_equal(F.crop_annos(kept.clone(), coor, crop[0], crop[1]).numpy(), gold["cropped_annos_%d" % i])
        th, tw = t.shape[-2:]
        t = torch.nn.functional.pad(t, [0, max(crop[1] - tw, 0), 0, max(crop[0] - th, 0)])
        px = Normalize(mean, std)((F.crop_tensor(t, coor), ta))[0]
        assert np.array_equal(C.bits(px.numpy()), C.bits(gold["pixels_%d" % i]))
    # the zero-area box of the fixture gives 0/0 = NaN and is dropped, as in the reference
    assert np.isnan(gold["overlap_0"]).any()


def test_integer_truncation_of_scaled_boxes():
    a = np.array([[517, 440, 25, 42, 1, 2, 0, 1]], dtype=np.int64)
    assert F.resize_annos(a, 1.15)[0, :4].tolist() == [594, 505, 28, 48]


@pytest.mark.parametrize("scale", [1, 1.15, 1.25, 1.35, 1.5, 1.1, 1.2, 1.3, 1.4])
def test_tap_tables_reproduce_pil(scale):
    """The five MultiScale factors and the six Val.scales on a random-noise 97x61 image."""
    img = np.random.default_rng(5).integers(0, 256, (61, 97, 3), dtype=np.uint8)
    oh, ow = F.scaled_size(61, 97, scale)
    ref = np.array(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
    assert np.array_equal(F.resize_u8_taps(img, oh, ow), ref)
    for n, o in ((61, oh), (97, ow)):
        t = F.pil_bilinear_taps(n, o)
        assert t[:, 0].min() >= 0 and (t[:, 0] + (t[:, 2] != 0)).max() < n and (np.diff(t[:, 0]) >= 0).all()


def test_shrinking_is_refused_with_the_limit_named():
    with pytest.raises(ValueError, match="scale factors >= 1"):
        A.chain_params(Compose([MultiScale((0.5, 1)), ToTensor(), Normalize(C.MEAN, C.STD)]))
    with pytest.raises(ValueError):
        F.pil_bilinear_taps(100, 50)


def test_demo_annotations_and_mask_ignore():
    annos = parse_annotations(os.path.join(C.DEMO_ROOT, "annotations", C.DEMO_NAME + ".txt"))
    assert annos.shape == (86, 8) and annos.dtype == np.int64 and not (annos[:, 5] == 11).any()
    assert int((annos[:, 5] == 0).sum()) == 5
    img = torch.rand(3, 540, 960)
    before = img.clone()
    out, kept = MaskIgnore(C.MEAN)((img, F.annos_to_tensor(annos)))
    assert kept.shape == (81, 8) and not (kept[:, 5] == 0).any()
    filled = torch.zeros(540, 960, dtype=torch.bool)
    for y0, y1, x0, x1 in F.ignore_rects(annos, 540, 960):
        filled[y0:y1, x0:x1] = True
    assert filled.any()
    mean = torch.tensor(C.MEAN).view(3, 1, 1)
    assert torch.equal(out[:, filled], mean.expand(3, 540, 960)[:, filled])
    assert torch.equal(out[:, ~filled], before[:, ~filled])


def _demo_sampler(crop=(96, 128), **kw):
    p = dict(C.PARAMS, scales=(1, 1.15, 1.25, 1.35, 1.5), crop=crop)
    return A.AugmentSampler(p, **kw), parse_annotations(os.path.join(C.DEMO_ROOT, "annotations", C.DEMO_NAME + ".txt"))


def test_sampler_is_independent_of_threads():
    s1, annos = _demo_sampler(seed=11)
    s2, _ = _demo_sampler(seed=11)
    jobs = [(e, i) for e in range(2) for i in range(24)]
    one = [s1.sample(annos, 540, 960, e, i).key() for e, i in jobs]
    with ThreadPoolExecutor(4) as ex:
        four = list(ex.map(lambda j: s2.sample(annos, 540, 960, *j).key(), reversed(jobs)))[::-1]
    assert one == four
    other, _ = _demo_sampler(seed=12)
    assert [other.sample(annos, 540, 960, e, i).key() for e, i in jobs] != one


def test_ranks_see_disjoint_indices_that_cover_the_set():
    for n, world in ((10, 2), (11, 2), (7, 3)):
        shards = [A.AugmentSampler(dict(C.PARAMS, crop=(64, 64)), seed=3, rank=r, world_size=world).indices(n, 4)
                  for r in range(world)]
        assert len({len(s) for s in shards}) == 1
        assert set(np.concatenate(shards).tolist()) == set(range(n))
        flat = np.concatenate(shards)
        assert len(flat) - len(set(flat.tolist())) == (-n) % world          # only the padding repeats
        again = A.AugmentSampler(dict(C.PARAMS, crop=(64, 64)), seed=3, rank=0, world_size=world).indices(n, 4)
        assert np.array_equal(again, shards[0])
        assert not np.array_equal(A.AugmentSampler(dict(C.PARAMS, crop=(64, 64)), seed=3).indices(n, 5),
                                  A.AugmentSampler(dict(C.PARAMS, crop=(64, 64)), seed=3).indices(n, 4))


def test_random_crop_invariants_over_200_draws():
    """Crop 128x96 on the demo annotations: every kept box lies in the window, kept boxes had overlap > 0.5, at least
    one box is always kept."""
    from rrnet_amd.utils.metrics.metrics import bbox_iou
    sampler, annos = _demo_sampler()
    H, W = 96, 128
    for i in range(200):
        d = sampler.sample(annos, 540, 960, 0, i)
        assert d.annos.size(0) >= 1
        a = d.annos
        assert (a[:, 0] >= 0).all() and (a[:, 1] >= 0).all() and (a[:, 0] + a[:, 2] <= W).all() and (a[:, 1] + a[:, 3] <= H).all()
        assert 0 <= d.crop_x0 <= max(d.dst_w, W) - W and 0 <= d.crop_y0 <= max(d.dst_h, H) - H
        # rebuild the boxes before the crop and match the kept ones
        t = F.annos_to_tensor(F.resize_annos(annos.copy(), d.scale))
        t = t[t[:, 5] != 0]
        if d.flip:
            F.flip_annos(t, d.dst_w)
        _, ov = bbox_iou(t, torch.tensor([[d.crop_x0, d.crop_y0, W, H]]), x1y1x2y2=False, overlap=True)
        big = (t[:, 2] > W) | (t[:, 3] > H)
        keep = (ov[:, 0] > 0.5) & ~big
        assert int(keep.sum()) == a.size(0)
        want = F.crop_annos(t[keep].clone(), (d.crop_x0, d.crop_y0, d.crop_x0 + W, d.crop_y0 + H), H, W)
        assert torch.equal(want, a)


def test_random_crop_transform_on_host_tensors():
    """The per-sample class itself (reference signature) keeps the same invariants and returns the crop size."""
    import random
    random.seed(4)
    np.random.seed(4)
    annos = parse_annotations(os.path.join(C.DEMO_ROOT, "annotations", C.DEMO_NAME + ".txt"))
    chain = Compose([MultiScale((1, 1.15)), ToTensor(), MaskIgnore(C.MEAN), HorizontalFlip(), RandomCrop((96, 128)),
                     Normalize(C.MEAN, C.STD)])
    frame = Image.open(os.path.join(C.DEMO_ROOT, "images", C.DEMO_NAME + ".jpg")).convert("RGB")
    for _ in range(3):
        img, a = chain((frame, annos.copy()))[:2]
        assert img.shape == (3, 96, 128) and a.size(0) >= 1 and a.shape[1] == 8
        assert (a[:, 0] + a[:, 2] <= 128).all() and (a[:, 1] + a[:, 3] <= 96).all()


@pytest.mark.parametrize("crop", C.CROPS)
def test_packed_records_reproduce_the_host_chain(crop):
    """pack_batch's windows, records and rectangles, run through the kernel's arithmetic in numpy, give the host chain's
    pixels bit for bit — the whole grid of the GPU test, so a wrong record is found without a GPU."""
    taps = A.TapCache()
    for name in C.SOURCES:
        cases = C.grid(name, crop)
        (src, params, rects, rect_off), refs = C.packed(cases, taps)
        got = C.kernel_model(src, params, rects, rect_off, taps.arena(), C.MEAN, C.STD, *crop)
        for k, c in enumerate(cases):
            assert np.array_equal(C.bits(got[k]), C.bits(refs[k])), c
        assert any(p[2] or p[3] for p in params)                         # some window does not start at (0, 0)
        h, w = C.source(name)[0].shape[:2]
        assert all(p[4] <= min(h, crop[0] + 2) and p[5] <= min(w, crop[1] + 2) for p in params)   # windows, not frames


def test_drones_det_index_and_collate(tmp_path):
    root = C.write_dataset(str(tmp_path), splits=("train",), extra=2)
    # an image whose only rows are an ignore region and class 11 is dropped at index time
    Image.fromarray(np.zeros((40, 40, 3), np.uint8)).save(os.path.join(root, "train", "images", "empty.jpg"))
    with open(os.path.join(root, "train", "annotations", "empty.txt"), "w") as f:
        f.write("1,1,5,5,0,0,0,0\n2,2,5,5,1,11,0,0,\n")
    ds = DronesDET(root, Compose([ToTensor(), Normalize(C.MEAN, C.STD)]), "train")
    assert len(ds) == 3 and ds.dropped == ["empty"] and ds.mdf == sorted(ds.mdf)
    batch = [ds[0], ds[1]]
    imgs_ok = batch[0][0].dtype == torch.float32 and batch[0][0].shape[0] == 3
    assert imgs_ok and batch[0][2] == ds.mdf[0]
    m = max(b[1].size(0) for b in batch)
    _, annos, names = DronesDET.collate_fn([(b[0][:, :32, :32], b[1], b[2]) for b in batch])
    assert annos.shape == (2, m, 8) and names == ds.mdf[:2]


def test_make_dataloader_without_a_dataset_is_unchanged(monkeypatch):
    """No <data_root>/train/images: exactly what it returned before, without touching the GPU here."""
    from rrnet_amd.configs.rrnet_config import Config as cfg
    from rrnet_amd.datasets import synthetic
    made = []

    class Fake:
        def __init__(self, *a, **k):
            made.append((a, k))

    monkeypatch.setattr(synthetic, "SyntheticDronesDET", Fake)
    monkeypatch.setattr(synthetic, "_LOADERS", {})
    assert not os.path.isdir(os.path.join(cfg.data_root, "train", "images"))
    train, val = synthetic.make_dataloader(cfg, collate_fn="rrnet")
    assert isinstance(train, Fake) and val is None and len(made) == 1
    assert made[0][0][1:] == (cfg.Train.batch_size,) + tuple(cfg.Train.crop_size)


def test_config_chains_are_the_reference_chain_without_fillduck():
    from rrnet_amd.configs.centernet_config import Config as ct
    from rrnet_amd.configs.rrnet_config import Config as rr
    for cfg in (rr, ct):
        assert [type(t) for t in cfg.Train.transforms.transforms] == [MultiScale, ToTensor, MaskIgnore, HorizontalFlip,
                                                                     RandomCrop, Normalize, ToHeatmap]
        assert [type(t) for t in cfg.Val.transforms.transforms] == [ToTensor, Normalize]
        p = A.chain_params(cfg.Train.transforms)
        assert p["scales"] == (1, 1.15, 1.25, 1.35, 1.5) and p["crop"] == (512, 512) and p["flip_p"] == 0.5
    import rrnet_amd.datasets as ds                  # what `import datasets` resolves to through shims/
    for name in ("DronesDET", "DeviceAugmentLoader", "HostAugmentLoader", "DeviceValLoader", "make_dataloader"):
        assert hasattr(ds, name)

"""CPU checks of FillDuck: fill_duck against the reference's recorded outputs (tests/golden/fillduck.npz), the host
pixel path against the float64 evaluation of the paste formula, chain_params, the sampler, road maps through DronesDET
and the transforms, and the nearest-neighbour resize."""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch
from PIL import Image

import augment_cases as C
import fillduck_cases as D
from rrnet_amd.datasets import augment as A
from rrnet_amd.datasets.drones_det import DronesDET, parse_annotations
from rrnet_amd.datasets.transforms import (Compose, FillDuck, HorizontalFlip, MaskIgnore, MultiScale, Normalize,
                                           RandomCrop, ToHeatmap, ToTensor)
from rrnet_amd.datasets.transforms import functional as F


def _to_tensor(frame):
    return torch.from_numpy(frame).permute(2, 0, 1).contiguous().float().div(255)


@pytest.mark.parametrize("name", [str(n) for n in D.golden()["names"]])
def test_fill_duck_reproduces_the_reference(name):
    """Torch-backed draws under the stored seed: annotations exactly (after the abort: the original rows, with the
    earlier pastes in the image), the same set of changed pixels, normalised values within E(depth)."""
    frame, road, annos, factor, seed, out_annos, idx, val = D.golden_case(name)
    img, before = _to_tensor(frame), _to_tensor(frame)
    torch.manual_seed(int(seed))
    plan = F.fill_duck_decide(torch.from_numpy(annos), torch.from_numpy(road).float() / 255, D.CLS_LIST, float(factor),
                              frame.shape[0], frame.shape[1], F.TorchRand)
    torch.manual_seed(int(seed))
    got_img, got_annos = F.fill_duck((img, torch.from_numpy(annos), torch.from_numpy(road).float() / 255),
                                     torch.tensor(D.CLS_LIST).unsqueeze(0), float(factor))
    assert got_img is img and np.array_equal(got_annos.numpy(), out_annos)
    changed = torch.nonzero((img.view(torch.int32) != before.view(torch.int32)).reshape(-1)).view(-1).numpy()
    assert np.array_equal(changed, idx)
    if name in ("noroad", "nocls"):
        assert len(plan.pastes) == 0 and plan.aborted_at == -1 and len(idx) == 0 and len(out_annos) == len(annos)
        return
    assert len(plan.pastes) > 0 and len(idx) > 0
    if name == "abort":
        assert plan.aborted_at == len(plan.pastes) >= 1 and len(out_annos) == len(annos) and plan.new_annos.size(0) == 0
    else:
        assert plan.aborted_at == -1 and len(out_annos) == len(annos) + plan.new_annos.size(0)
    std = torch.tensor(C.STD).view(3, 1, 1).expand(3, frame.shape[0], frame.shape[1]).reshape(-1)[idx]
    mean = torch.tensor(C.MEAN).view(3, 1, 1).expand(3, frame.shape[0], frame.shape[1]).reshape(-1)[idx]
    a = (img.reshape(-1)[idx] - mean) / std
    b = (torch.from_numpy(val) - mean) / std
    err = float((a.double() - b.double()).abs().max())
    print(name, "pastes", len(plan.pastes), "depth", plan.depth, "err", err, "E", D.bound(plan.depth))
    assert err <= D.bound(plan.depth)


def test_golden_cases_cover_what_they_claim():
    g = D.golden()
    base = D.golden_case("base")
    assert len(base[5]) - len(base[2]) > 5                       # 5 pastes, at least one of them a pair (two rows)
    assert not (D.golden_case("nodepth")[2][:, 5] == 1).any() and len(D.golden_case("two")[2]) <= 2
    assert D.golden_case("noroad")[1].sum() == 0
    assert all(g[n + "_frame"].shape[0] <= 96 and g[n + "_frame"].shape[1] <= 128 for n in g["names"])
    assert float(g["dense_factor"]) == 2e-3 and float(g["base_factor"]) == 5e-5


def test_apply_paste_plan_against_float64():
    """The hand-built plan (overlap, factor exactly 0.5 and 2, depth 3, 1 x k and k x 1 objects) on the host path."""
    frame = D.golden_case("base")[0]
    plan = D.hand_plan(*frame.shape[:2])
    img = F.apply_paste_plan(_to_tensor(frame), plan)
    ref = D.paste_f64(_to_tensor(frame).permute(1, 2, 0).numpy().astype(np.float64), plan)
    mask = D.pasted_mask(plan, *frame.shape[:2])
    got = img.permute(1, 2, 0).numpy()
    assert np.array_equal(got[~mask], _to_tensor(frame).permute(1, 2, 0).numpy()[~mask])
    mean, std = np.asarray(C.MEAN, np.float32), np.asarray(C.STD, np.float32)
    err = np.abs(((got - mean) / std).astype(np.float64) - (ref - mean.astype(np.float64)) / std.astype(np.float64))
    print("hand plan: host vs float64", err[mask].max(), "E", D.bound(plan.depth))
    assert err[mask].max() <= D.bound(plan.depth) and mask.sum() > 500
    rows = plan.pastes
    assert (rows[:, 6] == 2 * rows[:, 2]).any() and (2 * rows[:, 6] == rows[:, 2]).any()
    assert (rows[:, 6] == 1).any() and (rows[:, 7] == 1).any()


def test_interpolate_size_is_torchs():
    rng = np.random.default_rng(3)
    for _ in range(200):
        n, f = int(rng.integers(1, 40)), float(np.float32(rng.uniform(0.5, 2.0)))
        want = torch.nn.functional.interpolate(torch.zeros(1, 1, n, 1), scale_factor=(f, 1.0), mode='bilinear',
                                               align_corners=True).shape[2] if math.floor(n * f) > 0 else 0
        assert F.interpolate_size(n, f) == want, (n, f)
    for n, f in ((7, 0.5), (8, 0.5), (9, 2.0), (1, 0.5)):
        assert F.interpolate_size(n, f) == math.floor(n * f)


def _chain(fill_duck_at=3):
    ts = [MultiScale(scale=(1, 1.15, 1.5)), ToTensor(), MaskIgnore(C.MEAN), HorizontalFlip(), RandomCrop((64, 64)),
          Normalize(C.MEAN, C.STD), ToHeatmap(scale_factor=4)]
    if fill_duck_at is not None:
        ts.insert(fill_duck_at, FillDuck())
    return Compose(ts)


def test_chain_params_accepts_fillduck_only_after_maskignore():
    p = A.chain_params(_chain(3))
    assert p["fill_duck"] == dict(cls_list=(1, 2, 3, 7, 8, 10), factor=5e-5)
    assert A.chain_params(_chain(None))["fill_duck"] is None
    base, full = A.chain_params(_chain(None)), dict(p, fill_duck=None)
    assert base == full                                            # a chain without it lowers exactly as before
    for k in (0, 1, 2, 4, 5, 6, 7):
        with pytest.raises(NotImplementedError):
            A.chain_params(_chain(k))
    with pytest.raises(NotImplementedError):                       # no MaskIgnore in front of it
        A.chain_params(Compose([MultiScale((1,)), ToTensor(), FillDuck(), HorizontalFlip(), Normalize(C.MEAN, C.STD)]))
    from rrnet_amd.configs.rrnet_fillduck_config import Config
    from rrnet_amd.configs.rrnet_config import Config as Base
    assert [type(t) for t in Config.Train.transforms.transforms] == [MultiScale, ToTensor, MaskIgnore, FillDuck,
                                                                     HorizontalFlip, RandomCrop, Normalize, ToHeatmap]
    assert A.chain_params(Config.Train.transforms)["fill_duck"]["factor"] == 5e-5 and Config.Train.with_road
    assert len(Base.Train.transforms.transforms) == 7 and Config.Train.lr == Base.Train.lr


def _demo(crop=(96, 128), **kw):
    p = dict(D.PARAMS, scales=(1, 1.15, 1.25, 1.35, 1.5), crop=crop)
    annos = parse_annotations(os.path.join(C.DEMO_ROOT, "annotations", C.DEMO_NAME + ".txt"))
    road = np.zeros((540, 960), np.uint8)
    road[250:] = 255
    return p, annos, road


def test_sampler_without_a_road_map_decides_as_before():
    p, annos, _ = _demo()
    with_fd, without = A.AugmentSampler(p, seed=11), A.AugmentSampler(dict(p, fill_duck=None), seed=11)
    for i in range(24):
        a, b = with_fd.sample(annos, 540, 960, 1, i, None), without.sample(annos, 540, 960, 1, i)
        assert a.key() == b.key() and a.plan is None


def test_sampler_with_a_road_map_is_keyed_and_pastes_steer_the_crop():
    """Same keys whatever thread asks in whatever order; scale, flip and (where no redraw differs) the draws of the
    chain without FillDuck are untouched; pasted boxes reach d.annos after flip and crop."""
    p, annos, road = _demo()
    s1, s2 = A.AugmentSampler(p, seed=11), A.AugmentSampler(p, seed=11)
    jobs = [(e, i) for e in range(2) for i in range(10)]
    one = [s1.sample(annos, 540, 960, e, i, road) for e, i in jobs]
    with ThreadPoolExecutor(4) as ex:
        four = list(ex.map(lambda j: s2.sample(annos, 540, 960, *j, road).key(), reversed(jobs)))[::-1]
    assert [d.key() for d in one] == four
    plain = A.AugmentSampler(dict(p, fill_duck=None), seed=11)
    n_orig = int((annos[:, 5] != 0).sum())
    seen_pasted_box = 0
    for (e, i), d in zip(jobs, one):
        q = plain.sample(annos, 540, 960, e, i)
        if d.redraws == 0 and q.redraws == 0:
            assert (d.scale, d.flip) == (q.scale, q.flip)          # the first draws of the attempt are the same numbers
        assert d.plan is not None and len(d.plan.pastes) > 0
        for y0, x0, h, w in d.plan.pastes[:, [0, 1, 2, 3]].tolist() + d.plan.pastes[:, [4, 5, 6, 7]].tolist():
            assert 0 <= y0 and y0 + h <= d.dst_h and 0 <= x0 and x0 + w <= d.dst_w
        # rebuild: original rows + pasted rows -> flip -> the crop's filter
        t = F.annos_to_tensor(F.resize_annos(annos.copy(), d.scale))
        t = torch.cat((t[t[:, 5] != 0], d.plan.new_annos))
        if d.flip:
            F.flip_annos(t, d.dst_w)
        from rrnet_amd.utils.metrics.metrics import bbox_iou
        _, ov = bbox_iou(t, torch.tensor([[d.crop_x0, d.crop_y0, 128, 96]]), x1y1x2y2=False, overlap=True)
        keep = (ov[:, 0] > 0.5) & ~((t[:, 2] > 128) | (t[:, 3] > 96))
        want = F.crop_annos(t[keep].clone(), (d.crop_x0, d.crop_y0, d.crop_x0 + 128, d.crop_y0 + 96), 96, 128)
        assert torch.equal(want, d.annos)
        seen_pasted_box += int(keep[n_orig:].sum())
    assert seen_pasted_box > 0


def test_drones_det_road_maps_and_the_host_chain(tmp_path):
    root = C.write_dataset(str(tmp_path / "a"), splits=("train",), extra=2)
    chain = Compose(D.full_chain((64, 64)).transforms[:-1])                # ToHeatmap builds its targets on the GPU
    without = DronesDET(root, chain, "train", with_road_map=True)          # no roadmap folder: None, data unchanged
    assert without.load(0)[3] is None and len(without.load(0)) == 4
    assert len(DronesDET(root, chain, "train").load(0)) == 3
    D.write_roadmaps(root)
    ds = DronesDET(root, chain, "train", with_road_map=True)
    img, annos, name, road = ds.load(1)
    assert road.dtype == np.uint8 and road.shape == (img.size[1], img.size[0])
    assert road[-1, -1] >= 250 and road[0, 0] <= 5
    os.remove(os.path.join(root, "train", "roadmap", name + ".jpg"))
    assert ds.load(1)[3] is None and ds.load(0)[3] is not None
    # the transform classes carry the road map to FillDuck and two-element samples still pass
    import random
    random.seed(2)
    np.random.seed(2)
    torch.manual_seed(2)
    sample = ds[0]
    assert sample[0].shape == (3, 64, 64) and sample[1].shape[1] == 8 and len(sample) == 3
    t = Compose([MultiScale((1.5,)), ToTensor(), MaskIgnore(C.MEAN)])((img, annos.copy(), np.full((img.size[1], img.size[0]), 255, np.uint8)))
    assert t[2].shape == t[0].shape[1:] and t[2].dtype == torch.float32
    x, y, w, h = (int(v * 1.5) for v in annos[annos[:, 5] == 0][0, :4])
    assert float(t[2][y:y + h, x:x + w].sum()) == 0 and float(t[2].sum()) > 0
    two = Compose([MultiScale((1.5,)), ToTensor(), MaskIgnore(C.MEAN), FillDuck()])((img, annos.copy()))
    assert len(two) == 2 and torch.equal(two[0], t[0])
    none = FillDuck()((t[0], t[1], None))
    assert none[0] is t[0] and none[1] is t[1]


def test_nearest_resize_against_plain_loops():
    rng = np.random.default_rng(5)
    for (h, w), (oh, ow) in (((7, 5), (10, 7)), ((540, 960), (621, 1104)), ((13, 9), (13, 9)), ((30, 20), (45, 30))):
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        want = np.empty((oh, ow), np.uint8)
        for y in range(oh):
            sy = min(int(math.floor(y * (1.0 / (float(oh) / h)))), h - 1)
            for x in range(ow):
                want[y, x] = a[sy, min(int(math.floor(x * (1.0 / (float(ow) / w)))), w - 1)]
        assert np.array_equal(F.nearest_resize(a, oh, ow), want)
    assert np.array_equal(F.nearest_resize(np.arange(4).reshape(2, 2), 4, 4), np.repeat(np.repeat(np.arange(4).reshape(2, 2), 2, 0), 2, 1))


def test_packed_records_and_pastes_reproduce_the_reference():
    """pack_batch + pack_pastes for the mixed batch of the GPU test, run through the pasted kernel's arithmetic in numpy:
    unpasted pixels equal rr_augment_frames' arithmetic (augment_cases.kernel_model) bit for bit, pasted pixels lie
    within E(depth) of the float64 evaluation, and no pixel outside a frame's crop is read where the frame ships a
    window only — a wrong record is found without a GPU."""
    crop = (80, 112)
    cases = [("base", 1.5, 1, "interior"), ("dense", 1, 0, "flush"), ("noroad", 1, 1, "zero"), ("nocls", 1.5, 0, "flush"),
             ("abort", 1, 1, "zero"), ("hand", 1, 1, "flush")]
    taps = A.TapCache()
    items, refs, masks, ds = [], [], [], []
    for name, scale, flip, origin in cases:
        frame, annos, d = D.decision(name, scale, flip, crop, origin)
        items.append(D.item_of(frame, d, crop, taps))
        ref, mask = D.reference_f64(frame, annos, d, *crop)
        refs.append(ref), masks.append(mask), ds.append(d)
    src, params, rects, rect_off = A.pack_batch(items)
    pastes, paste_off, canvas_pix, scratch_pix = A.pack_pastes(ds)
    assert paste_off.tolist() == np.concatenate([[0], np.cumsum([A.n_pastes(d) for d in ds])]).tolist()
    assert canvas_pix == 144 * 192 and scratch_pix == int((pastes[:, 6] * pastes[:, 7]).max())
    whole = [int(p[4] * p[5]) == it[1] * it[2] for p, it in zip(params, items)]
    assert all(whole[k] for k in (0, 1, 4, 5)) and not whole[3]      # pasted samples ship frames, the others windows
    got = D.pasted_kernel_model(src, params, rects, rect_off, taps.arena(), pastes, paste_off, C.MEAN, C.STD, *crop)
    plain = C.kernel_model(src, params, rects, rect_off, taps.arena(), C.MEAN, C.STD, *crop)
    assert not np.isnan(got).any()
    for k, d in enumerate(ds):
        m = masks[k]
        assert np.array_equal(C.bits(got[k][~m]), C.bits(plain[k][~m])), cases[k]
        if m.any():
            assert np.abs(got[k].astype(np.float64) - refs[k])[m].max() <= D.bound(d.plan.depth), cases[k]
    bad = F.PastePlan()
    bad.pastes = D.plan_from_rows([(0, 0, 4, 4, 10, 10, 8, 8)], 96, 128).pastes.copy()
    bad.pastes[0, 5] = 125                                           # the object leaves the frame on the right
    ds[1].plan = bad
    with pytest.raises(RuntimeError):
        A.pack_pastes(ds)

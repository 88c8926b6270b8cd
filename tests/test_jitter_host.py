"""CPU checks of ColorJitter: the restatement of PIL's ImageEnhance chain (tests/jitter_cases.py) against PIL and against
the reference's recorded outputs (tests/golden/jitter.npz), the integer grey mean, chain_params, the sampler's factors,
the transform class, the packing precondition and the header."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image, ImageStat

import augment_cases as C
import fillduck_cases as D
import jitter_cases as J
from rrnet_amd.datasets import augment as A
from rrnet_amd.datasets.drones_det import parse_annotations
from rrnet_amd.datasets.transforms import (ColorJitter, Compose, HorizontalFlip, MaskIgnore, MultiScale, Normalize,
                                           RandomCrop, ToHeatmap, ToTensor)
from rrnet_amd.datasets.transforms import functional as F


def test_restatement_equals_pil_on_random_frames():
    """300 frames of 1x1 to 40x40 pixels (noise, dark, nearly saturated), factors in [0.5, 1.5] with draws of exactly 1,
    plus every fixed triple of the GPU test: byte for byte."""
    rng = np.random.default_rng(219)
    n_bytes = 0
    for k in range(300):
        h, w = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        img = J.random_frame(rng, h, w)
        f = [1.0 if rng.random() < 0.15 else float(rng.uniform(0.5, 1.5)) for _ in range(3)]
        assert np.array_equal(J.jitter(img, *f), J.pil_jitter(img, *f)), (k, h, w, f)
        n_bytes += img.size
    img = C.source("noise_97x61")[0]
    for f in J.TRIPLES:
        assert np.array_equal(J.jitter(img, *f), J.pil_jitter(img, *f)), f
    assert np.array_equal(J.jitter(img, 1, 1, 1), img)
    assert n_bytes > 100000


def test_restatement_and_host_function_equal_the_recorded_reference():
    g = J.golden()
    cut = C.source("demo_cut")[0]
    assert len(g["factors"]) == len(g["cases"]) == 6
    for i, f in enumerate(g["factors"].tolist()):
        want = g["out_%d" % i]
        assert want.shape == cut.shape and want.dtype == np.uint8
        assert np.array_equal(J.jitter(cut, *f), want), i
        assert np.array_equal(J.pil_jitter(cut, *f), want), i
    lo, hi = g["factors"].min(), g["factors"].max()
    assert lo < 0.3 and hi > 1.7                                   # the wide cases reach far from the identity
    assert any((g["out_%d" % i] == 0).any() and (g["out_%d" % i] == 255).any() for i in range(6))


def test_integer_mean_equals_pils_rounded_mean():
    halves = np.zeros((1, 2, 3), np.uint8)
    halves[0, 0], halves[0, 1] = 10, 11
    assert J.gray(halves).tolist() == [[10, 11]] and J.gray_mean(halves, 1.0) == 11
    rng = np.random.default_rng(5)
    for k in range(400):
        h, w = int(rng.integers(1, 9)), int(rng.integers(1, 9)) * 2
        img = J.random_frame(rng, h, w)
        if k % 2:                                                  # an exact half: grey pixels v and v + 1, half each
            v = int(rng.integers(0, 255))
            img = np.full((h, w, 3), v, np.uint8)
            img.reshape(-1, 3)[rng.permutation(h * w)[:h * w // 2]] = v + 1
            assert int(J.gray(img).sum()) * 2 == (2 * v + 1) * h * w
        want = int(ImageStat.Stat(Image.fromarray(img).convert("L")).mean[0] + 0.5)
        assert J.gray_mean(img, 1.0) == want, k
    assert np.array_equal(J.gray(C.source("demo_cut")[0]),
                          np.asarray(Image.fromarray(C.source("demo_cut")[0]).convert("L"), dtype=np.int64))


def _tail(crop=(64, 64)):
    return [MultiScale(scale=(1, 1.15, 1.5)), ToTensor(), MaskIgnore(C.MEAN), HorizontalFlip(), RandomCrop(crop),
            Normalize(C.MEAN, C.STD), ToHeatmap(scale_factor=4)]


def test_chain_params_accepts_color_jitter_first_only():
    ts = _tail()
    p = A.chain_params(Compose([ColorJitter(0.5, 0.3, 1.2)] + ts))
    assert p["jitter"] == ((0.5, 1.5), (0.7, 1.3), (0, 2.2))
    base = A.chain_params(Compose(ts))
    assert base["jitter"] is None and dict(p, jitter=None) == base  # everything else lowers as without it
    assert A.chain_params(Compose([ColorJitter()] + ts[1:]))["jitter"] is not None        # in front of ToTensor
    for bad in (ts[:1] + [ColorJitter()] + ts[1:],                 # behind MultiScale
                ts[:2] + [ColorJitter()] + ts[2:],                 # behind ToTensor
                [ColorJitter(), ColorJitter()] + ts):              # twice
        with pytest.raises(NotImplementedError, match="ColorJitter"):
            A.chain_params(Compose(bad))


def _demo(fill_duck):
    p = dict(D.PARAMS if fill_duck else C.PARAMS, scales=(1, 1.15, 1.25, 1.35, 1.5), crop=(96, 128))
    annos = parse_annotations(os.path.join(C.DEMO_ROOT, "annotations", C.DEMO_NAME + ".txt"))
    road = np.zeros((540, 960), np.uint8)
    road[250:] = 255
    return p, annos, (road if fill_duck else None)


@pytest.mark.parametrize("fill_duck", (False, True), ids=("plain", "fillduck"))
def test_sampler_draws_factors_from_a_generator_of_their_own(fill_duck):
    """With ColorJitter the decisions equal those of the chain without it in every field but the factors; the factors
    lie in their ranges and depend on (seed, rank, epoch, index) alone."""
    p, annos, road = _demo(fill_duck)
    ranges = ((0.5, 1.5), (0.7, 1.3), (0.0, 2.2))
    pj = dict(p, jitter=ranges)
    plain, jit, again = A.AugmentSampler(p, seed=11), A.AugmentSampler(pj, seed=11), A.AugmentSampler(pj, seed=11)
    seen = set()
    jobs = [(e, i) for e in range(2) for i in range(8 if fill_duck else 24)]
    for e, i in jobs:
        a, b = plain.sample(annos, 540, 960, e, i, road), jit.sample(annos, 540, 960, e, i, road)
        assert a.jitter is None and a.key()[:-1] == b.key()[:-1] and a.key()[-1] is None
        assert b.key()[-1] == b.jitter and len(b.jitter) == 3
        for f, (lo, hi) in zip(b.jitter, ranges):
            assert lo <= f <= hi and float(np.float32(f)) == f
        seen.add(b.jitter)
        if fill_duck:
            assert b.plan is not None and len(b.plan.pastes) > 0
    assert len(seen) == len(jobs)
    for e, i in reversed(jobs[:6]):                                 # any order, another sampler object
        assert again.sample(annos, 540, 960, e, i, road).jitter == jit.sample(annos, 540, 960, e, i, road).jitter
    e, i = jobs[3]
    base = jit.sample(annos, 540, 960, e, i, road).jitter
    for other in (A.AugmentSampler(pj, seed=12), A.AugmentSampler(pj, seed=11, rank=1, world_size=2)):
        assert other.sample(annos, 540, 960, e, i, road).jitter != base
    assert jit.sample(annos, 540, 960, e + 1, i, road).jitter != base
    assert jit.sample(annos, 540, 960, e, i + 1, road).jitter != base
    # the annotations passed in, another frame size: not an input of the factors
    assert jit.sample(annos[:40], 540, 960, e, i, road).jitter == base


def test_seek_reproduces_the_factors_of_a_batch(tmp_path):
    from rrnet_amd.datasets.drones_det import DronesDET
    root = C.write_dataset(str(tmp_path), splits=("train",), extra=3)
    chain = J.chain((64, 64))
    ds = DronesDET(root, chain, "train")
    p = A.chain_params(chain)
    one, two = A.HostAugmentLoader(ds, p, 2, seed=5, num_workers=2), A.HostAugmentLoader(ds, p, 2, seed=5, num_workers=2)
    try:
        batches = [[r[0].jitter for r in one._collect(j)] for j in range(4)]
        assert all(f is not None for b in batches for f in b) and len({f for b in batches for f in b}) == 8
        two.seek(3)
        assert two.position() == 3 and [r[0].jitter for r in two._collect(two.position())] == batches[3]
        two.seek(1)
        got = two._collect(two.position())
        assert [r[0].jitter for r in got] == batches[1]
        # the host loader's pixels are the chain with exactly these factors
        for k, (d, pix, name) in enumerate(got):
            image, annos = ds.load(ds.mdf.index(name))[:2]
            want = A.host_chain(F.color_jitter(image, *d.jitter), annos, _without_jitter(d), p, 64, 64)
            assert torch.equal(pix.view(torch.int32), want.view(torch.int32))
    finally:
        one.close()
        two.close()


def _without_jitter(d):
    q = A.Decision()
    for k in A.Decision.__slots__:
        setattr(q, k, getattr(d, k))
    q.jitter = None
    return q


def test_transform_class_draws_in_the_reference_order():
    t = ColorJitter(0.4, 0.3, 0.9)
    assert (t.brightness, t.contrast, t.saturation) == ([0.6, 1.4], [0.7, 1.3], [max(1 - 0.9, 0), 1.9])
    assert ColorJitter(1.5).brightness == [0, 2.5]
    d = ColorJitter()
    assert (d.brightness, d.contrast, d.saturation) == ([0.5, 1.5],) * 3
    img = Image.fromarray(C.source("demo_cut")[0])
    annos = C.source("demo_cut")[1]
    for seed in range(4):
        random.seed(seed)
        out = t((img, annos, "rest"))
        random.seed(seed)
        b, c, s = random.uniform(*t.brightness), random.uniform(*t.contrast), random.uniform(*t.saturation)
        assert out[1] is annos and out[2] == "rest" and isinstance(out[0], Image.Image)
        assert np.array_equal(np.asarray(out[0]), np.asarray(F.color_jitter(img, b, c, s)))
        assert np.array_equal(np.asarray(out[0]), J.jitter(np.asarray(img), b, c, s))
    import rrnet_amd.datasets.transforms as T
    assert T.ColorJitter is ColorJitter and T.functional.color_jitter is F.color_jitter


def test_a_jittered_sample_must_ship_its_whole_frame():
    img, annos = C.source("noise_160x90")
    taps = A.TapCache()
    d = J.jittered_decision(img, annos, (0.9, 1.1, 1.2), 1.5, 0, (64, 64), "interior")
    window = C.item_of(img, d, (64, 64), taps)
    assert tuple(window[3][:4]) != (0, 0, 90, 160)
    with pytest.raises(ValueError, match="whole frame"):
        A.pack_batch([window])
    with pytest.raises(ValueError, match="whole frame"):
        A.pack_jitter([window])
    whole = J.item_of(img, d, (64, 64), taps)
    src, params, _, _ = A.pack_batch([whole])
    factors, max_pixels = A.pack_jitter([whole, whole])
    assert src.size == img.size and params[0, 2:6].tolist() == [0, 0, 90, 160] and max_pixels == 90 * 160
    assert factors.dtype == np.float32 and factors.tolist() == [list(d.jitter)] * 2
    d.jitter = None                                                 # an unjittered sample may ship a window: factors 1
    assert A.pack_jitter([C.item_of(img, d, (64, 64), taps)])[0].tolist() == [[1, 1, 1]]


def test_whole_frame_records_reproduce_the_unjittered_host_chain():
    """Shipping the whole frame instead of the window changes the record, not the pixels (the kernel's arithmetic in
    numpy on both)."""
    taps = A.TapCache()
    for case in C.grid("noise_97x61", (50, 62))[::3]:
        img, annos = C.source(case[0])
        d = C.decision(img, annos, *case[1:])
        src, params, rects, rect_off = A.pack_batch([J.item_of(img, d, case[3], taps)])
        got = C.kernel_model(src, params, rects, rect_off, taps.arena(), C.MEAN, C.STD, *case[3])
        assert np.array_equal(C.bits(got[0]), C.bits(C.host_reference(*case))), case


def test_header_declares_the_jitter_entries():
    from ctypes import c_int, c_long, c_void_p
    from rrnet_amd import _C
    sigs = _C.header_signatures()
    assert sigs["rr_jitter_gray_mean"] == (c_int, [c_void_p, c_long] + [c_void_p] * 4 + [c_int, c_long, c_void_p])
    plain, jit = sigs["rr_augment_frames"][1], sigs["rr_augment_frames_jitter"][1]
    assert jit == plain[:9] + [c_void_p, c_void_p] + plain[9:]
    plain, jit = sigs["rr_augment_frames_pasted"][1], sigs["rr_augment_frames_pasted_jitter"][1]
    assert jit == plain[:11] + [c_void_p, c_void_p] + plain[11:]

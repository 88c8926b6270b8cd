"""ColorJitter on the device: rr_jitter_gray_mean against the integer restatement, the jittered kernels against the host
chain with PIL's ImageEnhance in front (bit for bit; pasted pixels within E(depth)), the identity at factors (1, 1, 1),
the two loaders and one run of tools/train.py --color-jitter.  Every comparison but the pasted pixels is integer
equality."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_cases as C
import fillduck_cases as D
import jitter_cases as J
from rrnet_amd.datasets import augment as A
from rrnet_amd.datasets.transforms import functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_gray_mean_equals_the_restatement():
    """Ten frames packed back to back (1x1, two pixels whose mean is 10.5, 3x5, 17x31, 64x64, the demo cut, 257x513, an
    all-255 frame at brightness 1.5, brightness 0, brightness 1): the sums and the rounded means, the same words on a
    second call, and on buffers that start 1, 2 and 3 bytes off a dword."""
    from rrnet_amd import ops
    frames = J.mean_batch()
    (src, params, _, _), factors = J.plain_records(frames)
    want_sum = [J.gray_sum(img, b) for _, img, b in frames]
    want_mean = [J.gray_mean(img, b) for _, img, b in frames]
    by_name = dict(zip((f[0] for f in frames), want_mean))
    assert by_name["halves"] == 11 and by_name["white"] == 255 and by_name["black_by_factor"] == 0
    offsets = params[:, 11].tolist()
    assert len({o % 4 for o in offsets}) == 4 and len({o % 16 for o in offsets}) >= 5
    max_pixels = max(img.shape[0] * img.shape[1] for _, img, _ in frames)
    prm, fac = _t(params), _t(factors)
    gray, sums = ops.jitter_gray_mean(_t(src.copy()), prm, fac, max_pixels)
    assert gray.dtype == torch.int32 and sums.dtype == torch.int64
    assert sums.cpu().tolist() == want_sum and gray.cpu().tolist() == want_mean
    gray2, sums2 = ops.jitter_gray_mean(_t(src.copy()), prm, fac, max_pixels, work=(sums.clone().fill_(77), gray.clone()))
    assert torch.equal(sums2, sums) and torch.equal(gray2, gray)
    gray3, _ = ops.jitter_gray_mean(_t(src.copy()), prm, fac)          # the largest frame read back from the records
    assert torch.equal(gray3, gray)
    for shift in (1, 2, 3):
        buf = torch.zeros(src.size + shift, dtype=torch.uint8, device=DEV)
        buf[shift:] = _t(src.copy())
        g, s = ops.jitter_gray_mean(buf[shift:], prm, fac, max_pixels)
        assert s.cpu().tolist() == want_sum and g.cpu().tolist() == want_mean, shift


def _run(cases, crop, taps):
    """cases: [(source, factors, scale, flip, crop, origin)] of one crop size -> (device [B,h,w,3], host [B,h,w,3])."""
    from rrnet_amd import ops
    items, refs = [], []
    for name, factors, scale, flip, _, origin in cases:
        img, annos = C.source(name)
        d = J.jittered_decision(img, annos, factors, scale, flip, crop, origin)
        items.append(J.item_of(img, d, crop, taps))
        refs.append(J.host_reference(name, tuple(factors), scale, flip, crop, origin))
    src, params, rects, rect_off = A.pack_batch(items)
    factors, max_pixels = A.pack_jitter(items)
    args = (_t(src.copy()), _t(params), _t(rects) if len(rects) else None, _t(rect_off), taps.device(DEV))
    mean, std = torch.tensor(C.MEAN, device=DEV), torch.tensor(C.STD, device=DEV)
    gray, _ = ops.jitter_gray_mean(args[0], args[1], _t(factors), max_pixels)
    out = ops.augment_frames_jitter(*args, _t(factors), gray, mean, std, crop[0], crop[1])
    assert out.shape == (len(cases), 3, crop[0], crop[1]) and out.is_contiguous(memory_format=torch.channels_last)
    return out.permute(0, 2, 3, 1).contiguous().cpu().numpy(), np.stack(refs), (args, mean, std)


@pytest.mark.parametrize("factors", J.TRIPLES, ids=lambda f: "b%g_c%g_s%g" % f)
def test_jittered_kernel_is_bit_identical_to_the_host_path(factors):
    """Every (scale, flip, origin) of augment_cases for each source and crop size, one launch per (source, crop):
    ignore rectangles crossing crop edges and moving under the flip, frames smaller than the crop (right and bottom
    padding), PIL's ImageEnhance on the CPU as the reference."""
    if factors == (1.5, 1.5, 1.5):
        out = J.jitter(C.source("noise_97x61")[0], *factors)
        assert (out == 0).any() and (out == 255).any()              # all three clip branches are taken
        x = J.brightness(C.source("noise_97x61")[0], 1.5)
        assert (x == 255).any() and ((x > 0) & (x < 255)).any()
    if factors == (1, 0, 1):
        img = C.source("demo_cut")[0]
        assert (J.jitter(img, *factors) == J.gray_mean(img, 1)).all()
    taps = A.TapCache()
    padded = ignored = 0
    for name in C.SOURCES:
        for crop in C.CROPS:
            cases = [(c[0], factors) + c[1:] for c in C.grid(name, crop)]
            got, ref, _ = _run(cases, crop, taps)
            for k, case in enumerate(cases):
                assert np.array_equal(C.bits(got[k]), C.bits(ref[k])), case
            h, w = C.source(name)[0].shape[:2]
            padded += sum(F.scaled_size(h, w, c[2])[0] < crop[0] and F.scaled_size(h, w, c[2])[1] < crop[1] for c in cases)
            ignored += int((got == 0).all(-1).sum())                # +0.0 in all channels: an ignore rectangle
    assert padded > 0 and ignored > 0


def test_jittered_kernel_mixed_batch_of_five():
    """Five frames of different sizes, scales, flips and origins in one launch, each with its own factors."""
    taps = A.TapCache()
    triples = ((0.73, 1.41, 0), (1.5, 1.5, 1.5), (1, 1, 1), (0.5, 1.3, 1.9), (1.21, 0, 0.4))
    for crop in C.CROPS:
        cases = [(n, f, s, fl, crop, o) for (n, s, fl, o), f in zip(C.MIXED, triples)]
        got, ref, _ = _run(cases, crop, taps)
        assert np.array_equal(C.bits(got), C.bits(ref)), crop


def test_identity_factors_reproduce_the_unjittered_entry():
    from rrnet_amd import ops
    taps = A.TapCache()
    crop = (50, 62)
    cases = [(n, (1, 1, 1), s, fl, crop, o) for n, s, fl, o in C.MIXED]
    got, _, (args, mean, std) = _run(cases, crop, taps)
    plain = ops.augment_frames(*args, mean, std, crop[0], crop[1]).permute(0, 2, 3, 1).contiguous().cpu().numpy()
    assert np.array_equal(C.bits(got), C.bits(plain))
    # the same samples as windows, as the unjittered loader ships them
    (src, params, rects, rect_off), refs = C.packed([(n, s, fl, crop, o) for n, s, fl, o in C.MIXED], taps)
    assert np.array_equal(C.bits(got), C.bits(refs))


def _pasted(cases, crop, taps):
    """cases: [(name, factors, scale, flip, origin)] -> (device [B,h,w,3], host chain [B,h,w,3], masks, decisions,
    the launch arguments)."""
    from PIL import Image
    from rrnet_amd import ops
    items, refs, masks, ds = [], [], [], []
    for name, factors, scale, flip, origin in cases:
        frame, annos, d = D.decision(name, scale, flip, crop, origin)
        d.jitter = tuple(float(np.float32(f)) for f in factors)
        items.append(J.item_of(frame, d, crop, taps))
        ref = A.host_chain(Image.fromarray(frame), annos, d, C.PARAMS, crop[0], crop[1])
        refs.append(ref.permute(1, 2, 0).contiguous().numpy())
        masks.append(D.to_crop(D.pasted_mask(d.plan, d.dst_h, d.dst_w), d, crop[0], crop[1], False))
        ds.append(d)
    src, params, rects, rect_off = A.pack_batch(items)
    pastes, paste_off, _, _ = A.pack_pastes(ds)
    factors, max_pixels = A.pack_jitter(items)
    args = (_t(src.copy()), _t(params), _t(rects) if len(rects) else None, _t(rect_off), taps.device(DEV),
            _t(pastes) if len(pastes) else None, _t(paste_off))
    mean, std = torch.tensor(C.MEAN, device=DEV), torch.tensor(C.STD, device=DEV)
    gray, _ = ops.jitter_gray_mean(args[0], args[1], _t(factors), max_pixels)
    got = ops.augment_frames_pasted_jitter(*args, _t(factors), gray, mean, std, crop[0], crop[1])
    return got.permute(0, 2, 3, 1).contiguous().cpu().numpy(), np.stack(refs), np.stack(masks), ds, (args, mean, std)


def test_pasted_kernel_with_jitter_against_the_host_chain():
    """FillDuck's pastes on the jittered canvas: unpasted pixels bit-identical to the host chain, pasted pixels within
    E(depth), the bound functional.apply_paste_plan states; a frame without pastes rides in the same launch."""
    crop = (80, 112)
    cases = [("hand", (0.73, 1.41, 0), 1, 0, "interior"), ("base", (1.5, 1.5, 1.5), 1.5, 1, "interior"),
             ("dense", (0.5, 0.5, 0.5), 1, 0, "flush"), ("noroad", (1.2, 0.8, 1.6), 1, 1, "zero"),
             ("hand", (1.31, 0.67, 1.9), 1.5, 1, "zero")]
    got, ref, masks, ds, _ = _pasted(cases, crop, A.TapCache())
    assert [A.n_pastes(d) > 0 for d in ds] == [True, True, True, False, True]
    pasted = 0
    for k, d in enumerate(ds):
        m = masks[k]
        assert np.array_equal(C.bits(got[k][~m]), C.bits(ref[k][~m])), (cases[k], "unpasted pixels")
        if m.any():
            err, e = float(np.abs(got[k].astype(np.float64) - ref[k])[m].max()), D.bound(d.plan.depth)
            print(cases[k], "pasted pixels", int(m.sum()), "depth", d.plan.depth, "err", err, "E", e)
            assert err <= e, (cases[k], err, e)
            pasted += 1
    assert pasted >= 3


def test_identity_factors_reproduce_the_unjittered_pasted_entry():
    from rrnet_amd import ops
    crop = (80, 112)
    cases = [("hand", (1, 1, 1), 1, 0, "interior"), ("base", (1, 1, 1), 1.5, 1, "interior"),
             ("noroad", (1, 1, 1), 1, 1, "zero")]
    got, _, masks, _, (args, mean, std) = _pasted(cases, crop, A.TapCache())
    plain = ops.augment_frames_pasted(*args, mean, std, crop[0], crop[1]).permute(0, 2, 3, 1).contiguous().cpu().numpy()
    assert masks.any() and np.array_equal(C.bits(got), C.bits(plain))


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    plain = C.write_dataset(str(tmp_path_factory.mktemp("visdrone_jitter")), extra=3)
    return plain, D.write_roadmaps(C.write_dataset(str(tmp_path_factory.mktemp("visdrone_jitter_road")), extra=3))


def _loaders(root, chain, road):
    from rrnet_amd.datasets.drones_det import DronesDET
    ds = DronesDET(root, chain, "train", with_road_map=road)
    assert len(ds) == 4
    p = A.chain_params(chain)
    assert p["jitter"] is not None
    return A.DeviceAugmentLoader(ds, p, 2, seed=5, num_workers=4), A.HostAugmentLoader(ds, p, 2, seed=5, num_workers=1)


def test_device_loader_equals_host_loader_with_jitter(roots):
    """The jittered chain on the generated data set, B=2, crop 128x128, two batches, same seed: pixels bit-identical,
    annotations and targets equal; the unjittered loader on the same seed gives other pixels and the same annotations."""
    dev, host = _loaders(roots[0], J.chain((128, 128)), False)
    from rrnet_amd.datasets.drones_det import DronesDET
    plain_chain = _chain_without_jitter((128, 128))
    plain = A.DeviceAugmentLoader(DronesDET(roots[0], plain_chain, "train"), A.chain_params(plain_chain), 2, seed=5,
                                  num_workers=4)
    try:
        assert dev.jitter and not plain.jitter
        for _ in range(2):
            a, b, c = dev.get_batch(), host.get_batch(), plain.get_batch()
            assert a[7] == b[7] == c[7]
            assert a[0].shape == (2, 3, 128, 128) and a[0].is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
            assert not torch.equal(a[0], c[0])
            for k in range(1, 7):
                assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    finally:
        for l in (dev, host, plain):
            l.close()


def _chain_without_jitter(crop):
    from rrnet_amd.datasets.transforms import Compose
    return Compose(J.chain(crop).transforms[1:])


def test_device_loader_equals_host_loader_with_jitter_and_pastes(roots):
    """ColorJitter and FillDuck in one chain: the loader takes rr_augment_frames_pasted_jitter; unpasted pixels
    bit-identical, pasted pixels within 2 E(depth) of the host chain (each side within E of the exact blend)."""
    dev, host = _loaders(roots[1], J.chain((128, 128), fill_duck=True), True)
    pasted = 0
    try:
        assert dev.jitter and dev.pasting
        for j in range(2):
            a, b = dev.get_batch(), host.get_batch()
            assert a[7] == b[7]
            for k in range(1, 7):
                assert torch.equal(a[k], b[k]), k
            x, y = a[0].permute(0, 2, 3, 1).cpu().numpy(), b[0].permute(0, 2, 3, 1).cpu().numpy()
            for k in range(2):
                d = host._decide(*host._where(j * 2 + k))[3]
                assert d.plan is not None and d.jitter is not None
                m = D.to_crop(D.pasted_mask(d.plan, d.dst_h, d.dst_w), d, 128, 128, False)
                assert np.array_equal(C.bits(x[k][~m]), C.bits(y[k][~m])), (j, k)
                if m.any():
                    pasted += 1
                    err, e = float(np.abs(x[k].astype(np.float64) - y[k])[m].max()), D.bound(d.plan.depth)
                    print("loader batch", j, k, "pasted pixels", int(m.sum()), "depth", d.plan.depth, "err", err, "2E", 2 * e)
                    assert err <= 2 * e
    finally:
        dev.close()
        host.close()
    assert pasted >= 1


def test_train_tool_with_color_jitter(roots, tmp_path):
    """tools/train.py --color-jitter 0.5 0.5 0.5 --iters 2 on the generated data set, in a child process: finite losses."""
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--color-jitter", "0.5", "0.5", "0.5", "--iters", "2",
           "--data-root", roots[0], "--batch", "2", "--crop", "128", "128", "--backbone", "hourglass_tiny",
           "--print-interval", "1"]
    out = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if re.match(r"step \d+  loss ", l)]
    assert len(lines) == 2, out.stdout[-2000:]
    for l in lines:
        vals = [float(v) for v in re.findall(r"(?:loss|hm|wh|off|s2) (\S+)", l)]
        assert len(vals) == 5 and all(math.isfinite(v) for v in vals), l

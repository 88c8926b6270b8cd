"""Shared by tests/test_fillduck_host.py and tests/test_fillduck_gpu.py: the recorded reference cases
(tests/golden/fillduck.npz, tools/gen_golden_fillduck.py), a hand-built paste plan, the float64 evaluation of the paste
formula, the derived bound E(depth) and a temporary dataset with road maps."""
import functools
import os

import numpy as np
import torch

import augment_cases as C
from rrnet_amd.datasets import augment as A
from rrnet_amd.datasets.transforms import functional as F

CLS_LIST = (1, 2, 3, 7, 8, 10)
PASTED_CASES = ("base", "dense", "nodepth", "two", "abort")
PARAMS = dict(C.PARAMS, fill_duck=dict(cls_list=CLS_LIST, factor=5e-5))


def bound(depth, std=C.STD):
    """E(depth) of a normalised pasted pixel against the float64 evaluation: canvas values lie in [0,1] and a bilinear
    blend is a convex combination, so each of the 9 float32 roundings of one paste adds at most 2**-25, a chain of
    `depth` pastes depth * 9 * 2**-25; Normalize divides by min(std) and adds two roundings of a result below 4, at
    most 2**-23 each."""
    return depth * 9 * 2.0 ** -25 / min(std) + 2 * 2.0 ** -23


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(C.GOLDEN, "fillduck.npz")))


def golden_case(name):
    """-> (uint8 frame [h,w,3], uint8 road [h,w], float32 annos [n,8], factor, seed, out_annos, changed idx, values)."""
    g = golden()
    return tuple(g["%s_%s" % (name, k)] for k in ("frame", "road", "annos", "factor", "seed", "out_annos", "idx", "val"))


def plan_from_rows(rows, frame_h, frame_w):
    """A PastePlan from (src_y, src_x, src_h, src_w, dst_y, dst_x, out_h, out_w) tuples."""
    plan = F.PastePlan()
    tab = []
    for sy, sx, sh, sw, dy, dx, oh, ow in rows:
        assert 0 <= sy and sy + sh <= frame_h and 0 <= sx and sx + sw <= frame_w
        assert 0 <= dy and dy + oh <= frame_h and 0 <= dx and dx + ow <= frame_w
        rh = np.float32(sh - 1) / np.float32(oh - 1) if oh > 1 else np.float32(0)
        rw = np.float32(sw - 1) / np.float32(ow - 1) if ow > 1 else np.float32(0)
        tab.append((sy, sx, sh, sw, dy, dx, oh, ow, int(np.float32(rh).view(np.int32)), int(np.float32(rw).view(np.int32)),
                    0, 0))
    plan.pastes = np.asarray(tab, np.int32).reshape(-1, F.PASTE_WORDS)
    plan.depth = F.paste_depth(plan.pastes, frame_h, frame_w)
    return plan


def hand_plan(frame_h, frame_w):
    """For a frame of at least 96 x 128: a paste whose source and destination overlap (same size, shifted), factor
    exactly 2, factor exactly 0.5, a paste that reads what the factor-2 paste wrote and one that reads that in turn
    (depth 3), a 1 x k and a k x 1 object (scale 0 along one axis), and a last paste over part of an earlier one."""
    assert frame_h >= 96 and frame_w >= 128
    rows = [(10, 10, 20, 30, 15, 22, 20, 30),            # overlap, factor 1
            (48, 5, 8, 9, 2, 100, 16, 18),               # factor 2 -> rows 2..17, columns 100..117
            (40, 60, 12, 10, 70, 70, 6, 5),              # factor 0.5
            (4, 104, 10, 12, 60, 20, 13, 15),            # reads the factor-2 object: depth 2
            (62, 22, 9, 9, 80, 100, 12, 11),             # reads the depth-2 object: depth 3
            (30, 3, 1, 7, 50, 40, 1, 10),                # 1 x k
            (33, 50, 7, 1, 52, 90, 9, 1),                # k x 1
            (20, 20, 6, 6, 64, 26, 9, 9)]                # overwrites part of the depth-2 object
    plan = plan_from_rows(rows, frame_h, frame_w)
    assert plan.depth == 3
    return plan


def paste_f64(canvas, plan):
    """The paste formula in float64 on a float64 [H,W,3] canvas (in place), with the SAME float32 r, c and weights the
    kernel and torch form: value = l0*(m0*a + m1*b) + l1*(m0*c + m1*d).  All reads of a paste precede its writes."""
    for sy, sx, sh, sw, dy, dx, oh, ow, rh, rw in plan.pastes[:, :10].tolist():
        rh, rw = np.int32(rh).view(np.float32), np.int32(rw).view(np.float32)
        r = (rh * np.arange(oh, dtype=np.float32)).astype(np.float32)
        c = (rw * np.arange(ow, dtype=np.float32)).astype(np.float32)
        y0, x0 = r.astype(np.int64), c.astype(np.int64)
        y1, x1 = np.minimum(y0 + 1, sh - 1), np.minimum(x0 + 1, sw - 1)
        l1 = (r - y0.astype(np.float32)).astype(np.float32)
        m1 = (c - x0.astype(np.float32)).astype(np.float32)
        l0, m0 = (np.float32(1) - l1).astype(np.float32), (np.float32(1) - m1).astype(np.float32)
        l0, l1 = l0.astype(np.float64)[:, None, None], l1.astype(np.float64)[:, None, None]
        m0, m1 = m0.astype(np.float64)[None, :, None], m1.astype(np.float64)[None, :, None]
        src = canvas[sy:sy + sh, sx:sx + sw].copy()
        a, b = src[y0][:, x0], src[y0][:, x1]
        cc, d = src[y1][:, x0], src[y1][:, x1]
        canvas[dy:dy + oh, dx:dx + ow] = l0 * (m0 * a + m1 * b) + l1 * (m0 * cc + m1 * d)
    return canvas


def pasted_mask(plan, frame_h, frame_w):
    m = np.zeros((frame_h, frame_w), bool)
    for dy, dx, oh, ow in plan.pastes[:, 4:8].tolist():
        m[dy:dy + oh, dx:dx + ow] = True
    return m


def to_crop(a, d, out_h, out_w, fill=0):
    """[H,W(,C)] array in scaled pre-flip coordinates -> the decision's crop (flip, right/bottom padding, crop)."""
    if d.flip:
        a = a[:, ::-1]
    pad = [(0, max(out_h - a.shape[0], 0)), (0, max(out_w - a.shape[1], 0))] + [(0, 0)] * (a.ndim - 2)
    a = np.pad(a, pad, constant_values=fill)
    return a[d.crop_y0:d.crop_y0 + out_h, d.crop_x0:d.crop_x0 + out_w]


def reference_f64(img, annos, d, out_h, out_w, params=C.PARAMS):
    """The chain for decision `d` with the pastes in float64 -> (normalised float64 [out_h,out_w,3], pasted mask
    [out_h,out_w]): PIL resize -> to_tensor -> mask_ignore in float32 as the host chain does, then paste_f64, flip,
    padding, crop and (x - mean) / std with the float32 mean and std, all in float64."""
    from PIL import Image
    a = annos.copy()
    pil = F.resize((Image.fromarray(img), a), d.scale)[0]
    t, ta = F.img_to_tensor(pil), F.annos_to_tensor(a)
    t = F.mask_ignore((t, ta), params["ignore_mean"], params["ignore_idx"])[0]
    canvas = t.permute(1, 2, 0).contiguous().numpy().astype(np.float64)
    paste_f64(canvas, d.plan)
    mean = np.asarray(params["mean"], np.float32).astype(np.float64)
    std = np.asarray(params["std"], np.float32).astype(np.float64)
    out = (to_crop(canvas, d, out_h, out_w) - mean) / std
    return out, to_crop(pasted_mask(d.plan, d.dst_h, d.dst_w), d, out_h, out_w, False)


def decision(name, scale, flip, crop, origin):
    """A hand-built Decision (augment_cases.decision) for a golden frame, or "hand" (the base frame with hand_plan),
    with the plan fill_duck_decide makes for the scaled frame under the case's torch seed (for "abort": the first seed
    from there on whose plan aborts after at least one paste)."""
    frame, road, annos, factor, seed = golden_case("base" if name == "hand" else name)[:5]
    annos = np.concatenate([annos.astype(np.int64), np.array([[40, 30, 12, 9, 0, 0, 0, 0]])])   # one ignore region
    d = C.decision(frame, annos, scale, flip, crop, origin)
    if name == "hand":
        d.plan = hand_plan(d.dst_h, d.dst_w)
    else:
        rm = torch.from_numpy(F.nearest_resize(road, d.dst_h, d.dst_w)).float() / 255
        for y0, y1, x0, x1 in d.rects.tolist():
            rm[y0:y1, x0:x1] = 0
        t = d.annos[d.annos[:, 5] != 0]
        for s in range(int(seed), int(seed) + 64):
            torch.manual_seed(s)
            d.plan = F.fill_duck_decide(t, rm, CLS_LIST, float(factor), d.dst_h, d.dst_w, F.TorchRand)
            if name != "abort" or d.plan.aborted_at >= 1:   # the abort case wants pastes in front of the failing one
                break
        assert len(d.plan.pastes) > 0 or name not in PASTED_CASES
    return frame, annos, d


def item_of(frame, d, crop, taps):
    """What a loader thread hands to pack_batch: the whole frame for a pasted sample, the crop's window otherwise."""
    h, w = frame.shape[:2]
    if A.n_pastes(d) == 0:
        return C.item_of(frame, d, crop, taps)
    win = (0, 0, h, w) + A.source_window(d, h, w, crop[0], crop[1], taps)[4:]
    return d, h, w, win, np.ascontiguousarray(frame)


def write_roadmaps(root, split="train"):
    """A road band across the lower 60 % of every image of the split, with a hole, written as JPEG."""
    from PIL import Image
    os.makedirs(os.path.join(root, split, "roadmap"), exist_ok=True)
    for f in sorted(os.listdir(os.path.join(root, split, "images"))):
        w, h = Image.open(os.path.join(root, split, "images", f)).size
        road = np.zeros((h, w, 3), np.uint8)
        road[int(h * 0.4):, :] = 255
        road[int(h * 0.6):int(h * 0.7), w // 4:w // 2] = 0
        Image.fromarray(road).save(os.path.join(root, split, "roadmap", f), quality=95)
    return root


def full_chain(crop, fill_duck=True):
    from rrnet_amd.datasets.transforms import (Compose, FillDuck, HorizontalFlip, MaskIgnore, MultiScale, Normalize,
                                               RandomCrop, ToHeatmap, ToTensor)
    ts = [MultiScale(scale=(1, 1.15, 1.25, 1.35, 1.5)), ToTensor(), MaskIgnore(C.MEAN), FillDuck(factor=2e-4),
          HorizontalFlip(), RandomCrop(crop), Normalize(C.MEAN, C.STD), ToHeatmap(scale_factor=4)]
    return Compose(ts if fill_duck else ts[:3] + ts[4:])


LOADER_SEED = 5


def pasted_kernel_model(src, params, rects, rect_off, taps, pastes, paste_off, mean, std, out_h, out_w):
    """rr_augment_frames_pasted's arithmetic in numpy float32 (same records, same clamps, same operation order): canvas
    (only the crop of a frame without pastes), pastes through a staged copy, finish."""
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    half = 1 << 21
    out = np.empty((len(params), out_h, out_w, 3), np.float32)
    for b, P in enumerate(params.astype(np.int64)):
        dst_h, dst_w = int(P[6]), int(P[7])
        sy, sx = np.mgrid[0:dst_h, 0:dst_w]
        sxp = dst_w - 1 - sx if P[8] else sx
        whole = paste_off[b + 1] > paste_off[b]
        need = whole | ((sy >= P[9]) & (sy < P[9] + out_h) & (sxp >= P[10]) & (sxp < P[10] + out_w))
        ign = np.zeros((dst_h, dst_w), bool)
        for y0, y1, x0, x1 in rects[rect_off[b]:rect_off[b + 1]]:
            ign |= (sy >= y0) & (sy < y1) & (sx >= x0) & (sx < x1)
        ty = taps[np.clip(P[13] + sy, 0, len(taps) - 1)].astype(np.int64)
        tx = taps[np.clip(P[14] + sx, 0, len(taps) - 1)].astype(np.int64)
        y0, y1 = np.clip(ty[..., 0] - P[2], 0, P[4] - 1), np.clip(ty[..., 0] + 1 - P[2], 0, P[4] - 1)
        x0, x1 = np.clip(tx[..., 0] - P[3], 0, P[5] - 1), np.clip(tx[..., 0] + 1 - P[3], 0, P[5] - 1)
        off = int(P[11] & 0xffffffff) | (int(P[12]) << 32)
        win = src[off:off + P[4] * P[5] * 3].reshape(P[4], P[5], 3).astype(np.int64)
        kx0, kx1, ky0, ky1 = tx[..., 1:2], tx[..., 2:3], ty[..., 1:2], ty[..., 2:3]
        h0 = np.clip((win[y0, x0] * kx0 + win[y0, x1] * kx1 + half) >> 22, 0, 255)
        h1 = np.clip((win[y1, x0] * kx0 + win[y1, x1] * kx1 + half) >> 22, 0, 255)
        v = np.clip((h0 * ky0 + h1 * ky1 + half) >> 22, 0, 255).astype(np.float32) / np.float32(255)
        canvas = np.where(ign[..., None], mean[None, None], v).astype(np.float32)
        canvas[~need] = np.float32(np.nan)                       # never written, must never be read
        for T in pastes[paste_off[b]:paste_off[b + 1]].tolist():
            py, px, sh, sw, dy, dx, oh, ow = T[:8]
            rh, rw = np.int32(T[8]).view(np.float32), np.int32(T[9]).view(np.float32)
            r, c = rh * np.arange(oh, dtype=np.float32), rw * np.arange(ow, dtype=np.float32)
            a0, b0 = np.minimum(r.astype(np.int64), sh - 1), np.minimum(c.astype(np.int64), sw - 1)
            a1, b1 = np.minimum(a0 + 1, sh - 1), np.minimum(b0 + 1, sw - 1)
            l1, m1 = (r - a0.astype(np.float32))[:, None, None], (c - b0.astype(np.float32))[None, :, None]
            l0, m0 = np.float32(1) - l1, np.float32(1) - m1
            rows0, rows1 = np.clip(py + a0, 0, dst_h - 1), np.clip(py + a1, 0, dst_h - 1)
            cols0, cols1 = np.clip(px + b0, 0, dst_w - 1), np.clip(px + b1, 0, dst_w - 1)
            pa, pb = canvas[rows0][:, cols0], canvas[rows0][:, cols1]
            pc, pd = canvas[rows1][:, cols0], canvas[rows1][:, cols1]
            staged = l0 * (m0 * pa + m1 * pb) + l1 * (m0 * pc + m1 * pd)
            assert staged.dtype == np.float32
            canvas[dy:dy + oh, dx:dx + ow] = staged
        full = np.zeros((max(dst_h, out_h + int(P[9])), max(dst_w, out_w + int(P[10])), 3), np.float32)
        full[:dst_h, :dst_w] = canvas[:, ::-1] if P[8] else canvas
        crop = full[P[9]:P[9] + out_h, P[10]:P[10] + out_w]
        out[b] = (crop - mean[None, None]) / std[None, None]
    return out

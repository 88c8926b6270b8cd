"""Loaders that feed real VisDrone frames to the hot path with the `get_batch()` surface of datasets/dataloader.py:27-37.

The host decodes the JPEG and DECIDES; the device produces the pixels.  Per sample the sampler draws (scale, flip, crop
origin) from a generator keyed by (seed, rank, epoch, index), runs FillDuck's and RandomCrop's decision logic on the
annotations (and the road map) alone and emits the final annotation rows, the record rr_augment_frames needs, the paste
plan and the source window the crop reads.  DeviceAugmentLoader ships the windows through pinned memory, one batch ahead
on a copy stream (the event hand-over of HostFedDronesDET), and runs rr_augment_frames (rr_augment_frames_pasted for a
batch with pastes, whose pasted samples ship their whole frame) + rr_ctnet_targets on the compute stream.  With
ColorJitter in front of the chain the sampler also draws the three factors, every sample ships its whole frame, and
rr_jitter_gray_mean (the grey mean PIL's contrast step needs) runs in front of the _jitter variant of either kernel.
HostAugmentLoader runs the reference's chain on the host for the SAME decisions: it is what the device path is checked
against, bit for bit except for pasted pixels (functional.apply_paste_plan states their bound).

Deviations from the reference chain (configs/rrnet_config.py:40-49), see DESIGN.md "Data layer":
  * ColorJitter is lowered only as the first transform (in front of MultiScale, or of ToTensor without MultiScale):
    anywhere else it would see other pixels, another grey mean and another order of rounding; its factors come from a
    generator keyed per sample, not from Python's global `random`;
  * FillDuck's draws come from a generator keyed per sample and attempt, not from the global torch generator;
  * where every box is larger than the crop the reference rescales the frame with F.interpolate
    (transforms.py:81-90); here the sampler redraws the MultiScale factor (and flip and origin) and counts it
    (`redraws`); a draw that keeps no box at all is redrawn too;
  * the "Fake image" fallback (transforms.py:114-117) is unreachable and absent: 50 failed draws raise;
  * scale factors below 1 are refused (PIL's filter then has more than two taps)."""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .transforms import (ColorJitter, Compose, FillDuck, HorizontalFlip, MaskIgnore, MultiScale, Normalize, RandomCrop,
                         ToHeatmap, ToTensor)
from .transforms import functional as F

MAX_THREADS = 16
MIN_SCALE = 1.0
P_WORDS = 16          # ops.AUGMENT_PARAMS
T_WORDS = F.PASTE_WORDS   # ops.PASTE_WORDS
FILL_DUCK_TAG = 0x46443031   # "FD01": keeps FillDuck's generator apart from the scale / flip / crop draws
JITTER_TAG = 0x434a3031      # "CJ01": likewise for ColorJitter's three factors


def chain_params(transforms):
    """Reads the parameters of the lowered chain out of a Compose of transform instances.  Anything the kernel does not
    implement is an error, not a silent difference."""
    p = dict(scales=(1,), flip_p=0.0, crop=None, keep_iou=0.5, mean=None, std=None, ignore_idx=None, ignore_mean=None,
             scale_factor=4, cls_num=10, fill_duck=None, jitter=None)
    seen = []
    for k, t in enumerate(transforms.transforms if isinstance(transforms, Compose) else transforms):
        if isinstance(t, ColorJitter):
            if k != 0:
                raise NotImplementedError("ColorJitter is lowered only as the first transform of the chain: behind %s it "
                                          "would need another grey mean and another order of rounding"
                                          % (seen[-1].__name__ if seen else "another ColorJitter"))
            p["jitter"] = (tuple(t.brightness), tuple(t.contrast), tuple(t.saturation))
            continue
        seen.append(type(t))
        if isinstance(t, MultiScale):
            p["scales"] = tuple(t.scale)
        elif isinstance(t, ToTensor):
            pass
        elif isinstance(t, MaskIgnore):
            p["ignore_idx"], p["ignore_mean"] = t.ignore_idx, tuple(t.mean)
        elif isinstance(t, FillDuck):
            p["fill_duck"] = dict(cls_list=tuple(int(c) for c in t.cls_list.view(-1).tolist()), factor=float(t.factor))
        elif isinstance(t, HorizontalFlip):
            p["flip_p"] = t.p
        elif isinstance(t, RandomCrop):
            p["crop"], p["keep_iou"] = (t.h, t.w), t.keep_iou
        elif isinstance(t, Normalize):
            p["mean"], p["std"] = tuple(t.mean), tuple(t.std)
        elif isinstance(t, ToHeatmap):
            p["scale_factor"], p["cls_num"] = t.scale_factor, t.cls_num
        else:
            raise NotImplementedError("transform %s is not lowered to rr_augment_frames" % type(t).__name__)
    order = [c for c in (MultiScale, ToTensor, MaskIgnore, FillDuck, HorizontalFlip, RandomCrop, Normalize, ToHeatmap)
             if c in seen]
    if [c for c in seen] != order:
        raise NotImplementedError("the lowered chain is MultiScale, ToTensor, MaskIgnore, FillDuck, HorizontalFlip, "
                                  "RandomCrop, Normalize, ToHeatmap in this order; got %s" % [c.__name__ for c in seen])
    if FillDuck in seen:
        k = seen.index(FillDuck)
        if seen[k - 1:k] != [MaskIgnore] or seen[k + 1:k + 2] != [HorizontalFlip] or k == 0:
            raise NotImplementedError("FillDuck is lowered only between MaskIgnore and HorizontalFlip; got %s"
                                      % [c.__name__ for c in seen])
    if p["mean"] is None:
        raise NotImplementedError("the lowered chain needs Normalize")
    if p["ignore_mean"] is not None and tuple(p["ignore_mean"]) != tuple(p["mean"]):
        raise NotImplementedError("MaskIgnore.mean must equal Normalize.mean (an ignore region is written as +0.0)")
    if min(p["scales"]) < MIN_SCALE:
        raise ValueError("MultiScale factor %g: the device path resizes with two taps per axis, which holds for scale "
                         "factors >= %g only" % (min(p["scales"]), MIN_SCALE))
    return p


class TapCache:
    """PIL's per-axis resize tables (functional.pil_bilinear_taps), one per (in, out) pair, appended to one arena so that
    a batch can name a table by its first row.  A dataset has few frame sizes; the arena only grows."""

    def __init__(self):
        self._off, self._tabs, self._rows = {}, [], 0
        self._lock = threading.Lock()
        self._dev = {}

    def get(self, in_size, out_size):
        """-> (first arena row, int32 [out,3] table)."""
        key = (int(in_size), int(out_size))
        with self._lock:
            hit = self._off.get(key)
            if hit is None:
                tab = F.pil_bilinear_taps(*key)
                hit = self._off[key] = (self._rows, tab)
                self._tabs.append(tab)
                self._rows += tab.shape[0]
            return hit

    def arena(self):
        with self._lock:
            return np.concatenate(self._tabs, 0) if self._tabs else np.zeros((1, 3), np.int32)

    def device(self, device):
        """The arena on `device`, uploaded again only after it has grown."""
        with self._lock:
            rows = self._rows
        hit = self._dev.get(str(device))
        if hit is None or hit[0] != rows:
            hit = self._dev[str(device)] = (rows, torch.from_numpy(self.arena()).to(device))
        return hit[1]


class _Rand:
    """RandomCrop's random source on a numpy Generator."""

    def __init__(self, rng):
        self.rng = rng

    def random(self):
        return float(self.rng.random())

    def integers(self, low, high):
        return int(self.rng.integers(low, high))


class Decision:
    """What the sampler decided for one sample."""
    __slots__ = ("index", "scale", "flip", "dst_h", "dst_w", "crop_y0", "crop_x0", "annos", "rects", "redraws", "plan",
                 "jitter")

    def key(self):
        plan = plan_of(self)
        return (self.index, self.scale, self.flip, self.dst_h, self.dst_w, self.crop_y0, self.crop_x0, self.redraws,
                self.annos.numpy().tobytes(), self.rects.tobytes(), plan.key() if plan is not None else None,
                jitter_of(self))


def plan_of(d):
    """The decision's FillDuck plan, or None (a chain without FillDuck, no road map, or a hand-built Decision)."""
    return getattr(d, "plan", None)


def jitter_of(d):
    """The decision's ColorJitter factors (brightness, contrast, saturation; Python floats that hold float32 values, the
    precision PIL's blend and the kernel both compute in), or None (a chain without ColorJitter, a hand-built
    Decision)."""
    return getattr(d, "jitter", None)


def n_pastes(d):
    plan = plan_of(d)
    return 0 if plan is None else len(plan.pastes)


class AugmentSampler:
    """Per-sample decisions and per-epoch sharding.  Randomness is a function of (seed, rank, epoch, index) alone — not
    of which thread asks, nor of the order of asking."""

    def __init__(self, params, seed=219, rank=0, world_size=1):
        self.p = params
        self.seed, self.rank, self.world_size = int(seed), int(rank), int(world_size)
        self.crop = RandomCrop(params["crop"], params["keep_iou"]) if params["crop"] is not None else None
        self.redraws = 0

    def indices(self, n, epoch):
        """This rank's share of a seeded permutation of range(n), padded to a multiple of the world size (no process
        group needed)."""
        perm = np.random.default_rng([self.seed, int(epoch)]).permutation(n)
        pad = (-n) % self.world_size
        if pad:
            perm = np.concatenate([perm, perm[:pad]])
        return perm[self.rank::self.world_size]

    def sample(self, annotations, src_h, src_w, epoch, index, roadmap=None):
        """annotations: the image's int64 [n,8] rows (not modified); roadmap: uint8 [src_h,src_w] or None -> Decision.
        With FillDuck in the chain and a road map, every draw attempt resizes and masks the map, plans the pastes
        (functional.fill_duck_decide, from a generator of its own keyed by the attempt, so that the scale, flip and
        crop draws are those of the chain without FillDuck) and appends the pasted boxes before the flip and the crop
        decision: they steer RandomCrop as in the reference."""
        rng = np.random.default_rng([self.seed, self.rank, int(epoch), int(index)])
        rand = _Rand(rng)
        p = self.p
        d = Decision()
        d.index, d.redraws, d.plan, d.jitter = int(index), 0, None, None
        if p.get("jitter") is not None:                     # a generator of its own: the other draws stay what they are
            cj_rng = np.random.default_rng([self.seed, self.rank, int(epoch), int(index), JITTER_TAG])
            d.jitter = tuple(float(np.float32(cj_rng.uniform(lo, hi))) for lo, hi in p["jitter"])
        duck = p.get("fill_duck") if roadmap is not None else None
        for attempt in range(50):
            d.scale = p["scales"][int(rng.integers(0, len(p["scales"])))]
            d.flip = bool(rng.random() <= p["flip_p"]) if p["flip_p"] > 0 else False
            d.dst_h, d.dst_w = F.scaled_size(src_h, src_w, d.scale)
            a = F.resize_annos(annotations.copy(), d.scale)                 # integer truncation (functional.py:81)
            t = F.annos_to_tensor(a)
            if p["ignore_idx"] is not None:
                d.rects = F.ignore_rects(a, d.dst_h, d.dst_w, p["ignore_idx"])
                t = t[~(t[:, 5] == p["ignore_idx"]), :]
            else:
                d.rects = np.zeros((0, 4), np.int32)
            if duck is not None:
                road = torch.from_numpy(F.nearest_resize(roadmap, d.dst_h, d.dst_w)).float() / 255
                for y0, y1, x0, x1 in d.rects.tolist():                     # functional.py:308-309
                    road[y0:y1, x0:x1] = 0
                fd_rng = np.random.default_rng([self.seed, self.rank, int(epoch), int(index), attempt, FILL_DUCK_TAG])
                d.plan = F.fill_duck_decide(t, road, duck["cls_list"], duck["factor"], d.dst_h, d.dst_w,
                                            F.GeneratorRand(fd_rng))
                if d.plan.new_annos.size(0):
                    t = torch.cat((t, d.plan.new_annos))
            if d.flip:
                F.flip_annos(t, d.dst_w)
            if self.crop is None:
                d.crop_y0 = d.crop_x0 = 0
                d.annos = t
                return d
            res = self.crop.decide(t, d.dst_h, d.dst_w, rand)
            if res is not None and res[1].size(0) > 0:
                d.crop_x0, d.crop_y0 = int(res[0][0]), int(res[0][1])
                d.annos = res[1]
                return d
            d.redraws += 1
        raise RuntimeError("AugmentSampler: no crop with a box after 50 draws (image index %d)" % index)


def source_window(d, src_h, src_w, out_h, out_w, taps):
    """The source rows and columns the crop of decision `d` reads -> (y0, x0, h, w, ytab_row, xtab_row)."""
    yrow, ytab = taps.get(src_h, d.dst_h)
    xrow, xtab = taps.get(src_w, d.dst_w)
    ys = ytab[d.crop_y0:min(d.crop_y0 + out_h, d.dst_h)]
    lo, hi = d.crop_x0, min(d.crop_x0 + out_w, d.dst_w)
    xs = xtab[d.dst_w - hi:d.dst_w - lo] if d.flip else xtab[lo:hi]
    assert len(ys) and len(xs)
    y0, y1 = int(ys[:, 0].min()), int((ys[:, 0] + (ys[:, 2] != 0)).max())
    x0, x1 = int(xs[:, 0].min()), int((xs[:, 0] + (xs[:, 2] != 0)).max())
    assert 0 <= y0 <= y1 < src_h and 0 <= x0 <= x1 < src_w
    return y0, x0, y1 - y0 + 1, x1 - x0 + 1, yrow, xrow


def param_record(d, src_h, src_w, win, src_offset):
    y0, x0, wh, ww, yrow, xrow = win
    return [src_h, src_w, y0, x0, wh, ww, d.dst_h, d.dst_w, int(d.flip), d.crop_y0, d.crop_x0,
            int(np.uint32(src_offset & 0xffffffff).astype(np.int32)), int(src_offset >> 32), yrow, xrow, 0]


def pack_batch(items, src_out=None):
    """items: [(Decision, src_h, src_w, window tuple, window pixels uint8 [h,w,3])] -> (src uint8 [bytes],
    params int32 [B,16], rects int32 [R,4], rect_off int32 [B+1]) as numpy arrays; `src_out` (a uint8 array, e.g. a
    view of pinned memory) receives the windows when given."""
    total = sum(it[4].size for it in items)
    src = src_out if src_out is not None else np.empty(max(total, 3), np.uint8)
    assert src.size >= total
    params = np.zeros((len(items), P_WORDS), np.int32)
    rect_off = np.zeros(len(items) + 1, np.int32)
    rects, off = [], 0
    for i, (d, src_h, src_w, win, pix) in enumerate(items):
        assert pix.dtype == np.uint8 and pix.shape == (win[2], win[3], 3)
        check_jitter_window(d, src_h, src_w, win)
        src[off:off + pix.size] = pix.reshape(-1)
        params[i] = param_record(d, src_h, src_w, win, off)
        off += pix.size
        rects.append(d.rects)
        rect_off[i + 1] = rect_off[i] + len(d.rects)
    rects = np.concatenate(rects, 0).astype(np.int32).reshape(-1, 4)
    return src[:max(total, 3)], params, rects, rect_off


def check_jitter_window(d, src_h, src_w, win):
    """Contrast blends towards the grey mean of the WHOLE frame: a jittered sample ships it."""
    if jitter_of(d) is not None and tuple(int(v) for v in win[:4]) != (0, 0, int(src_h), int(src_w)):
        raise ValueError("image index %d is colour-jittered and ships the window %s of its %dx%d frame; the grey mean "
                         "needs the whole frame" % (d.index, tuple(win[:4]), src_w, src_h))


def pack_jitter(items):
    """items as for pack_batch -> (factors float32 [B,3], the largest frame in pixels): what rr_jitter_gray_mean and the
    _jitter kernels take on top of pack_batch's records.  A sample without factors gets (1, 1, 1), the identity."""
    factors = np.ones((len(items), 3), np.float32)
    for i, (d, src_h, src_w, win, _) in enumerate(items):
        check_jitter_window(d, src_h, src_w, win)
        if jitter_of(d) is not None:
            factors[i] = jitter_of(d)
    return factors, max(int(it[3][2]) * int(it[3][3]) for it in items)


def pack_pastes(decisions):
    """[Decision] -> (pastes int32 [K,12], paste_off int32 [B+1], largest scaled frame in pixels, largest object in
    pixels).  Every rectangle is checked against its frame here, before anything is launched."""
    tabs, off = [], np.zeros(len(decisions) + 1, np.int32)
    for i, d in enumerate(decisions):
        tab = plan_of(d).pastes if n_pastes(d) else np.zeros((0, T_WORDS), np.int32)
        sy, sx, sh, sw, dy, dx, oh, ow = (tab[:, k].astype(np.int64) for k in range(8))
        ok = ((sy >= 0) & (sx >= 0) & (sh > 0) & (sw > 0) & (sy + sh <= d.dst_h) & (sx + sw <= d.dst_w) &
              (dy >= 0) & (dx >= 0) & (oh > 0) & (ow > 0) & (dy + oh <= d.dst_h) & (dx + ow <= d.dst_w))
        if not ok.all():
            raise RuntimeError("paste plan of image index %d leaves its %dx%d frame" % (d.index, d.dst_w, d.dst_h))
        tabs.append(tab)
        off[i + 1] = off[i] + len(tab)
    pastes = np.concatenate(tabs, 0).astype(np.int32).reshape(-1, T_WORDS)
    canvas = max(d.dst_h * d.dst_w for d in decisions)
    scratch = int((pastes[:, 6].astype(np.int64) * pastes[:, 7]).max()) if len(pastes) else 1
    return pastes, off, canvas, scratch


def host_chain(image, annotations, d, params, out_h, out_w):
    """The reference chain on the host for decision `d`: PIL image + int64 annotations -> float32 [3,out_h,out_w].
    (the decision's colour jitter -> resize -> to_tensor -> mask_ignore -> the decision's pastes -> flip -> pad/crop ->
    normalize; the annotations of the batch are d.annos.)"""
    a = annotations.copy()
    if jitter_of(d) is not None:
        image = F.color_jitter(image, *d.jitter)
    img, a = F.resize((image, a), d.scale)[:2]
    img, t = F.img_to_tensor(img), F.annos_to_tensor(a)
    if params["ignore_idx"] is not None:
        img, t = F.mask_ignore((img, t), params["ignore_mean"], params["ignore_idx"])
    if plan_of(d) is not None:
        F.apply_paste_plan(img, d.plan)
    if d.flip:
        img = F.flip_img(img)
    h, w = img.shape[-2:]
    if out_w > w or out_h > h:
        img = torch.nn.functional.pad(img, [0, max(out_w - w, 0), 0, max(out_h - h, 0)])
    img = F.crop_tensor(img, (d.crop_x0, d.crop_y0, d.crop_x0 + out_w, d.crop_y0 + out_h))
    return F.normalize(img, params["mean"], params["std"])


class _AugmentLoader:
    """Positions, sharding and the thread pool shared by the two training loaders.  Sample `pos` of this rank's stream is
    index `indices(epoch)[pos % L]` of epoch `pos // L`; batches are consecutive positions."""

    def __init__(self, dataset, params, batch_size, seed=219, rank=0, world_size=1, num_workers=4, device="cuda",
                 depth=3, taps=None):
        if params["crop"] is None:
            raise ValueError("a training loader needs RandomCrop (a batch has one size)")
        if len(dataset) == 0:
            raise ValueError("DronesDET: no image with a box under %s" % dataset.images_dir)
        self.dataset, self.p, self.bs = dataset, params, int(batch_size)
        self.out_h, self.out_w = params["crop"]
        self.sampler = AugmentSampler(params, seed, rank, world_size)
        self.device = torch.device(device) if not isinstance(device, torch.device) else device
        self.taps = taps if taps is not None else TapCache()
        self.pool = ThreadPoolExecutor(max_workers=max(1, min(int(num_workers), MAX_THREADS)))
        self.depth = depth
        self._epoch_idx = {}
        self.shard = len(self.sampler.indices(len(dataset), 0))
        self.futures = {}
        self.i = 0
        self.redraws = 0

    def __len__(self):
        return max(self.shard // self.bs, 1)

    def _where(self, pos):
        epoch, k = divmod(pos, self.shard)
        if epoch not in self._epoch_idx:
            self._epoch_idx = {e: v for e, v in self._epoch_idx.items() if e >= epoch - 1}
            self._epoch_idx[epoch] = self.sampler.indices(len(self.dataset), epoch)
        return epoch, int(self._epoch_idx[epoch][k])

    def _submit(self, j):
        if j not in self.futures:
            self.futures[j] = [self.pool.submit(self._job, *self._where(j * self.bs + k)) for k in range(self.bs)]

    def _collect(self, j):
        self._submit(j)
        res = [f.result() for f in self.futures.pop(j)]
        for k in range(1, self.depth):
            self._submit(j + k)
        self.redraws += sum(r[0].redraws for r in res)
        return res

    def _decide(self, epoch, index):
        loaded = self.dataset.load(index)
        image, annotations, name = loaded[:3]
        roadmap = loaded[3] if len(loaded) > 3 else None
        if roadmap is not None and roadmap.shape != (image.size[1], image.size[0]):
            raise ValueError("road map of %s is %s, the image %s" % (name, roadmap.shape[::-1], image.size))
        d = self.sampler.sample(annotations, image.size[1], image.size[0], epoch, index, roadmap)
        return image, annotations, name, d

    def position(self):
        """Batches handed out so far."""
        return self.i

    def seek(self, n):
        """The next get_batch() returns what a fresh loader returns as its n-th batch: every sample is a function of
        (seed, rank, epoch, index), so dropping the work queued for other positions is all there is to do.  Jobs already
        running finish on their threads and their results are discarded."""
        for fs in self.futures.values():
            for f in fs:
                f.cancel()
        self.futures = {}
        self.i = int(n)

    def close(self):
        self.pool.shutdown(wait=True, cancel_futures=True)


class HostAugmentLoader(_AugmentLoader):
    """The host path: every pixel step of the chain runs on the CPU threads (PIL + torch), the finished float frames
    cross to the device, and only the targets are built there (rr_ctnet_targets, as ToHeatmap does)."""

    def _job(self, epoch, index):
        image, annotations, name, d = self._decide(epoch, index)
        return d, host_chain(image, annotations, d, self.p, self.out_h, self.out_w), name

    def get_batch(self):
        from .synthetic import collate_ctnet_device
        res = self._collect(self.i)
        self.i += 1
        imgs = torch.stack([r[1] for r in res]).to(self.device).contiguous(memory_format=torch.channels_last)
        annos, hm, wh, ind, off, mask = collate_ctnet_device([r[0].annos for r in res], self.out_h, self.out_w,
                                                             self.p["scale_factor"], self.p["cls_num"], self.device)
        return imgs, annos, hm, wh, ind, off, mask, [r[2] for r in res]


class DeviceAugmentLoader(_AugmentLoader):
    """Decode and decide on the threads; windows, records and annotations go through two pinned staging slots to two
    device slots, one batch ahead on a copy stream; get_batch() makes the compute stream wait for the batch's copy event,
    runs rr_augment_frames and rr_ctnet_targets there and starts the next batch's copy, which may overwrite the other
    slot only after the work that read it has been enqueued (the copy stream waits for the compute stream).

    With FillDuck in the chain and road maps in the dataset, a sample whose plan has pastes ships its whole source frame
    and its paste table, and a batch with such a sample runs rr_augment_frames_pasted (its unpasted samples still ship
    windows; their pixels are bit-identical on either kernel).  Staging, device slots, the canvas and the scratch are
    sized once, from the largest frame of the dataset at the largest scale.

    With ColorJitter in the chain EVERY sample ships its whole frame (the contrast step needs its grey mean) and its
    three factors, which travel in the meta block; get_batch() runs rr_jitter_gray_mean and then the _jitter variant of
    the kernel the batch would have taken.  The factors are a function of (seed, rank, epoch, index) like every other
    draw, so seek() and resume need nothing more."""

    def __init__(self, dataset, params, batch_size, **kw):
        super().__init__(dataset, params, batch_size, **kw)
        from rrnet_amd import _C
        _C.lib()                                         # a missing library is an error here, not at the first batch
        b = self.bs
        self.m_cap = max(len(a) for a in dataset.annotations)
        r_cap = max(b * max(int((a[:, 5] == 0).sum()) for a in dataset.annotations), 1)
        # a crop of h x w reads at most h+1 rows and w+1 columns of the source at scale factors >= 1
        self.src_cap = b * (self.out_h + 2) * (self.out_w + 2) * 3
        self.pasting = params.get("fill_duck") is not None and bool(getattr(dataset, "with_road_map", False))
        self.jitter = params.get("jitter") is not None
        self.k_cap, self.canvas_pix, self.work, self.jitter_work = 0, 0, None, None
        if self.pasting or self.jitter:
            from PIL import Image
            from rrnet_amd import ops
            sizes = set()
            for k in range(len(dataset)):
                with Image.open(dataset.image_path(k)) as im:
                    sizes.add(im.size)
            self.src_cap = max(self.src_cap, b * max(w * h for w, h in sizes) * 3)
        if self.jitter:
            self.jitter_work = ops.jitter_workspace(b, self.device)
        if self.pasting:
            smax = max(params["scales"])
            self.canvas_pix = max(F.scaled_size(h, w, smax)[0] * F.scaled_size(h, w, smax)[1] for w, h in sizes)
            # total_n = max(int(factor * road pixels), 5) pastes per frame (functional.py:408)
            self.k_cap = b * max(int(params["fill_duck"]["factor"] * self.canvas_pix) + 1, 5)
            self.m_cap += 2 * (self.k_cap // b)             # a pair paste adds two rows
            # an object that does not fit its frame aborts the plan, so no object is larger than the largest frame
            self.work = ops.paste_workspace(b, self.canvas_pix, self.canvas_pix, self.device)
        self.factors_at = b * P_WORDS + (b + 1) + 4 * r_cap + b + (b + 1) + T_WORDS * self.k_cap
        self.meta_words = self.factors_at + 3 * b          # the factors' float32 bit patterns close the block
        self.r_cap = r_cap
        self.pinned = [(torch.empty(self.src_cap, dtype=torch.uint8).pin_memory(),
                        torch.empty(self.meta_words, dtype=torch.int32).pin_memory(),
                        torch.empty(b * self.m_cap * 8, dtype=torch.float32).pin_memory()) for _ in range(2)]
        self.slots = [tuple(torch.empty_like(t, device=self.device) for t in self.pinned[0]) for _ in range(2)]
        self.mean = torch.tensor(params["mean"], dtype=torch.float32, device=self.device)
        self.std = torch.tensor(params["std"], dtype=torch.float32, device=self.device)
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.events, self.info = [None, None], [None, None]
        self._prefetch(0)

    def _job(self, epoch, index):
        image, annotations, name, d = self._decide(epoch, index)
        src_w, src_h = image.size
        win = source_window(d, src_h, src_w, self.out_h, self.out_w, self.taps)
        if n_pastes(d) or jitter_of(d) is not None:        # a paste may read any pixel; the grey mean is over all of them
            win = (0, 0, src_h, src_w) + win[4:]
        y0, x0, wh, ww = win[:4]
        pix = np.asarray(image.crop((x0, y0, x0 + ww, y0 + wh)), dtype=np.uint8)
        return d, (src_h, src_w, win, pix), name

    def _prefetch(self, i):
        slot = i % 2
        res = self._collect(i)
        if self.events[slot] is not None:
            self.events[slot].synchronize()            # the copy that last read this pinned slot has finished
        p_src, p_meta, p_annos = self.pinned[slot]
        b = self.bs
        items = [(r[0],) + r[1] for r in res]
        src, params, rects, rect_off = pack_batch(items, p_src.numpy())
        if len(rects) > self.r_cap:
            raise RuntimeError("more ignore rectangles than the staging slot holds")
        m = max(int(r[0].annos.size(0)) for r in res)
        meta = p_meta.numpy()
        o1 = b * P_WORDS
        o2 = o1 + b + 1
        o3 = o2 + 4 * self.r_cap
        meta[:o1] = params.reshape(-1)
        meta[o1:o2] = rect_off
        meta[o2:o2 + rects.size] = rects.reshape(-1)
        meta[o3:o3 + b] = [int(r[0].annos.size(0)) for r in res]
        npaste = 0
        if self.pasting:
            pastes, paste_off, canvas, scratch = pack_pastes([r[0] for r in res])
            npaste = len(pastes)
            if npaste > self.k_cap or canvas > self.canvas_pix or scratch > self.canvas_pix:
                raise RuntimeError("paste plans exceed the staging slot or the canvas")
            o4 = o3 + b
            o5 = o4 + b + 1
            meta[o4:o5] = paste_off
            meta[o5:o5 + pastes.size] = pastes.reshape(-1)
        max_pixels = 0
        if self.jitter:
            factors, max_pixels = pack_jitter(items)
            meta[self.factors_at:self.factors_at + 3 * b] = factors.reshape(-1).view(np.int32)
        annos = p_annos[:b * m * 8].view(b, m, 8)
        annos.zero_()
        for k, r in enumerate(res):
            annos[k, :r[0].annos.size(0)] = r[0].annos[:, :8]
        taps = self.taps.device(self.device)
        cur = torch.cuda.current_stream(self.device)
        self.copy_stream.wait_stream(cur)              # the kernels that last read this device slot are enqueued on `cur`
        d_src, d_meta, d_annos = self.slots[slot]
        with torch.cuda.stream(self.copy_stream):
            d_src[:src.size].copy_(p_src[:src.size], non_blocking=True)
            d_meta.copy_(p_meta, non_blocking=True)
            d_annos[:b * m * 8].copy_(p_annos[:b * m * 8], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        self.events[slot] = ev
        self.info[slot] = (int(src.size), m, int(rects.shape[0]), taps, [r[2] for r in res], npaste, max_pixels)

    def get_batch(self):
        from rrnet_amd import ops
        i = self.i
        self.i += 1
        slot = i % 2
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(self.events[slot])
        d_src, d_meta, d_annos = self.slots[slot]
        nbytes, m, nrect, taps, names, npaste, max_pixels = self.info[slot]
        b = self.bs
        o1 = b * P_WORDS
        o2 = o1 + b + 1
        o3 = o2 + 4 * self.r_cap
        rects = d_meta[o2:o2 + 4 * nrect].view(nrect, 4) if nrect else None
        o4 = o3 + b
        o5 = o4 + b + 1
        if self.jitter:
            prm = d_meta[:o1].view(b, P_WORDS)
            factors = d_meta[self.factors_at:self.factors_at + 3 * b].view(torch.float32).view(b, 3)
            gray, _ = ops.jitter_gray_mean(d_src[:nbytes], prm, factors, max_pixels, work=self.jitter_work)
            if npaste:
                imgs = ops.augment_frames_pasted_jitter(d_src[:nbytes], prm, rects, d_meta[o1:o2], taps,
                                                        d_meta[o5:o5 + T_WORDS * npaste].view(npaste, T_WORDS),
                                                        d_meta[o4:o5], factors, gray, self.mean, self.std, self.out_h,
                                                        self.out_w, work=self.work)
            else:
                imgs = ops.augment_frames_jitter(d_src[:nbytes], prm, rects, d_meta[o1:o2], taps, factors, gray,
                                                 self.mean, self.std, self.out_h, self.out_w)
        elif npaste:
            imgs = ops.augment_frames_pasted(d_src[:nbytes], d_meta[:o1].view(b, P_WORDS), rects, d_meta[o1:o2], taps,
                                             d_meta[o5:o5 + T_WORDS * npaste].view(npaste, T_WORDS), d_meta[o4:o5],
                                             self.mean, self.std, self.out_h, self.out_w, work=self.work)
        else:
            imgs = ops.augment_frames(d_src[:nbytes], d_meta[:o1].view(b, P_WORDS), rects, d_meta[o1:o2], taps,
                                      self.mean, self.std, self.out_h, self.out_w)
        annos = d_annos[:b * m * 8].view(b, m, 8).clone()      # the criterion converts them to xyxy in place
        hm, wh, ind, off, mask = ops.ctnet_targets(annos, d_meta[o3:o3 + b], self.out_h, self.out_w,
                                                   self.p["scale_factor"], self.p["cls_num"])
        self._prefetch(i + 1)
        return imgs, annos, hm, wh, ind, off, mask, names

    def seek(self, n):
        """As _AugmentLoader.seek, and the device prefetch is redone for batch n: _prefetch waits for the copy that last
        read the pinned slot and orders the new copy behind the kernels that last read the device slot."""
        super().seek(n)
        self._prefetch(self.i)


class DeviceValLoader:
    """The validation chain (ToTensor -> Normalize) through the same kernel: batch 1, scale 1, no flip, crop = frame.
    Iterating yields (imgs [1,3,H,W] on the device, annos [1,n,8] on the host, [name]) like the reference's DataLoader
    with DronesDET.collate_fn; the images of this rank are `range(len(dataset))[rank::world_size]`, padded."""

    def __init__(self, dataset, params, rank=0, world_size=1, num_workers=4, device="cuda", taps=None):
        self.dataset, self.p = dataset, dict(params, crop=None, ignore_idx=None, scales=(1,), flip_p=0.0)
        self.device = torch.device(device) if not isinstance(device, torch.device) else device
        n = len(dataset)
        idx = np.arange(n)
        pad = (-n) % world_size
        if pad:
            idx = np.concatenate([idx, idx[:pad]])
        self.indices = [int(v) for v in idx[rank::world_size]]
        self.taps = taps if taps is not None else TapCache()
        self.workers = max(1, min(int(num_workers), MAX_THREADS))
        self.sampler = AugmentSampler(self.p)
        self.mean = self.std = None

    def __len__(self):
        return len(self.indices)

    def _job(self, index):
        image, annotations, name = self.dataset.load(index)
        src_w, src_h = image.size
        d = self.sampler.sample(annotations, src_h, src_w, 0, index)
        win = source_window(d, src_h, src_w, src_h, src_w, self.taps)
        return d, (src_h, src_w, win, np.asarray(image, dtype=np.uint8)), name

    def __iter__(self):
        from rrnet_amd import ops
        if self.mean is None:
            self.mean = torch.tensor(self.p["mean"], dtype=torch.float32, device=self.device)
            self.std = torch.tensor(self.p["std"], dtype=torch.float32, device=self.device)
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            ahead = 2 * self.workers
            futures = [pool.submit(self._job, i) for i in self.indices[:ahead]]
            for k in range(len(self.indices)):
                if k + ahead < len(self.indices):
                    futures.append(pool.submit(self._job, self.indices[k + ahead]))
                d, item, name = futures[k].result()
                futures[k] = None
                src, params, _, rect_off = pack_batch([(d,) + item])
                dev = self.device
                imgs = ops.augment_frames(torch.from_numpy(src).to(dev), torch.from_numpy(params).to(dev), None,
                                          torch.from_numpy(rect_off).to(dev), self.taps.device(dev), self.mean,
                                          self.std, item[0], item[1])
                yield imgs, d.annos.unsqueeze(0), [name]


def make_real_dataloaders(cfg, data_root):
    """(training loader, validation loader or None) over <data_root>/{train,val}."""
    import os
    from .drones_det import DronesDET
    rank, world = getattr(cfg.Distributed, "rank", 0), max(int(getattr(cfg.Distributed, "world_size", 1)), 1)
    taps = TapCache()
    params = chain_params(cfg.Train.transforms)
    road = bool(getattr(cfg.Train, "with_road", False)) if params["fill_duck"] is not None else False
    train = DeviceAugmentLoader(DronesDET(data_root, cfg.Train.transforms, 'train', with_road_map=road), params,
                                cfg.Train.batch_size, seed=cfg.seed, rank=rank, world_size=world,
                                num_workers=cfg.Train.num_workers, taps=taps)
    val = None
    if os.path.isdir(os.path.join(data_root, 'val', 'images')):
        val = DeviceValLoader(DronesDET(data_root, cfg.Val.transforms, 'val'), chain_params(cfg.Val.transforms),
                              rank=rank, world_size=world, num_workers=cfg.Val.num_workers, taps=taps)
    return train, val

"""Raw frames for batched inference (rrnet_amd.inference.detect_frames): decode with PIL in threads, group frames of
equal size, upload uint8.  No transform runs on the host; ToTensor -> Normalize -> rescale is rr_prepare_frames' work.

  FrameFolder         the *.jpg / *.png files of a directory, sorted by name, with DronesDET's `load` surface
  plan_buckets        the batching rule on a sequence of sizes (pure; what SizeBucketedFrames follows)
  SizeBucketedFrames  iterator of (frames uint8 [b,H,W,3] on the device, names)
  OrderedFrames       iterator of (list of uint8 [H_i,W_i,3] device tensors, names) in file order: for tiled detection"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .augment import MAX_THREADS

IMAGE_SUFFIXES = ('.jpg', '.jpeg', '.png', '.bmp')


class FrameFolder:
    """Images of one directory in name order.  load(i) -> (PIL RGB image, None, name without suffix)."""

    def __init__(self, images_dir):
        self.images_dir = images_dir
        files = sorted(f for f in os.listdir(images_dir) if f.lower().endswith(IMAGE_SUFFIXES))
        self.files = files
        self.mdf = [os.path.splitext(f)[0] for f in files]

    def __len__(self):
        return len(self.files)

    def load(self, item):
        from PIL import Image
        return Image.open(os.path.join(self.images_dir, self.files[item])).convert("RGB"), None, self.mdf[item]


class _Buckets:
    """Items grouped by key in arrival order: push returns a full batch as soon as a key holds `batch` items, flush the
    remainders in the order the keys were first seen."""

    def __init__(self, batch):
        self.batch = max(1, int(batch))
        self.open = {}                       # key -> items; dicts keep insertion order = first-seen order

    def push(self, key, item):
        items = self.open.setdefault(key, [])
        items.append(item)
        if len(items) == self.batch:
            self.open[key] = []
            return items
        return None

    def flush(self):
        rest = [items for items in self.open.values() if items]
        self.open = {}
        return rest


def plan_buckets(sizes, batch):
    """sizes: (H, W) of every frame in file order -> list of batches (lists of positions).  A batch holds frames of one
    size, at most `batch` of them; it is emitted when its bucket fills, the remainders at the end in first-seen bucket
    order.  Every position appears exactly once; the result depends on the sequence only."""
    buckets = _Buckets(batch)
    out = []
    for i, size in enumerate(sizes):
        full = buckets.push(tuple(size), i)
        if full is not None:
            out.append(full)
    return out + buckets.flush()


class SizeBucketedFrames:
    """Iterating yields (frames uint8 [b,H,W,3] on the device, [names]) with b <= batch and one (H, W) per batch, in
    plan_buckets' order over this rank's files `range(len(dataset))[rank::world_size]` (no padding: every index once).
    dataset needs `__len__` and `load(i) -> (PIL image, _, name)` (DronesDET, FrameFolder).  Decoding runs in threads
    (at most 16), ahead of the consumer, and is consumed in file order, so the emission order does not depend on timing."""

    def __init__(self, dataset, batch, rank=0, world_size=1, num_workers=4, device="cuda"):
        self.dataset, self.batch = dataset, max(1, int(batch))
        self.indices = list(range(len(dataset)))[rank::max(int(world_size), 1)]
        self.workers = max(1, min(int(num_workers), MAX_THREADS))
        self.device = torch.device(device) if not isinstance(device, torch.device) else device

    def __len__(self):
        return len(self.indices)

    def _job(self, index):
        loaded = self.dataset.load(index)
        return np.asarray(loaded[0], dtype=np.uint8), loaded[2]

    def _emit(self, items):
        frames = torch.from_numpy(np.stack([a for a, _ in items]))
        return frames.to(self.device, non_blocking=False), [n for _, n in items]

    def __iter__(self):
        buckets = _Buckets(self.batch)
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            ahead = max(2 * self.workers, self.batch)
            futures = [pool.submit(self._job, i) for i in self.indices[:ahead]]
            for k in range(len(self.indices)):
                if k + ahead < len(self.indices):
                    futures.append(pool.submit(self._job, self.indices[k + ahead]))
                arr, name = futures[k].result()
                futures[k] = None
                full = buckets.push(arr.shape[:2], (arr, name))
                if full is not None:
                    yield self._emit(full)
        for rest in buckets.flush():
            yield self._emit(rest)


class OrderedFrames(SizeBucketedFrames):
    """Iterating yields ([uint8 [H_i,W_i,3] device tensors], [names]) with `batch` frames per step (the last step may be
    shorter), in file order whatever the frames' sizes: the input of tiled detection, where tiles of one size make the batch.
    Same dataset surface, rank split and threaded decode consumed in file order as SizeBucketedFrames."""

    def _job(self, index):
        loaded = self.dataset.load(index)
        return np.array(loaded[0], dtype=np.uint8), loaded[2]       # a copy: PIL's buffer is read-only

    def _emit(self, items):
        return [torch.from_numpy(a).to(self.device, non_blocking=False) for a, _ in items], [n for _, n in items]

    def __iter__(self):
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            ahead = max(2 * self.workers, self.batch)
            futures = [pool.submit(self._job, i) for i in self.indices[:ahead]]
            items = []
            for k in range(len(self.indices)):
                if k + ahead < len(self.indices):
                    futures.append(pool.submit(self._job, self.indices[k + ahead]))
                items.append(futures[k].result())
                futures[k] = None
                if len(items) == self.batch:
                    yield self._emit(items)
                    items = []
        if items:
            yield self._emit(items)

"""DronesDET — datasets/drones_det.py:10-94 of the reference: the VisDrone-DET directory contract
`<root>/<split>/images/*.jpg` + `<root>/<split>/annotations/*.txt`, the per-sample transform chain, and the two
collate functions.

Differences from the reference, all on purpose:
  * annotations are parsed with numpy at index time (no pandas), first 8 columns, class 11 dropped (:40-42);
  * training images without a non-ignore box are dropped at index time — the reference crashes on them in RandomCrop
    (transforms.py:96: torch.randint(0, 0, ...)); `dropped` lists their names (other splits keep every image);
  * file names are sorted, so that an index means the same image on every rank and machine (os.listdir order is not
    defined);
  * with_road_map=True reads `<root>/<split>/roadmap/<name>.jpg` with PIL and keeps its blue channel (the reference
    takes channel 0 of cv2's BGR decode, drones_det.py:44-50; the two JPEG decoders may differ by a grey level, which a
    0/255 road mask does not notice); a missing file gives None, which FillDuck hands through.  A sample is then
    (image, annotations, road map); without the flag it is (image, annotations) as before."""
import os

import numpy as np
import torch

IGNORE_CLS = 0
OTHERS_CLS = 11


def parse_annotations(path):
    """One VisDrone annotation file -> int64 [n,8] rows x,y,w,h,score,cls,truncation,occlusion without class 11
    (drones_det.py:40-42).  Lines may end in a comma (some VisDrone files do)."""
    rows = []
    with open(path) as f:
        for line in f:
            parts = [p for p in line.strip().split(',') if p.strip() != '']
            if parts:
                rows.append([int(float(p)) for p in parts[:8]])
    annos = np.asarray(rows, dtype=np.int64).reshape(-1, 8)
    return annos[annos[:, 5] != OTHERS_CLS]


class DronesDET(torch.utils.data.Dataset):
    def __init__(self, root_dir, transforms=None, split='train', with_road_map=False):
        self.with_road_map = bool(with_road_map)
        self.roadmap_dir = os.path.join(root_dir, split, 'roadmap')
        self.images_dir = os.path.join(root_dir, split, 'images')
        self.annotations_dir = os.path.join(root_dir, split, 'annotations')
        self.transforms = transforms
        self.mdf, self.annotations, self.dropped = [], [], []
        for name in sorted(f[:-4] for f in os.listdir(self.images_dir) if f.endswith('.jpg')):
            annos = parse_annotations(os.path.join(self.annotations_dir, name + '.txt'))
            if split != 'train' or (annos[:, 5] != IGNORE_CLS).any():
                self.mdf.append(name)
                self.annotations.append(annos)
            else:
                self.dropped.append(name)

    def __len__(self):
        return len(self.mdf)

    def image_path(self, item):
        return os.path.join(self.images_dir, self.mdf[item] + '.jpg')

    def load_roadmap(self, item):
        """-> uint8 [H,W] (the blue channel of the road-map JPEG) or None where the file is missing."""
        from PIL import Image
        path = os.path.join(self.roadmap_dir, self.mdf[item] + '.jpg')
        if not os.path.isfile(path):
            return None
        return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)[:, :, 2])

    def load(self, item):
        """-> (PIL RGB image, a fresh copy of the int64 annotations, name[, road map when with_road_map]); the
        transforms write into the copy."""
        from PIL import Image
        out = Image.open(self.image_path(item)).convert("RGB"), self.annotations[item].copy(), self.mdf[item]
        return out + (self.load_roadmap(item),) if self.with_road_map else out

    def __getitem__(self, item):
        loaded = self.load(item)
        image, annotation, name = loaded[:3]
        sample = (image, annotation) + tuple(loaded[3:])
        if self.transforms:
            sample = self.transforms(sample)
        return tuple(sample) + (name,)

    @staticmethod
    def collate_fn(batch):
        """drones_det.py:56-67: [(img, annos, name)] -> imgs [B,3,H,W], annos [B,M,8] zero padded, names."""
        max_n = max(b[1].size(0) for b in batch)
        annos = torch.zeros(len(batch), max_n, 8)
        for i, b in enumerate(batch):
            annos[i, :b[1].size(0), :] = b[1][:, :8]
        return torch.cat([b[0].unsqueeze(0) for b in batch]), annos, [b[2] for b in batch]

    @staticmethod
    def collate_fn_ctnet(batch):
        """drones_det.py:69-94: [(img, annos, hm, wh, ind, offset, reg_mask, name)] -> the 8-tuple of the hot path."""
        max_n = max(b[1].size(0) for b in batch)
        bs = len(batch)
        annos, whs, offsets = torch.zeros(bs, max_n, 8), torch.zeros(bs, max_n, 2), torch.zeros(bs, max_n, 2)
        inds, reg_masks = torch.zeros(bs, max_n, 1), torch.zeros(bs, max_n, 1)
        for i, b in enumerate(batch):
            annos[i, :b[1].size(0), :] = b[1][:, :8]
            whs[i, :b[3].size(0), :] = b[3]
            inds[i, :b[4].size(0), :] = b[4]
            offsets[i, :b[5].size(0), :] = b[5]
            reg_masks[i, :b[6].size(0), :] = b[6]
        imgs = torch.cat([b[0].unsqueeze(0) for b in batch])
        hms = torch.cat([b[2].unsqueeze(0) for b in batch])
        return imgs, annos, hms, whs, inds, offsets, reg_masks, [b[7] for b in batch]

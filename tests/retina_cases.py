"""Inputs and plain-torch restatements for the RetinaNet tests (tests/test_retina_host.py, test_retina_gpu.py,
test_retina_model_gpu.py).

The restatements are written from the description of the operations (anchor assignment by IoU, focal loss, smooth-L1, box
decode, 3x3/2 max-pool, bilinear upsample-add, ResNet + FPN + shared heads), in tensor operations that run in float64 or
float32 on the CPU: `nn.Conv2d`, `F.max_pool2d`, `F.interpolate`, `F.batch_norm`.  They are the reference side of every
comparison; tests/test_retina_host.py pins the criterion restatement to recorded results of the original criterion."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

U32 = 2.0 ** -24

# ---- criterion inputs -----------------------------------------------------------------------------------------------
GT_XYXY = [(4, 4, 20, 20), (10, 6, 40, 30), (0, 0, 0, 0), (30, 20, 33, 24), (2, 30, 50, 54), (20, 8, 31, 30)]
GT_CLASSES = [3, 1, 0, 7, 10, 2]
ANCHOR_COUNTS = {(64, 64): 756, (72, 56): 801, (40, 104): 846}


def anchors_of(size):
    from rrnet_amd.modules.anchor import Anchors
    return Anchors(sizes=(16, 64, 128))(size)


def annos_of(boxes_xyxy, classes, rows=None):
    """xyxy boxes + classes -> one image's [rows, 8] float32 annotation block: (x, y, w, h, score, class, trunc, occl),
    zero rows behind the boxes (what the collate pads with)."""
    rows = len(boxes_xyxy) if rows is None else rows
    out = np.zeros((rows, 8), dtype=np.float32)
    for i, ((x1, y1, x2, y2), c) in enumerate(zip(boxes_xyxy, classes)):
        out[i, :6] = (x1, y1, x2 - x1, y2 - y1, 1.0 if c else 0.0, c)
    return out


def criterion_batch(kind, num_classes=10):
    """-> (annos [B,M,8] float32 numpy, note).  kinds: 'base' (B=3: the six rows, no annotations, the rows reversed),
    'duplicate' (one image, box 1 twice with the same class), 'bad_class' (box 0 carries class num_classes + 3)."""
    cls = [min(c, num_classes) if c else 0 for c in GT_CLASSES]
    if kind == "base":
        a = annos_of(GT_XYXY, cls, 7)
        return np.stack([a, np.zeros_like(a), annos_of(GT_XYXY[::-1], cls[::-1], 7)])
    if kind == "duplicate":
        return annos_of(GT_XYXY + [GT_XYXY[1]], cls + [cls[1]])[None]
    if kind == "bad_class":
        bad = list(cls)
        bad[0] = num_classes + 3
        return annos_of(GT_XYXY, bad)[None]
    raise KeyError(kind)


# The criterion's launch routes (tests/test_retina_gpu.py runs each against float64; tests/test_retina_host.py proves on the
# host that each input sits on its route and that float64 can make every discrete decision of it on its own).
# name: (kind, anchors, classes, seed of the predictions, saturated logits); anchors = an image size for `anchors_of`, a
# number of synthetic anchors, or None where the kind brings its own.
CRIT_ROUTE_CASES = {
    # C % 4 == 0: the float4 loss kernels.  4 classes: the rows carry 3, 1, 0, 4, 4, 2, every lane of the one vector is hot
    # somewhere; 8: class 8 is lane 3 of the second vector; 12: class 10 is in the third vector.  Row 3 (the 3x4 box) wins no
    # anchor, so its class 7 is never hot: c12_swapped moves 7 and 10 to rows 0 and 1, which do win.
    "c4": ("base", (64, 64), 4, 41, False),
    "c8": ("base", (64, 64), 8, 42, False),
    "c12": ("base", (64, 64), 12, 43, False),
    "c12_swapped": ("swapped", (64, 64), 12, 44, False),
    "c8_saturated": ("base", (64, 64), 8, 45, True),
    # M against ANNO_CHUNK = 256: exactly one chunk, one row into the second, one row into the third
    "many_256": (("many", 256, 3), (64, 64), 10, 46, False),
    "many_257": (("many", 257, 6), (72, 56), 10, 47, False),
    "many_513": (("many", 513, 2), (64, 64), 10, 48, False),
    # IoU exactly 0.5 (positive), 0.75, 0.75, 0 and 2/5 (not below 0.4: ignored)
    "exact_thresholds": ("exact", None, 10, 49, False),
    # rr_retina_loss_blocks at both ends: 1 workgroup; the cap of 1024, where 1 048 700 elements make the stride loops of
    # 262 144 threads wrap a fifth time for the last 124
    "one_block_100": (("synthetic", 11), 100, 10, 50, False),
    "one_anchor": (("synthetic", 12), 1, 10, 51, False),
    "block_cap": (("synthetic", 21), 104870, 10, 52, False),
}
MANY_DUPLICATE = (3, 300)            # many_513: row 300 repeats row 3, class included
EXACT_ANCHORS = [[0, 0, 4, 4], [10, 10, 14, 14], [20, 20, 24, 24], [30, 30, 34, 34], [40, 40, 45, 45]]
EXACT_XYXY = [(0, 0, 4, 2), (40, 40, 45, 42), (10, 10, 13, 14), (20, 20, 24, 23)]
EXACT_STATE, EXACT_ARGMAX = [1, 1, 1, 0, -1], [0, 2, 3, 0, 1]
SWAPPED_CLASSES = [7, 10, 0, 3, 1, 2]


def many_boxes(m, seed):
    """-> [2, m, 8]: m boxes with corners uniform in (-4, 56) and sizes uniform in (3, 48), snapped to quarter pixels, classes
    uniform in 1..10; from 301 rows on, row 300 repeats row 3.  The second image holds the same rows in reverse order, so a
    tie across a chunk boundary is met from both sides."""
    g = np.random.default_rng(seed)
    xy = np.round(g.uniform(-4, 56, (m, 2)) * 4) / 4
    wh = np.round(g.uniform(3, 48, (m, 2)) * 4) / 4
    out = np.zeros((m, 8), dtype=np.float32)
    out[:, 0:2], out[:, 2:4], out[:, 4] = xy, wh, 1.0
    out[:, 5] = g.integers(1, 11, m)
    if m > MANY_DUPLICATE[1]:
        out[MANY_DUPLICATE[1]] = out[MANY_DUPLICATE[0]]
    return np.stack([out, out[::-1].copy()])


def synthetic_anchors(a, seed):
    """a boxes (xyxy float32): centres uniform in a square of side 1024 (64 for fewer than 1000), sides 16, 64 or 128 times
    uniform(0.7, 1.4)."""
    g = np.random.default_rng(seed)
    ctr = g.uniform(0, 1024 if a >= 1000 else 64, (a, 2))
    half = 0.5 * g.choice([16.0, 64.0, 128.0], (a, 1)) * g.uniform(0.7, 1.4, (a, 2))
    return np.concatenate([ctr - half, ctr + half], axis=1).astype(np.float32)


def synthetic_batch(anchors, seed):
    """-> [1, 7, 8]: seven boxes, box i being anchor (i * A) // 7 with its sides scaled by uniform(0.85, 1.2) and its centre
    moved by up to 8 % of them, so that every box has anchors on either side of both thresholds."""
    g = np.random.default_rng(seed + 1000)
    a = anchors.shape[0]
    src = anchors[[(i * a) // 7 for i in range(7)]].astype(np.float64)
    wh = src[:, 2:4] - src[:, 0:2]
    ctr = 0.5 * (src[:, 0:2] + src[:, 2:4]) + g.uniform(-0.08, 0.08, (7, 2)) * wh
    wh = wh * g.uniform(0.85, 1.2, (7, 2))
    boxes = np.round(np.concatenate([ctr - 0.5 * wh, ctr + 0.5 * wh], axis=1) * 4) / 4
    return annos_of([tuple(r) for r in boxes], [1 + (3 * i) % 10 for i in range(7)])[None]


def criterion_inputs(kind, where, num_classes=10):
    """-> (annos [B,M,8] float32 numpy, anchors [A,4] float32 tensor) of a CRIT_CASES / CRIT_ROUTE_CASES entry."""
    if kind == "swapped":
        a = annos_of(GT_XYXY, SWAPPED_CLASSES, 7)
        return np.stack([a, np.zeros_like(a), annos_of(GT_XYXY[::-1], SWAPPED_CLASSES[::-1], 7)]), anchors_of(where)
    if kind == "exact":
        return annos_of(EXACT_XYXY, [1, 2, 3, 4])[None], torch.tensor(EXACT_ANCHORS, dtype=torch.float32)
    if isinstance(kind, tuple) and kind[0] == "many":
        return many_boxes(kind[1], kind[2]), anchors_of(where)
    if isinstance(kind, tuple) and kind[0] == "synthetic":
        anchors = synthetic_anchors(where, kind[1])
        return synthetic_batch(anchors, kind[1]), torch.from_numpy(anchors)
    return criterion_batch(kind, num_classes), anchors_of(where)


def loss_blocks(a, c):
    """rr_retina_loss_blocks of the built library (a host function: no GPU)."""
    from rrnet_amd import _C
    return int(_C.fn("rr_retina_loss_blocks")(int(a), int(c)))


def input_margins(annos, anchors, num_classes):
    """What makes an input decidable by float64 alone -> dict: `agree` (the float32 and float64 restatements give the same
    states, argmax and classes), `threshold` (smallest distance of a best IoU from 0.4 or 0.5), `gap` (smallest best minus
    second-best IoU on a positive anchor, rows that repeat the winner's box exactly left out), `repeats` (rows whose box
    equals an earlier row's, per image), `a64` (the float64 assignment)."""
    a64 = assign(annos, anchors, num_classes, torch.float64)
    a32 = assign(annos, anchors, num_classes, torch.float32)
    agree = all(bool(torch.equal(a64[k], a32[k])) for k in ("state", "argmax", "cls", "npos"))
    best = a64["max_iou"]
    threshold = min(float((best - 0.4).abs().min()), float((best - 0.5).abs().min()))
    gap, repeats = float("inf"), []
    for i in range(annos.shape[0]):
        rows = torch.from_numpy(np.ascontiguousarray(annos[i, :, :4]))
        same = (rows[:, None, :] == rows[None, :, :]).all(dim=2)                # [M, M]
        live = rows[:, 2:4].abs().sum(dim=1) > 0                                # padding rows repeat each other by design
        repeats.append(int((torch.triu(same, 1) & live[:, None] & live[None, :]).any(dim=0).sum()))
        pos = torch.nonzero(a64["state"][i] == 1)[:, 0]
        if pos.numel():
            iou = a64["iou"][i][:, pos].clone()
            iou[same[a64["argmax"][i][pos]].T] = -1.0                           # the winner and its exact repeats
            gap = min(gap, float((best[i][pos] - iou.max(dim=0).values).min()))
    return {"agree": agree, "threshold": threshold, "gap": gap, "repeats": repeats, "a64": a64}


def criterion_preds(b, a, c, seed, saturate=False):
    g = np.random.default_rng(seed)
    logits = (g.standard_normal((b, a, c)) * 2.0 - 2.0).astype(np.float32)
    loc = (g.standard_normal((b, a, 4)) * 0.7).astype(np.float32)
    if saturate:
        pick = g.random((b, a, c))
        logits[pick < 0.15] = 40.0
        logits[pick > 0.85] = -40.0
    return loc, logits


# ---- criterion ------------------------------------------------------------------------------------------------------
def pairwise_iou(boxes, anchors):
    """[M,4] x [A,4] (both xyxy) -> [M,A]; the union is kept away from zero at 1e-8."""
    area_b = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    area_a = (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])
    iw = torch.minimum(boxes[:, None, 2], anchors[None, :, 2]) - torch.maximum(boxes[:, None, 0], anchors[None, :, 0])
    ih = torch.minimum(boxes[:, None, 3], anchors[None, :, 3]) - torch.maximum(boxes[:, None, 1], anchors[None, :, 1])
    inter = iw.clamp(min=0) * ih.clamp(min=0)
    union = (area_b[:, None] + area_a[None, :] - inter).clamp(min=1e-8)
    return inter / union


def assign(annos, anchors, num_classes, dtype):
    """annos [B,M,8] (xywh rows), anchors [A,4] -> dict of per-(image, anchor) tensors: max_iou, argmax (lowest index on
    ties), state (1 positive: IoU >= 0.5; 0 negative: IoU < 0.4; -1 between), cls (class of a positive inside
    [1, num_classes], else 0), target [B,A,4] (positives; 0 elsewhere), npos [B]."""
    annos = torch.as_tensor(annos).to(dtype)
    anchors = torch.as_tensor(anchors).to(dtype)
    b, a = annos.shape[0], anchors.shape[0]
    xyxy = annos[..., :4].clone()
    xyxy[..., 2:4] = xyxy[..., 2:4] + xyxy[..., 0:2]
    aw, ah = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    acx, acy = anchors[:, 0] + 0.5 * aw, anchors[:, 1] + 0.5 * ah
    out = {k: [] for k in ("max_iou", "argmax", "state", "cls", "target", "iou")}
    for i in range(b):
        iou = pairwise_iou(xyxy[i], anchors)
        best = iou.max(dim=0).values
        first = (iou == best[None, :]).to(torch.int64).argmax(dim=0)       # argmax of a 0/1 table: the first 1
        pos = best >= 0.5
        state = torch.where(pos, 1, torch.where(best < 0.4, 0, -1))
        g = xyxy[i][first]
        klass = annos[i][first, 5].to(torch.int64)
        klass = torch.where(pos & (klass >= 1) & (klass <= num_classes), klass, torch.zeros_like(klass))
        gw, gh = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
        gcx, gcy = g[:, 0] + 0.5 * gw, g[:, 1] + 0.5 * gh
        gw, gh = gw.clamp(min=1), gh.clamp(min=1)
        scale = torch.tensor([0.1, 0.1, 0.2, 0.2], dtype=dtype)
        t = torch.stack(((gcx - acx) / aw, (gcy - acy) / ah, torch.log(gw / aw), torch.log(gh / ah)), dim=1) / scale
        t = torch.where(pos[:, None], t, torch.zeros_like(t))
        for k, v in (("max_iou", best), ("argmax", first), ("state", state), ("cls", klass), ("target", t), ("iou", iou)):
            out[k].append(v)
    out = {k: torch.stack(v) for k, v in out.items()}
    out["npos"] = (out["state"] == 1).sum(dim=1)
    return out


def focal_terms(logits, hot):
    """Element-wise focal loss of logits against the boolean table `hot`: p = sigmoid clamped to [1e-7, 1 - 1e-7];
    0.75 (1-p)^2 (-log p) on a target, 0.25 p^2 (-log(1-p)) elsewhere."""
    p = torch.sigmoid(logits).clamp(1e-7, 1. - 1e-7)
    return torch.where(hot, 0.75 * (1. - p) ** 2 * -torch.log(p), 0.25 * p ** 2 * -torch.log(1. - p))


def smooth_l1_terms(diff):
    d = diff.abs()
    return torch.where(d <= 1.0 / 9.0, 0.5 * 9.0 * d ** 2, d - 0.5 / 9.0)


def criterion(loc, logits, annos, anchors, num_classes, dtype):
    """-> (cls_loss, loc_loss, assignment): per image the focal sum over the not-ignored anchors / max(1, positives) and the
    smooth-L1 mean over the positives' 4 values (0 without positives), both averaged over the batch."""
    asg = assign(annos, anchors, num_classes, dtype)
    b, a, c = logits.shape
    cls_losses, loc_losses = [], []
    for i in range(b):
        used = asg["state"][i] >= 0
        pos = asg["state"][i] == 1
        hot = asg["cls"][i][:, None] == torch.arange(1, c + 1)[None, :]
        npos = int(pos.sum())
        cls_losses.append(focal_terms(logits[i][used], hot[used]).sum() / max(1, npos))
        if npos:
            loc_losses.append(smooth_l1_terms(asg["target"][i][pos] - loc[i][pos]).mean())
        else:
            loc_losses.append(loc.sum() * 0)
    return sum(cls_losses) / b, sum(loc_losses) / b, asg


def criterion_with_grads(loc, logits, annos, anchors, num_classes, dtype, w_cls=1.0, w_loc=1.0):
    """numpy in -> dict(cls_loss, loc_loss, dloc, dlogits, asg) of the restatement in `dtype`, backward driven by
    w_cls * cls_loss + w_loc * loc_loss."""
    lo = torch.from_numpy(loc).to(dtype).requires_grad_()
    lg = torch.from_numpy(logits).to(dtype).requires_grad_()
    cl, ll, asg = criterion(lo, lg, annos, anchors, num_classes, dtype)
    (w_cls * cl + w_loc * ll).backward()
    return {"cls_loss": float(cl.detach()), "loc_loss": float(ll.detach()), "dloc": lo.grad.numpy().astype(np.float64),
            "dlogits": lg.grad.numpy().astype(np.float64), "asg": asg}


# ---- decode -----------------------------------------------------------------------------------------------------------
def decode(logits, loc, anchors, dtype, thr=0.1):
    """One image: logits [A,C], loc [A,4], anchors [A,4] -> (rows [k,6] = x, y, w, h, prob, class + 1 in anchor order,
    kept anchor indices).  First maximum over the classes; kept when prob > thr."""
    logits, loc, anchors = (torch.as_tensor(t).to(dtype) for t in (logits, loc, anchors))
    p = torch.sigmoid(logits)
    best = p.max(dim=1).values
    first = (p == best[:, None]).to(torch.int64).argmax(dim=1)
    keep = torch.nonzero(best > thr)[:, 0]
    box, d = anchors[keep], loc[keep]
    w, h = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
    cx, cy = box[:, 0] + 0.5 * w, box[:, 1] + 0.5 * h
    pw, ph = torch.exp(d[:, 2] * 0.2) * w, torch.exp(d[:, 3] * 0.2) * h
    px, py = cx + d[:, 0] * 0.1 * w - 0.5 * pw, cy + d[:, 1] * 0.1 * h - 0.5 * ph
    rows = torch.stack((px, py, pw, ph, best[keep], (first[keep] + 1).to(dtype)), dim=1)
    return rows, keep


def hard_nms_sorted(xyxy_sorted, thresh):
    """Greedy hard NMS over float32 rows [n, >=4] (x1, y1, x2, y2) already in visiting order, the "+1" pixel convention,
    IoU > thresh suppresses, all arithmetic in float32 -> kept row indices."""
    d = np.ascontiguousarray(xyxy_sorted, dtype=np.float32)
    one = np.float32(1)
    x1, y1, x2, y2 = (d[:, i] for i in range(4))
    areas = (x2 - x1 + one) * (y2 - y1 + one)
    dead = np.zeros(d.shape[0], dtype=bool)
    keep = []
    for i in range(d.shape[0]):
        if dead[i]:
            continue
        keep.append(i)
        r = np.arange(i + 1, d.shape[0])
        w = np.maximum(np.float32(0), np.minimum(x2[i], x2[r]) - np.maximum(x1[i], x1[r]) + one)
        h = np.maximum(np.float32(0), np.minimum(y2[i], y2[r]) - np.maximum(y1[i], y1[r]) + one)
        inter = w * h
        dead[r[inter / (areas[i] + areas[r] - inter) > np.float32(thresh)]] = True
    return keep


# ---- max-pool, bilinear upsample-add -----------------------------------------------------------------------------------
def maxpool(x):
    """x NCHW (CPU) -> (y, tap): MaxPool2d(3, 2, 1) and the winning tap ky*3+kx of every window, from ATen's flat index."""
    y, flat = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    w = x.shape[3]
    oy = torch.arange(y.shape[2])[:, None]
    ox = torch.arange(y.shape[3])[None, :]
    ky = flat // w - (2 * oy - 1)
    kx = flat % w - (2 * ox - 1)
    return y, (ky * 3 + kx).to(torch.uint8)


def bilinear_add(x, y):
    return y + F.interpolate(x, size=y.shape[2:], mode='bilinear', align_corners=False)


# ---- the model --------------------------------------------------------------------------------------------------------
class _Block(nn.Module):
    def __init__(self, cin, planes, stride, project):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = None
        if project:
            self.downsample = nn.Sequential(nn.Conv2d(cin, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4))

    def forward(self, x):
        skip = x if self.downsample is None else self.downsample(x)
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.relu(self.bn2(self.conv2(x)))
        return F.relu(self.bn3(self.conv3(x)) + skip)


IDENTITY_DEPTHS = (2, 1, 1, 2)       # the smallest ResNet with identity blocks at its narrowest (256) and widest (2048) stage


class _Backbone(nn.Module):
    def __init__(self, depths):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cin = 64
        for i, (planes, depth) in enumerate(zip((64, 128, 256, 512), depths)):
            stride = 1 if i == 0 else 2
            blocks = [_Block(cin, planes, stride, True)] + [_Block(planes * 4, planes, 1, False) for _ in range(depth - 1)]
            setattr(self, "layer%d" % (i + 1), nn.Sequential(*blocks))
            cin = planes * 4

    def stages(self, x):
        """-> (l1, l2, l3, l4), what the package's ResNet returns."""
        x = F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        l1 = self.layer1(x)
        l2 = self.layer2(l1)
        l3 = self.layer3(l2)
        return l1, l2, l3, self.layer4(l3)

    def forward(self, x):
        return self.stages(x)[1:]


class _Pyramid(nn.Module):
    def __init__(self):
        super().__init__()
        self.lat_layer1 = nn.Conv2d(2048, 256, 1)
        self.lat_layer2 = nn.Conv2d(1024, 256, 1)
        self.lat_layer3 = nn.Conv2d(512, 256, 1)
        self.top_layer1 = nn.Conv2d(256, 256, 3, 1, 1)
        self.top_layer2 = nn.Conv2d(256, 256, 3, 1, 1)

    def forward(self, c3, c4, c5):
        p5 = self.lat_layer1(c5)
        p4 = self.top_layer1(bilinear_add(p5, self.lat_layer2(c4)))
        p3 = self.top_layer2(bilinear_add(p4, self.lat_layer3(c3)))
        return p3, p4, p5


class _Head(nn.Module):
    def __init__(self, planes):
        super().__init__()
        seq = []
        for _ in range(4):
            seq += [nn.Conv2d(256, 256, 3, 1, 1), nn.ReLU()]
        self.detect_layer = nn.Sequential(*seq, nn.Conv2d(256, planes, 3, 1, 1))

    def forward(self, x):
        return self.detect_layer(x)


class PlainRetinaNet(nn.Module):
    """The whole model in stock torch modules, with the parameter names of the package's RetinaNet (strict loading)."""
    DEPTHS = {"resnet10": (1, 1, 1, 1), "resnet50": (3, 4, 6, 3), "resnet101": (3, 4, 23, 3)}

    def __init__(self, backbone="resnet10", num_classes=10, num_anchors=9):
        super().__init__()
        self.num_classes = num_classes
        self.backbone = _Backbone(self.DEPTHS[backbone])
        self.fpn = _Pyramid()
        self.cls = _Head(num_anchors * num_classes)
        self.loc = _Head(num_anchors * 4)

    def forward(self, x):
        n = x.shape[0]
        locs, clss = [], []
        for fm in self.fpn(*self.backbone(x)):
            locs.append(self.loc(fm).permute(0, 2, 3, 1).reshape(n, -1, 4))
            clss.append(self.cls(fm).permute(0, 2, 3, 1).reshape(n, -1, self.num_classes))
        return torch.cat(locs, 1), torch.cat(clss, 1)


def retina_cfg(backbone="resnet10", num_classes=10, crop=(128, 128), batch=2):
    import copy
    from rrnet_amd.configs.retinanet_config import Config
    cfg = copy.deepcopy(Config)
    cfg.Model.backbone = backbone
    cfg.num_classes = num_classes
    cfg.Train.pretrained = False
    cfg.Train.crop_size = tuple(crop)
    cfg.Train.batch_size = batch
    cfg.data_root = None
    cfg.Distributed.gpu_id, cfg.Distributed.rank, cfg.Distributed.world_size = 0, 0, 1
    return cfg


def state_keys(model):
    return [[k, list(v.shape)] for k, v in model.state_dict().items()]


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = math.sqrt(float((b * b).sum()))
    return math.sqrt(float(((a - b) ** 2).sum())) / den if den > 0 else math.sqrt(float((a * a).sum()))

"""Host side of RetinaNet (no GPU): anchors, the criterion restatement of tests/retina_cases.py and `focal_loss` against
recorded results of the reference (tests/golden/retina.npz, tools/gen_golden_retina.py), the `state_dict` key lists, the
import lines of the reference's scripts/RetinaNet/{train,eval}.py, tools/train.py's configuration and the refusal of
data-parallel runs.

Loss bounds are derived, not measured: a loss is a sum of n non-negative float32 terms, each carrying a few roundings of
its own (sigmoid, log, products: at most 16 u relative), summed in any order: |a - b| <= (n + 16) u |sum|, u = 2^-24."""
import hashlib
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import retina_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "retina.npz"))


@pytest.mark.parametrize("size", [(64, 64), (72, 56), (40, 104), (512, 512)])
def test_anchors_bit_equal_to_the_reference(golden, size):
    got = rc.anchors_of(size).numpy()
    assert got.dtype == np.float32
    key = "anchors_%dx%d" % size
    if key in golden:
        assert got.shape == golden[key].shape == (rc.ANCHOR_COUNTS[size], 4)
        assert np.array_equal(got.view(np.uint32), golden[key].view(np.uint32))
    else:                                     # the large table: digest of its bytes plus both ends
        assert got.shape == (int(golden[key + "_rows"]), 4)
        assert np.array_equal(got[:64].view(np.uint32), golden[key + "_head"].view(np.uint32))
        assert np.array_equal(got[-64:].view(np.uint32), golden[key + "_tail"].view(np.uint32))
        assert hashlib.sha256(got.tobytes()).digest() == golden[key + "_sha256"].tobytes()


def test_anchors_are_cached_and_not_aliased():
    from rrnet_amd.modules.anchor import Anchors
    maker = Anchors(sizes=(16, 64, 128))
    a = maker((64, 64))
    a += 1
    assert torch.equal(maker((64, 64)) + 1, a)


@pytest.mark.parametrize("case", range(4))
def test_restated_criterion_equals_the_reference(golden, case):
    k = "crit%d_" % case
    annos, loc, logits = golden[k + "annos"], golden[k + "loc"], golden[k + "logits"]
    size = tuple(int(v) for v in golden[k + "size"])
    ref_cls, ref_loc = golden[k + "losses"]
    b, a, c = logits.shape
    anchors = rc.anchors_of(size)
    for dtype in (torch.float32, torch.float64):
        r = rc.criterion_with_grads(loc, logits, annos, anchors, c, dtype)
        npos = r["asg"]["npos"].numpy()
        tol_cls = (a * c + 16) * rc.U32 * abs(ref_cls)
        tol_loc = (4 * int(npos.max()) + 16) * rc.U32 * abs(ref_loc)
        print("criterion case %d %s: cls %.9g (ref %.9g, tol %.3g)  loc %.9g (ref %.9g, tol %.3g)  npos %s"
              % (case, dtype, r["cls_loss"], ref_cls, tol_cls, r["loc_loss"], ref_loc, tol_loc, npos.tolist()))
        assert abs(r["cls_loss"] - ref_cls) <= tol_cls
        assert abs(r["loc_loss"] - ref_loc) <= tol_loc


HOT_VECTORS = {"c4": {0}, "c8": {0, 1}, "c12": {0, 2}, "c12_swapped": {0, 1, 2}, "c8_saturated": {0, 1}}
LOSS_BLOCKS = {"one_block_100": 1, "one_anchor": 1, "exact_thresholds": 1, "block_cap": 1024}


@pytest.mark.parametrize("name", list(rc.CRIT_ROUTE_CASES))
def test_criterion_route_inputs_are_decidable_and_on_their_route(name):
    """Every input of rc.CRIT_ROUTE_CASES, before any kernel sees it.  Decidable: the float32 and float64 restatements agree
    on every state, argmax and class; every best IoU is more than 1e-6 from 0.4 and 0.5 (exact_thresholds sits on them on
    purpose, with IoUs that both formats hold exactly or round alike); on every positive anchor the best IoU is more than
    1e-6 above the best of the other boxes (many_513's one repeated row apart).  On its route: C % 4, M against the chunk of
    256 with winners behind each chunk boundary, rr_retina_loss_blocks at 1 and at 1024."""
    kind, where, classes, _seed, _sat = rc.CRIT_ROUTE_CASES[name]
    annos, anchors = rc.criterion_inputs(kind, where, classes)
    r = rc.input_margins(annos, anchors, classes)
    a64 = r["a64"]
    b, m, a = annos.shape[0], annos.shape[1], anchors.shape[0]
    blocks = rc.loss_blocks(a, classes)
    print("\n%s: B=%d M=%d A=%d C=%d loss blocks %d  npos %s  threshold margin %.3g  top-2 gap %.3g  repeated rows %s"
          % (name, b, m, a, classes, blocks, a64["npos"].tolist(), r["threshold"], r["gap"], r["repeats"]))
    assert r["agree"]
    assert int(a64["npos"][0]) > 0
    assert r["gap"] > 1e-6
    assert r["repeats"] == ([1, 1] if name == "many_513" else [0] * b)
    if name == "exact_thresholds":
        assert a64["state"][0].tolist() == rc.EXACT_STATE and a64["argmax"][0].tolist() == rc.EXACT_ARGMAX
        assert a64["max_iou"][0].tolist() == [0.5, 0.75, 0.75, 0.0, 10.0 / 25.0]
        a32 = rc.assign(annos, anchors, classes, torch.float32)
        assert a32["max_iou"][0].tolist() == [0.5, 0.75, 0.75, 0.0, float(np.float32(10.0) / np.float32(25.0))]
    else:
        assert r["threshold"] > 1e-6
    if name in HOT_VECTORS:
        assert classes % 4 == 0 and a == rc.ANCHOR_COUNTS[where]
        hot = set()
        for i in (0, 2):
            rows_cls = annos[i, :, 5].astype(int).tolist()
            got = set(a64["cls"][i][a64["state"][i] == 1].tolist())
            box3 = 3 if i == 0 else 2                                           # the 3x4 box wins no anchor; 0 is the padding row
            assert got == set(c for j, c in enumerate(rows_cls) if c and j != box3), (got, rows_cls)
            hot |= got
        if classes == 4:
            assert hot == {1, 2, 3, 4}                                          # every lane of the one vector
        assert set((c - 1) // 4 for c in hot) == HOT_VECTORS[name]
    if isinstance(kind, tuple) and kind[0] == "many":
        assert m == kind[1] and (m - 1) // 256 == {256: 0, 257: 1, 513: 2}[m]
        for i in range(b):
            winners = a64["argmax"][i][a64["state"][i] == 1]
            behind = [int((winners >= 256).sum()), int((winners >= 512).sum())]
            print("  image %d: positives won by rows >= 256: %d, >= 512: %d" % (i, behind[0], behind[1]))
            assert (behind[0] > 0) == (m > 256) and (behind[1] > 0) == (m > 512)
        if m == 513:
            lo, hi = rc.MANY_DUPLICATE
            assert np.array_equal(annos[0, lo], annos[0, hi])
            tied = (a64["state"][0] == 1) & (a64["argmax"][0] == lo)
            assert int(tied.sum()) > 0 and bool((a64["iou"][0][lo][tied] == a64["iou"][0][hi][tied]).all())
            tied = (a64["state"][1] == 1) & (a64["argmax"][1] == m - 1 - hi)     # reversed rows: 212 before 509
            assert int(tied.sum()) > 0 and bool((a64["iou"][1][m - 1 - hi][tied] == a64["iou"][1][m - 1 - lo][tied]).all())
    if name in LOSS_BLOCKS:
        assert blocks == LOSS_BLOCKS[name]
    if name == "block_cap":
        # 1024 workgroups of 256 threads: the class loop wraps a fifth time, for rows that include a positive
        assert a * classes > 4 * 1024 * 256
        assert int(torch.nonzero(a64["state"][0] == 1).max()) * classes >= 4 * 1024 * 256


def test_loss_blocks_ends():
    assert [rc.loss_blocks(a, 10) for a in (1, 100, 102, 103, 104857, 104858, 104870, 10 ** 7)] == [1, 1, 1, 2, 1024, 1024, 1024, 1024]
    assert [rc.loss_blocks(a, 12) for a in (1, 341, 342, 756)] == [1, 1, 2, 3]   # C % 4 == 0 counts vectors of four
    assert rc.loss_blocks(0, 10) == 0


def test_gpu_case_tables_name_their_routes():
    """The size pairs, class counts, thresholds and convolution shapes of tests/test_retina_gpu.py, read without a GPU."""
    import test_retina_gpu as T
    pairs = T.BILINEAR_CASES
    assert len(set(pairs)) == len(pairs)
    assert any(s == (1, 1) and d != (1, 1) for s, d in pairs)                               # one source pixel feeds everything
    assert any(d[0] > 4 * s[0] for s, d in pairs)                                           # ratio above 4
    assert any(d[0] * 2 == s[0] and d[1] * 3 == s[1] for s, d in pairs)                     # shrinking, integer ratios
    assert any(d[0] < s[0] and s[0] % d[0] and d[1] < s[1] and s[1] % d[1] for s, d in pairs)   # shrinking, non-integer
    assert any(s == d and s != (1, 1) for s, d in pairs)                                    # same size
    cases = [p.values for p in T.DECODE_CASES]
    assert {c for _a, _m, c, _t in cases} == {1, 4, 10, 80} and {t for _a, _m, _c, t in cases} == {None, 0.05, 0.5}
    assert all((a, "mixed", c, None) in cases for c in (1, 4, 80) for a in (65, 1025))
    assert {m for _a, m, _c, _t in cases} == {"none", "all", "mixed", "batch3", "special"}
    rows = sorted(r for at in T.SPECIAL_ROWS.values() for r in at)
    assert len(set(rows)) == 8 and rows[0] < 64 <= rows[1] and any(r >= 256 for r in rows) and rows[-1] == 299
    strided = [v for v in T.CONV_SHAPES.values() if v[7] == 2 and v[5] == 1]
    assert any(v[2] % 2 and v[3] % 2 for v in strided) and any(v[4] == 2048 for v in strided)
    assert any(v[1] == 2048 and v[5] == 1 for v in T.CONV_SHAPES.values())


def test_identity_block_backbone_shares_its_keys_with_the_restatement():
    """ResNet(Bottleneck, [2, 1, 1, 2]) of tests/test_retina_model_gpu.py: the second blocks of stages 1 and 4 carry no
    projection (256 and 2048 channels), and the restatement loads its state strictly."""
    from rrnet_amd.backbones.resnet import Bottleneck, ResNet
    net = ResNet(Bottleneck, list(rc.IDENTITY_DEPTHS))
    assert [len(getattr(net, "layer%d" % i)) for i in (1, 2, 3, 4)] == list(rc.IDENTITY_DEPTHS)
    for stage, channels in ((net.layer1, 256), (net.layer4, 2048)):
        assert stage[0].downsample is not None and stage[1].downsample is None
        assert stage[1].conv1.in_channels == channels == stage[1].conv3.out_channels
    plain = rc._Backbone(rc.IDENTITY_DEPTHS)
    assert rc.state_keys(plain) == rc.state_keys(net)
    plain.load_state_dict(net.state_dict(), strict=True)


def test_focal_loss_equals_the_reference(golden):
    from rrnet_amd.modules.loss.focalloss import FocalLoss
    from rrnet_amd.modules.loss.functional import focal_loss
    x, t, ref = torch.from_numpy(golden["focal_x"]), torch.from_numpy(golden["focal_t"]), float(golden["focal_loss"])
    tol = (x.numel() + 16) * rc.U32 * abs(ref)
    assert abs(float(focal_loss(x, t)) - ref) <= tol
    assert abs(float(FocalLoss()(x, t)) - ref) <= tol
    # the restated terms in float32, the reference's format: in float64 the upper clamp 1 - 1e-7 is not the float32 one
    # (1 - 2^-23), which moves a saturated non-target term, -log(1 - p) / 4, by 0.044
    assert abs(float(rc.focal_terms(x, t == 1).sum()) - ref) <= tol


@pytest.mark.parametrize("backbone", ["resnet10", "resnet50"])
def test_state_dict_keys_equal_the_reference(golden, backbone):
    from rrnet_amd.models.retinanet import RetinaNet
    want = json.loads(str(golden["state_keys_" + backbone]))
    model = RetinaNet(rc.retina_cfg(backbone))
    assert rc.state_keys(model) == want
    assert rc.state_keys(rc.PlainRetinaNet(backbone)) == want


def test_backbone_names_and_missing_weights():
    from rrnet_amd.backbones.resnet import ResNet
    from rrnet_amd.utils.model_tools import get_backbone
    with pytest.raises(NotImplementedError):
        get_backbone('resnet18')
    with pytest.raises(NotImplementedError):
        get_backbone('dla34')
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        net = get_backbone('resnet10', pretrained=True)
    assert isinstance(net, ResNet)
    assert any(issubclass(w.category, RuntimeWarning) and "not found" in str(w.message) for w in seen)
    # the reference's initialisation: BatchNorm 1 / 0, convolutions normal(0, sqrt(2 / (k*k*out)))
    assert float(net.bn1.weight.detach().min()) == 1.0 and float(net.bn1.bias.detach().abs().max()) == 0.0
    w = net.layer4[0].conv2.weight
    assert abs(float(w.detach().std()) - (2.0 / (9 * 512)) ** 0.5) < 0.02 * (2.0 / (9 * 512)) ** 0.5


def test_reference_retinanet_scripts_resolve_through_shims(tmp_path):
    """The import blocks of scripts/RetinaNet/train.py and eval.py, in a fresh interpreter outside the repository with
    PYTHONPATH=<repo>/shims, and the wrapper call train.py makes."""
    code = (
        "from operators.distributed_wrapper import DistributedWrapper\n"
        "from utils.metrics.metrics import evaluate_results\n"
        "from configs.retinanet_config import Config\n"
        "from operators.retinanet_operator import RetinaNetOperator\n"
        "import models.retinanet, rrnet_amd.models.retinanet, modules.fpn, modules.anchor, detectors.retinanet_detector\n"
        "from modules.loss.focalloss import FocalLoss\n"
        "from backbones.resnet import resnet10, resnet50, resnet101\n"
        "assert models.retinanet is rrnet_amd.models.retinanet\n"
        "assert Config.Model.backbone == 'resnet50' and Config.Model.num_anchors == 9 and Config.Train.lr == 1e-5\n"
        "assert Config.Train.lr_milestones == [60000, 80000] and Config.Train.iter_num == 90000 and Config.Train.batch_size == 2\n"
        "for m in ('make_anchor', 'criterion', 'train_step', 'training_process', 'transform_bbox', 'save_result',\n"
        "          'evaluate_images', 'evaluation_process'):\n"
        "    assert hasattr(RetinaNetOperator, m), m\n"
        "DistributedWrapper(Config, RetinaNetOperator)\n"
        "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "shims"))
    out = subprocess.check_output([sys.executable, "-c", code], text=True, cwd=str(tmp_path), env=env, timeout=300)
    assert out.strip().endswith("ok")


def test_train_tool_accepts_the_config():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train as train_tool
    finally:
        sys.path.pop(0)
    args = train_tool.parse(["--config", "retinanet_config", "--backbone", "resnet10", "--iters", "3", "--crop", "128", "128"])
    cfg = train_tool.configure(args)
    from rrnet_amd.datasets.transforms import RandomCrop
    assert cfg.Model.backbone == "resnet10" and cfg.Train.iter_num == 3 and tuple(cfg.Train.crop_size) == (128, 128)
    assert [(t.h, t.w) for t in cfg.Train.transforms.transforms if isinstance(t, RandomCrop)] == [(128, 128)]
    assert cfg.Distributed.world_size == 1
    with pytest.raises(SystemExit):
        train_tool.configure(train_tool.parse(["--config", "retinanet_config", "--bf16"]))
    from rrnet_amd.configs.retinanet_config import Config
    assert Config.Model.backbone == "resnet50" and tuple(Config.Train.crop_size) == (512, 512)     # the module's table is untouched


def test_data_parallel_is_refused():
    from rrnet_amd.operators.retinanet_operator import RetinaNetOperator
    cfg = rc.retina_cfg()
    cfg.Distributed.world_size = 2
    with pytest.raises(NotImplementedError, match="world_size"):
        RetinaNetOperator(cfg)

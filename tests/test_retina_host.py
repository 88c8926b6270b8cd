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

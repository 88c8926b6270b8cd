"""Host-side tests of the dense and the SE hourglass (no GPU): the plain-torch restatements of tests/hgvariant_cases.py
reproduce every record the reference's own classes left in tests/golden/hgvariants.npz; the package's module trees have the
reference's keys and shapes and the restatement's seeded default initialisation; the names reach get_backbone, the shims
and the tools; cfg.Model.bf16 is refused; and for every kernel-level case of tests/test_hgvariants_gpu.py float32 decides
each ReLU mask bit and each pool tap as float64 does."""
import json
import os
import subprocess
import sys
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import hgvariant_cases as hc
from helpers import det_fill, shapes_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("dense_hourglass", "dense_hourglass_tiny", "se_hourglass", "se_hourglass_tiny")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "hgvariants.npz"))


def _load_det(mod, seed):
    mod.load_state_dict(det_fill(shapes_of(mod.state_dict()), seed), strict=True)
    return mod.double()


def _same(golden, record):
    """Every array of `record` is in the golden and equals it to float64 rounding (1e-9 of the record's scale: the tiny
    networks' BatchNorm over a few hundred samples amplifies a 1e-16 re-association by up to 1e5)."""
    assert record
    for k, v in record.items():
        g = golden[k]
        assert g.shape == v.shape and g.dtype == np.float64, k
        scale = max(float(np.abs(g).max(initial=0.0)), 1e-30)
        assert float(np.abs(g - v).max(initial=0.0)) <= 1e-9 * scale, (k, float(np.abs(g - v).max()), scale)
    return set(record)


def test_restatements_reproduce_every_golden_record(golden):
    seen = set()
    for tag, ((cin, cout, stride), shape) in hc.BLOCK_CASES.items():
        seen |= _same(golden, hc.block_record(tag, _load_det(hc.Block(cin, cout, stride, se=True), 40), hc.det_input(shape, 41)))
    seen |= _same(golden, hc.block_record("selayer", _load_det(hc.SELayer(32, 16), 42), hc.det_input((2, 32, 4, 5), 43)))

    class Pool(nn.Module):                       # the restated pool, differentiable through its taps
        def forward(self, x):
            y, tap = hc.pool_reference(x.detach())
            taps = torch.stack([x[:, :, ky:2 * y.shape[2]:2, kx:2 * y.shape[3]:2] for ky in (0, 1) for kx in (0, 1)], -1)
            return torch.gather(taps, -1, tap.long().unsqueeze(-1)).squeeze(-1)

    for h, w in ((5, 7), (8, 8)):
        seen |= _same(golden, hc.block_record("pool_%dx%d" % (h, w), Pool(), hc.pool_case(h, w, 4, nan=False).double()))
    for tag, (variant, stacks, batch) in hc.NET_CASES.items():
        seen |= _same(golden, hc.net_record(tag, _settled_net(golden, tag), hc.det_input((batch, 3) + hc.NET_HW, 61)))
        seen |= {tag + "/nudge_keys", tag + "/nudge_ch", tag + "/nudge_val"}
    assert seen == set(golden.files)


def _settled_net(golden, tag, dtype=torch.float64):
    """The restated tiny network of a case with det_fill's weights, the golden's settled BatchNorm biases and momentum 1."""
    variant, stacks, _ = hc.NET_CASES[tag]
    net = hc.tiny_net(variant, stacks)
    state = hc.apply_nudges(det_fill(shapes_of(net.state_dict()), 60), golden[tag + "/nudge_keys"], golden[tag + "/nudge_ch"],
                            golden[tag + "/nudge_val"])
    net.load_state_dict(state, strict=True)
    return hc.full_momentum(net.to(dtype))


@pytest.mark.parametrize("tag", sorted(hc.NET_CASES))
def test_float32_decides_every_relu_of_the_tiny_networks_as_float64(golden, tag):
    """With the settled biases no ReLU input of the train-mode pass lies within RELU_MARGIN of 0 in float64, the float32
    restatement's inputs are within a tenth of that margin of float64's, so every decision is the same — the networks'
    float64 gradients are ones a float32 evaluation can be held to.  The settled values are float32 numbers, and settling
    again moves nothing."""
    _, _, batch = hc.NET_CASES[tag]
    x = hc.det_input((batch, 3) + hc.NET_HW, 61)
    pre = {}
    for dtype in (torch.float64, torch.float32):
        net = _settled_net(golden, tag, dtype).train()
        with torch.no_grad(), hc.ReluSites() as sites:
            net(x.to(dtype))
        pre[dtype] = [p.double() for p in sites.pre]
    assert len(pre[torch.float64]) == len(pre[torch.float32]) > 20
    nearest = min(float(a.abs().min()) for a in pre[torch.float64])
    err32 = max(float((a - b).abs().max()) for a, b in zip(pre[torch.float64], pre[torch.float32]))
    print("%s: %d ReLU sites, %d inputs, nearest to 0 %.3g, float32 restatement off by at most %.3g"
          % (tag, len(sites.pre), sum(a.numel() for a in sites.pre), nearest, err32))
    assert nearest >= hc.RELU_MARGIN and err32 <= 0.1 * hc.RELU_MARGIN
    assert all(torch.equal(a > 0, b > 0) for a, b in zip(pre[torch.float64], pre[torch.float32]))
    vals = golden[tag + "/nudge_val"]
    assert len(vals) > 0 and np.array_equal(vals.astype(np.float32).astype(np.float64), vals)
    assert hc.settle_relus(_settled_net(golden, tag), x) == []


def test_restated_pool_backward_is_the_gather_of_its_taps():
    x = hc.pool_case(5, 7, 4, nan=False).double().requires_grad_()
    y = torch.nn.functional.max_pool2d(x, 2)
    dy = hc.det_input(tuple(y.shape), 3)
    y.backward(dy)
    y2, tap = hc.pool_reference(x.detach())
    assert torch.equal(y2, y.detach()) and torch.equal(hc.pool_backward_reference(dy, tap, 5, 7), x.grad)


def test_full_size_keys_and_shapes_equal_the_reference(golden_dir):
    from rrnet_amd.backbones import dense_hourglass, hourglass, se_hourglass
    keys = json.load(open(os.path.join(golden_dir, "hgvariants_keys.json")))
    with torch.device("meta"):
        dense, se, plain = dense_hourglass.HourglassNet(2), se_hourglass.HourglassNet(2), hourglass.HourglassNet(2)
        assert hc.key_shapes(hc.Net("dense", 2)) == keys["dense_hourglass"] and hc.key_shapes(hc.Net("se", 2)) == keys["se_hourglass"]
    assert hc.key_shapes(dense) == keys["dense_hourglass"]
    assert hc.key_shapes(se) == keys["se_hourglass"]
    assert hc.key_shapes(dense) == hc.key_shapes(plain)
    assert sum(k.endswith(".se.fc.0.weight") for k, _ in keys["se_hourglass"]) == 70      # per stack 5 levels x 6 blocks + 4 innermost; + residual[0] + the stem's


@pytest.mark.parametrize("name,variant", [("dense_hourglass_tiny", "dense"), ("se_hourglass_tiny", "se")])
def test_default_initialisation_under_a_seed_equals_the_restatement(name, variant):
    from rrnet_amd.utils.model_tools import get_backbone
    torch.manual_seed(7)
    ours = get_backbone(name, num_stacks=3)
    torch.manual_seed(7)
    ref = hc.tiny_net(variant, 3)
    a, b = ours.state_dict(), ref.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_get_backbone_knows_the_names_and_the_shims_resolve(tmp_path):
    from rrnet_amd.backbones import dense_hourglass, se_hourglass
    from rrnet_amd.utils.model_tools import get_backbone
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.device("meta"):
            assert type(get_backbone("dense_hourglass", num_stacks=1)) is dense_hourglass.HourglassNet
            assert type(get_backbone("se_hourglass", num_stacks=1)) is se_hourglass.HourglassNet
    assert sum("hourglass.pth" in str(w.message) for w in caught) == 2          # the missing weights file warns, as hourglass_net
    assert type(get_backbone("dense_hourglass_tiny", num_stacks=3)) is dense_hourglass.HourglassNet
    tiny = get_backbone("se_hourglass_tiny")
    assert type(tiny) is se_hourglass.HourglassNet and tiny.hgs[0].up1[0].se.fc[0].weight.shape == (2, 32)
    assert tiny.hgs[0].low2.low2[1].se.fc[2].weight.shape == (48, 3)
    with pytest.raises(NotImplementedError, match="dense_hourglass.*se_hourglass"):
        get_backbone("hrnet")
    with pytest.raises(ValueError, match="num_feats"):
        dense_hourglass.HourglassNet(num_stacks=1, **hc.HG_TINY)              # 32 channels cannot be added to 256
    code = ("from backbones.dense_hourglass import dense_hourglass_net\n"
            "from backbones.se_hourglass import se_hourglass_net, SELayer\n"
            "import rrnet_amd.backbones.dense_hourglass as d, rrnet_amd.backbones.se_hourglass as s\n"
            "assert dense_hourglass_net is d.dense_hourglass_net and se_hourglass_net is s.se_hourglass_net\n"
            "from utils.model_tools import get_backbone\n"
            "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "shims"))
    out = subprocess.check_output([sys.executable, "-c", code], text=True, cwd=str(tmp_path), env=env, timeout=300)
    assert out.strip().endswith("ok")


@pytest.mark.parametrize("name", NEW_NAMES)
def test_bf16_is_refused_with_the_new_backbones(name):
    from rrnet_amd.models.centernet import CenterNet
    from rrnet_amd.models.rrnet import RRNet
    model = dict(num_stacks=1, backbone=name, nms_type_for_stage1="nms", nms_per_class_for_stage1=True)
    for extra in (dict(bf16=True), dict(conv_math="bf16")):
        cfg = SimpleNamespace(num_classes=10, Model=SimpleNamespace(**model, **extra))
        for cls in (RRNet, CenterNet):
            with pytest.raises(NotImplementedError, match="bf16"):
                cls(cfg)
    if name.endswith("_tiny"):                                                 # fp32 and the split-operand mode build
        for extra in ({}, dict(conv_math="f16x3")):
            RRNet(SimpleNamespace(num_classes=10, Model=SimpleNamespace(**model, **extra)))


def test_tools_take_the_names():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train as train_tool
    finally:
        sys.path.pop(0)
    for name in NEW_NAMES:
        for config in ("rrnet_config", "centernet_config"):
            assert train_tool.configure(train_tool.parse(["--config", config, "--backbone", name])).Model.backbone == name


def test_se_node_refuses_a_reduction_wider_than_the_channels():
    from rrnet_amd import functional as RF
    u = torch.zeros(1, 4, 2, 2)
    with pytest.raises(ValueError, match="reduction 16"):
        RF.se_scale_res_relu(u, torch.zeros(0, 4), torch.zeros(4, 0), u, 16)


@pytest.mark.parametrize("name", sorted(hc.SE_CASES))
def test_float32_decides_every_relu_mask_bit_as_float64(name):
    case = hc.se_case(name)
    r64, r32 = hc.se_reference(case, torch.float64), hc.se_reference(case, torch.float32)
    assert float(np.abs(r64["pre"]).min()) >= hc.MASK_MARGIN
    assert np.array_equal(r64["mask"], r32["mask"]) and np.array_equal(r64["hmask"], r32["hmask"])
    kind = hc.SE_CASES[name][4]
    if kind == "empty":
        assert not r64["mask"][1].any() and r64["mask"][0].any() and r64["mask"][2].any()
        assert not r64["dskip"][1].any() and not r64["du"][1].any() and not r64["dm"][1].any()   # nothing flows into that sample
    else:
        assert r64["mask"].any() and not r64["mask"].all()
    n, (h, w), c, r, _ = hc.SE_CASES[name]
    assert r64["h"].shape == (n, c // r) and r64["dw1"].shape == (c // r, c) and r64["dw2"].shape == (c, c // r)


def test_se_case_table_covers_what_the_kernels_branch_on():
    from rrnet_amd import ops
    hws = sorted({h * w for (_, (h, w), _, _, _) in hc.SE_CASES.values()})
    assert hws == [1, 63, 64, 65, 300]
    assert ops.se_chunk_rows(300) == (128, 3) and 300 % 128 not in (0,) and ops.se_chunk_rows(64) == (128, 1)
    assert ops.se_chunk_rows(512 * 512) == (1024, 256) and ops.se_chunk_rows(256 * 256) == (256, 256)
    assert sorted({c // r for (_, _, c, r, _) in hc.SE_CASES.values()}) == [1, 2, 3, 8, 16, 32]
    assert {n for (n, _, _, _, _) in hc.SE_CASES.values()} == {1, 3}


@pytest.mark.parametrize("h,w", hc.POOL_SIZES[1:])
@pytest.mark.parametrize("c", hc.POOL_CHANNELS)
def test_float32_decides_every_pool_tap_as_float64(h, w, c):
    x = hc.pool_case(h, w, c)
    y32, t32 = hc.pool_reference(x)
    y64, t64 = hc.pool_reference(x.double())
    assert torch.equal(t32, t64) and torch.equal(y32.double().nan_to_num(7.0), y64.nan_to_num(7.0))
    assert int(t32[0, 0, 0, 0]) == 0 and int(t32[1, 0, -1, -1]) == 2           # the planted ties: the first tap of the maximum
    assert bool(torch.isnan(y32[1, c - 1, 0, 0])) and int(t32[1, c - 1, 0, 0]) == 2          # the NaN at row 1, column 0 wins
    assert h * w < 16 or sorted(torch.unique(t32).tolist()) == [0, 1, 2, 3]


# ----------------------------------------------------------------------------------------------------------------------
# the family's header, include/rrnet_hip_se.h: what tests/test_abi.py and tests/test_call_host.py ask of include/rrnet_hip.h
# ----------------------------------------------------------------------------------------------------------------------
SE_ENTRIES = {"rr_se_squeeze", "rr_se_excite_fwd", "rr_se_scale_res_relu_fwd", "rr_se_bwd_reduce", "rr_se_excite_bwd",
              "rr_se_bwd_apply", "rr_maxpool2x2_fwd", "rr_maxpool2x2_bwd"}


def test_companion_header_declares_the_eight_entries_and_the_library_exports_them():
    import re
    from rrnet_amd import _C
    from rrnet_amd.csrc import build
    sigs = _C.family_signatures("rrnet_hip_se.h")
    assert set(sigs) == SE_ENTRIES and not (set(sigs) & set(_C.header_signatures()))      # no name is declared twice
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build(verbose=False)], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not (SE_ENTRIES - exported)
    for name, sig in sigs.items():
        assert sig[0] is _C.c_int and sig.pointees[-1] == "hipStream_t" and "hipStream_t" not in sig.pointees[:-1], name
        for argtype, pointee in zip(sig[1], sig.pointees):
            if pointee is None:
                assert argtype is not _C.c_void_p, name
            else:
                assert argtype is _C.c_void_p and (pointee == "hipStream_t" or _C.POINTEE_DTYPES[pointee]), (name, pointee)
        assert _C.declared(name) == (sig, "rrnet_hip_se.h")
    assert sigs["rr_se_squeeze"].pointees[:2] == ("float", "double") and sigs["rr_maxpool2x2_fwd"].pointees[2] == "unsigned char"
    # the bindings reach the family through its Family object only, and only with names its header declares
    text = open(os.path.join(ROOT, "rrnet_amd", "ops.py")).read()
    used = set(re.findall(r'_SE\.call\("(\w+)"', text))
    assert used == SE_ENTRIES
    for dp, _, files in os.walk(os.path.join(ROOT, "rrnet_amd")):
        for f in files:
            if f.endswith(".py"):
                assert not re.findall(r'_C\.(?:fn|call)\("(rr_se_\w+|rr_maxpool2x2_\w+)"', open(os.path.join(dp, f)).read()), f


def test_family_call_is_the_typed_helper():
    from rrnet_amd import _C
    se = _C.Family("rrnet_hip_se.h")
    with pytest.raises(_C.RRNetHipError, match="not declared in include/rrnet_hip_se.h"):
        se.call("rr_relu_fwd", None, None, 0)                                  # a name of the main header
    with pytest.raises(_C.RRNetHipError, match="not a header"):
        _C.Family("other.h").signatures()
    with pytest.raises(_C.RRNetHipError, match="takes 6 arguments and the stream"):
        se.call("rr_se_squeeze", None, None, 1, 1, 4)
    with pytest.raises(_C.RRNetHipError, match="no CPU fallback"):
        se.call("rr_se_squeeze", torch.zeros(4), None, 1, 1, 4, 1)             # a host tensor for a device pointer
    with pytest.raises(_C.RRNetHipError, match="declares a number"):
        se.call("rr_se_squeeze", None, None, torch.zeros(1), 1, 4, 1)

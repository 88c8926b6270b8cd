"""Host-side tests of ShuffleNetV2 (no GPU): the float64 oracle of tests/shufflenet_cases.py reproduces what the reference's
own InvertedResidual units left in tests/golden/shufflenet.npz (measured: outputs and data gradient within 2.7e-15, parameter
gradients within 5.0e-14, BatchNorm buffers within 1.2e-16; the bound is 1e-12); the package's classes have the reference's keys,
shapes and seeded initialisation; include/rrnet_hip_dw.h is a companion header as include/rrnet_hip_se.h is; get_backbone knows
the three built widths and refuses width 1.0; FPN takes the backbone's widths; the tools take the names; the shims resolve."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import shufflenet_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DW_ENTRIES = {"rr_dwconv3x3_fwd", "rr_dwconv3x3_bwd_data", "rr_dwconv3x3_bwd_weight", "rr_shuffle_interleave",
              "rr_shuffle_deinterleave", "rr_channel_copy", "rr_channel_join"}


@pytest.fixture(scope="module")
def golden():
    return sc.load_golden()


# ---- the oracle against the reference's record --------------------------------------------------------------------------
def test_oracle_reproduces_the_golden_units(golden):
    state = sc.golden_state(golden)
    x, gy = sc.nhwc(golden["x"].astype(np.float64)), sc.nhwc(golden["gy"].astype(np.float64))
    r = sc.chain(x, state, gy, train=True)
    assert float(np.abs(sc.nchw(r["y"]) - golden["y"]).max()) <= 1e-12
    assert float(np.abs(sc.nchw(r["dx"]) - golden["dx"]).max()) <= 1e-12
    names = [k[5:] for k in golden if k.startswith("grad/")]
    assert sorted(names) == sorted(r["grads"]) and len(names) == 24
    for k in names:
        assert r["grads"][k].shape == golden["grad/" + k].shape and float(np.abs(r["grads"][k] - golden["grad/" + k]).max()) <= 1e-12, k
    bufs = [k[4:] for k in golden if k.startswith("buf/")]
    assert sorted(bufs) == sorted(r["bufs"])
    for k in bufs:
        assert float(np.abs(r["bufs"][k] - golden["buf/" + k]).max()) <= 1e-12, k
    after = dict(state)
    after.update(r["bufs"])
    e = sc.chain(x, after, train=False)
    assert float(np.abs(sc.nchw(e["y"]) - golden["y_eval"]).max()) <= 1e-12
    assert float(golden["margin"]) > sc.RELU_MARGIN and r["margin"] > sc.RELU_MARGIN
    # the float32 run of the reference is a usable yardstick: it differs from the float64 run, by float32's worth
    for k in ("y", "dx", "y_eval"):
        d = float(np.abs(golden["f32/" + k] - golden[k]).max())
        assert 0.0 < d < 1e-4, k


@pytest.mark.parametrize("case", sc.DW_CASES[:6], ids=str)
def test_the_three_depthwise_rules_agree_with_each_other(case):
    """<dw_fwd(x, f), dy> = <x, dw_bwd_data(dy, f)> = <f, dw_bwd_weight(x, dy)>: one bilinear form, three oracles; the
    chained-float32 yardstick stays within float32's distance of them; the interleave's inverse is exact."""
    n, h, w, c, s = case
    x, f, bias, dy, df0 = sc.dw_inputs(case)
    y = sc.dw_fwd(x, f, s)
    assert y.shape == dy.shape == (n,) + sc.out_hw(h, w, s) + (c,)
    form = float((y * dy).sum())
    scale = float(np.abs(y * dy).sum()) + 1e-300
    assert abs(form - float((x * sc.dw_bwd_data(dy, f, s, h, w)).sum())) <= 1e-12 * scale
    assert abs(form - float((f * sc.dw_bwd_weight(x, dy, s)).sum())) <= 1e-12 * scale
    assert np.array_equal(sc.dw_fwd(x, f, s, bias), y + bias)
    assert float(np.abs(sc.dw_bwd_weight(x, dy, s, df0) - (sc.dw_bwd_weight(x, dy, s) + df0)).max()) <= 1e-12 * (1 + np.abs(df0).max())
    for seq, ref in ((sc.dw_fwd(x, f, s, bias, dtype=np.float32), y + bias),
                     (sc.dw_bwd_data(dy, f, s, h, w, dtype=np.float32), sc.dw_bwd_data(dy, f, s, h, w)),
                     (sc.dw_bwd_weight(x, dy, s, df0, dtype=np.float32), sc.dw_bwd_weight(x, dy, s, df0))):
        assert seq.dtype == np.float32 and float(np.abs(seq - ref).max()) <= 1e-5 * (1.0 + float(np.abs(ref).max()))
    a, b = x[..., :c // 2], x[..., c // 2:]
    out = sc.interleave(a, b)
    assert np.array_equal(out[..., 0], a[..., 0]) and np.array_equal(out[..., 1], b[..., 0]) and np.array_equal(out[..., 2], a[..., 1])
    back = sc.deinterleave(out)
    assert np.array_equal(back[0], a) and np.array_equal(back[1], b)
    # torch's channel_shuffle(cat(a, b), 2) in the reference's words: view(groups, c/2), transpose, flatten
    t = torch.from_numpy(np.concatenate([a, b], -1))
    want = t.view(t.shape[:-1] + (2, c // 2)).transpose(-1, -2).reshape(t.shape)
    assert np.array_equal(out, want.numpy())


def test_yardstick_is_a_chained_float32_sum():
    from helpers import _seq32
    x, f, _, dy, _ = sc.dw_inputs((2, 7, 9, 8, 1))
    seq = sc.dw_bwd_weight(x, dy, 1, dtype=np.float32)
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    terms = (xp[:, 2:9, 1:10, 3] * dy[..., 3]).reshape(1, -1)                  # channel 3, tap (2, 1)
    assert float(seq[3, 2, 1]) == float(_seq32(terms)[1][0])
    y32 = sc.dw_fwd(x, f, 1, dtype=np.float32)
    taps = np.array([[f[5, a, b] * xp[1, 3 + a, 4 + b, 5] for a in range(3) for b in range(3)]])
    assert float(y32[1, 3, 4, 5]) == float(_seq32(taps)[1][0])


# ---- the classes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", sc.WIDTHS)
def test_class_has_the_reference_keys_and_shapes(width):
    from rrnet_amd.backbones.shufflenet import ShuffleNetV2
    want = sc.load_keys()[str(width)]
    net = ShuffleNetV2(width_mult=width)
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert got == want                                                         # names, shapes and order
    assert net.out_channels == (net.stage_out_channels[2], net.stage_out_channels[3], net.stage_out_channels[-1])
    assert [n for n, _ in net.named_children()] == ["conv1", "maxpool", "features", "conv_last"]
    assert [type(u).__name__ for u in net.features] == ["InvertedResidual"] * 16
    assert [(u.benchmodel, u.stride) for u in net.features][:5] == [(2, 2), (1, 1), (1, 1), (1, 1), (2, 2)]


def test_units_draw_the_reference_initial_weights_and_load_its_state(golden):
    from rrnet_amd.backbones.shufflenet import InvertedResidual
    torch.manual_seed(int(golden["seed"]))
    m = torch.nn.Sequential(*[InvertedResidual(*u) for u in sc.UNITS])
    state = m.state_dict()
    want = sc.golden_state(golden)
    assert list(state) == list(want)
    assert {k: tuple(v.shape) for k, v in state.items()} == {k: tuple(a.shape) for k, a in want.items()}
    inits = [k[5:] for k in golden if k.startswith("init/")]
    assert len(inits) == 8
    for k in inits:
        assert np.array_equal(state[k].numpy(), golden["init/" + k]), k
    assert [n for n, _ in m[0].named_children()] == ["banch1", "banch2"] and [n for n, _ in m[1].named_children()] == ["banch2"]
    m.load_state_dict({k: torch.as_tensor(a) for k, a in want.items()}, strict=True)
    with pytest.raises(ValueError, match="not supported"):
        from rrnet_amd.backbones.shufflenet import ShuffleNetV2
        ShuffleNetV2(width_mult=0.75)


def test_shufflenet_v2_loads_a_file_from_disk_and_warns_without_one(tmp_path):
    import warnings
    from rrnet_amd.backbones.shufflenet import shufflenet_v2
    torch.manual_seed(1)
    src = shufflenet_v2(width_mult=0.5)
    path = str(tmp_path / "w.pth")
    torch.save(src.state_dict(), path)
    torch.manual_seed(2)
    got = shufflenet_v2(pretrained=True, width_mult=0.5, weights_path=path)
    assert all(torch.equal(v, src.state_dict()[k]) for k, v in got.state_dict().items())
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        shufflenet_v2(pretrained=True, width_mult=0.5, weights_path=str(tmp_path / "absent.pth"))
    assert any(issubclass(w.category, RuntimeWarning) and "not found" in str(w.message) for w in seen)


# ---- the family's header --------------------------------------------------------------------------------------------
def test_companion_header_declares_the_entries_and_the_library_exports_them():
    from rrnet_amd import _C
    from rrnet_amd.csrc import build
    assert "rrnet_hip_dw.h" in _C.COMPANION_HEADERS
    sigs = _C.family_signatures("rrnet_hip_dw.h")
    assert set(sigs) == DW_ENTRIES
    others = set(_C.header_signatures())
    for h in _C.COMPANION_HEADERS:
        if h != "rrnet_hip_dw.h":
            others |= set(_C.family_signatures(h))
    assert not (set(sigs) & others)                                            # no name is declared twice
    assert "depthwise.hip" in build.sources() and build.PER_FILE["depthwise.hip"] == ["-ffp-contract=off"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build(verbose=False)], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not (DW_ENTRIES - exported)
    for name, sig in sigs.items():
        assert sig[0] is _C.c_int and sig.pointees[-1] == "hipStream_t" and "hipStream_t" not in sig.pointees[:-1], name
        for argtype, pointee in zip(sig[1], sig.pointees):
            if pointee is None:
                assert argtype is _C.c_int, name
            else:
                assert argtype is _C.c_void_p and pointee in ("hipStream_t", "float", "double"), (name, pointee)
        assert _C.declared(name) == (sig, "rrnet_hip_dw.h")
    assert sigs["rr_dwconv3x3_fwd"].pointees.count("float") == 4 and sigs["rr_dwconv3x3_fwd"].pointees.count("double") == 1
    assert sigs["rr_dwconv3x3_bwd_weight"].pointees.count("double") == 1 and sigs["rr_dwconv3x3_bwd_data"].pointees.count(None) == 5
    # the slab tile of the header is the one the binding sizes the slab with
    from rrnet_amd import ops
    header = open(os.path.join(ROOT, "include", "rrnet_hip_dw.h")).read()
    assert int(re.search(r"#define RR_DW_SLAB_PIXELS (\d+)", header).group(1)) == ops.DW_SLAB_PIXELS
    # the bindings reach the family through its Family object only, and only with names its header declares
    text = open(os.path.join(ROOT, "rrnet_amd", "ops.py")).read()
    assert '_DW = _C.Family("rrnet_hip_dw.h")' in text and "call=_DW.call" in text
    assert set(re.findall(r'_dw_launch\("(\w+)"', text)) == DW_ENTRIES
    for dp, _, files in os.walk(os.path.join(ROOT, "rrnet_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.findall(r'_C\.(?:fn|call)\("(rr_(?:dwconv|shuffle|channel)_\w+)"', src), f
                assert not re.findall(r'_launch\([^)]*"(rr_(?:dwconv|shuffle|channel)_\w+)"', src.replace("_dw_launch(", "")), f


def test_family_call_is_the_typed_helper_and_tiles_are_bounded():
    from rrnet_amd import _C, ops
    fam = _C.Family("rrnet_hip_dw.h")
    with pytest.raises(_C.RRNetHipError, match="not declared in include/rrnet_hip_dw.h"):
        fam.call("rr_se_squeeze", None, None, 1, 1, 4, 1)
    with pytest.raises(_C.RRNetHipError, match="takes 10 arguments and the stream"):
        fam.call("rr_dwconv3x3_fwd", None, None, None, None, None, 1, 1, 1, 4)
    with pytest.raises(_C.RRNetHipError, match="no CPU fallback"):
        fam.call("rr_dwconv3x3_fwd", torch.zeros(4), None, None, None, None, 1, 1, 1, 4, 1)
    with pytest.raises(_C.RRNetHipError, match="declares a number"):
        fam.call("rr_shuffle_interleave", None, torch.zeros(1), None, 4, None, 8, 1, 4)
    with pytest.raises(_C.RRNetHipError, match="no CPU fallback"):
        ops.shuffle_interleave(torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 2, 2))
    assert ops.dw_tile_pixels(1) == (128, 1) and ops.dw_tile_pixels(4290) == (128, 34)
    assert ops.dw_tile_pixels(8 * 128 * 128) == (512, 256) and ops.dw_out_hw(9, 11, 2) == (5, 6) and ops.dw_out_hw(8, 6, 2) == (4, 3)
    # a channel slice of an NHWC tensor is described in place; an NCHW-contiguous one is refused
    x = ops.empty_nhwc(2, 16, 3, 5, "cpu")
    assert ops.pixel_rows(x) == (30, 16, 16) and ops.pixel_rows(x[:, :8]) == (30, 8, 16) and ops.pixel_rows(x[:, 8:]) == (30, 8, 16)
    with pytest.raises(ValueError, match="channel slice"):
        ops.pixel_rows(torch.zeros(2, 16, 3, 5))


# ---- wiring ---------------------------------------------------------------------------------------------------------------
def test_get_backbone_names_and_the_width_1_refusal():
    from rrnet_amd.backbones.shufflenet import ShuffleNetV2
    from rrnet_amd.utils.model_tools import get_backbone
    for name, halves in (("shufflenet_v2_x0_5", (24, 48, 96)), ("shufflenet_v2_x1_5", (88, 176, 352)),
                         ("shufflenet_v2_x2_0", (112, 244, 488))):
        net = get_backbone(name)
        assert type(net) is ShuffleNetV2
        assert tuple(c // 2 for c in net.stage_out_channels[2:5]) == halves and all(h % 4 == 0 for h in halves)
    with pytest.raises(NotImplementedError, match=r"58 channels.*c % 4 == 0"):
        get_backbone("shufflenet_v2_x1_0")
    with pytest.raises(NotImplementedError, match="outside the accelerated path .*'resnet10' / 'resnet50' / 'resnet101'.*"
                                                  "'shufflenet_v2_x0_5' / 'shufflenet_v2_x1_5' / 'shufflenet_v2_x2_0'"):
        get_backbone("shufflenet")


def test_fpn_default_is_unchanged_and_takes_a_backbones_widths():
    from rrnet_amd.modules.fpn import FPN
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    old = shapes(FPN())
    assert old["lat_layer1.weight"] == (256, 2048, 1, 1) and old["lat_layer2.weight"] == (256, 1024, 1, 1)
    assert old["lat_layer3.weight"] == (256, 512, 1, 1) and old["top_layer1.weight"] == (256, 256, 3, 3) and len(old) == 10
    assert list(old) == ["lat_layer1.weight", "lat_layer1.bias", "lat_layer2.weight", "lat_layer2.bias", "lat_layer3.weight",
                         "lat_layer3.bias", "top_layer1.weight", "top_layer1.bias", "top_layer2.weight", "top_layer2.bias"]
    torch.manual_seed(4)
    a = FPN()
    torch.manual_seed(4)
    b = FPN(in_channels=(512, 1024, 2048))
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    new = shapes(FPN(in_channels=(48, 96, 1024)))
    assert new["lat_layer3.weight"] == (256, 48, 1, 1) and new["lat_layer2.weight"] == (256, 96, 1, 1)
    assert new["lat_layer1.weight"] == (256, 1024, 1, 1) and list(new) == list(old)


def test_retinanet_builds_its_fpn_from_the_backbone():
    import retina_cases as rc
    from rrnet_amd.models.retinanet import RetinaNet
    net = RetinaNet(rc.retina_cfg("shufflenet_v2_x0_5"))
    assert net.fpn.lat_layer3.in_channels == 48 and net.fpn.lat_layer2.in_channels == 96 and net.fpn.lat_layer1.in_channels == 1024
    assert RetinaNet(rc.retina_cfg("resnet10")).fpn.lat_layer1.in_channels == 2048
    dw = [n for n, p in net.named_parameters() if p.dim() == 4 and p.shape[1] == 1 and p.shape[2:] == (3, 3)]
    assert len(dw) == 19                                                       # 3 stride-2 units with two, 13 stride-1 units with one


def test_tools_take_the_backbone_names():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train as train_tool
    finally:
        sys.path.pop(0)
    for name in ("shufflenet_v2_x0_5", "shufflenet_v2_x1_5", "shufflenet_v2_x2_0"):
        cfg = train_tool.configure(train_tool.parse(["--config", "retinanet_config", "--backbone", name]))
        assert cfg.Model.backbone == name
    for bad in (["--config", "retinanet_config", "--backbone", "shufflenet_v2_x0_5", "--bf16"],
                ["--config", "rrnet_config", "--backbone", "shufflenet_v2_x0_5"]):
        with pytest.raises(SystemExit):
            train_tool.configure(train_tool.parse(bad))
    for tool in ("detect.py", "bench_detect.py", "train.py"):
        text = open(os.path.join(ROOT, "tools", tool)).read()
        assert '"--backbone"' in text and "shufflenet_v2_x0_5" in text, tool
    text = open(os.path.join(ROOT, "tools", "bench_shufflenet.py")).read()
    assert "profiles" in text and "shufflenet.json" in text and "bench_detect.py" in text


def test_shims_give_the_same_class_object(tmp_path):
    code = ("from backbones.shufflenet import ShuffleNetV2, InvertedResidual, shufflenet_v2\n"
            "from utils.model_tools import get_backbone\n"
            "import rrnet_amd.backbones.shufflenet as own\n"
            "assert ShuffleNetV2 is own.ShuffleNetV2 and InvertedResidual is own.InvertedResidual\n"
            "assert type(get_backbone('shufflenet_v2_x0_5')) is own.ShuffleNetV2\n"
            "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "shims"))
    out = subprocess.check_output([sys.executable, "-c", code], text=True, cwd=str(tmp_path), env=env, timeout=300)
    assert out.strip().endswith("ok")

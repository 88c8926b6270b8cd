"""Host-side tests of the dilated-window attention (no GPU): the float64 oracle of tests/attn_cases.py reproduces what the
reference's own SelfAttentionModule left in tests/golden/self_attention.npz; include/rrnet_hip_attn.h is a companion header
as include/rrnet_hip_se.h is; the package's module has the reference's keys, shapes and zero `W`; unsupported geometries,
scale, stride and bf16 are refused; cfg.Model.attention = None builds the models as before; the shims resolve the module."""
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTN_ENTRIES = {"rr_attn_fwd", "rr_attn_bwd_q", "rr_attn_bwd_kv"}


@pytest.fixture(scope="module")
def golden():
    return ac.load_golden()


# ---- the oracle against the reference's record --------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(ac.MODULE_CASES))
def test_oracle_reproduces_the_golden_context_and_gradients(golden, tag):
    c = ac.MODULE_CASES[tag]
    q, k, v, dctx = (ac.nhwc(golden["%s/%s" % (tag, n)]) for n in ("q", "k", "v", "dctx"))
    r = ac.window_rule(q, k, v, c["kernel"], c["dilation"], c["padding"], dctx)
    for name in ("ctx", "dq", "dk", "dv"):
        want = ac.nhwc(golden["%s/%s" % (tag, name)])
        assert r[name].shape == want.shape and float(np.abs(r[name] - want).max()) <= 1e-12, name
    assert float(np.abs(r["p"].sum(-1) - 1.0).max()) < 1e-14
    assert float(golden[tag + "/margin"]) > ac.RELU_MARGIN


def test_case_c_leaves_query_rows_unread_and_case_b_is_mostly_padding():
    c = ac.CASES["C"]
    oh, ow, cy, cx = ac.geometry(*c["hw"], c["kernel"], c["dilation"], c["padding"])
    assert (oh, ow, cy, cx) == (5, 10, 1, 0)
    q, k, v, dctx = ac.case_inputs("C")
    r = ac.window_rule(q, k, v, c["kernel"], c["dilation"], c["padding"], dctx)
    assert not r["dq"][:, 0].any() and r["dq"][:, 1:].all()
    b = ac.CASES["B"]
    h, w = b["hw"]
    ys = np.arange(h)[:, None] - 12 + 6 * np.arange(5)[None, :]
    xs = np.arange(w)[:, None] - 12 + 6 * np.arange(5)[None, :]
    inside = ((ys >= 0) & (ys < h)).sum(1)[:, None] * ((xs >= 0) & (xs < w)).sum(1)[None, :]
    assert inside.mean() < 25 / 2                                              # most of the 25 taps are padded
    q, k = ac.case_inputs("E")[:2]
    e = ac.CASES["E"]
    logit = ac.window_rule(q, k, np.zeros(q.shape[:3] + (4,)), e["kernel"], e["dilation"], e["padding"])
    assert logit["p"].max() <= 1.0
    kp = np.pad(k, ((0, 0), (2, 2), (2, 2), (0, 0)))
    big = max(float(np.abs((q * kp[:, a * 2:a * 2 + 7, b * 2:b * 2 + 9]).sum(-1)).max()) for a in range(3) for b in range(3))
    assert big > 100.0                                                         # exp() of it overflows float32 (88.7)


def test_yardstick_is_a_chained_float32_sum():
    """window_rule(dtype=float32) on one pixel and one tap-free dimension equals helpers._seq32's chain."""
    from helpers import _seq32
    rng = np.random.default_rng(5)
    q = rng.standard_normal((1, 1, 1, 8)).astype(np.float32).astype(np.float64)
    k = rng.standard_normal((1, 1, 1, 8)).astype(np.float32).astype(np.float64)
    v = rng.standard_normal((1, 1, 1, 4)).astype(np.float32).astype(np.float64)
    dctx = np.ones((1, 1, 1, 4))
    r = ac.window_rule(q, k, v, 1, 1, 0, dctx, dtype=np.float32)
    # one tap: P = 1, ctx = v, dP = dctx . v as a chained float32 sum
    _, seq = _seq32((dctx * v).reshape(1, -1))
    assert r["p"].dtype == np.float32 and float(r["p"][0, 0, 0, 0]) == 1.0 and np.array_equal(r["ctx"], v.astype(np.float32))
    dp = ac._dot(dctx.astype(np.float32), v.astype(np.float32), np.float32)
    assert float(dp[0, 0, 0]) == float(seq[0])


# ---- the family's header --------------------------------------------------------------------------------------------
def test_companion_header_declares_the_entries_and_the_library_exports_them():
    from rrnet_amd import _C
    from rrnet_amd.csrc import build
    assert "rrnet_hip_attn.h" in _C.COMPANION_HEADERS and "rrnet_hip_se.h" in _C.COMPANION_HEADERS
    sigs = _C.family_signatures("rrnet_hip_attn.h")
    assert set(sigs) == ATTN_ENTRIES
    others = set(_C.header_signatures()) | set(_C.family_signatures("rrnet_hip_se.h"))
    assert not (set(sigs) & others)                                            # no name is declared twice
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build(verbose=False)], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not (ATTN_ENTRIES - exported)
    for name, sig in sigs.items():
        assert sig[0] is _C.c_int and sig.pointees[-1] == "hipStream_t" and "hipStream_t" not in sig.pointees[:-1], name
        for argtype, pointee in zip(sig[1], sig.pointees):
            if pointee is None:
                assert argtype is _C.c_int, name
            else:
                assert argtype is _C.c_void_p and pointee in ("hipStream_t", "float"), (name, pointee)
        assert _C.declared(name) == (sig, "rrnet_hip_attn.h")
        assert sig.pointees.count(None) == 11 and sig.pointees.count("float") == (5 if name == "rr_attn_fwd" else 6)
    # the bindings reach the family through its Family object only, and only with names its header declares
    text = open(os.path.join(ROOT, "rrnet_amd", "ops.py")).read()
    assert '_ATTN = _C.Family("rrnet_hip_attn.h")' in text and "call=_ATTN.call" in text
    assert set(re.findall(r'_attn_launch\("(\w+)"', text)) == ATTN_ENTRIES
    for dp, _, files in os.walk(os.path.join(ROOT, "rrnet_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.findall(r'_C\.(?:fn|call)\("(rr_attn_\w+)"', src), f
                assert not re.findall(r'_launch\([^)]*"(rr_attn_\w+)"', src.replace("_attn_launch(", "")), f


def test_family_call_is_the_typed_helper():
    from rrnet_amd import _C
    fam = _C.Family("rrnet_hip_attn.h")
    with pytest.raises(_C.RRNetHipError, match="not declared in include/rrnet_hip_attn.h"):
        fam.call("rr_se_squeeze", None, None, 1, 1, 4, 1)                      # a name of another family
    with pytest.raises(_C.RRNetHipError, match="takes 16 arguments and the stream"):
        fam.call("rr_attn_fwd", None, None, None, None, None, 1, 1, 1, 4, 4)
    with pytest.raises(_C.RRNetHipError, match="no CPU fallback"):
        fam.call("rr_attn_fwd", torch.zeros(4), None, None, None, None, 1, 1, 1, 4, 4, 1, 1, 1, 1, 0, 0)
    with pytest.raises(_C.RRNetHipError, match="declares a number"):
        fam.call("rr_attn_fwd", None, None, None, None, None, torch.zeros(1), 1, 1, 4, 4, 1, 1, 1, 1, 0, 0)


# ---- the module ---------------------------------------------------------------------------------------------------------
def _module(case, **extra):
    from rrnet_amd.modules.self_attention import SelfAttentionModule
    return SelfAttentionModule(case["cin"], case["ck"], case["cv"], kernel_size=case["kernel"], dilation=case["dilation"],
                               padding=case["padding"], **extra)


@pytest.mark.parametrize("tag", sorted(ac.MODULE_CASES))
def test_module_has_the_golden_keys_and_shapes_and_a_zero_w(golden, tag):
    m = _module(ac.MODULE_CASES[tag])
    state = m.state_dict()
    want = ac.golden_state(golden, tag)
    assert set(state) == set(want)
    assert {k: tuple(v.shape) for k, v in state.items()} == {k: tuple(a.shape) for k, a in want.items()}
    assert not m.W.weight.any() and not m.W.bias.any()
    assert [n for n, _ in m.named_children()] == ["pool", "f_key", "f_query", "f_value", "W"]
    # the default initialisation under the golden's seed: the convolutions draw what the reference's drew
    torch.manual_seed(int(golden[tag + "/seed"]))
    seeded = _module(ac.MODULE_CASES[tag]).state_dict()
    for key in ("f_key.0.weight", "f_key.3.bias", "f_query.0.weight", "f_query.3.weight", "f_value.weight", "f_value.bias"):
        assert np.array_equal(seeded[key].double().numpy(), want[key]), key
    m.load_state_dict({k: torch.as_tensor(a) for k, a in want.items()}, strict=True)


def test_module_refuses_what_the_device_path_lacks():
    x = torch.zeros(1, 16, 6, 6)
    base = dict(cin=16, ck=8, cv=12, kernel=3, dilation=2, padding=2)
    for case, extra, what in ((base, dict(scale=2), "scale"), (base, dict(stride=2), "stride"),
                              (dict(base, padding=1), {}, "padding"), (dict(base, padding=0), {}, "padding"),
                              (dict(base, kernel=(2, 3), dilation=(1, 2), padding=(0, 2)), {}, "padding|even"),
                              (dict(base, ck=6), {}, "multiples of 4")):
        m = _module(case, **extra)                              # the constructor takes everything the reference's takes
        with pytest.raises(NotImplementedError, match=what):
            m(x)
    from rrnet_amd import _C
    with pytest.raises(_C.RRNetHipError, match="no CPU fallback"):             # a supported geometry, a host tensor
        _module(base)(x)


# ---- the model switch ---------------------------------------------------------------------------------------------------
def _cfg(**model):
    base = dict(num_stacks=2, backbone="hourglass_tiny", nms_type_for_stage1="nms", nms_per_class_for_stage1=True)
    base.update(model)
    return SimpleNamespace(num_classes=10, Model=SimpleNamespace(**base))


ATTENTION = dict(key_channels=8, value_channels=12, kernel_size=3, dilation=2, padding=2)


@pytest.mark.parametrize("which", ["rrnet", "centernet"])
def test_attention_none_builds_the_parent_model_and_a_dict_adds_only_attention(which):
    from rrnet_amd.models.centernet import CenterNet
    from rrnet_amd.models.rrnet import RRNet
    cls = RRNet if which == "rrnet" else CenterNet
    torch.manual_seed(3)
    absent = cls(_cfg())
    torch.manual_seed(3)
    none = cls(_cfg(attention=None))
    torch.manual_seed(3)
    with_attn = cls(_cfg(attention=dict(ATTENTION)))
    plain = absent.state_dict()
    assert none.attention is None and list(none.state_dict()) == list(plain)
    assert [n for n, _ in none.named_parameters()] == [n for n, _ in absent.named_parameters()]
    full = with_attn.state_dict()
    assert list(full)[:len(plain)] == list(plain) and all(k.startswith("attention.") for k in list(full)[len(plain):])
    for k, v in plain.items():                                   # constructed last: every other parameter draws the same values
        assert torch.equal(v, none.state_dict()[k]) and torch.equal(v, full[k]), k
    assert len(with_attn.attention) == 2 and with_attn.attention[0].in_channels == 256
    missing = with_attn.load_state_dict(plain, strict=False)
    assert missing.missing_keys and all(k.startswith("attention.") for k in missing.missing_keys) and not missing.unexpected_keys


def test_attention_is_refused_with_bf16_and_with_unsupported_geometry():
    from rrnet_amd.models.centernet import CenterNet
    from rrnet_amd.models.rrnet import RRNet
    for extra in (dict(bf16=True), dict(conv_math="bf16")):
        for cls in (RRNet, CenterNet):
            with pytest.raises(NotImplementedError, match="bf16"):
                cls(_cfg(num_stacks=1, attention=dict(ATTENTION), **extra))
    RRNet(_cfg(num_stacks=1, attention=dict(ATTENTION), conv_math="f16x3"))
    with pytest.raises(NotImplementedError, match="scale"):
        CenterNet(_cfg(num_stacks=1, attention=dict(ATTENTION, scale=2)))
    with pytest.raises(ValueError, match="out_channels"):
        CenterNet(_cfg(num_stacks=1, attention=dict(ATTENTION, out_channels=64)))


def test_tools_take_the_attention_flag():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train as train_tool
    finally:
        sys.path.pop(0)
    cfg = train_tool.configure(train_tool.parse(["--attention", "5", "6"]))
    assert cfg.Model.attention == dict(key_channels=64, value_channels=64, kernel_size=5, dilation=6, padding=12)
    assert getattr(train_tool.configure(train_tool.parse([])).Model, "attention", None) is None
    assert train_tool.configure(train_tool.parse(["--config", "centernet_config", "--attention", "3", "2"])).Model.attention["padding"] == 2
    for bad in (["--attention", "5", "6", "--bf16"], ["--config", "retinanet_config", "--attention", "5", "6"]):
        with pytest.raises(SystemExit):
            train_tool.configure(train_tool.parse(bad))
    text = open(os.path.join(ROOT, "tools", "detect.py")).read()
    assert '"--attention"' in text and "attention_kwargs(*args.attention)" in text


def test_shims_give_the_same_class_object(tmp_path):
    code = ("from modules.self_attention import SelfAttentionModule\n"
            "import rrnet_amd.modules.self_attention as own\n"
            "assert SelfAttentionModule is own.SelfAttentionModule\n"
            "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "shims"))
    out = subprocess.check_output([sys.executable, "-c", code], text=True, cwd=str(tmp_path), env=env, timeout=300)
    assert out.strip().endswith("ok")

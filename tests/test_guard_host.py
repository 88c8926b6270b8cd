"""Host side of the guarded optimiser step, no GPU: the numpy restatement of tests/guard_cases.py against
torch.optim.Adam + clip_grad_norm_ + a float64 EMA loop, WarmupMultiStepLR against sequences recorded from the
reference's class and against the closed formula, argument errors, tools/train.py's flags, the state file's keys and
load rules, and the header's declarations."""
import json
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import guard_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "warmup_lr.npz")


# ---- the restatement against torch ----------------------------------------------------------------------------------
def _torch_run(p0, grads, skip_steps, lr, max_norm, grad_scale, ema_decay):
    """torch.optim.Adam (float64, CPU) + clip_grad_norm_ + an EMA loop over the gradients whose index is not in
    skip_steps: the run that never saw the others."""
    p = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=lr)
    ema = p.detach().clone()
    applied, norms = 0, []
    for t, g in enumerate(grads):
        if t in skip_steps:
            continue
        p.grad = torch.tensor(g, dtype=torch.float64) * grad_scale
        norms.append(float(torch.nn.utils.clip_grad_norm_([p], max_norm)))
        opt.step()
        applied += 1
        d = min(ema_decay, (1.0 + applied) / (10.0 + applied))
        ema = ema * d + p.detach() * (1.0 - d)
    st = opt.state[p]
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), ema.numpy(), norms


def _restated_run(p0, grads, lr, max_norm, grad_scale, ema_decay, order=None):
    p = np.array(p0, dtype=np.float64)
    m, v, ema = np.zeros_like(p), np.zeros_like(p), p.copy()
    ctl = G.fresh_ctl()
    trace = []
    for g in grads:
        S, B = G.sum_squares(g) if order is None else G.device_order_sum(g, *order)
        ctl = G.decide(ctl, S, B, grad_scale, max_norm, True, lr, 0.9, 0.999, ema_decay, True)
        p, m, v, ema = G.adam_ema(p, m, v, ema, g, ctl)
        trace.append(ctl.copy())
    return p, m, v, ema, trace


@pytest.mark.parametrize("max_norm,binding", [(0.05, True), (1e4, False), (math.inf, False)])
def test_restatement_matches_torch_adam_clip_and_ema(max_norm, binding):
    """12 steps, n = 4 * 751, grad_scale 0.5, one gradient with a NaN in the middle: the restatement skips it and must
    equal the torch run that never saw it.  The restatement rounds scale, step_size, bc2_sqrt and the betas to float
    (as the kernel receives them): four factors of relative error 2^-24 per step on updates of at most a few lr, so
    12 * 4 * 2^-24 = 2.9e-6 relative bounds every buffer, with an absolute floor of that times 10 lr."""
    n, lr, steps = 4 * 751, 1e-3, 12
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [G.gradient(n, 100 + t, scale=0.1 * (1 + t % 3)) for t in range(steps)]
    grads[6][1234] = np.nan
    p, m, v, ema, trace = _restated_run(p0, grads, lr, max_norm, 0.5, 0.5)
    tp, tm, tv, tema, norms = _torch_run(p0, grads, {6}, lr, max_norm, 0.5, 0.5)
    rtol = steps * 4 * 2.0 ** -24
    for got, want in ((p, tp), (m, tm), (v, tv), (ema, tema)):
        np.testing.assert_allclose(got, want, rtol=rtol, atol=rtol * 10 * lr)
    last = trace[-1]
    assert last[G.IX["applied"]] == 11 and last[G.IX["skipped"]] == 1
    assert last[G.IX["clipped"]] == (11 if binding else 0)
    assert trace[6][G.IX["skip"]] == 1 and trace[6][G.IX["bad"]] == 1 and math.isinf(trace[6][G.IX["norm"]])
    # the skipped step advanced nothing that Adam reads
    for slot in ("applied", "beta1_pow", "beta2_pow", "scale", "step_size", "bc2_sqrt", "ema_d", "ema_omd"):
        assert trace[6][G.IX[slot]] == trace[5][G.IX[slot]], slot
    seen = [c[G.IX["norm"]] for i, c in enumerate(trace) if i != 6]
    np.testing.assert_allclose(seen, norms, rtol=1e-12)
    assert last[G.IX["norm_max"]] == max(seen)
    assert last[G.IX["beta1_pow"]] == pytest.approx(0.9 ** 11, rel=1e-14)
    # the warm-up ramp governs while (1 + t) / (10 + t) < 0.5, i.e. t < 8, then the decay does
    ds = [c[G.IX["ema_d"]] for i, c in enumerate(trace) if i != 6]
    assert ds[:7] == [float(np.float32((1.0 + t) / (10.0 + t))) for t in range(1, 8)] and ds[7:] == [0.5] * 4


def test_device_order_sum_is_the_float64_sum_up_to_rounding():
    """The summation order of the kernels, walked in numpy, against the plain float64 sum: equal to N * 2^-53 relative,
    the count exact; a grid of one partial block, of several blocks, and more blocks than decide lanes."""
    for n, blocks, threads in ((4, 1, 256), (1020, 1, 256), (4 * 256 * 5 + 148, 6, 256), (4 * 64 * 700, 300, 64)):
        g = G.gradient(n, n)
        g[::97] = np.inf
        g[-1] = -np.inf
        S, B = G.device_order_sum(g, blocks, threads)
        S0, B0 = G.sum_squares(g)
        assert B == B0 == len(range(0, n, 97)) + ((n - 1) % 97 != 0)
        assert abs(S - S0) <= n * 2.0 ** -53 * S0
    assert G.device_order_sum(np.zeros(0, np.float32), 0, 256) == (0.0, 0)


def test_decide_rules():
    c = G.decide(G.fresh_ctl(), 16.0, 0, grad_scale=0.5, max_norm=1.0, lr=1e-3)
    assert c[G.IX["norm"]] == 2.0 and c[G.IX["clipped"]] == 1
    assert c[G.IX["scale"]] == float(np.float32(0.5 * (1.0 / (2.0 + 1e-6))))
    assert c[G.IX["step_size"]] == float(np.float32(1e-3 / (1.0 - 0.9)))
    assert c[G.IX["bc2_sqrt"]] == float(np.float32(math.sqrt(1.0 - 0.999)))
    # a non-finite gradient that is NOT skipped: the norm is +inf, nothing is clipped, the step applies
    c2 = G.decide(c, 1.0, 3, max_norm=1.0, skip_nonfinite=False)
    assert c2[G.IX["skip"]] == 0 and math.isinf(c2[G.IX["norm"]]) and c2[G.IX["scale"]] == 1.0 and c2[G.IX["applied"]] == 2
    assert c2[G.IX["norm_max"]] == 2.0 and c2[G.IX["clipped"]] == 1 and c2[G.IX["bad"]] == 3
    c3 = G.decide(c2, 1.0, 3, max_norm=1.0, skip_nonfinite=True)
    assert c3[G.IX["skip"]] == 1 and c3[G.IX["skipped"]] == 1 and c3[G.IX["applied"]] == 2
    assert c3[G.IX["beta1_pow"]] == c2[G.IX["beta1_pow"]] == 0.9 * 0.9


# ---- WarmupMultiStepLR ----------------------------------------------------------------------------------------------
def _closed_form(case, t):
    if t >= case["warmup_iters"]:
        w = 1.0
    elif case["warmup_method"] == "constant":
        w = case["warmup_factor"]
    else:
        w = case["warmup_factor"] * (1 - t / case["warmup_iters"]) + t / case["warmup_iters"]
    return case["base_lr"] * w * case["gamma"] ** sum(1 for m in case["milestones"] if m <= t)


def test_warmup_multistep_lr_matches_the_recorded_reference_and_the_formula():
    """tests/golden/warmup_lr.npz (tools/gen_golden_warmup.py ran the reference's class): linear and constant, a
    milestone inside and after the warm-up, a resume through state_dict into a new scheduler.  Same arithmetic, same
    order of operations: the rates are equal to the last bit; the closed formula to a few ulp."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_golden_warmup as T
    finally:
        sys.path.pop(0)
    from rrnet_amd.utils.warmup_lr import WarmupMultiStepLR
    z = np.load(GOLDEN)
    cases = json.loads(str(z["cases"]))
    assert cases == json.loads(json.dumps(T.CASES)), "the fixture is stale: rerun tools/gen_golden_warmup.py"
    assert {c["warmup_method"] for c in cases} == {"linear", "constant"} and any("resume_at" in c for c in cases)
    assert any(min(c["milestones"]) < c["warmup_iters"] for c in cases)
    for i, case in enumerate(cases):
        got = T.run_case(WarmupMultiStepLR, case)
        want = z["lr_%d" % i]
        assert got.shape == want.shape == (case["steps"] + 1,)
        assert np.array_equal(got, want), (case["name"], np.flatnonzero(got != want)[:5])
        formula = np.array([_closed_form(case, t) for t in range(case["steps"] + 1)])
        np.testing.assert_allclose(got, formula, rtol=1e-14, atol=0)


def test_warmup_multistep_lr_arguments():
    from rrnet_amd.utils.warmup_lr import WarmupMultiStepLR
    import inspect
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    sig = inspect.signature(WarmupMultiStepLR.__init__)
    assert list(sig.parameters) == ["self", "optimizer", "milestones", "gamma", "warmup_factor", "warmup_iters",
                                    "warmup_method", "last_epoch"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["gamma"], d["warmup_factor"], d["warmup_iters"], d["warmup_method"], d["last_epoch"]) == \
        (0.1, 1.0 / 3, 1250, "linear", -1)
    with pytest.raises(ValueError, match="increasing"):
        WarmupMultiStepLR(opt, [30, 10])
    with pytest.raises(ValueError, match="warmup_method"):
        WarmupMultiStepLR(opt, [10, 30], warmup_method="cosine")
    sch = WarmupMultiStepLR(opt, [10, 30])
    assert opt.param_groups[0]["lr"] == 0.1 * (1.0 / 3)            # t = 0 of the default linear ramp


def test_warmup_lr_resolves_through_the_shims():
    """`from utils.warmup_lr import WarmupMultiStepLR` under PYTHONPATH=shims is this package's class, as for the other
    utils modules (the shim aliases the whole package)."""
    code = ("from utils.warmup_lr import WarmupMultiStepLR as A\n"
            "from rrnet_amd.utils.warmup_lr import WarmupMultiStepLR as B\n"
            "assert A is B\nprint('ok')\n")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "shims"))
    out = subprocess.check_output([sys.executable, "-c", code], text=True, cwd="/tmp", env=env, timeout=300)
    assert out.strip().endswith("ok")


def test_operators_choose_the_scheduler_and_the_guard_from_opt_in_keys():
    from rrnet_amd.operators.base_operator import guard_options, make_lr_scheduler
    from rrnet_amd.utils.warmup_lr import WarmupMultiStepLR
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    plain = SimpleNamespace(Train=SimpleNamespace(lr_milestones=[3, 5]))
    assert guard_options(plain) == {}
    assert type(make_lr_scheduler(plain, opt)) is torch.optim.lr_scheduler.MultiStepLR
    cfg = SimpleNamespace(Train=SimpleNamespace(lr_milestones=[3, 5], warmup_iters=4, warmup_factor=0.5, warmup_method="constant",
                                                max_grad_norm=35.0, skip_nonfinite=True, ema_decay=0.999, ema_warmup=False))
    sch = make_lr_scheduler(cfg, opt)
    assert type(sch) is WarmupMultiStepLR and (sch.warmup_iters, sch.warmup_factor, sch.warmup_method) == (4, 0.5, "constant")
    assert list(sch.milestones) == [3, 5] and sch.gamma == 0.1
    assert guard_options(cfg) == dict(max_grad_norm=35.0, skip_nonfinite=True, ema_decay=0.999, ema_warmup=False)


# ---- tools/train.py -------------------------------------------------------------------------------------------------
def _train_tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("rr_tools_train_guard", os.path.join(ROOT, "tools", "train.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    return T


def test_train_tool_guard_flags_set_the_config_keys():
    T = _train_tool()
    cfg = T.configure(T.parse(["--config", "retinanet_config", "--clip-grad-norm", "35", "--skip-nonfinite", "--ema", "0.9998",
                               "--no-ema-warmup", "--warmup", "500", "--warmup-factor", "0.1"]))
    tr = cfg.Train
    assert (tr.max_grad_norm, tr.skip_nonfinite, tr.ema_decay, tr.ema_warmup) == (35.0, True, 0.9998, False)
    assert (tr.warmup_iters, tr.warmup_factor) == (500, 0.1)
    plain = T.configure(T.parse(["--config", "retinanet_config"]))
    for key in ("max_grad_norm", "skip_nonfinite", "ema_decay", "ema_warmup", "warmup_iters", "warmup_factor", "warmup_method"):
        assert not hasattr(plain.Train, key), key
    only_ema = T.configure(T.parse(["--ema", "0.99"])).Train
    assert only_ema.ema_decay == 0.99 and not hasattr(only_ema, "ema_warmup") and not hasattr(only_ema, "max_grad_norm")
    for bad in (["--clip-grad-norm", "0"], ["--ema", "1.5"], ["--no-ema-warmup"], ["--warmup-factor", "0.5"]):
        with pytest.raises(SystemExit):
            T.configure(T.parse(bad))


# ---- FlatParams / FlatAdam on the host ------------------------------------------------------------------------------
def _small_module():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 6, 3), torch.nn.BatchNorm2d(6), torch.nn.Conv2d(6, 5, (1, 2)))


def test_views_of_gives_the_parameters_logical_layout():
    from rrnet_amd.flat import FlatParams
    m = _small_module()
    want = {k: v.detach().clone() for k, v in m.named_parameters()}
    fp = FlatParams(m)
    for buf in (fp.flat, fp.flat.clone()):
        views = fp.views_of(buf)
        assert list(views) == [k for k, _ in m.named_parameters()]
        for k, v in views.items():
            assert v.shape == want[k].shape and torch.equal(v, want[k]), k
    # a view, not a copy; and filters lie OHWI in the buffer
    other = fp.flat.clone()
    fp.views_of(other)["0.weight"][1, 2, 0, 1] = 7.0
    k, c, r, s = 6, 3, 3, 3
    assert other[((1 * r + 0) * s + 1) * c + 2] == 7.0
    with pytest.raises(ValueError):
        fp.views_of(torch.zeros(fp.numel + 4))


def test_flat_adam_guard_options_need_the_device():
    from rrnet_amd.flat import FlatAdam, FlatParams
    fp = FlatParams(_small_module())
    opt = FlatAdam(fp)                                  # the default path is still fine on a CPU FlatParams
    assert not opt.guarded and opt.ema is None and opt.ctl is None
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True), dict(ema_decay=0.99)):
        with pytest.raises(RuntimeError, match="device only"):
            FlatAdam(fp, **kw)
    with pytest.raises(ValueError):
        FlatAdam(fp, max_grad_norm=0.0)
    with pytest.raises(ValueError):
        FlatAdam(fp, ema_decay=1.5)
    with pytest.raises(RuntimeError):
        opt.guard_stats()
    with pytest.raises(RuntimeError):
        opt.ema_state_dict(fp)


# ---- state files ----------------------------------------------------------------------------------------------------
def _fake_optimizer(ema, guard):
    from rrnet_amd.flat import FlatParams
    from rrnet_amd import ops
    m = _small_module()
    fp = FlatParams(m)
    opt = SimpleNamespace(fp=fp, exp_avg=torch.full_like(fp.flat, 0.5), exp_avg_sq=torch.full_like(fp.flat, 0.25),
                          step_count=7, param_groups=[{"lr": 1e-3, "betas": (0.9, 0.999)}],
                          ema=(fp.flat * 2 if ema else None), ctl=(ops.guard_ctl_fresh() + 3 if guard else None))
    return m, opt


def _written_keys(tmp_path, ema, guard):
    """StateWriter with its staging filled on the host (what _allocate and the copy stream do on the device), then the
    writer thread's own _write: the file as it lands on disk."""
    from rrnet_amd import checkpoint as K
    m, opt = _fake_optimizer(ema, guard)
    w = K.StateWriter(m, opt, str(tmp_path))
    try:
        w.names = K.state_names(opt)
        src = (opt.fp.flat, opt.exp_avg, opt.exp_avg_sq) + ((opt.ema,) if ema else ())
        w.h_stage = [s.detach().clone() for s in src]
        w.h_digest = torch.stack([torch.from_numpy(K.digest_reference(s.detach().numpy(), w.chunk).view(np.int64)) for s in src])
        w.buf_index, _ = K._buffer_index(m)
        w.h_bufs = {}
        w.h_guard = opt.ctl.clone() if guard else None
        meta = {"format": K.FORMAT_VERSION, "step": 11, "step_count": 7, "lr": 1e-3, "lr_sch": None, "loader_position": None,
                "fingerprint": K.layout_fingerprint(m, opt.fp), "buffer_index": w.buf_index, "chunk": w.chunk}
        path = w._write(meta, SimpleNamespace(synchronize=lambda: None))
    finally:
        w.close()
    return torch.load(path, map_location="cpu", weights_only=False), opt


BASE_KEYS = {"format", "step", "step_count", "lr", "lr_sch", "loader_position", "fingerprint", "buffer_index", "chunk", "flat",
             "exp_avg", "exp_avg_sq", "digests", "buffers"}


def test_state_file_keys_with_the_options_off_and_on(tmp_path):
    from rrnet_amd import checkpoint as K
    sd, _ = _written_keys(tmp_path / "off", False, False)
    assert set(sd) == BASE_KEYS and sd["format"] == 1 and sd["digests"].shape[0] == 3
    sd, opt = _written_keys(tmp_path / "guard", False, True)
    assert set(sd) == BASE_KEYS | {"guard"} and sd["format"] == 1 and sd["digests"].shape[0] == 3
    assert sd["guard"].dtype == torch.float64 and torch.equal(sd["guard"], opt.ctl)
    sd, opt = _written_keys(tmp_path / "ema", True, True)
    assert set(sd) == BASE_KEYS | {"guard", "ema"} and sd["digests"].shape[0] == 4
    assert torch.equal(sd["ema"], opt.ema)
    assert np.array_equal(sd["digests"][3].numpy().view(np.uint64), K.digest_reference(opt.ema.numpy(), sd["chunk"]))
    assert K.state_names(opt) == ("flat", "exp_avg", "exp_avg_sq", "ema")
    assert K.state_names(SimpleNamespace()) == K.FLAT_NAMES


def test_state_writer_refuses_a_nan_in_the_averaged_weights(tmp_path):
    from rrnet_amd import checkpoint as K
    m, opt = _fake_optimizer(True, True)
    w = K.StateWriter(m, opt, str(tmp_path))
    try:
        w.names = K.state_names(opt)
        w.h_digest = torch.zeros((4, 1, 3), dtype=torch.int64)
        w.h_digest[3, 0, 2] = 2
        assert w._write({"step": 5}, SimpleNamespace(synchronize=lambda: None)) is None
        assert "ema holds 2 NaN/Inf" in w.warnings[0] and not os.listdir(tmp_path)
        w._reported = len(w.warnings)
    finally:
        w.close()


def test_load_rules_for_the_optional_entries():
    from rrnet_amd import checkpoint as K
    on = SimpleNamespace(ema=torch.zeros(4), ctl=torch.zeros(20))
    guard_only = SimpleNamespace(ema=None, ctl=torch.zeros(20))
    off = SimpleNamespace(ema=None, ctl=None)
    full, bare = {"ema": 1, "guard": 2}, {}
    assert K.extras_plan(full, on) == ("restore", "restore")
    assert K.extras_plan(bare, on) == ("init", "derive")
    assert K.extras_plan(full, off) == ("ignore", None)
    assert K.extras_plan(bare, off) == (None, None)
    assert K.extras_plan({"ema": 1}, guard_only) == ("ignore", "derive")
    assert K.extras_plan({"guard": 1}, on) == ("init", "restore")
    assert K.extras_plan(full, SimpleNamespace()) == ("ignore", None)          # an optimiser from before the options


def test_guard_record_derived_from_a_step_count():
    """A state without a guard entry: applied = step_count, the running products as the device would have multiplied
    them one step at a time (equal to the restatement's record after that many applied steps), other counters 0."""
    from rrnet_amd import checkpoint as K
    ctl = G.fresh_ctl()
    for _ in range(37):
        ctl = G.decide(ctl, 1.0, 0)
    got = K.guard_ctl_from_step_count(37, 0.9, 0.999)
    assert got.dtype == np.float64 and got.shape == (len(G.SLOTS),)
    assert got[0] == 37 and got[3] == ctl[G.IX["beta1_pow"]] and got[4] == ctl[G.IX["beta2_pow"]]
    assert not got[[1, 2, 5, 6, 7, 8]].any()
    fresh = K.guard_ctl_from_step_count(0, 0.9, 0.999)
    assert np.array_equal(fresh, G.fresh_ctl())


# ---- the ABI --------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_in_the_header():
    from ctypes import c_double, c_float, c_int, c_long, c_void_p
    from rrnet_amd import _C, ops
    sigs = _C.header_signatures()
    assert sigs["rr_grad_norm_blocks"] == (c_int, [c_long])
    assert sigs["rr_grad_norm"] == (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p])
    assert sigs["rr_guard_decide"] == (c_int, [c_void_p, c_void_p, c_int, c_double, c_double, c_int, c_double, c_double, c_double,
                                               c_double, c_int, c_void_p, c_void_p])
    assert sigs["rr_adam_step_guarded"] == (c_int, [c_void_p] * 5 + [c_long, c_float, c_void_p, c_void_p])
    assert G.header_define("RR_GUARD_CTL_WORDS") == ops.GUARD_CTL_WORDS == len(G.SLOTS) == ops.guard_ctl_fresh().numel()
    assert ops.GUARD_CTL_SLOTS == G.SLOTS and G.header_define("RR_GRAD_NORM_THREADS") % 64 == 0
    assert G.header_define("RR_ABI_VERSION") == 1
    for t in (torch.zeros(8),):
        with pytest.raises(_C.RRNetHipError):
            ops.grad_norm(t)
        with pytest.raises(_C.RRNetHipError):
            ops.adam_step_guarded(t, t, t, t, None, 1e-8, ops.guard_ctl_fresh())
        with pytest.raises(_C.RRNetHipError):
            ops.guard_decide(torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int32), ops.guard_ctl_fresh())

"""Host-side logic that needs no GPU: the collective trace / counters (rrnet_amd/dptrace.py), the launch-sampling rule of
bench.py's kernel timer, the zero pool's slice independence, the defaults of the gradient-link bookkeeping."""
import torch


def test_dptrace_counts_and_sequences():
    from rrnet_amd import dptrace
    dptrace.reset()
    was = dptrace.ENABLED
    try:
        dptrace.ENABLED = True
        dptrace.record("default", "all_reduce", 513, "syncbn_fwd")
        dptrace.mark("param 3 bucket 0")
        dptrace.record("grads", "all_reduce", 4096, "bucket 0")
        dptrace.record("default", "all_reduce", 1024, "syncbn_bwd")
        assert dptrace.counts() == {"default": 2, "grads": 1}
        assert [e[:3] for e in dptrace.sequence("default")] == [("default", "all_reduce", 513), ("default", "all_reduce", 1024)]
        assert len(dptrace.sequence()) == 3 and len(dptrace.EVENTS) == 4          # the mark is kept, but is no collective
        dptrace.ENABLED = False
        dptrace.record("default", "broadcast", 7)
        assert dptrace.counts()["default"] == 3 and len(dptrace.EVENTS) == 4       # counters always on, trace only on request
    finally:
        dptrace.ENABLED = was
        dptrace.reset()


def test_kernel_timer_samples_every_nth_launch_of_a_name(monkeypatch):
    from rrnet_amd import ops

    class FakeEvent:
        def __init__(self, enable_timing=True):
            pass

        def record(self):
            pass

    monkeypatch.setattr(torch.cuda, "Event", FakeEvent)
    t = ops.KernelTimer(only={"a"}, every=4)
    ran = []
    for i in range(10):
        t.launch("a", 1.0, lambda i=i: ran.append(("a", i)))
        t.launch("b", 1.0, lambda i=i: ran.append(("b", i)))
    assert len(ran) == 20                                   # every launch runs
    assert len(t.records) == 3                              # launches 0, 4, 8 of "a" carry events; "b" is not timed at all
    assert all(r[0] == "a" for r in t.records)


def test_zero_pool_slices_are_independent_tensors():
    from rrnet_amd.ops import _ZeroPool
    p = _ZeroPool()
    a, b = p.take(5, torch.device("cpu")), p.take(6, torch.device("cpu"))
    va, vb = a._version, b._version
    a[0] = 3.0
    assert a._version == va + 1 and b._version == vb        # an in-place write does not touch the sibling's version counter
    assert float(b.abs().sum()) == 0.0 and b.data_ptr() - a.data_ptr() == 48       # 16-byte aligned, disjoint


def test_gradient_link_defaults():
    from rrnet_amd import functional as RF, ops
    link = ops.BnLink()
    assert link.sums is None and link.dz is None and link.consumers == 0 and not link.use_z and not link.relu_bias
    acc = RF.GradAcc()
    assert acc.buf is None and acc.pending == 0 and acc.link is None


def test_conv_math_switch_and_split_layer_policy():
    """cfg.Model.conv_math -> ops.math_mode, and the layer policy of the split-operand arithmetic (ops._bf16_ok): host logic
    only — no kernel is launched."""
    from types import SimpleNamespace
    import pytest
    import torch
    from rrnet_amd import ops
    assert ops.math_mode(SimpleNamespace()) == ops.MATH_F32
    assert ops.math_mode(SimpleNamespace(bf16=True)) == ops.MATH_BF16
    assert ops.math_mode(SimpleNamespace(bf16=True, conv_math="f16x3")) == ops.MATH_F16X3      # conv_math wins
    assert ops.math_mode(SimpleNamespace(conv_math="f32")) == ops.MATH_F32
    assert ops.math_mode(SimpleNamespace(conv_math=None, bf16=False)) == ops.MATH_F32
    with pytest.raises(ValueError):
        ops.math_mode(SimpleNamespace(conv_math="fp8"))
    t = torch.empty(4)
    saved = ops.BF16
    try:
        ops.BF16 = ops.MATH_F32
        assert ops._bf16_ok(256, 256, 3, 3, t, pixels=1 << 20) == 0
        ops.BF16 = ops.MATH_BF16
        assert ops._bf16_ok(256, 256, 3, 3, t) == ops.MATH_BF16
        assert ops._bf16_ok(254, 256, 3, 3, t) == 0                        # C not a multiple of 4: fp32 kernels
        ops.BF16 = ops.MATH_F16X3
        assert ops._bf16_ok(256, 256, 3, 3, t, pixels=8 * 256 * 256) == ops.MATH_F16X3
        assert ops._bf16_ok(384, 384, 3, 3, t, pixels=8 * 16 * 16) == ops.MATH_F16X3
        assert ops._bf16_ok(512, 512, 3, 3, t, pixels=8 * 8 * 8) == 0      # 512 output pixels: stays on the fp32-MFMA kernel
        assert ops._bf16_ok(256, 256, 1, 1, t, pixels=8 * 256 * 256) == 0  # reduction length 256 < 1024
        assert ops._bf16_ok(256, 36, 3, 3, t, pixels=8 * 256 * 256) == 0   # narrow output (WH head)
        assert ops._bf16_ok(256, 256, 3, 3, t) == 0                        # a caller that does not state its size
        with ops.bf16_scope(ops.MATH_BF16):
            assert ops.BF16 == ops.MATH_BF16
        assert ops.BF16 == ops.MATH_F16X3
    finally:
        ops.BF16 = saved


def test_conv_math_switch_is_per_thread_and_checked():
    """The arithmetic switch lives in a threading.local: another thread reads the environment's default whatever
    this one set; bf16_scope(0, force=True) means the fp32 kernels; an unknown RR_CONV_MATH raises instead of meaning f32."""
    import subprocess
    import sys
    import threading
    from rrnet_amd import ops
    saved = ops.BF16
    seen = {}
    try:
        ops.BF16 = ops.MATH_F16X3

        def other():
            seen["default"] = ops.BF16
            with ops.bf16_scope(ops.MATH_BF16):
                seen["inside"] = ops.BF16
            seen["after"] = ops.BF16
        th = threading.Thread(target=other)
        th.start()
        th.join()
        assert seen == {"default": ops._BF16_ENV, "inside": ops.MATH_BF16, "after": ops._BF16_ENV}
        assert ops.BF16 == ops.MATH_F16X3                       # untouched by the other thread's scope
        with ops.bf16_scope(0, force=True):
            assert ops.BF16 == ops.MATH_F32
        assert ops.BF16 == ops.MATH_F16X3
    finally:
        ops.BF16 = saved
    r = subprocess.run([sys.executable, "-c", "import rrnet_amd.ops"], env={**__import__("os").environ, "RR_CONV_MATH": "fp8"},
                       capture_output=True, text=True, cwd=__import__("os").path.dirname(__import__("os").path.dirname(__file__)))
    assert r.returncode != 0 and "RR_CONV_MATH" in r.stderr


def test_stride2_parity_class_padding_rule():
    """ops._s2_parity_pads_ok mirrors dgrad_s2_impl's lead >= 0 test (csrc/conv_bf16.hip): the hourglass shapes pass, a 3x3
    stride-2 pad-2 layer falls back to rr_conv_dgrad instead of raising."""
    from rrnet_amd import ops
    assert ops._s2_parity_pads_ok(3, 3, (1, 1)) and ops._s2_parity_pads_ok(1, 1, (0, 0)) and ops._s2_parity_pads_ok(7, 7, (3, 3))
    assert not ops._s2_parity_pads_ok(3, 3, (2, 2)) and not ops._s2_parity_pads_ok(3, 3, (1, 2))
    assert not ops._s2_parity_pads_ok(1, 1, (1, 1))


def test_profiles_index_names_only_files_that_exist():
    """profiles/README.md is the evidence index DESIGN.md and the commit titles point to: every file name it quotes must be
    tracked under profiles/ (round 4 indexed two files that only existed in the untracked gpurun_out/)."""
    import itertools
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    text = open(os.path.join(root, "README.md")).read()
    names = set()
    for quoted in re.findall(r"`([^`\n]+)`", text):
        if not re.fullmatch(r"[\w{},.\-]+\.(json|csv|txt|log)", quoted) or quoted.startswith("."):
            continue                                   # commands, kernel names, `..._suffix` continuations, `r04_infer_*` globs
        parts = re.split(r"\{([^}]*)\}", quoted)      # r04_config4_bf16_{dcn,plain}_bench.json -> both names
        alts = [p.split(",") if i % 2 else [p] for i, p in enumerate(parts)]
        names.update("".join(c) for c in itertools.product(*alts))
    assert len(names) >= 25, sorted(names)
    missing = sorted(n for n in names if not os.path.exists(os.path.join(root, n)))
    assert not missing, "profiles/README.md indexes files that are not in profiles/: %s" % missing


def test_bf16_only_tensor_is_recognised_by_identity():
    """ops.is_phantom (host logic, CPU tensors suffice): a bf16-only activation is a zero-stride view of the per-device NaN stub;
    views keep the identity, an expanded scalar (autograd's gradient of .sum()) or a look-alike built by hand does not have it."""
    import torch
    from rrnet_amd import ops
    img = torch.zeros((2, 3, 4, 8), dtype=torch.bfloat16).permute(0, 3, 1, 2)
    p = ops.phantom_f32((2, 8, 3, 4), torch.device("cpu"), img)
    assert ops.is_phantom(p) and ops.is_phantom(p.view_as(p)) and ops.image_of(p) is img
    assert not ops.is_phantom(torch.ones(1).expand(2, 8, 3, 4))
    assert not ops.is_phantom(torch.empty(2)[1:].expand(2, 8, 3, 4))          # round 5's signature alone is not enough any more
    assert not ops.is_phantom(torch.zeros(2, 8, 3, 4)) and not ops.is_phantom(None)
    assert ops.to_nhwc(p, keep_phantom=True) is p


def test_bf16_only_handle_reads_as_nan_for_torch_native_consumers():
    """a bf16-only tensor is an fp32 handle WITHOUT memory; a torch-native consumer that slips past the
    kernel wrappers (a forward hook, `+`, .sum(), a print) must not read one repeated garbage value silently — the stub it
    expands from holds NaN, so the accident poisons the result loudly.  The structural signature and the image link stay."""
    import torch
    from rrnet_amd import ops
    img = torch.ones((2, 3, 4, 8), dtype=torch.bfloat16).permute(0, 3, 1, 2)
    p = ops.phantom_f32((2, 8, 3, 4), torch.device("cpu"), img)
    q = ops.phantom_f32((1, 8, 5, 4), torch.device("cpu"), img)
    assert ops.is_phantom(p) and ops.is_phantom(q) and ops.image_of(p) is img
    assert (p + 0).isnan().all() and p.sum().isnan() and p.float().isnan().all() and (q * 2).isnan().all()
    assert ops.is_phantom(p.view_as(p)) and p.view_as(p).isnan().all()
    try:
        ops.image_of(p.view_as(p))               # a view made outside the wrappers has lost the image: loud, not silent
    except RuntimeError as e:
        assert "without its bf16 image" in str(e)
    else:
        raise AssertionError("a handle without its image link must raise")


def _b16_image(n, c, h, w):
    import torch
    return torch.zeros((n, h, w, c), dtype=torch.bfloat16).permute(0, 3, 1, 2)


def test_phantom_image_does_not_depend_on_the_shared_stub_version():
    """Every bf16-only handle of a device views one stub and shares its version counter; its image is its value and is never
    updated in place.  A write of the stub must not unlink the image of any live handle, nor of a restored view of one."""
    import torch
    from rrnet_amd import ops
    dev = torch.device("cpu")
    img_p, img_q = _b16_image(2, 8, 3, 4), _b16_image(1, 8, 5, 4)
    p, q = ops.phantom_f32((2, 8, 3, 4), dev, img_p), ops.phantom_f32((1, 8, 5, 4), dev, img_q)
    assert ops.b16_carry(p) is img_p and ops.b16_carry(q) is img_q
    carried = ops.side_carry(p)
    v = p.view_as(p)
    ops.side_restore(carried, v)
    ops._PHANTOM_STUB[dev].fill_(float("nan"))
    assert ops.b16_carry(p) is img_p and ops.b16_carry(q) is img_q
    assert ops.image_of(p) is img_p and ops.image_of(q) is img_q
    assert ops.image_of(v) is img_p and ops.bf16_of(v) is img_p
    v2 = p.view_as(p)
    ops.side_restore(ops.side_carry(p), v2)
    ops._PHANTOM_STUB[dev].fill_(float("nan"))
    assert ops.image_of(v2) is img_p and ops.b16_side.now(v2) is img_p


def test_sidecars_of_ordinary_tensors_go_stale_with_the_version_and_drop_together():
    import torch
    from rrnet_amd import ops
    t, img, word = torch.zeros(1, 8, 2, 2), _b16_image(1, 8, 2, 2), torch.zeros(1, dtype=torch.float64)
    ops.b16_side.attach(t, img)                 # (not on the GPU: no stream to be valid on)
    ops.amax_side.attach(t, word)
    assert ops.b16_carry(t) is img and ops.amax_carry(t) is word and ops.b16_side.now(t) is img and ops.amax_side.now(t) is word
    a, b = torch.zeros(1, 8, 2, 2), torch.zeros(1, 8, 2, 2)
    ops.side_restore(ops.side_carry(t, None, t), a, None, b)       # both kinds of the first tensor, the images of the rest
    assert ops.amax_carry(a) is word and ops.b16_carry(a) is img and ops.amax_carry(b) is None and ops.b16_carry(b) is img
    t.add_(1)
    assert ops.b16_carry(t) is None and ops.amax_carry(t) is None and ops.b16_side.now(t) is None and ops.amax_side.now(t) is None
    ops.b16_side.attach(t, img)
    ops.amax_side.attach(t, word)
    assert ops.b16_carry(t) is img and ops.amax_carry(t) is word
    ops.amax_drop(t)                            # a raw-pointer write: both kinds
    assert ops.b16_carry(t) is None and ops.amax_carry(t) is None
    ops.amax_drop(None)


def test_sidecars_are_shared_with_views_and_restored_for_use_now():
    import torch
    from rrnet_amd import ops
    t, img, word = torch.zeros(1, 8, 2, 2), _b16_image(1, 8, 2, 2), torch.zeros(1, dtype=torch.float64)
    ops.b16_side.attach(t, img)
    ops.amax_side.attach(t, word)
    a, b = t.view_as(t), t.view_as(t)
    ops.b16_side.share(t, (a, b))
    ops.amax_side.share(t, (a, b))
    for o in (a, b):
        assert ops.b16_carry(o) is img and ops.amax_carry(o) is word and ops.b16_side.now(o) is img
    fresh = torch.zeros(1, 8, 2, 2)
    ops.side_restore(ops.side_carry(t), fresh)
    assert ops.b16_side.now(fresh) is img and ops.amax_side.now(fresh) is word
    ops.side_restore(None, fresh)               # a node that carried nothing
    ops.side_restore((None, None, None), fresh, None)
    assert ops.b16_side.now(fresh) is img and ops.amax_side.now(fresh) is word
    stale = torch.zeros(1, 8, 2, 2)
    ops.b16_side.attach(stale, img)
    stale.add_(1)
    c = stale.view_as(stale)
    ops.b16_side.share(stale, (c,))             # nothing valid rides on it: nothing travels
    assert ops.b16_carry(c) is None


def test_publication_truth_tables():
    """ops.image_wanted / amax_wanted: the conditions bn_apply, bn_bwd_apply, upsample_add_fwd and the fan-out used to restate
    (C % 128 == 0 and >= 8192 pixels under bf16 with the conv16 kernels on; >= 2048 pixels under f16x3; on the GPU only)."""
    import torch
    from rrnet_amd import ops
    gpu, cpu = torch.device("cuda"), torch.device("cpu")
    assert ops._CONV16_MIN_PIXELS == 8192 and ops._SPLIT_MIN_PIXELS == 2048
    saved = ops._CONV16
    try:
        ops._CONV16 = True
        with ops.bf16_scope(ops.MATH_BF16, force=True):
            assert ops.image_wanted(128, 8192, gpu) and ops.image_wanted(384, 10000, gpu)
            assert not ops.image_wanted(127, 8192, gpu) and not ops.image_wanted(128, 8191, gpu) and not ops.image_wanted(128, 8192, cpu)
            assert ops.image_wanted(256, 8192, gpu, 256) and not ops.image_wanted(128, 8192, gpu, 256)
            assert not ops.amax_wanted(128, 8192, gpu)
            ops._CONV16 = False
            assert not ops.image_wanted(128, 8192, gpu)
            ops._CONV16 = True
        with ops.bf16_scope(ops.MATH_F16X3, force=True):
            assert ops.amax_wanted(12, 2048, gpu) and not ops.amax_wanted(12, 2047, gpu) and not ops.amax_wanted(12, 2048, cpu)
            assert not ops.image_wanted(128, 8192, gpu)
        with ops.bf16_scope(ops.MATH_F32, force=True):
            assert not ops.image_wanted(128, 8192, gpu) and not ops.amax_wanted(12, 2048, gpu)
    finally:
        ops._CONV16 = saved


def test_bench_self_launches_child_ranks_when_no_launcher_started_it():
    """VERDICT r5 missing #3 (reference: operators/distributed_wrapper.py:47-61 spawns its own workers): `python bench.py --gpus 2`
    without launcher variables must become the launcher — `torch.distributed.run` with two ranks as a CHILD process, decided
    before anything touches the GPU — and hand the launcher's exit code on.  On this GPU-less container every rank ends with
    bench.py's "no GPU visible" exit (3), which is what shows that two ranks really started; the GPU form of the same call is
    tests/test_dp_gpu.py::test_bench_two_ranks_through_the_launcher."""
    import os
    import subprocess
    import sys
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU box: the self-launch is exercised with real ranks in tests/test_dp_gpu.py")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-extras"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "starting 2 ranks" in r.stderr and "torch.distributed.run" in r.stderr, r.stderr[-1500:]
    assert r.stderr.count("no GPU visible") >= 2, r.stderr[-1500:]            # both child ranks ran bench.py's own check
    assert '{"metric"' not in r.stdout


def test_bench_dump_outputs_writes_float32_arrays_and_a_fixed_sample(tmp_path):
    """bench.py --dump-outputs: the last timed step's heat-map / size / offset logits and losses as <name>.npy in float32,
    arrays above the per-array cap as <name>_sample.npy at the same positions on every call, all files together under 64 MB
    (outputs shaped as the 1024x1024, B=8 step hands them out; host tensors stand in for device ones).  The RoI outputs,
    whose number and order depend on near-tied scores, are not written: a step keeping other RoIs writes the same files."""
    import os
    import sys
    import numpy as np
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    g = torch.Generator().manual_seed(0)
    n_hm = 8 * 10 * 256 * 256             # heat-map values = their flat position (exact in float32)
    hms = [torch.arange(n_hm, dtype=torch.float32).view(8, 10, 256, 256).to(memory_format=torch.channels_last) for _ in range(2)]
    whs = [torch.randn(8, 2, 256, 256, generator=g) for _ in range(2)]
    losses = tuple(torch.tensor(float(i)) for i in range(5))

    def step_outputs(r):
        rois = torch.cat([torch.randint(0, 8, (r, 1), generator=g).float(), torch.rand(r, 4, generator=g) * 1000], 1)
        return (hms, whs, whs, torch.randn(r, 4, generator=g), rois, torch.rand(r, generator=g),
                torch.randint(0, 10, (r,), generator=g))

    outs = step_outputs(9000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs, losses)
    bench.dump_outputs(str(tmp_path / "c"), step_outputs(8999), losses)
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == sorted(["hm_0_sample.npy", "hm_1_sample.npy", "wh_0.npy", "wh_1.npy", "offset_0.npy", "offset_1.npy", "loss.npy", "hm_loss.npy", "wh_loss.npy", "offset_loss.npy", "s2_reg_loss.npy"])
    assert sum(os.path.getsize(str(tmp_path / "a" / n)) for n in names) <= 64 << 20
    for n in names:
        a, b, c = (np.load(str(tmp_path / d / n)) for d in "abc")
        assert a.dtype == np.float32 and np.array_equal(a, b) and np.array_equal(a, c) and a.size > 0, n
    hm = np.load(str(tmp_path / "a" / "hm_0_sample.npy"))
    assert np.all(np.diff(hm) > 0) and hm[0] >= 0 and hm[-1] < n_hm   # distinct positions, sorted, in logical order
    assert np.array_equal(np.load(str(tmp_path / "a" / "wh_1.npy")), whs[1].numpy())
    assert np.load(str(tmp_path / "a" / "wh_loss.npy")) == 2.0


# ---- promises of the seeded generators behind the fp64 kernel checks (tests/helpers.py) ----------------------------
def test_focal_inputs_keep_out_of_the_clamp_band():
    """No logit within FOCAL_BAND of +-logit(1e-4), where fp32 and fp64 clamp masks may disagree; saturated logits,
    exact peaks, exact zeros and nextafter(1, 0) are all present; the N_pos == 0 variant has no peak."""
    import numpy as np
    from helpers import FOCAL_BAND, FOCAL_CLAMP_LOGIT, focal_inputs
    assert abs(FOCAL_CLAMP_LOGIT + 9.21024) < 1e-5
    for shape, pos in [((1, 1, 1, 1), True), ((3, 7, 37, 41), True), ((2, 10, 128, 128), True),
                       ((8, 10, 256, 256), True), ((8, 10, 256, 256), False)]:
        x, gt = focal_inputs(shape, seed=sum(shape) + 7 * pos, with_pos=pos)
        assert x.shape == gt.shape == shape and x.dtype == gt.dtype == np.float32
        d = np.abs(np.abs(x.astype(np.float64)) - abs(FOCAL_CLAMP_LOGIT))
        assert d.min() >= FOCAL_BAND, (shape, d.min())
        assert (gt == 1).any() == pos
        if x.size > 1000:
            for v in (-100, -30, 30, 100):
                assert (x == v).any()
            assert (gt == 0).any() and (gt == np.nextafter(np.float32(1), np.float32(0))).any()
            assert ((gt > 0) & (gt < 0.99)).any()


def test_regl1_inputs_hold_the_edge_cases():
    import numpy as np
    from helpers import regl1_inputs
    pred, mask, ind, target = regl1_inputs(8, 64, 64, seed=31, slots=64)
    hw = 64 * 64
    assert mask.shape == ind.shape == (8, 64, 1) and target.shape == (8, 64, 2)
    for b in range(8):
        valid = ind[b, mask[b, :, 0] == 1, 0]
        _, cnt = np.unique(valid, return_counts=True)
        assert cnt.max() == 3 and (cnt == 2).any()
        masked = ind[b, mask[b, :, 0] == 0, 0]
        assert (masked == hw - 1).any() and np.isin(masked[masked != 0], valid).sum() >= 2
        flat = pred[b].reshape(2, hw)
        same = [(flat[:, int(ind[b, s, 0])] == target[b, s]).any() for s in range(64) if mask[b, s, 0] == 1]
        assert sum(same) >= 3
    assert regl1_inputs(8, 16, 24, seed=31, slots=0)[1].shape == (8, 0, 1)


def test_stage2_inputs_keep_out_of_the_iou_band():
    """No fp64 IoU within STAGE2_IOU_BAND of 0.5, no near-tie between differing gt boxes for a positive RoI, images
    interleaved, one image without a positive and one with only positives, zero and duplicated gt rows present."""
    import numpy as np
    from helpers import STAGE2_IOU_BAND, stage2_best_iou, stage2_inputs, stage2_iou_margins
    for scale in (4.0, 1.0):
        rois, reg, gt = stage2_inputs(seed=int(scale) + 40, scale=scale)
        assert rois.shape == (2400, 5) and reg.shape == (2400, 4) and gt.shape == (8, 100, 8)
        d05, gap = stage2_iou_margins(rois, gt, scale)
        best = np.array([stage2_best_iou(r, gt, scale) for r in rois])
        assert d05.min() > STAGE2_IOU_BAND
        assert gap[best > 0.5].min() > STAGE2_IOU_BAND
        img = rois[:, 0].astype(int)
        assert (np.diff(img) != 0).mean() > 0.5                         # interleaved
        npos = np.array([(best[img == b] > 0.5).sum() for b in range(8)])
        assert npos[3] == 0 and npos[5] == 300 and (npos > 0).sum() == 7
        assert np.all(rois[:, 3] > rois[:, 1]) and np.all(rois[:, 4] > rois[:, 2])
        for b in range(8):
            assert np.all(gt[b, -5:] == 0) and np.array_equal(gt[b, 0], gt[b, 1]) and np.array_equal(gt[b, 5], gt[b, 7])


def test_dyadic_roi_set_is_exact_in_fp32():
    """Every sample position of the dyadic RoIAlign set, evaluated as oracle.ops.roi_align does in fp32, equals its
    fp64 evaluation, and so do the bilinear weights of oracle.ops._bilinear_weights and weight / count."""
    import numpy as np
    from helpers import ROI_DYADIC_CASES, ROI_DYADIC_MAP, bilinear_weights64, roi_dyadic_case, roi_sample_grid
    from oracle.ops import _bilinear_weights
    _, H, W = ROI_DYADIC_MAP
    for size, sr, scale, ch in ROI_DYADIC_CASES:
        rois = np.unique(roi_dyadic_case(size, sr, scale, ch), axis=0)
        for roi in rois:
            y32, x32, cnt = roi_sample_grid(roi, size, scale, sr, np.float32)
            y64, x64, cnt64 = roi_sample_grid(roi, size, scale, sr, np.float64)
            assert cnt == cnt64 and cnt & (cnt - 1) == 0
            assert np.array_equal(y32.astype(np.float64), y64) and np.array_equal(x32.astype(np.float64), x64)
            for y in y32.ravel()[::3]:
                for x in x32.ravel()[::3]:
                    ok, idx, w = _bilinear_weights(y, x, H, W)
                    ok64, idx64, w64 = bilinear_weights64(float(y), float(x), H, W)
                    assert ok == ok64
                    if ok:
                        assert idx == idx64
                        assert [float(v) for v in w] == list(w64)
                        assert [float(np.float32(v / np.float32(cnt))) for v in w] == [v / cnt for v in w64]


def test_dyadic_roi_set_without_race_rows_and_unchanged_with_them():
    """roi_dyadic_set(race=0) adds no race rows and takes any number of bins; the arrays of ROI_DYADIC_CASES (which the
    backward tests use) are bit for bit what they were before race became optional (CRC-32 over the twelve arrays)."""
    import zlib
    import numpy as np
    from helpers import ROI_DYADIC_CASES, roi_dyadic_case, roi_dyadic_set
    crc = 0
    for case in ROI_DYADIC_CASES:
        rois = roi_dyadic_case(*case)
        assert rois.shape == (542, 5) and rois.dtype == np.float32
        crc = zlib.crc32(rois.tobytes(), crc)
        assert np.array_equal(roi_dyadic_case(*case, race=0), rois[:42])
        assert np.array_equal(roi_dyadic_case(*case, race=3), rois[:45])
    assert crc == 0x49ad707
    assert roi_dyadic_set(5, (9, 9), -1, 1.0, 30, 36, race=0).shape == (42, 5)


def _roi_fwd_cells(rois, size, sr, scale, ch):
    from helpers import roi_forward_route
    return ["%s-%s" % roi_forward_route(r, size, scale, sr, ch) for r in rois]


def test_roi_forward_route_restates_the_dispatch():
    import numpy as np
    from helpers import roi_forward_route
    small, wide, huge = (np.array([0, 2.0, 3.0, 2.0 + s, 3.0 + s], np.float32) for s in (9.0, 48.75, 150.0))
    assert roi_forward_route(small, (3, 3), 1.0, -1, 256) == ("3x3", "F")
    assert roi_forward_route(small, (3, 3), 1.0, 2, 256) == ("3x3", "P")           # bins of 3 > 2 samples
    assert roi_forward_route(small, (3, 3), 0.25, 2, 256) == ("3x3", "F")
    assert roi_forward_route(small, (3, 3), 1.0, -1, 6) == ("generic", "P")
    assert roi_forward_route(wide, (3, 3), 1.0, -1, 4) == ("3x3", "P")             # 17 samples per bin
    assert roi_forward_route(wide[[0, 1, 2, 3, 2]] + [0, 0, 0, 0, 9], (3, 3), 1.0, -1, 4) == ("3x3", "P")   # one axis decides
    assert roi_forward_route(wide, (7, 7), 1.0, -1, 4) == ("sep", "F")
    assert roi_forward_route(huge, (7, 7), 1.0, -1, 4) == ("sep", "P")
    assert roi_forward_route(small, (8, 8), 1.0, -1, 4) == ("sep", "F")
    assert roi_forward_route(small, (8, 1), 1.0, -1, 4) == ("sep", "F")
    assert roi_forward_route(small, (9, 1), 1.0, -1, 4) == ("generic", "P")
    assert roi_forward_route(small, (1, 9), 1.0, -1, 8) == ("generic", "P")


def test_roi_forward_cases_reach_every_route_under_both_sampling_modes():
    """Across ROI_FWD_CASES each of the five (kernel, branch) cells of rr_roi_align_fwd holds at least 5 RoIs under
    adaptive and at least 5 under fixed sampling; the RoIs entirely outside the map sit at ROI_FWD_OUTSIDE; every RoI
    names image 0 or 1 of the batch of 3."""
    import numpy as np
    from helpers import ROI_DYADIC_MAP, ROI_FWD_CASES, ROI_FWD_OUTSIDE, roi_fwd_case, roi_sample_grid
    B, H, W = ROI_DYADIC_MAP
    assert len(ROI_FWD_CASES) == 18
    cells = {}
    for size, sr, scale, ch in ROI_FWD_CASES:
        rois = roi_fwd_case(size, sr, scale, ch)
        assert rois.shape == (50, 5) and rois.dtype == np.float32
        assert set(rois[:, 0]) == {0.0, 1.0} and B == 3
        for cell in _roi_fwd_cells(rois, size, sr, scale, ch):
            cells[cell, sr > 0] = cells.get((cell, sr > 0), 0) + 1
        assert all(not ((g >= -1) & (g <= lim)).any() for r, (k, lim) in zip(ROI_FWD_OUTSIDE, ((0, H), (1, W)))
                   for g in [roi_sample_grid(rois[r], size, scale, sr, np.float64)[k]])
    print(sorted(cells.items()))
    assert set(cells) == {(c, m) for c in ("3x3-F", "3x3-P", "sep-F", "sep-P", "generic-P") for m in (False, True)}
    assert min(cells.values()) >= 5, cells


def test_roi_forward_sets_are_exact_in_fp32():
    """Every sample position of every dyadic and boundary RoI of ROI_FWD_CASES, evaluated as oracle.ops.roi_align does
    in fp32, equals its fp64 evaluation; the samples per bin are a power of two; and the boundary RoIs put their limit
    samples exactly on -1, H and W, their twins 1/16 beyond."""
    import numpy as np
    from helpers import ROI_DYADIC_MAP, ROI_FWD_CASES, roi_fwd_case, roi_sample_grid
    _, H, W = ROI_DYADIC_MAP
    for size, sr, scale, ch in ROI_FWD_CASES:
        rois = roi_fwd_case(size, sr, scale, ch)
        for roi in rois:
            y32, x32, cnt = roi_sample_grid(roi, size, scale, sr, np.float32)
            y64, x64, cnt64 = roi_sample_grid(roi, size, scale, sr, np.float64)
            assert cnt == cnt64 and cnt & (cnt - 1) == 0
            assert np.array_equal(y32.astype(np.float64), y64) and np.array_equal(x32.astype(np.float64), x64)
            assert np.array_equal(y64 * 256, np.round(y64 * 256)) and np.array_equal(x64 * 256, np.round(x64 * 256))
        edge = [roi_sample_grid(roi, size, scale, sr, np.float32) for roi in rois[-8:]]
        assert all(e[2] == 4 for e in edge)
        assert [edge[0][0].min(), edge[1][0].min()] == [-1.0, -1.0625]
        assert [edge[2][0].max(), edge[3][0].max()] == [H, H + 0.0625]
        assert [edge[4][1].min(), edge[5][1].min()] == [-1.0, -1.0625]
        assert [edge[6][1].max(), edge[7][1].max()] == [W, W + 0.0625]
        for k, e in enumerate(edge):                  # the other axis stays inside the map
            other = e[1 if k < 4 else 0]
            assert other.min() >= 0 and other.max() <= (W if k < 4 else H) - 1


def test_roi_random_set_keeps_clear_of_the_inside_limits():
    """helpers.roi_random_set: its first 44 rows are the backward tests' set; with the large RoIs at least 10 take
    per-sample taps at (3,3) bins and at least 5 at (7,7) under adaptive sampling; for every size and sampling mode
    float32 and float64 agree on the sampling grid and on every sample's inside test, no float64 sample lies within
    1e-3 of -1, H or W, and every RoI names image 0 or 1."""
    import numpy as np
    from helpers import ROI_RANDOM_MAP, ROI_RANDOM_SIZES, roi_random_set, roi_sample_grid
    B, H, W = ROI_RANDOM_MAP
    rois = roi_random_set(large=True)
    assert rois.shape == (56, 5) and np.array_equal(rois[:44], roi_random_set()) and roi_random_set().shape == (44, 5)
    assert set(rois[:, 0]) == {0.0, 1.0} and B == 3
    assert _roi_fwd_cells(rois, (3, 3), -1, 1.0, 256).count("3x3-P") >= 10
    assert _roi_fwd_cells(rois, (7, 7), -1, 1.0, 256).count("sep-P") >= 5
    nearest = np.inf
    for size in ROI_RANDOM_SIZES:
        for sr in (-1, 2):
            for roi in rois:
                y32, x32, _ = roi_sample_grid(roi, size, 1.0, sr, np.float32)
                y64, x64, _ = roi_sample_grid(roi, size, 1.0, sr, np.float64)
                assert y32.shape == y64.shape and x32.shape == x64.shape, (roi, size, sr)
                for g32, g64, lim in ((y32, y64, H), (x32, x64, W)):
                    assert np.array_equal((g32 >= -1) & (g32 <= lim), (g64 >= -1) & (g64 <= lim)), (roi, size, sr)
                    nearest = min(nearest, np.abs(g64 + 1).min(), np.abs(g64 - lim).min())
    print("nearest sample to a limit: %.3g" % nearest)
    assert nearest > 1e-3


def _syncbn_shards(seed, shapes, c):
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    ys = [torch.from_numpy(rng.normal(0.4, 1.3, (n, c, h, w))) for n, h, w in shapes]
    dzs = [torch.from_numpy(rng.normal(0.0, 1.0, tuple(y.shape))) for y in ys]
    masks = [torch.from_numpy((rng.random(tuple(y.shape)) < 0.6).astype(np.float64)) for y in ys]
    gamma = torch.from_numpy(rng.normal(1.0, 0.3, c))
    beta = torch.from_numpy(rng.normal(0.0, 0.5, c))
    rm0 = torch.from_numpy(rng.normal(0.0, 1.0, c))
    rv0 = torch.from_numpy(rng.uniform(0.5, 2.0, c))
    return ys, dzs, masks, gamma, beta, rm0, rv0


def test_syncbn_reference_equals_torch_batch_norm_on_the_concatenated_shards():
    """helpers.syncbn_ref64 (the float64 reference of tests/test_syncbn_gpu.py) against torch.nn.functional.batch_norm in
    double + autograd on the concatenation of ragged shards: outputs, dx, dgamma, dbeta and the running statistics, with
    and without a mask on the incoming gradient, at momentum 0.1 and 0.37, down to a global count of 2.  Both are float64
    evaluations of the same formulas: they agree to 1e-12 of each quantity's scale."""
    import torch
    import torch.nn.functional as F
    from helpers import syncbn_ref64
    for seed, shapes, c, mom in ((0, [(5, 3, 3), (131, 3, 3)], 8, 0.1), (1, [(1, 4, 6), (2, 4, 6), (4, 4, 6)], 5, 0.37),
                                 (2, [(1, 1, 1), (1, 1, 1)], 4, 0.1)):
        ys, dzs, masks, gamma, beta, rm0, rv0 = _syncbn_shards(seed, shapes, c)
        for use_mask in (False, True):
            r = syncbn_ref64(ys, gamma, beta, 1e-5, mom, rm0, rv0, dzs, masks if use_mask else None)
            x = torch.cat(ys).clone().requires_grad_()
            g, b = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
            rm, rv = rm0.clone(), rv0.clone()
            out = F.batch_norm(x, rm, rv, g, b, True, mom, 1e-5)
            cot = torch.cat(dzs) * (torch.cat(masks) if use_mask else 1.0)
            out.backward(cot)
            n = [y.shape[0] for y in ys]

            def close(a, ref):
                assert float((a - ref).abs().max()) <= 1e-12 * max(float(ref.abs().max()), 1.0), (seed, use_mask)
            close(torch.cat(r["out"]), out.detach())
            close(torch.cat(r["dx"]), x.grad)
            close(r["bwd_sums"][:c], b.grad)
            close(r["bwd_sums"][c:], g.grad)
            close(r["running_mean"], rm)
            close(r["running_var"], rv)
            close(r["var_one_pass"], r["var"])
            assert r["count"] == sum(k * h * w for k, h, w in shapes) and [t.shape[0] for t in r["dx"]] == n


def test_syncbn_reference_local_sums_add_up_to_the_global_sums():
    """What each virtual rank contributes to the two exchanges — [sum y | sum y^2] forward, [sum d | sum d * xhat] backward —
    adds up to the sums over the concatenated batch; a rank's backward sums are its own dbeta | dgamma."""
    import torch
    from helpers import syncbn_ref64
    ys, dzs, masks, gamma, beta, rm0, rv0 = _syncbn_shards(3, [(2, 5, 7), (3, 5, 7), (1, 5, 7)], 12)
    r = syncbn_ref64(ys, gamma, beta, 1e-5, 0.1, rm0, rv0, dzs, masks)
    y, d = torch.cat(ys), torch.cat(dzs) * torch.cat(masks)
    xh = (y - r["mean"].view(1, -1, 1, 1)) * r["invstd"].view(1, -1, 1, 1)
    for got, ref in ((torch.stack(r["local_sums"]).sum(0), torch.cat([y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))])),
                     (torch.stack(r["local_bwd"]).sum(0), torch.cat([d.sum((0, 2, 3)), (d * xh).sum((0, 2, 3))]))):
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert torch.equal(r["sums"], torch.stack(r["local_sums"]).sum(0))
    assert torch.equal(r["bwd_sums"], torch.stack(r["local_bwd"]).sum(0))
    for i in range(3):          # a shard's own sums: not a share of the total
        di, xi = dzs[i] * masks[i], xh[sum(t.shape[0] for t in ys[:i]):][:ys[i].shape[0]]
        assert float((r["local_bwd"][i][12:] - (di * xi).sum((0, 2, 3))).abs().max()) <= 1e-12 * float(di.abs().sum())


# ---- the float64 convolution checks (tests/test_conv_fp64_gpu.py): reference, yardstick, acceptance rule, route labels ----
def test_conv_ref64_equals_a_hand_written_float64_loop():
    """helpers.conv_ref64 (F.conv2d in float64 + autograd) against plain loops on one tiny strided, asymmetric-filter,
    biased, ReLU'd shape: y, dx, dw; and helpers.conv_terms' gathered products add up to the same three tensors."""
    import numpy as np
    import torch
    from helpers import conv_ref64, conv_terms
    rng = np.random.default_rng(5)
    n, c, h, w, k, r, s, st, ph, pw = 2, 3, 6, 7, 4, 3, 2, 2, 1, 1
    x, wt, b = rng.standard_normal((n, c, h, w)), rng.standard_normal((k, c, r, s)), rng.standard_normal(k)
    p, q = (h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1
    gy = rng.standard_normal((n, k, p, q))
    y = np.zeros((n, k, p, q))
    dx, dw = np.zeros_like(x), np.zeros_like(wt)
    for pas in (0, 1):                       # pass 0: y; pass 1: the gradients through the ReLU mask of y
        for i in range(n):
            for ko in range(k):
                for a in range(p):
                    for bq in range(q):
                        acc = b[ko]
                        for ci in range(c):
                            for rr in range(r):
                                for ss in range(s):
                                    ih, iw = a * st - ph + rr, bq * st - pw + ss
                                    if 0 <= ih < h and 0 <= iw < w:
                                        if pas == 0:
                                            acc += x[i, ci, ih, iw] * wt[ko, ci, rr, ss]
                                        elif y[i, ko, a, bq] > 0:
                                            dx[i, ci, ih, iw] += gy[i, ko, a, bq] * wt[ko, ci, rr, ss]
                                            dw[ko, ci, rr, ss] += gy[i, ko, a, bq] * x[i, ci, ih, iw]
                        if pas == 0:
                            y[i, ko, a, bq] = max(acc, 0.0)
    yr, dxr, dwr = conv_ref64(torch.from_numpy(x), torch.from_numpy(wt), torch.from_numpy(b), st, (ph, pw), True, torch.from_numpy(gy))
    assert yr.dtype == dxr.dtype == dwr.dtype == torch.float64
    for got, ref in ((yr, y), (dxr, dx), (dwr, dw)):
        assert np.abs(got.numpy() - ref).max() <= 1e-13 * np.abs(ref).max()
    gm = gy * (y > 0)
    for kind, ref, args in (("fprop", y, dict(bias=b)), ("dgrad", dx, {}), ("wgrad", dw, {})):
        idx = np.unravel_index(np.arange(ref.size), ref.shape)
        tot = np.concatenate([t.sum(1) for t in conv_terms(kind, idx, x, wt, gm, st, (ph, pw), chunk=200, **args)])
        tot = np.maximum(tot, 0.0) if kind == "fprop" else tot
        assert np.abs(tot - ref.ravel()).max() <= 1e-13 * np.abs(ref).max(), kind
    # an accumulating call's starting value is one more term
    base = rng.standard_normal(dw.shape)
    idx = np.unravel_index(np.arange(dw.size), dw.shape)
    tot = np.concatenate([t.sum(1) for t in conv_terms("wgrad", idx, x, (r, s), gm, st, (ph, pw), base=base)])
    assert np.abs(tot - (dw + base).ravel()).max() <= 1e-13 * np.abs(dw).max()


def test_conv_acceptance_rule_sees_what_a_loose_float32_comparison_cannot():
    """The rule of tests/test_conv_fp64_gpu.py (error at the sampled outputs <= margin x the error of a chained float32 sum of
    the same products: helpers.seq32_error / conv_error_ratios / conv_accepts) at its cap, margin = 8, at reduction lengths
    2304 and 288: it REJECTS a host-simulated kernel that rounds one operand to 11 significant bits, one that rounds both
    to fp16, and one that loses the last 4 products (scaled to 1e-4 of the output) — each otherwise summed exactly — and
    ACCEPTS a float32 pairwise sum."""
    import numpy as np
    from helpers import CONV_MARGIN_CAP, CONV_SAMPLES, conv_accepts, conv_error_ratios, round_sig_bits, seq32_error
    for kg in (2304, 288):
        rng = np.random.default_rng(kg)
        a = rng.standard_normal((CONV_SAMPLES, kg)).astype(np.float32).astype(np.float64)
        b = (rng.standard_normal((CONV_SAMPLES, kg)) / np.sqrt(kg)).astype(np.float32).astype(np.float64)
        tail_scale = 1e-4 * np.sqrt(kg) / 2.0                        # rms of 4 products = 2/sqrt(kg): 1e-4 of the unit output
        a_tail = a.copy()
        a_tail[:, -4:] *= np.float32(tail_scale)

        def verdict(got, terms):
            ref = terms.sum(1)
            max_seq, rms_seq = seq32_error(terms)
            assert 0 < rms_seq < max_seq < 1e-5
            return conv_accepts(conv_error_ratios(got, ref, max_seq, rms_seq, got, ref), CONV_MARGIN_CAP), np.abs(got - ref).max()
        terms = a * b
        for name, got in (("one operand at 11 bits", (a * round_sig_bits(b, 11)).sum(1)),
                          ("both operands fp16", (a.astype(np.float16).astype(np.float64) * b.astype(np.float16).astype(np.float64)).sum(1))):
            ok, err = verdict(got, terms)
            assert not ok, (kg, name, err)
        terms_t = a_tail * b
        ok, err = verdict(np.sum(terms_t[:, :-4].astype(np.float32), axis=1, dtype=np.float32).astype(np.float64), terms_t)
        assert not ok, (kg, "lost K tail", err)
        for t in (terms, terms_t):
            ok, _ = verdict(np.sum(t.astype(np.float32), axis=1, dtype=np.float32).astype(np.float64), t)
            assert ok, (kg, "float32 pairwise sum")
    # a zero yardstick (exact operands) asks for a zero error
    assert conv_accepts(conv_error_ratios(np.ones(4), np.ones(4), 0.0, 0.0)) and not conv_accepts(conv_error_ratios(np.ones(4) + 1e-7, np.ones(4), 0.0, 0.0))


def test_conv_route_mirror_and_grid_coverage():
    """helpers.conv_routes restates the host dispatch of rrnet_amd/csrc/conv.hip: its split-K rule equals the library's own
    pick_ksplit wherever asked, the tile thresholds equal the library's, and the grid of tests/test_conv_fp64_gpu.py reaches
    every route label at least once — and the combinations the grid was laid out for."""
    import ctypes
    from helpers import CONV64_GRID, CONV_ROUTE_LABELS, _MID_TILES, _SMALL_TILES, conv_grid_routes, conv_routes, pick_ksplit_mirror
    from rrnet_amd import _C, ops
    L = _C.lib()
    pick = getattr(L, "_Z19rr_conv_pick_ksplitii")                  # int rr_conv_pick_ksplit(int, int): C++ linkage
    pick.restype, pick.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int]
    bad = [(b, nk) for b in range(1, 260) for nk in list(range(1, 160)) + [288, 432, 1000] if pick(b, nk) != pick_ksplit_mirror(b, nk)]
    assert not bad, bad[:8]
    for name, want in (("_Z19rr_conv_small_tilesv", _SMALL_TILES), ("_Z17rr_conv_mid_tilesv", _MID_TILES)):
        f = getattr(L, name)
        f.restype, f.argtypes = ctypes.c_int, []
        assert f() == want
    assert (ops._SMALL_TILES, ops._MID_TILES) == (_SMALL_TILES, _MID_TILES)
    seen = conv_grid_routes()
    missing = {p: sorted(CONV_ROUTE_LABELS[p] - seen[p]) for p in seen if CONV_ROUTE_LABELS[p] - seen[p]}
    assert not missing, "route labels no grid shape reaches: %s" % missing

    def route(i, ws=False):
        n, c, h, w, k, r, s, st, ph, pw, bias, relu = CONV64_GRID[i][:12]
        return conv_routes(n, c, h, w, k, r, s, st, (ph, pw), bias, relu, ws)
    combos = [(rt["fprop"], rt["dgrad"], rt["wgrad"]) for i in range(len(CONV64_GRID)) for rt in (route(i, False), route(i, True))]
    for pas, want in ((0, {"bn128"}), (0, {"bn128", "ksplit>1+stats"}), (0, {"bn64", "ksplit>1+stats"}), (0, {"bn32", "ksplit>1+stats"}),
                      (0, {"bn128", "scalar"}), (0, {"bn32", "scalar"}), (0, {"bn64", "pos_major"}), (0, {"rows"}),
                      (1, {"bn128", "parity_live<4"}), (1, {"bn32", "parity4"}), (1, {"bn32", "ksplit>1"}), (1, {"bn128", "scalar"}),
                      (2, {"128x32", "a_scalar", "b_scalar"}), (2, {"32x128", "a_scalar"}), (2, {"32x32"}),
                      (2, {"128x128", "a_scalar", "b_scalar"}), (2, {"pipe3", "splits>1"}), (2, {"pipe1"})):
        assert any(cmb[pas] == want for cmb in combos), (pas, want)
    # bias / ReLU keep split-K off on a shape that would otherwise split
    assert route(14)["fprop"] == {"bn32"} and CONV64_GRID[14][10:12] == (True, True)


def _plan_cases():
    """-> [(source, (n, c, h, w, k, r, s, stride, ph, pw), dict(bias, relu, want_stats, link, strided, out_hw))]: what
    test_library_plan_equals_the_mirror asks the library and the mirror about, in every arithmetic."""
    import numpy as np
    from conv_route_cases import cases
    from helpers import CONV64_GRID
    plain = dict(bias=False, relu=False, want_stats=False, link=None, strided=False, out_hw=None)
    out = []

    def add(src, geo, **kw):
        out.append((src, geo, dict(plain, **kw)))

    def via_forward(src, n, c, h, w, k, r, s, stride, ph, pw, link=None):
        """the forward-kernel launches of the data gradient of this convolution: stride 1 on (dy, flipped filter); stride 2 one
        per output parity class on its sub-filter, into a strided destination (the rule of ops._s2_parity_pads_ok restated)"""
        p, q = (h + 2 * ph - r) // stride + 1, (w + 2 * pw - s) // stride + 1
        if stride == 1 and ph < r and pw < s:
            add(src + "/via", (n, k, p, q, c, r, s, 1, r - 1 - ph, s - 1 - pw), link=link)
        if stride == 2:
            for cl in range(4):
                (a, b), (r0, s0) = (cl >> 1, cl & 1), (((cl >> 1) + ph) & 1, ((cl & 1) + pw) & 1)
                rc, sc = ((r - r0 + 1) // 2 if r0 < r else 0), ((s - s0 + 1) // 2 if s0 < s else 0)
                lead = (rc - 1 - (a + ph - r0) // 2, sc - 1 - (b + pw - s0) // 2)
                grid = ((h - a + 1) // 2, (w - b + 1) // 2)
                if rc * sc > 0 and min(lead) >= 0 and min(grid) > 0:
                    add(src + "/class%d" % cl, (n, k, p, q, c, rc, sc, 1) + lead, strided=True, out_hw=grid)

    for i, (n, c, h, w, k, r, s, st, ph, pw, bias, relu, stats, _) in enumerate(CONV64_GRID):
        for ws in stats:
            add("grid%d" % i, (n, c, h, w, k, r, s, st, ph, pw), bias=bias, relu=relu, want_stats=ws)
        via_forward("grid%d" % i, n, c, h, w, k, r, s, st, ph, pw)
    for case in cases():
        (n, c, h, w), k, (r, s), st, (ph, pw) = case["x"], case["k"], case["f"], case["stride"], case["pad"]
        if h + 2 * ph < r or case["mode"] != "f32" or case.get("accumulate"):
            continue                                                    # (the record's arithmetics and accumulate repeat the geometry)
        add(case["id"], (n, c, h, w, k, r, s, st, ph, pw))
        if case["op"] == "dgrad":
            link = {"bn_z": "bn", "mask_only": "relu_bias"}.get(case["link"], case["link"])
            via_forward(case["id"], n, c, h, w, (k + 3) // 4 * 4 if link == "relu_bias" else k, r, s, st, ph, pw, link)
    # relu_bias is refused unless N*P*Q is a multiple of 128, which random maps seldom are: drawn with 0.2 so that, with the
    # 4 / 15 of the channel counts the 16-bit kernels refuse, fewer than half of the draws are refused in any arithmetic
    rng = np.random.default_rng(219)
    for i in range(2400):
        add("random%d" % i, _random_geometry(rng), bias=bool(rng.integers(2)), relu=bool(rng.integers(2)), want_stats=bool(rng.integers(2)),
            link=(None, "bn", "relu_bias")[rng.choice(3, p=(0.6, 0.2, 0.2))])
    return out


_PLAN_CHANS = (3, 6, 10, 24, 34, 36, 48, 64, 128, 160, 256, 384, 512, 1024, 2048)
_PLAN_FILTERS = ((1, 1), (3, 3), (7, 7), (17, 1))


def _random_geometry(rng, chan_p=None, filter_p=None, stride_p=None, pad_hi=4):
    """One (n, c, h, w, k, r, s, stride, ph, pw) of _plan_cases' generator.  Uniform by default; *_p: draw probabilities over
    _PLAN_CHANS / _PLAN_FILTERS / strides 1..3, pad_hi: pads below this — for the families that refuse most uniform draws."""
    def pick(count, p):
        return int(rng.integers(count)) if p is None else int(rng.choice(count, p=p))
    r, s = _PLAN_FILTERS[pick(4, filter_p)]
    return (int(rng.integers(1, 17)), _PLAN_CHANS[pick(15, chan_p)], int(rng.integers(1, 161)), int(rng.integers(1, 161)), _PLAN_CHANS[pick(15, chan_p)],
            r, s, 1 + pick(3, stride_p), int(rng.integers(0, pad_hi)), int(rng.integers(0, pad_hi)))


def test_library_plan_equals_the_mirror():
    """rr_conv_fprop_plan — the plan of rrnet_amd/csrc/conv_plan.h that both fprop_impl launch from — equals helpers._fprop_route,
    the Python restatement of the host code that preceded it, field by field and in each arithmetic: over the grid of
    tests/test_conv_fp64_gpu.py, the forward-kernel launches of its data gradients, the geometries of tests/conv_route_cases.py
    and 2400 seeded random geometries; what an arithmetic refuses, the mirror refuses.  Of the random draws at most half are
    refused per arithmetic, and together the cases reach every route label and every pass around a launch."""
    import ctypes
    from helpers import CONV_PLAN_FIELDS, CONV_ROUTE_LABELS, MATH_BF16, MATH_F16X3, MATH_F32, _fprop_route
    from rrnet_amd import _C
    plan_fn = _C.fn("rr_conv_fprop_plan")
    buf = (ctypes.c_int * len(CONV_PLAN_FIELDS))()
    link_code = {None: 0, "bn": 1, "relu_bias": 2}
    cases = _plan_cases()
    n_random = sum(src.startswith("random") for src, _, _ in cases)
    assert n_random >= 2000
    for math in (MATH_F32, MATH_BF16, MATH_F16X3):
        labels, reached, refused, first3 = set(), set(), 0, set()
        for src, (n, c, h, w, k, r, s, st, ph, pw), f in cases:
            valid = h + 2 * ph >= r and w + 2 * pw >= s                        # (below that the mirror's floor division is not C's)
            want = _fprop_route(n, c, h, w, k, r, s, st, ph, pw, f["bias"], f["relu"], f["want_stats"], math, f["strided"], f["link"],
                                False, f["out_hw"]) if valid else None
            if want is None:
                refused += src.startswith("random")
            if not valid:
                continue
            flags = f["bias"] | f["relu"] << 1 | f["want_stats"] << 2 | f["strided"] << 4 | link_code[f["link"]] << 8
            rc = plan_fn(math, n, h, w, c, k, r, s, st, ph, pw, *(f["out_hw"] or (0, 0)), flags, buf)
            assert (rc != 0) == (want is None), (src, math, rc, want, _C.lib().rr_last_error())
            if want is None:
                continue
            got = dict(zip(CONV_PLAN_FIELDS, buf))
            assert got == {name: want[name] for name in CONV_PLAN_FIELDS}, (src, math, got, want)
            labels |= want["labels"]
            if src in ("grid0", "grid1", "grid2"):
                first3 |= want["labels"]
            reached |= {name for name in ("xcd_n", "fused", "zero_dst", "zero_slab") if got[name]} | {"after%d" % got["after"]}
        assert refused <= n_random // 2, (math, refused, n_random)
        sixteen = {"bn128", "bn64", "bn32", "ksplit>1", "ksplit>1+stats"}
        assert labels == (CONV_ROUTE_LABELS["fprop"] if math == MATH_F32 else sixteen), (math, sorted(labels))
        assert first3 >= sixteen, (math, sorted(first3))
        assert reached == {"fused", "zero_dst", "zero_slab", "after0", "after1", "after2", "after3"} | ({"xcd_n"} if math else set()), (math, sorted(reached))


# ---- the gradient plans of conv_plan.h (rr_conv_grad_plan) against their mirrors ------------------------------------------------
def _grad_plan_of_library(pas, family, geo, out_hw=(0, 0), accumulate=False):
    """rr_conv_grad_plan -> the pass's fields under the mirrors' names, or None where the library refuses the call."""
    import ctypes
    from helpers import CONV_GRAD_FIELDS, CONV_GRAD_PLAN_INTS, GRAD_DGRAD_S2
    from rrnet_amd import _C
    n, c, h, w, k, r, s, st, ph, pw = geo
    buf = (ctypes.c_int * CONV_GRAD_PLAN_INTS)()
    if _C.fn("rr_conv_grad_plan")(pas, family, n, h, w, c, k, r, s, st, ph, pw, out_hw[0], out_hw[1], int(accumulate), buf, len(buf)) != 0:
        return None
    got = dict(zip(CONV_GRAD_FIELDS[pas], buf))
    used = len(CONV_GRAD_FIELDS[pas])
    if pas == GRAD_DGRAD_S2:
        got["launches"] = [tuple(buf[4 + 10 * i:14 + 10 * i]) for i in range(got["n_launch"])]
        used += 10 * got["n_launch"]
    assert not any(buf[used:]), (pas, family, geo, list(buf))
    return got


def _grad_plan_of_mirror(pas, family, geo, out_hw=(0, 0), accumulate=False):
    from helpers import FAM_CONV16, GRAD_DGRAD, GRAD_DGRAD_S2, MATH_F32, _dgrad_route, _wgrad_route, dgrad_s2_mirror, wgrad16_mirror
    n, c, h, w, k, r, s, st, ph, pw = geo
    if pas == GRAD_DGRAD:
        return _dgrad_route(*geo, accumulate)
    if pas == GRAD_DGRAD_S2:
        return dgrad_s2_mirror(family, n, c, h, w, k, r, s, ph, pw, accumulate)
    if family == MATH_F32:
        return _wgrad_route(*geo, *out_hw)
    return wgrad16_mirror(family, *geo, tuple(out_hw) if any(out_hw) and family != FAM_CONV16 else None)


def _grad_plan_combos():
    from helpers import FAM_CONV16, GRAD_DGRAD, GRAD_DGRAD_S2, GRAD_WGRAD, MATH_BF16, MATH_F16X3, MATH_F32
    return [(GRAD_DGRAD, MATH_F32)] + [(GRAD_DGRAD_S2, f) for f in (MATH_BF16, MATH_F16X3, FAM_CONV16)] + \
           [(GRAD_WGRAD, f) for f in (MATH_F32, MATH_BF16, MATH_F16X3, FAM_CONV16)]


def _grad_draw_weights(pas, family):
    """How _random_geometry draws for one pass and family.  Uniform draws are refused too often by the families with shape
    conditions — 4 of the 15 channel counts are no multiple of 4, 9 no multiple of 128, conv16 takes strides 1 and 2 and at most 16
    taps, and a parity-class gradient takes a 1x1 filter with pad 0 only, a 3x3 with pads below 2 — so those get 0.1 of the
    refused channel counts, 0.1 of stride 3, few 1x1 / 7x7 / 17x1 filters and pads below 2: at most half of the draws refused."""
    from helpers import FAM_CONV16, GRAD_DGRAD_S2, GRAD_WGRAD, MATH_F32
    kw = {}
    if family == FAM_CONV16:
        kw["chan_p"] = [0.9 / 6 if ch % 128 == 0 else 0.1 / 9 for ch in _PLAN_CHANS]
    elif family != MATH_F32:
        kw["chan_p"] = [0.9 / 11 if ch % 4 == 0 else 0.1 / 4 for ch in _PLAN_CHANS]
    if pas == GRAD_DGRAD_S2:
        kw.update(filter_p=(0.1, 0.8, 0.05, 0.05) if family == FAM_CONV16 else (0.1, 0.5, 0.3, 0.1), pad_hi=2)
    if pas == GRAD_WGRAD and family == FAM_CONV16:
        kw["stride_p"] = (0.45, 0.45, 0.1)
    return kw


def test_library_gradient_plans_equal_their_mirrors():
    """rr_conv_grad_plan — dgrad_plan, dgrad_s2_plan and wgrad_plan of rrnet_amd/csrc/conv_plan.h, which the gradient entry points
    of conv.hip, conv_bf16.hip and conv16.hip launch from — equals the Python restatements of the host code that preceded them
    (helpers._dgrad_route, dgrad_s2_mirror, _wgrad_route, wgrad16_mirror) field by field, for every pass and family: over
    CONV64_GRID, CONV64_ASYM_WGRAD, CONV16_GRID, CONV16_ASYM_WGRAD, the geometries of tests/conv_route_cases.py and 2400 seeded
    random geometries per pass and family, with and without accumulate.  What a family refuses, the mirror refuses; at most half of
    the random draws are refused per pass and family; together the cases reach every value the plans can take."""
    import numpy as np
    from conv_route_cases import cases
    from helpers import (CONV16_ASYM_WGRAD, CONV16_GRID, CONV64_ASYM_WGRAD, CONV64_GRID, CONV_ROUTE_LABELS, FAM_CONV16, GRAD_DGRAD, GRAD_DGRAD_S2,
                         GRAD_WGRAD, MATH_F32)
    fixed = [("grid64/%d" % i, cfg[:10], (0, 0)) for i, cfg in enumerate(CONV64_GRID)]
    fixed += [("grid16/%d" % i, cfg[:10], (0, 0)) for i, cfg in enumerate(CONV16_GRID)]
    fixed += [("asym64", CONV64_ASYM_WGRAD[:10], CONV64_ASYM_WGRAD[10:]), ("asym16", CONV16_ASYM_WGRAD[:10], CONV16_ASYM_WGRAD[10:])]
    for case in cases():
        (n, c, h, w), k, (r, s), st, (ph, pw) = case["x"], case["k"], case["f"], case["stride"], case["pad"]
        if case["mode"] == "f32" and not case.get("accumulate"):
            fixed.append((case["id"], (n, c, h, w, k, r, s, st, ph, pw), tuple(case.get("dy_hw") or (0, 0))))
    for pas, family in _grad_plan_combos():
        rng = np.random.default_rng(219)
        draws = [("random%d" % i, _random_geometry(rng, **_grad_draw_weights(pas, family)), (0, 0)) for i in range(2400)]
        seen, refused = [], 0
        for src, geo, out_hw in fixed + draws:
            n, c, h, w, k, r, s, st, ph, pw = geo
            if pas == GRAD_DGRAD_S2 and st != 2 and not src.startswith("random"):
                continue                                                    # (a random draw's stride is not looked at by this pass)
            if pas != GRAD_WGRAD or family == FAM_CONV16:
                out_hw = (0, 0)
            valid = h + 2 * ph >= r and w + 2 * pw >= s                        # (below that the mirrors' floor division is not C's)
            for acc in ((False,) if pas == GRAD_WGRAD else (False, True)):
                want = _grad_plan_of_mirror(pas, family, geo, out_hw, acc) if valid else None
                if want is None and not acc:
                    refused += src.startswith("random")
                if not valid:
                    continue
                got = _grad_plan_of_library(pas, family, geo, out_hw, acc)
                assert (got is None) == (want is None), (src, pas, family, geo, got, want)
                if want is not None:
                    assert got == {name: want[name] for name in got}, (src, pas, family, geo, acc, got, want)
                    seen.append(want)
        assert refused <= 2400 // 2, (pas, family, refused)

        def values(name):
            return {pl[name] for pl in seen}
        labels = set().union(*(pl.get("labels", set()) for pl in seen))
        if pas == GRAD_DGRAD:
            assert labels == CONV_ROUTE_LABELS["dgrad"], sorted(labels)
            assert values("zero_dst") == {0, 1} and values("scalar") == {0, 1} and values("bn") == {128, 64, 32}
            assert {pl["gy"] for pl in seen if pl["parity"]} == {1, 2, 4} and {pl["ks"] > 1 for pl in seen} == {False, True}
            assert len({pl["parity_order"] for pl in seen if pl["parity"]}) > 2
        elif pas == GRAD_DGRAD_S2:
            assert values("zero_dst") == {0, 1} and values("n_launch") >= {1, 4}
            if family == FAM_CONV16:
                assert {row[9] > 0 for pl in seen for row in pl["launches"]} == {True}
        else:
            assert {pl["splits"] > 1 for pl in seen} == {False, True}
            if family == MATH_F32:
                assert labels == CONV_ROUTE_LABELS["wgrad"], sorted(labels)
                assert {(pl["bm"], pl["bn"]) for pl in seen} == {(128, 128), (128, 32), (32, 128), (32, 32)}
                assert values("pipe") == {0, 1, 3} and values("a_scalar") == {0, 1} and values("b_scalar") == {0, 1}
            else:
                assert {(pl["bm"], pl["bn"]) for pl in seen} == ({(256, 256), (256, 128)} if family == FAM_CONV16 else {(128, 128)})


def test_refused_gradient_calls_say_what_they_said(golden_dir):
    """tests/golden/conv_grad_refusals.json: the error text of refused gradient (and conv16 forward) calls — every refusal branch of
    every entry point whose host code moved to the plans — recorded from the library before they existed.  Dummy non-null
    pointers: a refused call returns before it touches a device."""
    import json
    import os
    from helpers import refused_call
    with open(os.path.join(golden_dir, "conv_grad_refusals.json")) as fh:
        recorded = json.load(fh)
    assert len(recorded) >= 36
    for rec in recorded:
        rc, text = refused_call(rec["entry"], rec["ints"], rec["null"])
        assert rc != 0 and text == rec["text"], (rec, rc, text)


def test_s2_parity_pads_rule_is_the_plans_padding_refusal():
    """ops._s2_parity_pads_ok (which keeps a layer off rr_conv_dgrad_s2_* / rr_conv16_dgrad_s2) says no exactly where
    dgrad_s2_plan refuses for its padding, for all r, s <= 7 and pads <= 3, in each of the three families."""
    from helpers import FAM_CONV16, GRAD_DGRAD_S2, MATH_BF16, MATH_F16X3
    from rrnet_amd import _C, ops
    n_no = 0
    for family in (MATH_BF16, MATH_F16X3, FAM_CONV16):
        for r in range(1, 8):
            for s in range(1, 8):
                for ph in range(4):
                    for pw in range(4):
                        if family == FAM_CONV16 and r * s > 16:
                            continue                                        # (refused for its shape before the padding is looked at)
                        got = _grad_plan_of_library(GRAD_DGRAD_S2, family, (2, 128, 32, 32, 128, r, s, 2, ph, pw))
                        assert (got is not None) == ops._s2_parity_pads_ok(r, s, (ph, pw)), (family, r, s, ph, pw)
                        if got is None:
                            n_no += 1
                            assert _C.lib().rr_last_error().decode() == "rr_conv_grad_plan: unsupported padding %d,%d" % (ph, pw)
    assert n_no > 100


def test_conv_gpu_shapes_reach_every_gradient_plan_label():
    """The shapes the GPU tests run — CONV64_GRID and CONV64_ASYM_WGRAD (tests/test_conv_fp64_gpu.py), CONV16_GRID and
    CONV16_ASYM_WGRAD in both arithmetics (tests/test_conv_lowp_fp64_gpu.py), SHAPES of tests/test_conv16_gpu.py — reach every
    label the gradient plans can name, per pass and family, as the library's own plans (rr_conv_grad_plan) name them."""
    from helpers import (CONV16_ASYM_WGRAD, CONV16_GRID, CONV64_ASYM_WGRAD, CONV64_GRID, FAM_CONV16, GRAD_DGRAD, GRAD_DGRAD_S2, GRAD_WGRAD,
                         MATH_BF16, MATH_F16X3, MATH_F32)
    from rrnet_amd import _C
    from test_conv16_gpu import SHAPES

    def labels(pas, family, pl):
        if pas == GRAD_DGRAD:
            lab = {"bn%d" % pl["bn"]} | ({"scalar"} if pl["scalar"] else set()) | ({"ksplit>1"} if pl["ks"] > 1 else set())
            lab |= {"zero fill" if pl["zero_dst"] else "no zero fill"}
            return lab | ({"parity4" if pl["gy"] == 4 else "parity_live<4"} if pl["parity"] else set())
        if pas == GRAD_DGRAD_S2:
            lab = {"zero fill" if pl["zero_dst"] else "no zero fill", "4 launches" if pl["n_launch"] == 4 else "fewer launches"}
            return lab | {"ragged classes"} if len({row[6:8] for row in pl["launches"]}) > 1 else lab
        lab = {"splits>1" if pl["splits"] > 1 else "one split", "%dx%d" % (pl["bm"], pl["bn"])}
        if family == MATH_F32:
            lab = {"splits>1"} & lab | {"pipe%d" % pl["pipe"] if pl["pipe"] else "%dx%d" % (pl["bm"], pl["bn"])}
            lab |= {name for name in ("a_scalar", "b_scalar") if pl[name]}
        return lab
    seen = {combo: set() for combo in _grad_plan_combos()}

    def run(pas, family, geo, out_hw=(0, 0), accs=(False,)):
        for acc in accs:
            pl = _grad_plan_of_library(pas, family, geo, out_hw, acc)
            assert pl is not None, (pas, family, geo, _C.lib().rr_last_error())
            seen[pas, family] |= labels(pas, family, pl)
    for cfg in CONV64_GRID:                                                      # test_conv_fp64_gpu.py: rr_conv_dgrad / rr_conv_wgrad
        if "d" in cfg[13]:
            run(GRAD_DGRAD, MATH_F32, cfg[:10], accs=(False, True))
        if "w" in cfg[13]:
            run(GRAD_WGRAD, MATH_F32, cfg[:10])
    run(GRAD_WGRAD, MATH_F32, CONV64_ASYM_WGRAD[:10], CONV64_ASYM_WGRAD[10:])
    for family in (MATH_BF16, MATH_F16X3):                                       # test_conv_lowp_fp64_gpu.py
        for cfg in CONV16_GRID:
            if "d" in cfg[13] and cfg[7] == 2:
                run(GRAD_DGRAD_S2, family, cfg[:10], accs=(False, True))
            if "w" in cfg[13]:
                run(GRAD_WGRAD, family, cfg[:10])
        run(GRAD_WGRAD, family, CONV16_ASYM_WGRAD[:10], CONV16_ASYM_WGRAD[10:])
    for n, c, h, w, k, r, st in SHAPES:                                          # test_conv16_gpu.py, under its own conditions
        geo = (n, c, h, w, k, r, r, st, r // 2, r // 2)
        if st == 2 and k % 64 == 0 and c % 128 == 0:
            run(GRAD_DGRAD_S2, FAM_CONV16, geo, accs=(False, True))
        if k % 128 == 0 and c % 128 == 0 and r * r <= 64:
            run(GRAD_WGRAD, FAM_CONV16, geo)
    s2 = {"zero fill", "no zero fill", "4 launches", "fewer launches", "ragged classes"}
    want = {(GRAD_DGRAD, MATH_F32): {"bn128", "bn64", "bn32", "scalar", "ksplit>1", "parity4", "parity_live<4", "zero fill", "no zero fill"},
            (GRAD_WGRAD, MATH_F32): {"pipe3", "pipe1", "128x128", "128x32", "32x128", "32x32", "a_scalar", "b_scalar", "splits>1"},
            (GRAD_WGRAD, MATH_BF16): {"128x128", "splits>1", "one split"}, (GRAD_WGRAD, MATH_F16X3): {"128x128", "splits>1", "one split"},
            (GRAD_WGRAD, FAM_CONV16): {"256x256", "256x128", "splits>1", "one split"},
            (GRAD_DGRAD_S2, MATH_BF16): s2, (GRAD_DGRAD_S2, MATH_F16X3): s2, (GRAD_DGRAD_S2, FAM_CONV16): s2}
    missing = {combo: sorted(want[combo] - seen[combo]) for combo in want if want[combo] - seen[combo]}
    assert not missing, "gradient-plan labels no GPU test shape reaches (pass, family): %s" % missing
    assert all(seen[combo] <= want[combo] for combo in want), seen


# ---- the data-gradient selector (ops.dgrad_route) against the recorded launches (tests/golden/conv_bwd_routes.json) -----------
def test_dgrad_route_names_the_kernel_each_recorded_call_launched(golden_dir):
    """For every conv_dgrad case of tests/conv_route_cases.py, ops.dgrad_route — asked with shapes and the link's facts only, the
    device asserted, no tensor in sight — names the route whose entry point is the last launch of that case's record, taken on an
    MI355X from the dispatch that preceded it; its arithmetic is the one the entry point's suffix says; ops.dgrad16_takes agrees."""
    import json
    import os
    from conv_route_cases import cases, configured, dy_shape
    from rrnet_amd import ops
    with open(os.path.join(golden_dir, "conv_bwd_routes.json")) as fh:
        golden = json.load(fh)
    entry_route = {"rr_conv16_dgrad_s1_relumask": ("relumask", 1), "rr_head_dgrad_relubias": ("head", 0), "rr_conv16_dgrad_s1": ("conv16_s1", 1),
                   "rr_conv16_dgrad_s2": ("conv16_s2", 1), "rr_conv_dgrad_s2_bf16": ("parity_s2", 1), "rr_conv_dgrad_s2_f16x3": ("parity_s2", 2),
                   "rr_conv_dgrad": ("dgrad", 0)}
    for stem, label in (("rr_conv_dgrad_s1_relubias", "relubias"), ("rr_conv_dgrad_s1_bnsum", "fprop_bnsum"), ("rr_conv_dgrad_s1", "fprop")):
        for math, sfx in enumerate(("", "_bf16", "_f16x3")):
            entry_route[stem + sfx] = (label, math)
    seen = set()
    for case in cases():
        if case["op"] != "dgrad":
            continue
        want = entry_route[golden[case["id"]][-1][1]]
        n, c, h, w = case["x"]
        shapes = (dy_shape(case), (case["k"], c) + tuple(case["f"]), tuple(case["x"]), case["stride"], tuple(case["pad"]))
        link = {"bn_z": "bn"}.get(case["link"], case["link"])
        with configured(ops, case):
            got = ops.dgrad_route(*shapes, link, bool({"y", "z"} & set(case["b16"])), link is not None, True)
            takes = ops.dgrad16_takes(*shapes, relu_bias_link=link in ("relu_bias", "mask_only"))
        assert got == want, (case["id"], got, want)
        assert takes == (want[0] in ("conv16_s1", "conv16_s2")), case["id"]
        seen.add(want[0])
    assert seen == {"relumask", "head", "relubias", "conv16_s1", "fprop_bnsum", "fprop", "conv16_s2", "parity_s2", "dgrad"}


# ---- the bf16 / f16x3 convolution checks (tests/test_conv_lowp_fp64_gpu.py): routes, references, acceptance rule ------------------
def test_conv16_grid_reaches_every_route():
    """helpers.CONV16_GRID, CONV16_LINKS and CONV16_ASYM_WGRAD reach every label of helpers.CONV16_ROUTE_LABELS in both 16-bit
    arithmetics.  The labels come from helpers._fprop_route, and for every forward-kernel launch of the grid — forward pass,
    stride-1 data gradient with and without a link, each parity class of a stride-2 one — the library's own plan
    (rr_conv_fprop_plan) equals that mirror field by field; the combinations the grid was laid out for are there."""
    import ctypes
    from helpers import (CONV16_GRID, CONV16_LINKS, CONV16_ROUTE_LABELS, CONV_PLAN_FIELDS, MATH_BF16, MATH_F16X3, _fprop_route, _parity_launches,
                         conv16_case_labels, conv16_grid_labels)
    from rrnet_amd import _C
    plan_fn = _C.fn("rr_conv_fprop_plan")
    buf = (ctypes.c_int * len(CONV_PLAN_FIELDS))()
    link_code = {None: 0, "bn": 1, "relu_bias": 2}

    def same_plan(math, geo, bias=False, relu=False, ws=False, strided=False, link=None, out_hw=None):
        n, c, h, w, k, r, s, st, ph, pw = geo
        want = _fprop_route(n, c, h, w, k, r, s, st, ph, pw, bias, relu, ws, math, strided, link, False, out_hw)
        flags = bias | relu << 1 | ws << 2 | strided << 4 | link_code[link] << 8
        assert plan_fn(math, n, h, w, c, k, r, s, st, ph, pw, *(out_hw or (0, 0)), flags, buf) == 0 and want is not None, (math, geo)
        assert dict(zip(CONV_PLAN_FIELDS, buf)) == {name: want[name] for name in CONV_PLAN_FIELDS}, (math, geo, list(buf), want)
        return want
    for math in (MATH_BF16, MATH_F16X3):
        seen = conv16_grid_labels(math)
        missing = sorted(CONV16_ROUTE_LABELS[math] - seen)
        assert not missing, "math %d: route labels no case reaches: %s" % (math, missing)
        combos = []
        for cfg in CONV16_GRID:
            n, c, h, w, k, r, s, st, ph, pw, bias, relu, stats, passes = cfg
            p, q = (h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1
            for ws in stats:
                same_plan(math, cfg[:10], bias, relu, ws)
                combos.append(conv16_case_labels(math, cfg, ws)["fprop"])
            if "d" in passes and st == 1:
                same_plan(math, (n, k, p, q, c, r, s, 1, r - 1 - ph, s - 1 - pw))
            if "d" in passes and st == 2:
                sizes = set()
                for _, rc, sc, lh, lw, hc, wc, _ in _parity_launches(h, w, r, s, ph, pw)[0]:
                    pl = same_plan(math, (n, k, p, q, c, rc, sc, 1, lh, lw), strided=True, out_hw=(hc, wc))
                    assert pl["ks"] == 1 and not pl["zero_dst"]
                    sizes.add((hc, wc))
                if (n, c, h, w, k) == (2, 256, 79, 81, 16):
                    assert len(sizes) == 4                                   # four classes of four different sizes
        for (n, c, h, w), k, link, _ in CONV16_LINKS:
            pl = same_plan(math, (n, k, h, w, c, 3, 3, 1, 1, 1), link=link)
            assert n * h * w % 128 == 0 and (pl["after"] == 2) == (pl["ks"] > 1)
        for want in ({"bn32", "ksplit>1+stats", "xcd_n"}, {"bn32", "ragged M", "xcd_off,tiles>1"}, {"bn64", "xcd_off,tiles>1", "ksplit>1"},
                     {"bn128", "xcd_n", "ksplit>1+stats"}, {"bn128", "ragged filter tile", "fused stats"}, {"partial K-step", "C%8: image refused"},
                     {"bn32", "bias+relu", "fused stats"}, {"stride 2", "ragged M"}):
            assert any(want <= cmb for cmb in combos), (math, want)
        # bias / ReLU keep split-K off on a shape that would otherwise split
        assert not any("bias+relu" in cmb and ("ksplit>1" in cmb or "ksplit>1+stats" in cmb) for cmb in combos)
        assert _fprop_route(1, 256, 10, 10, 256, 3, 3, 1, 1, 1, False, False, False, math)["ks"] > 1


def test_lowp_references_are_what_they_claim():
    """helpers.lowp_image / lowp_fprop_ref64 / lowp_grads_ref64 / lowp_terms on one small strided shape with bias and one stride-1
    shape: the f16x3 forward reference IS oracle.split.conv2d; the f16x3 gradient references equal conv_ref64 on hi + lo up to the
    dropped lo*lo term, bounded by the same convolution of |lo| with |lo|; the bf16 references equal conv_ref64 on operands
    rounded by torch; the gathered products add up to the references; the scale follows the word it is given."""
    import numpy as np
    import torch
    from oracle import split as osp
    from helpers import (LOWP_PAIRS, MATH_BF16, MATH_F16X3, conv_ref64, lowp_fprop_ref64, lowp_grads_ref64, lowp_image, lowp_terms)
    for n, c, h, w, k, r, s, st, ph, pw in ((2, 8, 7, 9, 12, 3, 3, 2, 1, 1), (1, 12, 6, 5, 8, 3, 2, 1, 1, 0)):
        rng = np.random.default_rng(h)
        p, q = (h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1
        x = torch.from_numpy((rng.standard_normal((n, c, h, w)) * 3e-3).astype(np.float32))
        wt = torch.from_numpy((rng.standard_normal((k, c, r, s)) * 0.05).astype(np.float32))
        gy = torch.from_numpy((rng.standard_normal((n, k, p, q)) * 40.0).astype(np.float32))
        b = torch.from_numpy(rng.standard_normal(k).astype(np.float32) * 1e-4)
        base = rng.standard_normal((k, c, r, s)) * 1e-2
        for math in (MATH_BF16, MATH_F16X3):
            xi, wi, gi = (lowp_image(math, t) for t in (x, wt, gy))
            y = lowp_fprop_ref64(math, xi, wi, b, st, (ph, pw), False)
            dx, dw = lowp_grads_ref64(math, xi, wi, gi, st, (ph, pw))
            if math == MATH_BF16:
                rd = lambda t: t.to(torch.bfloat16).float()
                y0, dx0, dw0 = conv_ref64(rd(x), rd(wt), b, st, (ph, pw), False, rd(gy))
                for got, ref in ((y, y0), (dx, dx0), (dw, dw0)):
                    assert float((got - ref).abs().max()) <= 1e-14 * float(ref.abs().max())
            else:
                y0 = osp.conv2d(x.numpy(), wt.numpy(), st, (ph, pw)) + b.double().numpy()[None, :, None, None]
                assert np.abs(y.numpy() - y0).max() <= 1e-14 * np.abs(y0).max()
                for (parts, sc), t in ((xi, x), (wi, wt), (gi, gy)):
                    assert float(sc) == float(osp.scale_of(osp.absmax_bits(t.numpy()))) and 2.0 ** 14 <= np.abs(parts[0]).max() <= 2.0 ** 15
                    assert np.abs((parts[0] + parts[1]) / sc - t.double().numpy()).max() <= 2.0 ** -21 * float(t.abs().max())
                full = lambda im: torch.from_numpy((im[0][0] + im[0][1]) / im[1])
                lo = lambda im: torch.from_numpy(np.abs(im[0][1]) / im[1])
                _, dx1, dw1 = conv_ref64(full(xi), full(wi), None, st, (ph, pw), False, full(gi))
                _, bx, bw = conv_ref64(lo(xi), lo(wi), None, st, (ph, pw), False, lo(gi))          # sum |lo| |lo|: the dropped term at most
                assert bool(((dx - dx1).abs() <= bx * (1 + 1e-9) + 1e-14 * dx1.abs().max()).all()) and 0 < float(bx.max()) < 1e-5 * float(dx1.abs().max())
                assert bool(((dw - dw1).abs() <= bw * (1 + 1e-9) + 1e-14 * dw1.abs().max()).all()) and 0 < float(bw.max()) < 1e-5 * float(dw1.abs().max())
                # ... and the dropped term is exactly what is missing
                ddx, ddw = lowp_grads_ref64(math, xi, wi, gi, st, (ph, pw), pairs=((1, 1),))
                assert float((dx + ddx - dx1).abs().max()) <= 1e-14 * float(dx1.abs().max())
                assert float((dw + ddw - dw1).abs().max()) <= 1e-14 * float(dw1.abs().max())
                # the scale is the given word's: a tensor whose maximum is infinite keeps no finite value
                parts, sc = lowp_image(math, x, bits=0x7f800000)
                assert float(sc) == 2.0 ** -114 and not parts[0].any() and not parts[1].any()
            for kind, ref, a, bb, kw in (("fprop", y, xi, wi, dict(bias=b)), ("dgrad", dx, gi, wi, {}), ("wgrad", dw + torch.from_numpy(base), xi, gi, dict(rs=(r, s), base=base))):
                idx = np.unravel_index(np.arange(ref.numel()), tuple(ref.shape))
                chunks = list(lowp_terms(math, kind, idx, a, bb, st, (ph, pw), **kw))
                per = {"fprop": c * r * s, "dgrad": k * r * s, "wgrad": n * p * q}[kind] + 1
                assert all(t.shape[1] == per * len(LOWP_PAIRS[math]) for t in chunks)
                tot = np.concatenate([t.sum(1) for t in chunks])
                assert np.abs(tot - ref.numpy().ravel()).max() <= 1e-13 * float(ref.abs().max()), (math, kind)
                if kind == "dgrad":                                     # (no bias, no base:) every product is exact in float32
                    assert all(np.array_equal(t.astype(np.float32).astype(np.float64), t) for t in chunks)


def test_lowp_acceptance_rule_rejects_modelled_kernel_faults():
    """On three helpers.CONV16_GRID shapes the rule of tests/test_conv_lowp_fp64_gpu.py (conv_accepts at CONV_MARGIN_CAP, against the
    chained-float32 yardstick of the image products) ACCEPTS a faithful numpy model — the image products added in float32, pairwise
    — and REJECTS a model of each of these faults, everything else summed exactly in float64: f16x3 without the hi*lo term; a bf16
    operand left unrounded; one rounded twice (to 12 significant bits, then to bf16: the values next to a tie move); the last
    K-step of 32 channels — where C % 32 != 0, the partial one — skipped; two 32-column tiles swapped; one parity class of a
    stride-2 data gradient left at the value the accumulating call found there."""
    import numpy as np
    import torch
    from helpers import (CONV16_GRID, CONV_MARGIN_CAP, MATH_BF16, MATH_F16X3, bf16_exact, conv_accepts, conv_error_ratios, conv_sample_positions,
                         conv_yardstick, lowp_fprop_ref64, lowp_grads_ref64, lowp_image, lowp_terms, round_sig_bits)
    ran = {}
    for gi_ in (1, 6, 13):
        n, c, h, w, k, r, s, st, ph, pw = CONV16_GRID[gi_][:10]
        rng = np.random.default_rng(90 + gi_)
        p, q = (h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1
        x = rng.standard_normal((n, c, h, w)).astype(np.float32)
        wt = (rng.standard_normal((k, c, r, s)) / np.sqrt(c * r * s)).astype(np.float32)
        gy = rng.standard_normal((n, k, p, q)).astype(np.float32)
        base = rng.standard_normal((n, c, h, w)).astype(np.float32)
        for math in (MATH_BF16, MATH_F16X3):
            xi, wi, gim = (lowp_image(math, t) for t in (x, wt, gy))
            y = lowp_fprop_ref64(math, xi, wi, None, st, (ph, pw), False).numpy()
            idx = conv_sample_positions(y.shape, 3)
            terms = np.concatenate(list(lowp_terms(math, "fprop", idx, xi, wi, st, (ph, pw))))
            ref_s, max_seq, rms_seq = conv_yardstick([terms])
            assert 0 < rms_seq < max_seq and np.abs(ref_s - y[idx]).max() <= 1e-12 * np.abs(y).max()

            def verdict(name, got_s, got_all=None, want=False, ref_all=y, ref_at=ref_s, yard=(max_seq, rms_seq)):
                ok = conv_accepts(conv_error_ratios(got_s, ref_at, *yard, got_all, None if got_all is None else ref_all), CONV_MARGIN_CAP)
                assert ok == want, (gi_, math, name, float(np.abs(got_s - ref_at).max()), yard)
                ran[name] = ran.get(name, 0) + 1
            verdict("faithful", np.sum(terms.astype(np.float32), axis=1, dtype=np.float32).astype(np.float64), want=True)
            exact = lambda a, b, **kw: np.concatenate([t.sum(1) for t in lowp_terms(math, "fprop", idx, a, b, st, (ph, pw), **kw)])
            if math == MATH_F16X3:
                verdict("no hi*lo", exact(xi, wi, pairs=((0, 0), (1, 0))))
            else:
                raw = ((x.astype(np.float64),), np.float64(1.0))
                twice = ((bf16_exact(round_sig_bits(x, 12).astype(np.float32)).astype(np.float64),), np.float64(1.0))
                assert 0 < np.mean(twice[0][0] != xi[0][0]) < 0.2
                verdict("unrounded operand", exact(raw, wi))
                verdict("operand rounded twice", exact(twice, wi))
            cut = (c - 1) // 32 * 32                                            # first channel of the last K-step
            short = (tuple(np.where(np.arange(c)[None, :, None, None] < cut, part, 0.0) for part in xi[0]), xi[1])
            if cut > 0:
                verdict("last K-step skipped" + (" (partial)" if c % 32 else ""), exact(short, wi))
            if k >= 64:
                sw = y.copy()
                sw[:, 0:32], sw[:, 32:64] = y[:, 32:64], y[:, 0:32]
                verdict("column tiles swapped", sw[idx], sw)
            if st == 2:
                dx = lowp_grads_ref64(math, xi, wi, gim, st, (ph, pw))[0].numpy() + base.astype(np.float64)
                didx = conv_sample_positions(dx.shape, 4)
                dref, dmax, drms = conv_yardstick(lowp_terms(math, "dgrad", didx, gim, wi, st, (ph, pw), base=base))
                stale = dx.copy()
                stale[:, :, 1::2, 1::2] = base[:, :, 1::2, 1::2]
                verdict("stale parity class", stale[didx], stale, ref_all=dx, ref_at=dref, yard=(dmax, drms))
                verdict("faithful", dx[didx], dx, want=True, ref_all=dx, ref_at=dref, yard=(dmax, drms))
    assert set(ran) == {"faithful", "no hi*lo", "unrounded operand", "operand rounded twice", "last K-step skipped", "last K-step skipped (partial)",
                        "column tiles swapped", "stale parity class"}, ran
    assert all(v >= 2 for name, v in ran.items() if "partial" not in name and name != "last K-step skipped"), ran


# ---- the launch plans of the deformable convolutions (csrc/dcn_plan.h) ------------------------------------------------------------
_DCN_BENCH_LAYER = (8, 256, 256, 256, 256, 3, 3, 1, 1, 1, 1, 1)             # bench.py's config4 head layer


def _dcn_geo(cfg):
    """(N, C, H, W, K, ksize, stride, pad, dil, dg) of tests/test_dcn_gpu.py -> the geometry dcn_plan_mirror takes."""
    n, c, h, w, k, ks, stride, pad, dil, dg = cfg
    return (n, c, h, w, k, ks, ks, stride, pad, pad, dil, dg)


def _dcn_gpu_test_shapes():
    """test_dcn_gpu.CASES and the shapes of its other parametrised tests -> ([geometry of every CASES entry], [(test, geometry)])."""
    import test_dcn_gpu as t

    def params(fn):
        return [m.args[1] for m in fn.pytestmark if m.name == "parametrize"][0]
    others = [("bf16_dgrad", (n, c, h, w, k, 3, 3, 1, 1, 1, 1, dg)) for n, c, h, w, k, dg in params(t.test_dcn_bf16_dgrad_equals_fp32_dgrad_on_rounded_operands)]
    others += [("bf16_wgrad", (n, c, h, w, k, 3, 3, 1, 1, 1, 1, dg)) for n, c, h, w, k, dg, _ in params(t.test_dcn_bf16_wgrad_equals_gemm_of_rounded_operands)]
    others.append(("column_path", (2, 256, 24, 40, 256, 3, 3, 1, 1, 1, 1, 1)))
    return [_dcn_geo(cfg) for cfg in t.CASES], others


def _dcn_plan_of_library(pas, bf16, geo, margin, flags):
    """rr_dcn_plan -> {field: int} or None where the library refuses (a refusal must come with a reason)."""
    import ctypes
    from helpers import DCN_PLAN_FIELDS, DCN_PLAN_INTS
    from rrnet_amd import _C
    buf = (ctypes.c_int * DCN_PLAN_INTS)(*([-7] * DCN_PLAN_INTS))
    n, c, h, w, k, r, s, stride, ph, pw, dil, dg = geo
    rc = _C.fn("rr_dcn_plan")(pas, bf16, n, h, w, c, k, r, s, stride, ph, pw, dil, dg, margin, flags, buf, DCN_PLAN_INTS)
    if rc != 0:
        assert _C.lib().rr_last_error().decode().startswith("rr_dcn"), (geo, _C.lib().rr_last_error())
        return None
    names = DCN_PLAN_FIELDS[pas]
    own = names[8:]
    assert all(v == 0 for v in buf[8 + len(own):]), (pas, list(buf))
    return dict(zip(names, list(buf[:8]) + list(buf[8:8 + len(own)])))


def test_dcn_library_plans_equal_the_mirror():
    """rr_dcn_plan — the three plans of rrnet_amd/csrc/dcn_plan.h that every rr_dcn_* entry point launches from — equals
    helpers.dcn_plan_mirror, the Python restatement of the host code that preceded the header, field by field: for every entry of
    test_dcn_gpu.CASES, the shapes of its other parametrised tests, bench.py's config-4 layer, shapes at the 2 GiB / 2^30 / 32768
    limits and 2400 seeded random shapes (dilation 1-4; 3x3, 5x5 and 1x1 filters; stride 1 and 2; 1, 2 and 4 groups), in both
    precisions, with every flag combination an entry point can produce and at margins 0, 1, 2 and 3.  What the library refuses, the
    mirror refuses; fewer than half of the random draws are refused in any pass."""
    import numpy as np
    from helpers import DCN_DGRAD, DCN_ENTRY_FLAGS, DCN_FWD, DCN_PLAN_FIELDS, DCN_WGRAD, dcn_plan_mirror
    cases_geo, others = _dcn_gpu_test_shapes()
    shapes = [("case", g) for g in cases_geo] + others + [("bench", _DCN_BENCH_LAYER)]
    shapes += [("limit", g) for g in (
        (8, 64, 2048, 2048, 64, 3, 3, 1, 1, 1, 1, 1),          # x above 2 GiB: no window DMA, no dY DMA, no DMA sweep
        (1, 32, 32768, 16, 64, 3, 3, 1, 1, 1, 1, 1),           # h == 32768: the backward windows step aside
        (1, 32, 16, 32768, 64, 3, 3, 1, 1, 1, 1, 2),
        (1, 32, 40000, 30000, 64, 3, 3, 1, 1, 1, 1, 1),        # h * w >= 2^30: the forward window steps aside
        (2, 32, 40000, 30000, 64, 3, 3, 1, 1, 1, 1, 1),        # too many output pixels
        (4, 4, 30000, 20000, 64, 3, 3, 1, 1, 1, 1, 1),         # n * h * w >= 2^31: the data gradient refuses
        (1, 2048, 8, 16, 65536, 3, 3, 1, 1, 1, 1, 1),          # packed weights of 2 GiB and more
        (16, 32, 1024, 1024, 128, 3, 3, 1, 1, 1, 1, 1),        # dY's bf16 image of 2 GiB and more
        (1, 64, 2, 2, 64, 5, 5, 2, 0, 0, 1, 1),                # the filter does not fit (C divides towards zero)
        (1, 30, 9, 9, 64, 3, 3, 1, 1, 1, 1, 1), (1, 64, 9, 9, 64, 3, 3, 1, 1, 1, 1, 4), (1, 96, 9, 9, 30, 3, 3, 1, 1, 1, 1, 3))]
    rng = np.random.default_rng(355)
    chans, filts = (8, 16, 32, 64, 96, 128, 160, 256, 384, 512), (4, 12, 30, 32, 36, 64, 96, 132, 256, 260, 388, 512)
    for i in range(2400):
        ks = (3, 3, 3, 5, 1)[rng.integers(5)]
        shapes.append(("random%d" % i, (int(rng.integers(1, 5)), chans[rng.integers(10)], int(rng.integers(1, 71)), int(rng.integers(1, 71)),
                                        filts[rng.integers(12)], ks, ks, int(rng.integers(1, 3)), int(rng.integers(0, 4)), int(rng.integers(0, 4)),
                                        int(rng.integers(1, 5)), (1, 1, 2, 4)[rng.integers(4)])))
    n_random = sum(src.startswith("random") for src, _ in shapes)
    assert n_random >= 2000
    seen = {pas: set() for pas in (DCN_FWD, DCN_WGRAD, DCN_DGRAD)}
    refused_at_3 = dict.fromkeys(seen, 0)
    for src, geo in shapes:
        for pas in seen:
            for margin in (0, 1, 2, 3):
                for bf16 in (0, 1):
                    for flags in sorted({f for _, f in DCN_ENTRY_FLAGS[pas].values()}):
                        want = dcn_plan_mirror(pas, bf16, geo, margin, flags)
                        got = _dcn_plan_of_library(pas, bf16, geo, margin, flags)
                        if want is None or got is None:
                            assert want is None and got is None, (src, geo, pas, bf16, margin, flags, got, want)
                            continue
                        assert got == {name: want[name] for name in DCN_PLAN_FIELDS[pas]}, (src, geo, pas, bf16, margin, flags, got, want)
                        seen[pas] |= want["labels"]
            refused_at_3[pas] += src.startswith("random") and dcn_plan_mirror(pas, 0, geo, 3, 0) is None
    assert all(v < n_random // 2 for v in refused_at_3.values()), (refused_at_3, n_random)
    assert refused_at_3[DCN_FWD] < refused_at_3[DCN_WGRAD] <= refused_at_3[DCN_DGRAD]        # the forward refuses dimensions only
    assert seen[DCN_FWD] == {"window256", "window256+packed", "window256:k>384", "window256+packed:k>384", "window128", "gather128", "gather32",
                             "margin_shrunk"}
    assert seen[DCN_WGRAD] == {"window_f32", "window_bf16", "window_dy_dma", "gather"}
    assert seen[DCN_DGRAD] == {"window_f32", "window_bf16_fp32dy", "window_bf16_convert", "window_bf16_image", "window_dma", "gather"}
    # margin < 0 asks with the library's own margin (RR_DCN_WINDOW, 3 when unset)
    import os
    own = int(os.environ.get("RR_DCN_WINDOW", "3"))
    assert _dcn_plan_of_library(DCN_DGRAD, 1, _DCN_BENCH_LAYER, -1, 7) == _dcn_plan_of_library(DCN_DGRAD, 1, _DCN_BENCH_LAYER, own, 7)


def test_dcn_fused_bwd_supported_answers_as_recorded(golden_dir):
    """rr_dcn_fused_bwd_supported_dil — now "both backward plans of csrc/dcn_plan.h accept the shape" — answers exactly as the
    predicate it replaced did: tests/golden/dcn_bwd_supported.json holds that predicate's answers over 3360 layer shapes, recorded
    from the library of the commit before the header.  The same answers follow from the mirror's two backward plans."""
    import json
    import os
    import pytest
    from helpers import DCN_DGRAD, DCN_WGRAD, dcn_plan_mirror
    from rrnet_amd import _C
    if int(os.environ.get("RR_DCN_WINDOW", "3")) != 3:
        pytest.skip("the answers were recorded with the default window margin")
    with open(os.path.join(golden_dir, "dcn_bwd_supported.json")) as fh:
        doc = json.load(fh)
    ax = doc["axes"]
    assert doc["order"] == ["c", "k", "filter", "stride", "dilation", "groups"]
    fn = _C.fn("rr_dcn_fused_bwd_supported_dil")
    got, mirrored = [], []
    for c in ax["c"]:
        for k in ax["k"]:
            for f in ax["filter"]:
                for st in ax["stride"]:
                    for d in ax["dilation"]:
                        for g in ax["groups"]:
                            got.append(str(int(fn(c, k, f, f, st, d, g))))
                            geo = (1, c, d * (f - 1) + 1, d * (f - 1) + 1, k, f, f, st, 0, 0, d, g)
                            mirrored.append(str(int(all(dcn_plan_mirror(pas, 0, geo, 3) is not None for pas in (DCN_WGRAD, DCN_DGRAD)))))
    assert len(got) == 3360 == len(doc["answers"])
    assert "".join(got) == doc["answers"]
    assert "".join(mirrored) == doc["answers"]
    assert 0 < doc["answers"].count("1") < 3360
    assert _C.fn("rr_dcn_fused_bwd_supported")(64, 64, 3, 3, 1, 2) == fn(64, 64, 3, 3, 1, 1, 2) == 1


def test_dcn_gpu_shapes_reach_every_route():
    """Every route label the three plans can produce (helpers.DCN_ROUTE_LABELS, per operand precision) is reached by a call
    tests/test_dcn_gpu.py makes, with the flags that call's entry point hands its plan: CASES through functional.dcn_v2_conv in
    fp32 and in bf16 (forward packed; backward with dY's bf16 image, the data gradient packed — only where both backward plans
    accept the layer, the column path runs otherwise and the refusing plan counts as `refused`), and the shapes of the tests that
    call ops.dcn_dgrad / ops.dcn_wgrad directly.  The plans are the library's (equal to the mirror, as checked above)."""
    from helpers import (DCN_DGRAD, DCN_DYB_READY, DCN_FWD, DCN_HAS_DYB, DCN_HAS_WPACK, DCN_ROUTE_LABELS, DCN_WGRAD, dcn_plan_mirror)
    cases_geo, others = _dcn_gpu_test_shapes()
    seen = {(pas, bf): set() for pas in (DCN_FWD, DCN_WGRAD, DCN_DGRAD) for bf in (0, 1)}

    def call(pas, bf16, geo, flags):
        want = dcn_plan_mirror(pas, bf16, geo, 3, flags)
        assert (want is None) == (_dcn_plan_of_library(pas, bf16, geo, 3, flags) is None)
        return want
    img = DCN_HAS_DYB | DCN_DYB_READY
    for geo in cases_geo:
        for bf in (0, 1):
            seen[DCN_FWD, bf] |= call(DCN_FWD, bf, geo, DCN_HAS_WPACK if bf else 0)["labels"]
            plans = {DCN_WGRAD: call(DCN_WGRAD, bf, geo, img if bf else 0), DCN_DGRAD: call(DCN_DGRAD, bf, geo, (DCN_HAS_WPACK | img) if bf else 0)}
            fused = all(call(pas, 0, geo, 0) is not None for pas in plans)            # ops.dcn_fused_bwd_supported
            for pas, pl in plans.items():
                if pl is None:
                    seen[pas, bf].add("refused")
                elif fused:
                    seen[pas, bf] |= pl["labels"]
    for test, geo in others:
        if test == "bf16_dgrad":          # fp32, rr_dcn_dgrad_bf16_packed without an image, then rr_dcn_dgrad_bf16_ws
            seen[DCN_DGRAD, 0] |= call(DCN_DGRAD, 0, geo, 0)["labels"]
            seen[DCN_DGRAD, 1] |= call(DCN_DGRAD, 1, geo, DCN_HAS_WPACK | DCN_HAS_DYB)["labels"] | call(DCN_DGRAD, 1, geo, DCN_HAS_DYB)["labels"]
        elif test == "bf16_wgrad":        # rr_dcn_wgrad_bf16, rr_dcn_wgrad_bf16_img, rr_dcn_wgrad
            seen[DCN_WGRAD, 1] |= call(DCN_WGRAD, 1, geo, 0)["labels"] | call(DCN_WGRAD, 1, geo, img)["labels"]
            seen[DCN_WGRAD, 0] |= call(DCN_WGRAD, 0, geo, 0)["labels"]
        else:
            for pas in (DCN_FWD, DCN_WGRAD, DCN_DGRAD):
                seen[pas, 0] |= call(pas, 0, geo, 0)["labels"]
    for (pas, bf), labels in seen.items():
        missing = sorted(DCN_ROUTE_LABELS[pas][bf] - labels)
        assert not missing, "pass %d, %s: route labels no shape of test_dcn_gpu.py reaches: %s" % (pas, ("fp32", "bf16")[bf], missing)


# ---- the float64 pin of the deformable convolutions (tests/test_dcn_fp64_gpu.py): what helpers promises, checked on the CPU --------
_DCN64_HOST_SAMPLES = 1024          # the rule is the one the GPU test applies; fewer sampled outputs keep these tests quick


def test_dcn64_grid_reaches_every_route_and_entry_point():
    """helpers.DCN64_GRID through helpers.dcn64_entries — the calls tests/test_dcn_fp64_gpu.py makes — reaches every route label of
    DCN_ROUTE_LABELS (refusals excepted: they have their own test) in both operand precisions and every entry point of
    DCN_ENTRY_FLAGS, by the plan mirror and by the library's rr_dcn_plan alike; the shapes stay within the limits set for them."""
    import helpers as H
    seen = {(pas, bf): set() for pas in (H.DCN_FWD, H.DCN_WGRAD, H.DCN_DGRAD) for bf in (0, 1)}
    entries, splits, ktiles = set(), set(), set()
    for name, geo in H.DCN64_GRID.items():
        n, c, h, w, k, r, s, stride, ph, pw, dil, dg = geo
        assert n <= 2 and h <= 24 and w <= 24 and k in (12, 32, 36, 48, 64, 256, 260, 388), name
        p, q = H.dcn_out_hw(h, w, r, s, stride, ph, pw, dil)
        assert H._cdiv(p, 8) * H._cdiv(q, 16) >= 2 and (p % 8 or q % 16), name
        for pas, entry, bf, flags, labels in H.dcn64_entries(name):
            got = _dcn_plan_of_library(pas, bf, geo, 3, flags)
            want = H.dcn_plan_mirror(pas, bf, geo, 3, flags)
            assert got == {f: want[f] for f in H.DCN_PLAN_FIELDS[pas]}, (name, entry)
            seen[pas, bf] |= labels
            entries.add(entry)
            if pas == H.DCN_WGRAD:
                splits.add(want["splits"])
                ktiles.add(want["ktiles"])
    for (pas, bf), labels in seen.items():
        missing = sorted(H.DCN_ROUTE_LABELS[pas][bf] - labels - {"refused"})
        assert not missing, (pas, bf, missing)
    assert "window_bf16_fp32dy" in seen[H.DCN_DGRAD, 1]                          # rr_dcn_dgrad_bf16: fp32 dY converted while staging
    assert entries == {e for pas in H.DCN_ENTRY_FLAGS for e in H.DCN_ENTRY_FLAGS[pas]}
    assert len([v for v in splits if v > 1]) >= 2 and 2 in ktiles
    blocks = [H._cdiv(p_, 8) >= 2 and H._cdiv(q_, 16) >= 2 for p_, q_ in
              (H.dcn_out_hw(g[2], g[3], g[5], g[6], g[7], g[8], g[9], g[10]) for g in (H.DCN64_GRID[nm] for nm in H.DCN64_EDGE_CASES))]
    assert blocks[0]                                                             # the window edge case has at least 2 x 2 blocks
    print("entry points compared with float64:", sorted(entries))
    print("route labels compared with float64:", {k_: sorted(v) for k_, v in seen.items()})


def test_dcn_ref64_is_what_it_claims():
    """dcn_ref64: at zero offsets and unit mask it is float64 F.conv2d; on a tiny case it equals a plain Python loop over the definition
    (values and all gradients); helpers.dcn_model in float64 equals it on grouped, strided and dilated shapes, bf16 included; and the
    float64 bf16 image is round-to-nearest-even of the float64 value, not a double rounding through float32."""
    import numpy as np
    import torch.nn.functional as F
    import helpers as H
    from oracle import dcn as odcn
    g = torch.Generator().manual_seed(1)
    for stride, pad, dil in ((1, 1, 1), (2, 1, 1), (1, 2, 2)):
        x, wt, b = torch.randn(2, 8, 9, 11, generator=g), torch.randn(12, 8, 3, 3, generator=g), torch.randn(12, generator=g)
        p, q = H.dcn_out_hw(9, 11, 3, 3, stride, pad, pad, dil)
        ref = H.dcn_ref64(x, torch.zeros(2, 18, p, q), torch.ones(2, 9, p, q), wt, b, stride, pad, dil, 1)
        want = F.conv2d(x.double(), wt.double(), b.double(), stride=stride, padding=pad, dilation=dil).numpy()
        assert np.abs(ref["out"] - want).max() <= 1e-13
    # a plain loop over the definition: N=1, C=2, 4x5, K=2, 3x3, pad 1
    n, c, h, w, k = 1, 2, 4, 5, 2
    x, off, mask = torch.randn(n, c, h, w, generator=g), torch.randn(n, 18, h, w, generator=g) * 1.5, torch.rand(n, 9, h, w, generator=g)
    wt, b, gy = torch.randn(k, c, 3, 3, generator=g), torch.randn(k, generator=g), torch.randn(n, k, h, w, generator=g)
    ref = H.dcn_ref64(x, off, mask, wt, b, 1, 1, 1, 1, gy=gy)
    X, O, M, W_, G = (t.double().numpy() for t in (x, off, mask, wt, gy))
    out, dx, doff, dm, dw = np.zeros((n, k, h, w)), np.zeros(X.shape), np.zeros(O.shape), np.zeros(M.shape), np.zeros(W_.shape)
    for pp in range(h):
        for qq in range(w):
            for tap in range(9):
                i, j = divmod(tap, 3)
                hp = float(np.float32(pp - 1 + i) + np.float32(O[0, 2 * tap, pp, qq]))
                wp = float(np.float32(qq - 1 + j) + np.float32(O[0, 2 * tap + 1, pp, qq]))
                if not (hp > -1 and wp > -1 and hp < h and wp < w):
                    continue
                h0, w0 = int(np.floor(hp)), int(np.floor(wp))
                lh, lw = hp - h0, wp - w0
                for hy, wx, wg, gh, gw in ((h0, w0, (1 - lh) * (1 - lw), -(1 - lw), -(1 - lh)), (h0, w0 + 1, (1 - lh) * lw, -lw, 1 - lh),
                                           (h0 + 1, w0, lh * (1 - lw), 1 - lw, -lh), (h0 + 1, w0 + 1, lh * lw, lw, lh)):
                    if not (0 <= hy <= h - 1 and 0 <= wx <= w - 1):
                        continue
                    for ch in range(c):
                        for ko in range(k):
                            gcol = G[0, ko, pp, qq] * W_[ko, ch, i, j]
                            out[0, ko, pp, qq] += W_[ko, ch, i, j] * M[0, tap, pp, qq] * wg * X[0, ch, hy, wx]
                            dw[ko, ch, i, j] += G[0, ko, pp, qq] * M[0, tap, pp, qq] * wg * X[0, ch, hy, wx]
                            dx[0, ch, hy, wx] += gcol * M[0, tap, pp, qq] * wg
                            dm[0, tap, pp, qq] += gcol * wg * X[0, ch, hy, wx]
                            doff[0, 2 * tap, pp, qq] += gcol * M[0, tap, pp, qq] * gh * X[0, ch, hy, wx]
                            doff[0, 2 * tap + 1, pp, qq] += gcol * M[0, tap, pp, qq] * gw * X[0, ch, hy, wx]
    out += b.double().numpy().reshape(1, -1, 1, 1)
    for name, a in (("out", out), ("dx", dx), ("doffset", doff), ("dmask", dm), ("dw", dw)):
        assert np.abs(ref[name] - a).max() <= 1e-12 * max(1.0, np.abs(a).max()), name
    assert np.abs(ref["db"] - G.sum((0, 2, 3))).max() <= 1e-12
    # helpers.dcn_model (the corner-by-corner numpy model the yardstick, the allowances and the modelled faults use) in float64
    for name, bf in (("g2", 0), ("stride2", 1), ("dil2", 1), ("k64", 0)):
        geo = H.DCN64_GRID[name]
        ins = H.dcn_edge_inputs("gauss", geo, 5)
        args = ins[:5] + (geo[7], (geo[8], geo[9]), geo[10], geo[11])
        ref = H.dcn_ref64(*args, gy=ins[5], bf16=bool(bf))
        mod = H.dcn_model(*args, gy=ins[5], bf16=bool(bf))
        for tensor in ("out", "dx", "doffset", "dmask", "dw", "db"):
            assert np.abs(ref[tensor] - mod[tensor]).max() <= 1e-12 * max(1.0, np.abs(ref[tensor]).max()), (name, tensor)
        assert np.abs(ref["cols"] - mod["col"]).max() <= 1e-13 * np.abs(ref["cols"]).max()
    # the bf16 image of a float64 value: 1 + 2^-8 + 2^-30 lies ABOVE the tie between 1 and 1 + 2^-7; float32 rounds it onto the tie
    v = 1.0 + 2.0 ** -8 + 2.0 ** -30
    assert float(torch.tensor([v], dtype=torch.float64).float().bfloat16()) == 1.0           # the double rounding this must not be
    assert float(odcn._bf16_round(torch.tensor([v], dtype=torch.float64))[0]) == 1.0 + 2.0 ** -7 == float(H.bf16_rne64(np.array([v]))[0])
    assert float(H.bf16_rne64(np.array([1.0 + 2.0 ** -8]))[0]) == 1.0 and float(H.bf16_rne64(np.array([1.0 + 3 * 2.0 ** -8]))[0]) == 1.0 + 2.0 ** -6
    a = np.random.default_rng(3).standard_normal(20000) * 10.0 ** np.random.default_rng(4).integers(-6, 7, 20000)
    q = H.bf16_rne64(a)
    assert (q == H.bf16_exact(q.astype(np.float32))).all()                                   # bf16 values
    ulp = 2.0 * H.bf16_half_ulp(q)
    assert (np.abs(a - q) <= np.minimum(np.abs(a - (q + ulp)), np.abs(a - (q - ulp)))).all() and (np.abs(a - q) <= 0.5 * ulp).all()
    assert (odcn._bf16_round(torch.from_numpy(a)).numpy() == q).all()


def test_dcn_edge_classes_hold_what_they_claim():
    """Every seeded edge class of helpers.dcn_edge_inputs contains what it claims, counted from the float64 geometry, on both shapes
    the GPU test runs them on (one window route, one gather route)."""
    import numpy as np
    import helpers as H
    for name in H.DCN64_EDGE_CASES:
        geo = H.DCN64_GRID[name]
        n, c, h, w, k, r, s, stride, ph, pw, dil, dg = geo
        plan = H.dcn_plan_mirror(H.DCN_DGRAD, 0, geo, 3, 0)
        margin = plan["margin"] if plan["window"] else 3
        res = {}
        for cls in H.DCN_EDGE_CLASSES:
            x, off, mask, wt, b, gy = H.dcn_edge_inputs(cls, geo, 11, margin)
            g_ = H.dcn_geometry(off, h, w, r, s, stride, (ph, pw), dil, dg)
            res[cls] = (g_, x, off, mask, gy)
            assert torch.isfinite(off).all()
        hw = {"h": h, "w": w}
        g_ = res["gauss"][0]
        assert 0.5 < g_["inside"].mean() < 1.0 and np.abs(res["gauss"][2].std().item() - 1.5) < 0.1
        # border band: every sample of a border output pixel in (-1, 0) / (H - 1, H); partial footprints; both at the corners
        g_ = res["border"][0]
        p, q = g_["inside"].shape[-2:]
        assert ((g_["h"][..., 0, :] > -1) & (g_["h"][..., 0, :] < 0)).all() and ((g_["h"][..., p - 1, :] > h - 1) & (g_["h"][..., p - 1, :] < h)).all()
        assert ((g_["w"][..., 0] > -1) & (g_["w"][..., 0] < 0)).all() and ((g_["w"][..., q - 1] > w - 1) & (g_["w"][..., q - 1] < w)).all()
        nvalid = g_["valid"].sum(0)
        assert (nvalid[..., 0, 0] == 1).all() and (nvalid[..., p - 1, q - 1] == 1).all() and (nvalid[g_["inside"]] >= 1).all()
        assert ((nvalid == 2) & g_["inside"]).sum() >= 2 * 9 * (p + q - 4) // 2
        # exact positions: integers (offset 0 among them), exactly -1 and H / W, one float32 ulp inside each
        g_, off = res["exact"][0], res["exact"][2]
        counts = {}
        for ax in ("h", "w"):
            v, size = g_[ax], hw[ax]
            counts[ax] = {"integer": int(((v == np.floor(v)) & (v >= 0) & (v <= size - 1)).sum()), "-1": int((v == -1).sum()),
                          "size": int((v == size).sum()), "-1+ulp": int((v == np.nextafter(np.float32(-1), np.float32(0))).sum()),
                          "size-ulp": int((v == np.nextafter(np.float32(size), np.float32(0))).sum())}
            assert all(cnt >= 10 for cnt in counts[ax].values()), (name, counts)        # (one ulp inside is representable next to few grid positions)
        assert int((off == 0).sum()) >= 100
        assert (~g_["inside"] & ((g_["h"] == -1) | (g_["h"] == h) | (g_["w"] == -1) | (g_["w"] == w))).sum() >= 80
        # beyond the margin: in each of the four directions, corners off the window that are inside the image (the direct global path)
        # and corners outside it, from source pixels of blocks on the image border
        g_, off = res["beyond"][0], res["beyond"][2].numpy().reshape(n, dg, r * s, 2, p, q)
        inwin = H.dcn_in_window(g_, r, s, (ph, pw), dil, margin)
        for ax, sign in ((0, -1), (0, 1), (1, -1), (1, 1)):
            o = off[:, :, :, ax] * sign
            sel = (o >= margin + 1) & (o <= margin + 6)
            assert sel.sum() >= 0.08 * sel.size, (name, ax, sign)
            if stride == 1:
                assert (g_["valid"] & ~inwin & sel[None]).sum() >= 10 and (~g_["valid"] & ~inwin & sel[None]).sum() >= 10, (name, ax, sign)
        # far away: a few percent of the samples at +-1e4, +-3e9, +-1e30, all outside; the neighbours keep their Gaussian offsets
        g_, off = res["far"][0], res["far"][2].numpy()
        for val in (1e4, 3e9, 1e30):
            assert (off == np.float32(val)).sum() >= 5 and (off == np.float32(-val)).sum() >= 5
        big = (np.abs(off) >= 1e4).reshape(n, dg, r * s, 2, p, q).any(3)
        assert 0.02 <= big.mean() <= 0.08 and not g_["inside"][big].any() and (np.abs(off[np.abs(off) < 1e4]) < 10).all()
        # pile-up: every sample on ONE fractional position
        g_ = res["pile"][0]
        assert len(np.unique(g_["idx"][0])) == 1 and g_["inside"].all() and (g_["lh"] > 0.05).all() and (g_["lw"] > 0.05).all()
        assert np.ptp(g_["lh"]) < 1e-5 and np.ptp(g_["lw"]) < 1e-5
        # operands: masks with exact zeros, negative values and values above 1; 2^+-12 dynamic range across channels
        _, x, _, mask, gy = res["operands"]
        assert (mask == 0).float().mean() > 0.05 and (mask < 0).float().mean() > 0.2 and (mask > 1).float().mean() > 0.05
        for t in (x, gy):
            rms = t.square().mean((0, 2, 3)).sqrt()
            assert rms.max() / rms.min() >= 2.0 ** 20


def test_dcn_tie_conditions_and_allowance_share():
    """On the reference alone: in every bf16 grid case (and every edge class on the edge cases) at most 1 % of the outputs and of the dw
    elements hold more than DCN_TIE_MAX near-tie terms (they are left out) and at least a third of each tensor's sampled outputs hold
    none and take the plain rule; no float32-model column rounds differently from the float64 column outside the band.  The
    fixed-point allowance of the window data gradient is the contract's WORST case (every one of an element's ~15 hits rounds half a
    unit the same way, the unit sized for the block's ~50 hits on its busiest pixel): on Gaussian inputs it is below 2^-17 of the
    tensor's maximum, but it is no small share of an element's bound at the cap margin — measured 0.38 to 0.59 (about as much as
    8 x the chained float32 sum), asserted below 0.75; the flush part alone stays below a quarter of 8 x the yardstick (measured: 0.14 at most).  What keeps
    the allowance honest is the modelled fault below: a unit of 2^-20 of the bound is refused."""
    import numpy as np
    import helpers as H
    cases = [(nm, "gauss") for nm in H.DCN64_GRID] + [(nm, cls) for nm in H.DCN64_EDGE_CASES for cls in H.DCN_EDGE_CLASSES[1:]]
    for name, cls in cases:
        geo = H.DCN64_GRID[name]
        cs = H.DcnCase(geo, cls, 1, samples=_DCN64_HOST_SAMPLES)
        for tensor in ("out", "dw") if name not in H.DCN64_BF16_PASSES else ():    # (shapes whose bf16 forward / weight gradient do not run)
            keep, cnt = cs.tie(tensor)
            assert 1.0 - keep.mean() <= H.DCN_TIE_LEFT_OUT, (name, cls, tensor, 1.0 - keep.mean())
            idx, _ = cs.yard(tensor)
            assert keep[idx].all()
            clean = float((cnt[idx] == 0).mean())
            assert clean >= H.DCN_TIE_CLEAN, (name, cls, tensor, clean)
        m32 = H.dcn_model(*cs.inputs[:5], geo[7], (geo[8], geo[9]), geo[10], geo[11], dtype=np.float32, bf16=True)
        flipped = m32["colq"].astype(np.float64) != cs.m64["colq"]
        assert not (flipped & ~cs.near).any(), (name, cls, int((flipped & ~cs.near).sum()))
        assert cs.near.mean() < 0.01
    for name in ("k64", "k36", "g2"):
        cs = H.DcnCase(H.DCN64_GRID[name], "gauss", 0, samples=_DCN64_HOST_SAMPLES)
        idx, yd = cs.yard("dx")
        al, fx = cs.allow[idx], cs.allow_fx[idx]
        share = al / (H.CONV_MARGIN_CAP * yd[0] + al)
        assert share.max() < 0.75 and ((al - fx) / (H.CONV_MARGIN_CAP * yd[0])).max() < 0.25, (name, share.max())
        assert al.max() < 2.0 ** -17 * np.abs(cs.ref["dx"]).max()


_DCN_FAULT_CASES = {            # fault -> (grid shape, edge class, bf16, accumulate) where the rule must refuse it
    "clamp": ("edge", "border", 0, False), "nonstrict": ("edge", "exact", 0, False), "swap_hw": ("k64", "gauss", 0, False),
    "group0": ("g2", "gauss", 0, False), "beyond_margin": ("edge", "beyond", 0, False), "tap_mask": ("k64", "gauss", 0, False),
    "skip_chunk": ("k64", "gauss", 0, False), "doffset_nomask": ("k64", "gauss", 0, False), "cols_unrounded": ("k64", "gauss", 1, False),
    "round_before_mask": ("k64", "gauss", 1, False), "dy_unrounded": ("k64", "gauss", 1, False), "base_ignored": ("k64", "gauss", 1, True),
    "fx_unit20": ("k64", "gauss", 0, False),
}


def test_dcn_modelled_faults_are_rejected():
    """The acceptance rule of tests/test_dcn_fp64_gpu.py (conv_accepts at the cap margin, with the fixed-point allowance on d input and
    the bf16 tie rule) refuses every modelled fault — applied on the CPU to the float32 evaluation — in the tensor the fault shows in,
    and accepts the unmodified float32 evaluation in every grid case and edge class, in both precisions."""
    import numpy as np
    import helpers as H
    assert set(_DCN_FAULT_CASES) == set(H.DCN_FAULTS)
    shows = {"clamp": {"out", "dw", "dmask", "doffset"}, "nonstrict": {"doffset"}, "doffset_nomask": {"doffset"}, "fx_unit20": {"dx"},
             "dy_unrounded": {"dw", "dx", "dmask", "doffset"}, "base_ignored": {"dw", "dx"}, "cols_unrounded": {"out", "dw"},
             "round_before_mask": {"out", "dw"}}
    tensors = ("out", "dw", "dmask", "doffset", "dx")

    def run(cs, fault):
        geo = cs.geo
        m = H.dcn_model(*cs.inputs[:5], geo[7], (geo[8], geo[9]), geo[10], geo[11], gy=cs.inputs[5], base_dx=cs.base_dx, base_dw=cs.base_dw,
                        dtype=np.float32, bf16=bool(cs.bf16), fault=fault, margin=cs.margin)
        return {t: cs.check(t, m[t], window=True) for t in tensors}

    built = {}
    for fault, key in _DCN_FAULT_CASES.items():
        if key not in built:
            name, cls, bf, acc = key
            built[key] = H.DcnCase(H.DCN64_GRID[name], cls, bf, accumulate=acc, samples=_DCN64_HOST_SAMPLES)
            clean = run(built[key], None)
            assert all(v[2] for v in clean.values()), (key, clean)
        res = run(built[key], fault)
        refused = {t for t, v in res.items() if not v[2]}
        assert refused, (fault, res)
        assert refused >= shows.get(fault, {"out"}), (fault, refused, res)
    # the unmodified float32 evaluation passes everywhere
    cases = [(nm, "gauss") for nm in H.DCN64_GRID] + [(nm, cls) for nm in H.DCN64_EDGE_CASES for cls in H.DCN_EDGE_CLASSES[1:]]
    worst = 0.0
    for name, cls in cases:
        for bf in (0, 1):
            key = (name, cls, bf, bool(bf))
            cs = built.get(key) or H.DcnCase(H.DCN64_GRID[name], cls, bf, accumulate=bool(bf), samples=_DCN64_HOST_SAMPLES)
            res = run(cs, None)
            assert all(v[2] for v in res.values()), (name, cls, bf, res)
            worst = max(worst, max(r for t, v in res.items() if t != "dx" for r in v[0]))
    assert worst < H.CONV_MARGIN_CAP / 2, worst

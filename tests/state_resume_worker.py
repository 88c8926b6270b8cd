"""Child process of tests/test_state_gpu.py::test_resumed_step_equals_the_uninterrupted_step: the step after a resume
against the same step of the run that was not interrupted, in ONE process (the parent sets RR_CONV_SPLITK=0, the
deterministic arm of tests/test_streams_gpu.py).

  operator A (seed 219)   steps 0..2, save_state(2), close, then step 3
  operator B (other seed, own loader)   one step of its own (its filter caches exist and are stale), load_state, step 3

Writes into --out: a_param.bin / b_param.bin (flat parameters after step 3), a_buffers.bin / b_buffers.bin (every
floating-point buffer), meta.json (the losses of step 3 of both, whether B's batch equals A's as bits, the step
load_state returned, the integer buffers' equality)."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def _cfg(bf16):
    from rrnet_amd.configs.rrnet_config import Config
    cfg = copy.deepcopy(Config)
    cfg.Train.batch_size = 2
    cfg.Train.crop_size = (256, 256)
    cfg.Model.backbone = "hourglass_tiny"
    cfg.Model.bf16 = bool(bf16)
    cfg.Distributed.gpu_id, cfg.Distributed.rank, cfg.Distributed.world_size = 0, 0, 1
    return cfg


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--bf16", action="store_true")
    a = ap.parse_args()
    from rrnet_amd.datasets import synthetic
    from rrnet_amd.operators.rrnet_operator import RRNetOperator
    torch.cuda.set_device(0)
    log_dir = os.path.join(a.out, "log")

    torch.manual_seed(219)
    op_a = RRNetOperator(_cfg(a.bf16))
    op_a.model.train()
    for step in range(3):
        op_a.train_step(step, op_a.training_loader.get_batch())
    op_a.save_state(2, log_dir)
    op_a.close_state()
    batch_a = op_a.training_loader.get_batch()
    kept = [t.clone() if torch.is_tensor(t) else t for t in batch_a]
    _, losses_a = op_a.train_step(3, batch_a)
    torch.cuda.synchronize()

    synthetic._LOADERS.clear()                         # B gets a loader of its own, at position 0
    torch.manual_seed(7)
    op_b = RRNetOperator(_cfg(a.bf16))
    op_b.model.train()
    assert op_b.training_loader is not op_a.training_loader
    assert not torch.equal(op_b.optimizer.fp.flat, op_a.optimizer.fp.flat)
    op_b.train_step(0, op_b.training_loader.get_batch())
    start = op_b.load_state(os.path.join(log_dir, "state-2.pth"))
    batch_b = op_b.training_loader.get_batch()
    same_batch = all(torch.equal(_bits(x), _bits(y)) if torch.is_tensor(x) else x == y for x, y in zip(kept, batch_b))
    _, losses_b = op_b.train_step(start, batch_b)
    torch.cuda.synchronize()

    ints_equal = True
    for tag, op in (("a", op_a), ("b", op_b)):
        op.optimizer.fp.flat.cpu().numpy().tofile(os.path.join(a.out, tag + "_param.bin"))
        fb = torch.cat([b.detach().float().reshape(-1) for b in op.model.buffers() if b.is_floating_point()])
        fb.cpu().numpy().tofile(os.path.join(a.out, tag + "_buffers.bin"))
    for x, y in zip(op_a.model.buffers(), op_b.model.buffers()):
        if not x.is_floating_point():
            ints_equal = ints_equal and x.dtype == y.dtype and bool(torch.equal(x, y))
    meta = {"start": start, "same_batch": bool(same_batch), "int_buffers_equal": bool(ints_equal),
            "losses_a": [float(v) for v in losses_a], "losses_b": [float(v) for v in losses_b],
            "step_count": [op_a.optimizer.step_count, op_b.optimizer.step_count],
            "splitk": os.environ.get("RR_CONV_SPLITK")}
    with open(os.path.join(a.out, "meta.json"), "w") as f:
        json.dump(meta, f)
    print("worker done:", json.dumps(meta), flush=True)


if __name__ == "__main__":
    main()

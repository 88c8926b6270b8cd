"""Record learning-rate sequences of the reference's WarmupMultiStepLR into tests/golden/warmup_lr.npz.

  python tools/gen_golden_warmup.py --reference <reference tree> [--out tests/golden/warmup_lr.npz]

Needs the reference tree: its utils/warmup_lr.py is loaded from there and run; nothing of it is copied.  The fixture
holds, per case, the constructor arguments (as JSON) and the rate after construction and after every step();
tests/test_guard_host.py holds rrnet_amd.utils.warmup_lr to it.  A case with `resume_at` runs that many steps, takes
state_dict(), builds a NEW optimizer and scheduler, loads the state and goes on: the sequence is the joined one."""
import argparse
import importlib.util
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [
    dict(name="linear-milestones-after-warmup", base_lr=0.01, milestones=[30, 60], gamma=0.1, warmup_factor=1.0 / 3,
         warmup_iters=20, warmup_method="linear", steps=80),
    dict(name="linear-milestone-inside-warmup", base_lr=2.5e-4, milestones=[4, 12], gamma=0.1, warmup_factor=1.0 / 3,
         warmup_iters=10, warmup_method="linear", steps=30),
    dict(name="constant-milestone-inside-and-after", base_lr=0.02, milestones=[5, 40], gamma=0.5, warmup_factor=0.25,
         warmup_iters=10, warmup_method="constant", steps=50),
    dict(name="linear-resume-through-state-dict", base_lr=0.01, milestones=[12, 25], gamma=0.1, warmup_factor=0.2,
         warmup_iters=16, warmup_method="linear", steps=40, resume_at=9),
    dict(name="constant-resume-after-warmup", base_lr=0.005, milestones=[20], gamma=0.1, warmup_factor=1.0 / 3,
         warmup_iters=8, warmup_method="constant", steps=30, resume_at=15),
]


def run_case(cls, case):
    """The rate after construction and after each of case['steps'] calls of step(), through `cls`."""
    def make():
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=case["base_lr"])
        sch = cls(opt, case["milestones"], gamma=case["gamma"], warmup_factor=case["warmup_factor"],
                  warmup_iters=case["warmup_iters"], warmup_method=case["warmup_method"])
        return opt, sch
    opt, sch = make()
    lrs = [opt.param_groups[0]["lr"]]
    for t in range(case["steps"]):
        if case.get("resume_at") == t:
            state = sch.state_dict()
            opt, sch = make()
            sch.load_state_dict(state)
        opt.step()
        sch.step()
        lrs.append(opt.param_groups[0]["lr"])
    return np.asarray(lrs, dtype=np.float64)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds utils/warmup_lr.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "warmup_lr.npz"))
    args = ap.parse_args(argv)
    spec = importlib.util.spec_from_file_location("reference_warmup_lr", os.path.join(args.reference, "utils", "warmup_lr.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {"cases": np.array(json.dumps(CASES))}
    for i, case in enumerate(CASES):
        out["lr_%d" % i] = run_case(mod.WarmupMultiStepLR, case)
    np.savez(args.out, **out)
    print("wrote %s: %d cases" % (args.out, len(CASES)))


if __name__ == "__main__":
    main()

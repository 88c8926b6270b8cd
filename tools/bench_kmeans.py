"""Times the device-side Lloyd loop (rr_kmeans_steps through ops.kmeans_lloyd) beside the reference's chain written in plain
torch operations on the device.

  python tools/bench_kmeans.py [--points 350000] [--reps 7] [--out profiles/kmeans.json]

Input: `--points` generated integer log-uniform box sizes in [3, 400] — a STAND-IN: how many boxes VisDrone's train split
holds has not been counted here — clustered with k = 3, M = 1 (one annotation column, what the reference's script does)
and with k = 9, M = 2 (both columns jointly).  The start is one seeded Forgy draw, the same for every variant.

Measured, per shape: the kernel loop at check_every = 1 and 16 with R = 1, and at R = 8 (eight restarts side by side,
check_every = 16; the eight starts are eight draws, so the run lasts as long as its slowest restart); and the reference's
iteration — pairwise distance table, argmin, k x (nonzero, index_select, mean), the shift tested on the host — as torch
operations on the same device.  Each figure is the median of HIP-event intervals around a whole run to convergence after
one warm-up run; time per iteration = that / the iterations of the run.  A report: nothing is asserted."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_lloyd(X, init, tol=1e-4, max_iter=10000):
    """The reference's loop (ext/kmeans/kmeans.py:18-34) in torch operations; max_iter only guards the benchmark."""
    state = init.clone()
    k = state.shape[0]
    iters = 0
    while iters < max_iter:
        dis = ((X.unsqueeze(1) - state.unsqueeze(0)) ** 2.0).sum(dim=-1)
        choice = torch.argmin(dis, dim=1)
        pre = state.clone()
        for j in range(k):
            sel = torch.nonzero(choice == j).squeeze(1)
            state[j] = torch.index_select(X, 0, sel).mean(dim=0)
        shift = torch.sum(torch.sqrt(torch.sum((state - pre) ** 2, dim=1)))
        iters += 1
        if shift ** 2 < tol:
            break
    return choice, state, iters


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=350000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_kmeans.py needs the GPU")
    from rrnet_amd import ops
    dev = torch.device("cuda", 0)
    g = np.random.default_rng(219)
    sizes = np.round(np.exp(g.uniform(np.log(3.0), np.log(400.0), (args.points, 2)))).astype(np.float32)
    report = {"device": torch.cuda.get_device_name(0), "points": args.points, "reps": args.reps,
              "input": "generated integer log-uniform sizes in [3, 400]: a stand-in, VisDrone's box count was not measured"}
    for k, m in ((3, 1), (9, 2)):
        X = torch.from_numpy(np.ascontiguousarray(sizes[:, :m])).to(dev)
        draw = np.random.RandomState(219)
        inits = torch.stack([X[draw.choice(args.points, k)] for _ in range(8)])
        entry = {}
        for name, r, ce in (("hip_R1_check1", 1, 1), ("hip_R1_check16", 1, 16), ("hip_R8_check16", 8, 16)):
            out = ops.kmeans_lloyd(X, inits[:r], check_every=ce)
            iters = out[4].tolist()
            ms, lo = timed(lambda: ops.kmeans_lloyd(X, inits[:r], check_every=ce), args.reps)
            entry[name] = {"restarts": r, "check_every": ce, "iters": iters, "converged": out[5].tolist(),
                           "to_convergence_ms": ms, "to_convergence_min_ms": lo, "per_iteration_us": 1e3 * ms / max(iters)}
        labels, centres, n_it = torch_lloyd(X, inits[0])
        ms, lo = timed(lambda: torch_lloyd(X, inits[0]), args.reps)
        hip = ops.kmeans_lloyd(X, inits[:1])
        entry["torch_chain"] = {"iters": n_it, "to_convergence_ms": ms, "to_convergence_min_ms": lo,
                                "per_iteration_us": 1e3 * ms / n_it,
                                "same_labels_as_hip": bool(torch.equal(labels.int(), hip[0][0])),
                                "max_abs_centre_diff": float((centres - hip[1][0]).abs().max())}
        entry["speedup_to_convergence_R1_check16"] = entry["torch_chain"]["to_convergence_ms"] / entry["hip_R1_check16"]["to_convergence_ms"]
        entry["speedup_per_iteration_R1_check16"] = entry["torch_chain"]["per_iteration_us"] / entry["hip_R1_check16"]["per_iteration_us"]
        report["k%d_M%d" % (k, m)] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(report, sort_keys=True))


if __name__ == "__main__":
    main()

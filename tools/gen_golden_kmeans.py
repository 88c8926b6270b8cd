"""Writes tests/golden/kmeans.npz: the reference's `ext.kmeans.kmeans.lloyd` on the inputs of tests/kmeans_cases.py,
computed on the CPU.

Needs the reference tree (tools/ref_shims.py makes it importable), so it runs in the build container only; the tests read
the file.  The reference's `lloyd` calls `.cuda(device)`: `torch.Tensor.cuda` is replaced by the identity at run time.  It
does not return when a cluster becomes empty (the NaN mean of nothing attracts every point and the shift stays NaN), so
each case runs under a 5 s alarm.  Data only, per case `<group>_s<seed>` (np.random.seed(seed) before the call):
  <case>_x4       the input times 4 as int16 [N,M] (the inputs are quarter-pixel dyadic below 2048: x = x4 / 4 exactly)
  <case>_forgy    the start indices np.random.choice draws under that seed
  <case>_labels   the reference's labels (uint8), <case>_centres its centres (float32 [k,M]) — for the cases that returned
  not_returned    the names of the cases that ran into the alarm (JSON text)

  python tools/gen_golden_kmeans.py
"""
import json
import os
import signal
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "kmeans.npz")
ALARM_SECONDS = 5


class _Alarm(Exception):
    pass


def _ring(signum, frame):
    raise _Alarm()


def main():
    import kmeans_cases as kc                  # before the reference is put in front of sys.path
    from tools import ref_shims
    ref_shims.install()
    torch.Tensor.cuda = lambda self, *a, **k: self
    from ext.kmeans.kmeans import lloyd
    assert os.sep + "rrnet_amd" + os.sep not in lloyd.__code__.co_filename

    out, hung = {}, []
    signal.signal(signal.SIGALRM, _ring)
    for group, (n, m, k) in kc.GROUPS.items():
        for seed in kc.SEEDS:
            name = "%s_s%d" % (group, seed)
            X = kc.case_input(group, seed)
            out[name + "_x4"] = (X * 4).astype(np.int16)
            assert np.array_equal(out[name + "_x4"].astype(np.float32) / 4, X)
            out[name + "_forgy"] = kc.forgy_indices(n, k, seed).astype(np.int32)
            np.random.seed(seed)
            signal.alarm(ALARM_SECONDS)
            try:
                with torch.no_grad():
                    labels, centres = lloyd(torch.from_numpy(X.copy()), k)
                signal.alarm(0)
            except _Alarm:
                hung.append(name)
                print("%-10s did not return in %d s" % (name, ALARM_SECONDS))
                continue
            assert labels.shape == (n,) and centres.shape == (k, m) and centres.dtype == np.float32 and labels.max() < 256
            out[name + "_labels"] = labels.astype(np.uint8)
            out[name + "_centres"] = centres
            mine = kc.run(X, X[out[name + "_forgy"]])
            same = np.array_equal(mine["labels"], labels) and np.array_equal(mine["centres"].view(np.uint32),
                                                                               centres.view(np.uint32))
            print("%-10s restatement: %2d iterations, %s" % (name, mine["iters"], "bit-equal" if same else "DIFFERENT"))
    out["not_returned"] = np.array(json.dumps(hung))
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d bytes, %d cases, %d not returned" % (OUT, os.path.getsize(OUT), len(kc.case_names()), len(hung)))


if __name__ == "__main__":
    main()

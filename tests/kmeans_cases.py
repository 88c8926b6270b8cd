"""The Lloyd step contract of DESIGN §17 restated in numpy, and the inputs the k-means tests and tools/gen_golden_kmeans.py
share.

The contract, per step:
  d[n,j]   = sum_m (x[n,m] - c[j,m])^2 with every difference, product and sum rounded to float32, m ascending;
  label[n] = argmin_j d[n,j] (the lowest index of the minimum);
  sum[j,m], count[j] over the members, sums in float64;
  c'[j,m]  = float32(sum[j,m] / count[j]), one rounding; where count[j] == 0 the centre stays as it was;
  shift    = sum_j sqrt(sum_m (c'[j,m] - c[j,m])^2) in float64 on the float32 values, j and m ascending;
  inertia  = sum_n d[n,label[n]] in float64 (like the labels it refers to the centres before the update);
  done and converged when shift^2 < tol, done and not converged when the iteration count reaches max_iter.

The inputs: cluster blobs are quarter-pixel dyadic (round(v * 4) / 4 with v < 2048) and the VisDrone-like sizes are
integers, so every float64 sum of members is exact whatever the order of addition (fewer than 2^20 points of at most 13
significant bits each): the contract then has ONE right answer bit for bit, and a kernel is compared with == on the bits
of its centres.  `assert_dyadic` states it."""
import functools
import json
import math
import os

import numpy as np

GROUPS = {                       # name -> (points, M, k)
    "blob1": (1500, 1, 3),
    "blob2": (2000, 2, 3),
    "blob9": (3000, 2, 9),
    "sizes": (4000, 1, 3),
}
SEEDS = range(6)


def assert_dyadic(X):
    X = np.asarray(X)
    assert X.dtype == np.float32 and np.isfinite(X).all() and (np.abs(X) < 2048).all()
    assert np.array_equal(X * 4, np.round(X * 4))


def blobs(n, m, k, seed, spread=24.0, base=1000, alpha=2.0):
    """n quarter-pixel points around k centres in [0, 2048)^m, the blobs of unequal weight (Dirichlet(alpha))."""
    g = np.random.default_rng(base + seed)
    centres = g.uniform(100.0, 1900.0, (k, m))
    which = g.choice(k, n, p=g.dirichlet(np.full(k, alpha)))
    v = centres[which] + g.normal(0.0, spread, (n, m))
    X = (np.round(np.clip(v, 0.0, 2047.0) * 4) / 4).astype(np.float32)
    assert_dyadic(X)
    return X


def sizes(n, seed, lo=3.0, hi=400.0, m=1):
    """n integer log-uniform box sizes in [lo, hi]: what an annotation column holds."""
    g = np.random.default_rng(2000 + seed)
    X = np.round(np.exp(g.uniform(np.log(lo), np.log(hi), (n, m)))).astype(np.float32)
    assert_dyadic(X)
    return X


EMPTY_CLUSTER_CASE = "blob9_s4"          # the case the reference never returns from


def case_input(group, seed):
    """blob9 draws very unequal blobs from a generator offset that was picked so that seed 4 — nine distinct start
    indices — loses a cluster in its third step while the other five seeds never do: that is the input on which the
    reference's loop does not end."""
    n, m, k = GROUPS[group]
    if group == "sizes":
        return sizes(n, seed)
    if group == "blob9":
        return blobs(n, m, k, seed, base=2660, alpha=0.5)
    return blobs(n, m, k, seed)


def case_names():
    return ["%s_s%d" % (g, s) for g in GROUPS for s in SEEDS]


@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/kmeans.npz (tools/gen_golden_kmeans.py) -> {case: dict(group, seed, k, x, forgy, labels, centres)},
    labels / centres None for the cases the reference did not return from.  Read once; nobody writes into it."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmeans.npz"))
    hung = set(json.loads(str(z["not_returned"])))
    out = {}
    for group, (n, m, k) in GROUPS.items():
        for seed in SEEDS:
            name = "%s_s%d" % (group, seed)
            x = z[name + "_x4"].astype(np.float32) / np.float32(4)
            x.setflags(write=False)
            done = name not in hung
            out[name] = {"group": group, "seed": seed, "k": k, "x": x, "forgy": z[name + "_forgy"].astype(np.int64),
                         "labels": z[name + "_labels"].astype(np.int64) if done else None,
                         "centres": z[name + "_centres"] if done else None}
    return out


def forgy_indices(n, k, seed):
    """What ext.kmeans.kmeans.forgy draws after np.random.seed(seed)."""
    return np.random.RandomState(seed).choice(n, k)


def step(X, C):
    """One Lloyd step -> (labels int64 [N], new centres float32 [k,M], counts int64 [k], shift, inertia)."""
    X, C = np.asarray(X, dtype=np.float32), np.asarray(C, dtype=np.float32)
    n, m = X.shape
    k = C.shape[0]
    d = np.zeros((n, k), dtype=np.float32)
    for i in range(m):
        t = X[:, i, None] - C[None, :, i]
        d = d + t * t
    assert d.dtype == np.float32
    labels = d.argmin(axis=1)
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    new = C.copy()
    for j in range(k):
        if counts[j]:
            new[j] = (X[labels == j].astype(np.float64).sum(axis=0) / float(counts[j])).astype(np.float32)
    shift = 0.0
    for j in range(k):
        d2 = 0.0
        for i in range(m):
            t = float(new[j, i]) - float(C[j, i])
            d2 = d2 + t * t
        shift += math.sqrt(d2)
    inertia = float(d[np.arange(n), labels].astype(np.float64).sum())
    return labels, new, counts, shift, inertia


def run(X, init, tol=1e-4, max_iter=10000):
    """Steps until done -> dict(labels, centres, counts, inertia, iters, converged) of one restart."""
    C = np.array(init, dtype=np.float32)
    iters = 0
    while True:
        labels, C, counts, shift, inertia = step(X, C)
        iters += 1
        if shift * shift < tol:
            converged = True
            break
        if iters >= max_iter:
            converged = False
            break
    return {"labels": labels, "centres": C, "counts": counts, "inertia": inertia, "iters": iters, "converged": converged}


@functools.lru_cache(maxsize=None)
def golden_run(name):
    """The restatement on a stored case from its stored Forgy start.  Computed once per process; read-only."""
    g = golden()[name]
    return run(g["x"], g["x"][g["forgy"]])


def centre_bound(X, labels, counts, eps):
    """(count_j + 1) * eps * mean_j |x| per cluster and column: the worst-case error of a mean in arithmetic of unit
    roundoff eps, whatever the order of summation (count_j - 1 additions and one division).  Empty clusters: 0."""
    X = np.asarray(X, dtype=np.float64)
    k = len(counts)
    out = np.zeros((k, X.shape[1]))
    for j in range(k):
        if counts[j]:
            out[j] = (counts[j] + 1) * eps * np.abs(X[labels == j]).mean(axis=0)
    return out

"""ext/kmeans/kmeans.py of the reference (`forgy`, `lloyd`) over rr_kmeans_steps: the whole Lloyd loop runs on the device,
restarts side by side, with one host read per `check_every` steps.

Deviations from the reference, both where it would never return: an empty cluster keeps its centre (the reference writes
the NaN mean of nothing, after which every point joins the NaN centre and the shift stays NaN), and `max_iter` bounds the
loop.  There is no CPU path."""
import warnings

import numpy as np
import torch

from rrnet_amd import ops
from .pairwise import pairwise_distance  # noqa: F401  (the reference's module has it in its namespace)


def forgy(X, n_clusters):
    """n_clusters rows of X drawn with replacement by `np.random.choice(len(X), n_clusters)`: the reference's call, so the
    same np.random.seed gives the same start."""
    indices = np.random.choice(len(X), n_clusters)
    return X[indices]


def _as_float_tensor(a, what):
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.array(a, dtype=np.float32))
    a = a.detach().float()
    if not bool(torch.isfinite(a).all()):
        raise ValueError("lloyd: %s holds non-finite values" % what)
    return a


def lloyd(X, n_clusters, device=0, tol=1e-4, *, init=None, restarts=1, max_iter=10000, return_info=False):
    """k-means of X [N,M] (tensor or array) -> (labels np.int64 [N], centres np.float32 [k,M]), the labels against the
    centres before the last update as in the reference.

    init: start centres [k,M] or [R,k,M] in place of the Forgy draw.  restarts=R: R Forgy draws in sequence, run in one
    launch sequence; the restart with the lowest inertia is returned (ties: the lowest index).  return_info=True adds a
    dict with `iters`, `converged`, `inertia`, `counts` of the returned restart and its index `restart`.  A returned run
    that ended at max_iter gives a RuntimeWarning.  Bad shapes and non-finite input raise ValueError before the device is
    touched."""
    k, restarts = int(n_clusters), int(restarts)
    if not torch.is_tensor(X):
        X = torch.from_numpy(np.array(X, dtype=np.float32))
    if X.dim() != 2:
        raise ValueError("lloyd: X must be [N,M], got %s" % (tuple(X.shape),))
    n, m = X.shape
    if not (n >= 1 and 1 <= m <= ops.KMEANS_MAX_M and 1 <= k <= ops.KMEANS_MAX_K):
        raise ValueError("lloyd: N=%d M=%d k=%d outside N >= 1, 1 <= M <= %d, 1 <= k <= %d"
                         % (n, m, k, ops.KMEANS_MAX_M, ops.KMEANS_MAX_K))
    if int(max_iter) < 1:
        raise ValueError("lloyd: max_iter=%d" % int(max_iter))
    X = _as_float_tensor(X, "X")
    if init is not None:
        init = _as_float_tensor(init, "init")
        if init.dim() == 2:
            init = init.unsqueeze(0)
        if init.dim() != 3 or tuple(init.shape[1:]) != (k, m) or not 1 <= init.shape[0] <= ops.KMEANS_MAX_R:
            raise ValueError("lloyd: init must be [%d,%d] or [R,%d,%d] with 1 <= R <= %d, got %s"
                             % (k, m, k, m, ops.KMEANS_MAX_R, tuple(init.shape)))
    elif not 1 <= restarts <= ops.KMEANS_MAX_R:
        raise ValueError("lloyd: restarts=%d outside 1..%d" % (restarts, ops.KMEANS_MAX_R))
    X = X.cuda(device)
    if init is None:
        init = torch.stack([forgy(X, k) for _ in range(restarts)])
    labels, centres, counts, inertia, iters, converged = ops.kmeans_lloyd(X, init.cuda(device).contiguous(), tol=tol,
                                                                          max_iter=max_iter)
    inertia = inertia.cpu().numpy()
    best = int(np.argmin(inertia))                       # the first of equal minima
    if not bool(converged[best]):
        warnings.warn("lloyd: restart %d stopped at max_iter=%d before shift^2 < %g" % (best, int(max_iter), tol),
                      RuntimeWarning, stacklevel=2)
    out = (labels[best].cpu().numpy().astype(np.int64), centres[best].cpu().numpy())
    if return_info:
        info = {"iters": int(iters[best]), "converged": bool(converged[best]), "inertia": float(inertia[best]),
                "counts": counts[best].cpu().numpy().astype(np.int64), "restart": best}
        return out + (info,)
    return out

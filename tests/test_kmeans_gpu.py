"""rr_kmeans_steps (ops.kmeans_lloyd) and ext.kmeans.kmeans.lloyd on the device against the numpy restatement of the Lloyd
step contract in tests/kmeans_cases.py and against the reference's recorded results (tests/golden/kmeans.npz).

The inputs are quarter-pixel dyadic or integer (kc.assert_dyadic), so every double sum of members is exact and the contract
has one right answer: labels, centres (as bits), counts, iteration counts and converged flags must be EQUAL; the inertia, a
double sum of inexact float32 distances, must be within N * 2^-53 * sum(d)."""
import functools
import warnings

import numpy as np
import pytest
import torch

import kmeans_cases as kc

pytestmark = pytest.mark.gpu


def device_run(X, inits, **kw):
    from rrnet_amd import ops
    out = ops.kmeans_lloyd(torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(inits)).cuda(), **kw)
    torch.cuda.synchronize()
    names = ("labels", "centres", "counts", "inertia", "iters", "converged")
    got = dict(zip(names, (t.cpu().numpy() for t in out)))
    r, k, m = inits.shape
    assert got["labels"].shape == (r, X.shape[0]) and got["labels"].dtype == np.int32
    assert got["centres"].shape == (r, k, m) and got["centres"].dtype == np.float32
    assert got["counts"].shape == (r, k) and got["counts"].dtype == np.int32
    assert got["inertia"].shape == (r,) and got["inertia"].dtype == np.float64
    assert got["iters"].shape == (r,) and got["iters"].dtype == np.int32
    assert got["converged"].shape == (r,) and got["converged"].dtype == np.bool_
    return got


def assert_equals_restatement(X, inits, got, tol=1e-4, max_iter=10000):
    refs = []
    for r in range(inits.shape[0]):
        ref = kc.run(X, inits[r], tol=tol, max_iter=max_iter)
        refs.append(ref)
        assert np.array_equal(got["labels"][r], ref["labels"]), r
        assert np.array_equal(got["centres"][r].view(np.uint32), ref["centres"].view(np.uint32)), (r, got["centres"][r], ref["centres"])
        assert np.array_equal(got["counts"][r], ref["counts"]), r
        assert int(got["iters"][r]) == ref["iters"] and bool(got["converged"][r]) == ref["converged"], r
        assert abs(float(got["inertia"][r]) - ref["inertia"]) <= X.shape[0] * 2.0 ** -53 * ref["inertia"], r
    return refs


def assert_same_outputs(a, b):
    for key in a:
        x, y = a[key], b[key]
        if x.dtype.kind == "f":
            x, y = x.view(np.uint32 if x.dtype == np.float32 else np.uint64), y.view(np.uint32 if y.dtype == np.float32 else np.uint64)
        assert np.array_equal(x, y), key


def starts(X, k, seed, restarts=1):
    g = np.random.RandomState(seed)
    return np.stack([X[g.choice(X.shape[0], k)] for _ in range(restarts)])


@functools.lru_cache(maxsize=None)
def three_restarts():
    """blob2_s0's points with three Forgy starts whose restatement iteration counts differ (asserted)."""
    X = kc.golden()["blob2_s0"]["x"]
    by_iters = {}
    for seed in range(12):
        init = X[kc.forgy_indices(X.shape[0], 3, seed)]
        by_iters.setdefault(kc.run(X, init)["iters"], init)
    picked = sorted(by_iters)[:3]
    assert len(picked) == 3 and len(set(picked)) == 3
    # the shortest restart in the middle: its neighbours go on while it is frozen
    inits = np.stack([by_iters[picked[1]], by_iters[picked[0]], by_iters[picked[2]]])
    inits.setflags(write=False)
    return X, inits, (picked[1], picked[0], picked[2])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_wave_and_workgroup_tails(n):
    X = kc.sizes(n, seed=n)
    inits = starts(X, 3, seed=n)
    assert_equals_restatement(X, inits, device_run(X, inits))


def test_capped_grid_stride_loop_turns_twice():
    from rrnet_amd import _C
    blocks = _C.fn("rr_kmeans_blocks")
    cap = blocks(1 << 40)
    n = cap * 256 + 13
    assert blocks(n) == cap and blocks(cap * 256) == cap and blocks(cap * 256 - 256) == cap - 1
    assert -(-n // (blocks(n) * 256)) == 2                     # the loop of the last 13 threads' workgroup turns twice
    X = kc.sizes(n, seed=77)
    inits = starts(X, 3, seed=77)
    assert_equals_restatement(X, inits, device_run(X, inits))


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_every_point_width(m):
    X = kc.blobs(515, m, 4, seed=40 + m)
    inits = starts(X, 4, seed=m, restarts=2)
    assert_equals_restatement(X, inits, device_run(X, inits))


@pytest.mark.parametrize("k", [1, 2, 9, 64])
def test_cluster_counts(k):
    X = kc.blobs(2000, 2, max(k, 2), seed=60 + k)
    inits = starts(X, k, seed=k)
    assert_equals_restatement(X, inits, device_run(X, inits))


def test_fewer_points_than_clusters():
    X = np.array([[1.0], [5.0]], dtype=np.float32)
    inits = np.array([[[1.0], [5.0], [100.0]]], dtype=np.float32)
    got = device_run(X, inits)
    assert_equals_restatement(X, inits, got)
    assert got["centres"][0].ravel().tolist() == [1.0, 5.0, 100.0] and got["counts"][0].tolist() == [1, 1, 0]


def test_ties_go_to_the_lowest_index_and_duplicate_starts_stay_empty():
    X = np.array([[0.0], [4.0], [8.0]], dtype=np.float32)
    inits = np.array([[[0.0], [8.0]]], dtype=np.float32)                  # the point 4 is midway: it joins centre 0
    got = device_run(X, inits, max_iter=1)
    assert_equals_restatement(X, inits, got, max_iter=1)
    assert got["labels"][0].tolist() == [0, 0, 1] and got["centres"][0].ravel().tolist() == [2.0, 8.0]
    assert float(got["inertia"][0]) == 16.0
    inits = np.array([[[2.0], [8.0], [8.0]]], dtype=np.float32)           # the second of two equal centres gets nothing
    got = device_run(X, inits)
    assert_equals_restatement(X, inits, got)
    assert got["labels"][0].tolist() == [0, 0, 1] and got["counts"][0].tolist() == [2, 1, 0]
    assert got["centres"][0].ravel().tolist() == [2.0, 8.0, 8.0] and int(got["iters"][0]) == 1 and bool(got["converged"][0])


def test_the_case_the_reference_never_returns_from():
    g = kc.golden()[kc.EMPTY_CLUSTER_CASE]
    inits = g["x"][g["forgy"]][None]
    got = device_run(g["x"], inits)
    ref = kc.golden_run(kc.EMPTY_CLUSTER_CASE)
    assert bool(got["converged"][0]) and int(got["iters"][0]) == ref["iters"] and np.isfinite(got["centres"]).all()
    assert np.array_equal(got["labels"][0], ref["labels"]) and np.array_equal(got["counts"][0], ref["counts"])
    assert np.array_equal(got["centres"][0].view(np.uint32), ref["centres"].view(np.uint32))
    assert (got["counts"][0] == 0).any()


def test_finished_restarts_keep_their_state():
    X, inits, iters = three_restarts()
    assert len(set(iters)) == 3
    got = device_run(X, inits)
    assert_equals_restatement(X, inits, got)
    assert got["iters"].tolist() == list(iters)
    for r in range(3):                                          # and each equals the same start run alone
        alone = device_run(X, inits[r:r + 1])
        for key in got:
            assert np.array_equal(got[key][r], alone[key][0]), (key, r)


def test_result_does_not_depend_on_check_every():
    X, inits, iters = three_restarts()
    runs = [device_run(X, inits, check_every=c) for c in (1, 4, 64)]
    assert_equals_restatement(X, inits, runs[0])
    assert_same_outputs(runs[0], runs[1])
    assert_same_outputs(runs[0], runs[2])
    # convergence exactly at the end of a batch of steps, and one step into the next batch
    one, i = inits[2:3], iters[2]
    assert i >= 3 and i % i == 0 and i % (i - 1) == 1
    base = device_run(X, one, check_every=1)
    assert int(base["iters"][0]) == i
    for c in (i, i - 1):
        assert_same_outputs(base, device_run(X, one, check_every=c))


@pytest.mark.parametrize("check_every", [1, 16])
def test_max_iter_stops_a_run(check_every):
    X, inits, iters = three_restarts()
    assert min(iters) > 2
    got = device_run(X, inits, max_iter=2, check_every=check_every)
    assert_equals_restatement(X, inits, got, max_iter=2)
    assert got["iters"].tolist() == [2, 2, 2] and not got["converged"].any()


def test_runs_repeat_bit_for_bit_on_inexact_sums():
    """Non-dyadic input: the double sums round, so the order of addition shows.  Two runs must agree bit for bit; against
    the restatement (numpy adds in another order) labels are equal and every centre is within (count_j + 1) * 2^-53 *
    mean_j|x| (two double sums of the same members) + 2^-24 * |c| (the one rounding to float32)."""
    g = np.random.default_rng(5)
    centres = g.uniform(10.0, 400.0, (5, 2))
    X = (centres[g.integers(0, 5, 5000)] + g.normal(0.0, 9.0, (5000, 2))).astype(np.float32)
    assert not np.array_equal(X * 4, np.round(X * 4))
    inits = starts(X, 5, seed=5, restarts=2)
    a, b = device_run(X, inits), device_run(X, inits)
    assert_same_outputs(a, b)
    for r in range(2):
        ref = kc.run(X, inits[r])
        assert np.array_equal(a["labels"][r], ref["labels"])
        bound = kc.centre_bound(X, ref["labels"], ref["counts"], 2.0 ** -53) + 2.0 ** -24 * np.abs(ref["centres"].astype(np.float64))
        assert (np.abs(a["centres"][r].astype(np.float64) - ref["centres"].astype(np.float64)) <= bound).all()


@pytest.mark.parametrize("name", kc.case_names())
def test_lloyd_gives_the_reference_result(name):
    from rrnet_amd.ext.kmeans.kmeans import lloyd
    g, ref = kc.golden()[name], kc.golden_run(name)
    np.random.seed(g["seed"])
    labels, centres = lloyd(torch.from_numpy(g["x"].copy()), g["k"])
    assert labels.dtype == np.int64 and labels.shape == (g["x"].shape[0],)
    assert centres.dtype == np.float32 and centres.shape == (g["k"], g["x"].shape[1])
    if g["labels"] is None:                                     # the reference has no answer: the restatement's
        assert np.array_equal(labels, ref["labels"]) and np.array_equal(centres.view(np.uint32), ref["centres"].view(np.uint32))
        return
    assert np.array_equal(labels, g["labels"])
    bound = kc.centre_bound(g["x"], g["labels"], ref["counts"], 2.0 ** -24)
    assert (np.abs(centres.astype(np.float64) - g["centres"].astype(np.float64)) <= bound).all()


def test_lloyd_restarts_pick_the_lowest_inertia():
    from rrnet_amd.ext.kmeans.kmeans import lloyd
    X = kc.golden()["blob9_s1"]["x"]
    inits = starts(X, 9, seed=11, restarts=4)                  # what four forgy calls draw after np.random.seed(11)
    refs = [kc.run(X, init) for init in inits]
    best = int(np.argmin([r["inertia"] for r in refs]))
    assert len({r["inertia"] for r in refs}) > 1
    np.random.seed(11)
    labels, centres, info = lloyd(X, 9, restarts=4, return_info=True)
    assert info["restart"] == best and info["iters"] == refs[best]["iters"] and info["converged"] is True
    assert np.array_equal(info["counts"], refs[best]["counts"])
    assert abs(info["inertia"] - refs[best]["inertia"]) <= X.shape[0] * 2.0 ** -53 * refs[best]["inertia"]
    assert np.array_equal(labels, refs[best]["labels"])
    assert np.array_equal(centres.view(np.uint32), refs[best]["centres"].view(np.uint32))
    # explicit starts in place of the draw, [k,M] and [R,k,M]
    l2, c2 = lloyd(X, 9, init=inits)
    assert np.array_equal(l2, labels) and np.array_equal(c2, centres)
    l3, c3 = lloyd(X, 9, init=inits[best])
    assert np.array_equal(l3, labels) and np.array_equal(c3, centres)


def test_lloyd_warns_at_max_iter():
    from rrnet_amd.ext.kmeans.kmeans import lloyd
    X, inits, iters = three_restarts()
    with pytest.warns(RuntimeWarning):
        labels, centres, info = lloyd(X, 3, init=inits[0], max_iter=2, return_info=True)
    assert info["iters"] == 2 and info["converged"] is False
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        lloyd(X, 3, init=inits[0])


def test_on_a_side_stream():
    X, inits, _ = three_restarts()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = device_run(X, inits)
    assert_equals_restatement(X, inits, got)

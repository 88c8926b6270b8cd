"""Host-side tests of the k-means anchor statistics: the numpy restatement of the Lloyd step contract against the
reference's recorded results, the reference's import lines, the Forgy draw, the argument checks (before any launch), the
size gathering of tools/kmeans_anchors.py and the header.  No GPU."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

import kmeans_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("rr_kmeans_blocks", "rr_kmeans_workspace_bytes", "rr_kmeans_steps")
RETURNED = [n for n in kc.case_names() if n != kc.EMPTY_CLUSTER_CASE]


def test_golden_file_holds_the_cases_of_kmeans_cases():
    g = kc.golden()
    assert sorted(g) == sorted(kc.case_names()) and len(g) == 24
    assert [n for n in g if g[n]["labels"] is None] == [kc.EMPTY_CLUSTER_CASE]
    for name, c in g.items():
        n, m, k = kc.GROUPS[c["group"]]
        kc.assert_dyadic(c["x"])
        assert np.array_equal(c["x"], kc.case_input(c["group"], c["seed"])) and c["x"].shape == (n, m)
        assert np.array_equal(c["forgy"], kc.forgy_indices(n, k, c["seed"]))
    assert (kc.golden()["sizes_s0"]["x"] == np.round(kc.golden()["sizes_s0"]["x"])).all()
    assert len(set(g[kc.EMPTY_CLUSTER_CASE]["forgy"].tolist())) == 9          # nine distinct start rows, and still it hangs


@pytest.mark.parametrize("name", RETURNED)
def test_restatement_gives_the_reference_result(name):
    """Labels equal; every centre within (count_j + 1) * 2^-24 * mean_j|x| of the reference's: the worst-case error of a
    float32 mean in any order of summation.  Derived, not measured (the observed difference is 0)."""
    g, mine = kc.golden()[name], kc.golden_run(name)
    assert mine["converged"] and 2 <= mine["iters"] < 100
    assert np.array_equal(mine["labels"], g["labels"])
    bound = kc.centre_bound(g["x"], mine["labels"], mine["counts"], 2.0 ** -24)
    assert (mine["counts"] > 0).all()
    diff = np.abs(mine["centres"].astype(np.float64) - g["centres"].astype(np.float64))
    assert (diff <= bound).all(), (diff.max(), bound.min())


def test_restatement_returns_where_the_reference_does_not():
    g, mine = kc.golden()[kc.EMPTY_CLUSTER_CASE], kc.golden_run(kc.EMPTY_CLUSTER_CASE)
    assert g["labels"] is None and g["centres"] is None
    assert mine["converged"] and mine["iters"] < 100
    assert mine["centres"].shape == (9, 2) and np.isfinite(mine["centres"]).all()
    assert (mine["counts"] == 0).sum() >= 1 and mine["counts"].sum() == g["x"].shape[0]
    empty = np.flatnonzero(mine["counts"] == 0)
    # the empty cluster kept a centre it had before: it is a value the data could produce, not NaN and not zero
    assert (mine["centres"][empty] > 0).all()


def test_step_contract_details():
    """Tie -> lowest index; an empty cluster keeps its centre; labels and inertia refer to the centres before the update."""
    X = np.array([[4.0], [0.0], [8.0]], dtype=np.float32)
    labels, new, counts, shift, inertia = kc.step(X, np.array([[0.0], [8.0]], dtype=np.float32))
    assert labels.tolist() == [0, 0, 1] and counts.tolist() == [2, 1] and new.ravel().tolist() == [2.0, 8.0]
    assert shift == 2.0 and inertia == 16.0
    labels, new, counts, shift, inertia = kc.step(X, np.array([[4.0], [4.0], [100.0]], dtype=np.float32))
    assert labels.tolist() == [0, 0, 0] and counts.tolist() == [3, 0, 0] and new.ravel().tolist() == [4.0, 4.0, 100.0]
    r = kc.run(X, np.array([[0.0], [8.0]], dtype=np.float32), max_iter=1)
    assert r["iters"] == 1 and not r["converged"]


def test_reference_import_lines_resolve_through_shims():
    """With PYTHONPATH=<repo>/shims, in a fresh interpreter started outside the repository, the import lines of the
    reference's scripts/kmeans.py and of ext/kmeans resolve to this package, and the Config table has the keys and values
    of the reference's configs/kmeans_config.py (written out here)."""
    code = (
        "from datasets import make_dataloader\n"
        "from configs.kmeans_config import Config\n"
        "from ext.kmeans.kmeans import lloyd, forgy\n"
        "from ext.kmeans.pairwise import pairwise_distance, group_pairwise\n"
        "import ext.kmeans, ext.kmeans.kmeans, rrnet_amd.ext.kmeans.kmeans, rrnet_amd.configs.kmeans_config as c2, inspect, os\n"
        "assert ext.kmeans.kmeans is rrnet_amd.ext.kmeans.kmeans and c2.Config is Config\n"
        "for f in (lloyd, forgy, pairwise_distance, group_pairwise):\n"
        "    assert os.sep + 'rrnet_amd' + os.sep in inspect.getfile(f), f\n"
        "assert ext.kmeans.kmeans.pairwise_distance is pairwise_distance\n"
        "assert sorted(Config.keys()) == ['Train', 'Val', 'data_root', 'dataset', 'seed']\n"
        "assert Config.seed == 219 and Config.dataset == 'drones_det' and Config.data_root == './data/DronesDET'\n"
        "assert sorted(Config.Train.keys()) == ['batch_size', 'mean', 'num_workers', 'pretrained', 'sampler', 'transforms']\n"
        "assert sorted(Config.Val.keys()) == ['batch_size', 'mean', 'num_workers', 'sampler', 'transforms']\n"
        "assert Config.Train.pretrained is True\n"
        "for part in (Config.Train, Config.Val):\n"
        "    assert part.batch_size == 1 and part.num_workers == 4 and part.sampler is None\n"
        "    assert part.mean == (0.485, 0.456, 0.406)\n"
        "    assert [type(t).__name__ for t in part.transforms.transforms] == ['ToTensor', 'MaskIgnore']\n"
        "import torch\n"
        "a = torch.tensor([[0., 0.], [3., 4.]]); b = torch.tensor([[0., 0.]])\n"
        "assert pairwise_distance(a).tolist() == [[0., 25.], [25., 0.]] and pairwise_distance(a, b).tolist() == [0., 25.]\n"
        "d = group_pairwise(a, [[0], [0, 1]], device=-1)\n"
        "assert sorted(d) == [(0, 0), (0, 1), (1, 0), (1, 1)] and d[(0, 1)].tolist() == [0., 25.] and d[(0, 0)].dim() == 0\n"
        "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "shims"))
    out = subprocess.check_output(["python", "-c", code], text=True, cwd="/tmp", env=env, timeout=300)
    assert out.strip().endswith("ok")


def test_forgy_draws_what_the_reference_draws():
    from rrnet_amd.ext.kmeans.kmeans import forgy
    X = torch.arange(40, dtype=torch.float32).reshape(20, 2)
    for seed in (0, 4, 219):
        np.random.seed(seed)
        want = np.random.choice(20, 5)
        np.random.seed(seed)
        got = forgy(X, 5)
        assert torch.equal(got, X[want]) and got.shape == (5, 2)
        np.random.seed(seed)
        assert np.array_equal(forgy(X.numpy(), 5), X.numpy()[want])
        assert np.array_equal(want, kc.forgy_indices(20, 5, seed))


def test_bad_arguments_raise_value_error_before_any_launch(monkeypatch):
    from rrnet_amd import _C, ops
    from rrnet_amd.ext.kmeans.kmeans import lloyd

    def no_launch(*a, **k):
        raise AssertionError("an entry point was looked up")

    monkeypatch.setattr(_C, "fn", no_launch)
    X = np.arange(40, dtype=np.float32).reshape(20, 2)
    bad = X.copy()
    bad[7, 1] = np.nan
    inf = X.copy()
    inf[0, 0] = np.inf
    for args, kw in (((X, 0), {}), ((X, 65), {}), ((np.zeros((20, 5), np.float32), 3), {}), ((X, 3), {"restarts": 65}),
                     ((X, 3), {"restarts": 0}), ((X, 3), {"init": np.zeros((2, 2), np.float32)}),
                     ((X, 3), {"init": np.zeros((2, 3, 1), np.float32)}), ((X, 3), {"init": np.zeros((65, 3, 2), np.float32)}),
                     ((bad, 3), {}), ((inf, 3), {}), ((torch.from_numpy(bad), 3), {}), ((X[:, 0], 3), {}),
                     ((np.zeros((0, 2), np.float32), 3), {}), ((X, 3), {"init": np.full((3, 2), np.nan, np.float32)}),
                     ((X, 3), {"max_iter": 0})):
        with pytest.raises(ValueError):
            lloyd(*args, **kw)
    Xt = torch.from_numpy(X)
    for x, init in ((Xt, torch.zeros(1, 0, 2)), (Xt, torch.zeros(1, 65, 2)), (torch.zeros(20, 5), torch.zeros(1, 3, 5)),
                    (Xt, torch.zeros(65, 3, 2)), (Xt, torch.zeros(3, 2)), (Xt, torch.zeros(1, 3, 1)),
                    (Xt.double(), torch.zeros(1, 3, 2)), (torch.zeros(0, 2), torch.zeros(1, 3, 2))):
        with pytest.raises(ValueError):
            ops.kmeans_lloyd(x, init)
    for kw in ({"max_iter": 0}, {"check_every": 0}):
        with pytest.raises(ValueError):
            ops.kmeans_lloyd(Xt, torch.zeros(1, 3, 2), **kw)


def _tool():
    spec = importlib.util.spec_from_file_location("kmeans_anchors_tool", os.path.join(ROOT, "tools", "kmeans_anchors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gather_sizes_reads_the_annotation_columns(golden_dir, tmp_path):
    tool = _tool()
    got = tool.gather_sizes(golden_dir, "visdrone_demo")
    rows = []
    for line in open(os.path.join(golden_dir, "visdrone_demo", "annotations", "0000364_01765_d_0000782.txt")):
        parts = [p for p in line.strip().split(",") if p.strip()]
        if parts and int(parts[5]) not in (0, 11):
            rows.append([int(parts[2]), int(parts[3])])
    want = np.asarray(rows, dtype=np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape and want.shape[0] > 10 and np.array_equal(got, want)
    # two files in name order, ignored regions and class 11 left out, a trailing comma tolerated
    d = tmp_path / "train" / "annotations"
    os.makedirs(d)
    (d / "b.txt").write_text("1,2,30,40,1,4,0,0\n5,6,7,8,0,0,0,0\n")
    (d / "a.txt").write_text("1,2,3,4,1,1,0,0,\n1,2,50,60,1,11,0,0\n9,9,10,20,1,10,0,0\n")
    assert tool.gather_sizes(str(tmp_path), "train").tolist() == [[3.0, 4.0], [10.0, 20.0], [30.0, 40.0]]
    assert tool.gather_sizes(str(tmp_path), "val").shape == (0, 2)
    s = tool.synthetic_sizes(500, 3)
    assert s.shape == (500, 2) and s.dtype == np.float32 and (s >= 5).all() and np.array_equal(s, np.round(s))


def test_entry_points_are_declared_and_plan_caps_the_grid():
    from rrnet_amd import _C, ops
    sigs = _C.header_signatures()
    for n in NEW_ENTRY_POINTS:
        assert n in sigs, n
    blocks, ws = _C.fn("rr_kmeans_blocks"), _C.fn("rr_kmeans_workspace_bytes")
    assert [blocks(n) for n in (0, 1, 256, 257, 512 * 256, 512 * 256 + 13, 1 << 33)] == [0, 1, 1, 2, 512, 512, 512]
    assert ws(1000, 2, 9, 3) == 3 * (9 * 3 + 1) * 4 * 8 and ws(0, 2, 9, 3) == 0
    assert (ops.KMEANS_MAX_K, ops.KMEANS_MAX_M, ops.KMEANS_MAX_R) == (64, 4, 64)
    assert _C.lib().rr_abi_version() == 1

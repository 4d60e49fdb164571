"""CPU checks of the HDBSCAN* oracle (tests/hdbscan_oracle.py) and of the host half of the product (``vfm_hdbscan_labels_host``):
the oracle anchored against ``sklearn.cluster.HDBSCAN(100, 25)`` on blob inputs, the library's labels equal to the oracle's on the
oracle's edges and on hand-made trees, the map filter's coin per cluster, and the refusals that need no device."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import hdbscan_oracle as ho

ROOT = Path(__file__).resolve().parent.parent
SEEDS = (0, 1, 2, 3)
_CACHE = {}


def blob_case(seed):
    """(points, labels, (lo, hi, w2)) of the oracle at (100, 25), computed once per seed"""
    if seed not in _CACHE:
        pts = ho.blobs(seed)
        labels, edges = ho.hdbscan(pts, 100, 25)
        for a in (pts, labels) + tuple(edges):
            a.setflags(write=False)
        _CACHE[seed] = (pts, labels, edges)
    return _CACHE[seed]


@pytest.fixture(scope="module")
def ops():
    subprocess.run([sys.executable, str(ROOT / "vfm-registration_amd" / "build.py")], check=True, stdout=subprocess.DEVNULL)
    from vfmreg import _lib, ops
    _lib.load()
    return ops


def mismatches_up_to_renumbering(a, b):
    """the points on which two labellings differ once every label of ``a`` is matched with the label of ``b`` it shares most points
    with (noise stays noise)"""
    wrong = int(np.sum((a == -1) != (b == -1)))
    both = (a != -1) & (b != -1)
    for label in np.unique(a[both]):
        theirs = b[both & (a == label)]
        wrong += len(theirs) - int(np.bincount(theirs).max())
    return wrong


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_against_sklearn_hdbscan(seed):
    cluster = pytest.importorskip("sklearn.cluster", reason="sklearn is absent: the oracle is not compared with its HDBSCAN")
    if not hasattr(cluster, "HDBSCAN"):
        pytest.skip("this sklearn has no cluster.HDBSCAN: the oracle is not compared with it")
    pts, labels, (lo, hi, w2) = blob_case(seed)
    assert len(pts) == 2700
    sk = cluster.HDBSCAN(min_cluster_size=100, min_samples=25).fit(pts)
    theirs = np.asarray(sk.labels_)
    assert labels.max() + 1 == theirs.max() + 1                                  # the number of clusters
    wrong = mismatches_up_to_renumbering(labels, theirs)
    print(f"seed {seed}: clusters {labels.max() + 1}, noise {np.sum(labels == -1)} / {np.sum(theirs == -1)}, differing points {wrong}")
    assert wrong <= 0.002 * len(pts)
    # the sorted single-linkage distances: sklearn works on roots
    np.testing.assert_allclose(np.sqrt(w2), np.sort(sk._single_linkage_tree_["value"]), rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------- hand-made trees
def sorted_edges(lo, hi, w2):
    lo, hi = np.minimum(lo, hi).astype(np.int32), np.maximum(lo, hi).astype(np.int32)
    w2 = np.asarray(w2, dtype=np.float64)
    order = np.lexsort((hi, lo, w2))
    return lo[order], hi[order], w2[order]


def sides(counts, rng):
    """random trees of ``counts`` points each with light edges, joined in a chain by heavy edges (100, 200, ...)"""
    lo, hi, w2, start = [], [], [], 0
    for s, count in enumerate(counts):
        for k in range(1, count):
            lo.append(start + int(rng.integers(0, k)))
            hi.append(start + k)
            w2.append(float(rng.uniform(0.5, 1.5)))
        if s:
            lo.append(start - 1), hi.append(start), w2.append(100.0 * s)
        start += count
    return sorted_edges(np.array(lo), np.array(hi), w2)


def hand_made_trees():
    rng = np.random.default_rng(7)
    n = 40
    random_tree = (np.array([int(rng.integers(0, k)) for k in range(1, n)]), np.arange(1, n))
    cases = {
        "all weights equal": (sorted_edges(*random_tree, np.ones(n - 1)), 5),
        "all weights equal, a path": (sorted_edges(np.arange(n - 1), np.arange(1, n), np.full(n - 1, 2.0)), 5),
        "star, equal weights": (sorted_edges(np.zeros(n - 1, int), np.arange(1, n), np.full(n - 1, 3.0)), 5),
        "star, ascending weights": (sorted_edges(np.zeros(n - 1, int), np.arange(1, n), np.arange(1, n, dtype=float)), 5),
        "path, random weights": (sorted_edges(np.arange(n - 1), np.arange(1, n), rng.uniform(0.1, 4, n - 1)), 4),
        "path, three dense stretches": (sorted_edges(np.arange(59), np.arange(1, 60),
                                                     np.where(np.arange(59) % 20 == 19, 50.0, rng.uniform(0.5, 1, 59))), 5),
        "w2 == 0 edges": (sorted_edges(*random_tree, np.where(np.arange(n - 1) % 3 == 0, 2.0, 0.0)), 5),
        "only w2 == 0 edges": (sorted_edges(*random_tree, np.zeros(n - 1)), 5),
        "two sides of w2 == 0": (sorted_edges(np.r_[np.arange(9), np.arange(10, 19), 0], np.r_[np.arange(1, 10), np.arange(11, 20), 19],
                                              np.r_[np.zeros(18), 4.0]), 10),
        "exactly min_cluster_size per side": (sides((12, 12), rng), 12),
        "one fewer than min_cluster_size on one side": (sides((12, 11), rng), 12),
        "one fewer on both sides": (sides((11, 11), rng), 12),
        "three sides": (sides((15, 9, 15), rng), 6),
        "four sides, one too small": (sides((8, 8, 3, 8), rng), 4),
        "no cluster at all": (sorted_edges(np.arange(5), np.arange(1, 6), rng.uniform(1, 2, 5)), 5),
        "two points": (sorted_edges(np.array([0]), np.array([1]), [1.0]), 2),
    }
    return cases


def test_hand_made_trees_are_what_they_say():
    cases = hand_made_trees()
    lo, hi, w2 = cases["exactly min_cluster_size per side"][0]
    assert sorted(np.unique(ho.labels_from_edges(lo, hi, w2, 12), return_counts=True)[1].tolist()) == [12, 12]
    for name in ("one fewer than min_cluster_size on one side", "one fewer on both sides", "no cluster at all", "two points"):
        edges, mcs = cases[name]
        assert (ho.labels_from_edges(*edges, mcs) == -1).all(), name
    labels = ho.labels_from_edges(*cases["path, three dense stretches"][0], 5)
    assert labels.max() == 2 and [len(set(labels[a:a + 20])) for a in (0, 20, 40)] == [1, 1, 1]


@pytest.mark.parametrize("name", sorted(hand_made_trees()))
def test_library_labels_equal_the_oracles_on_hand_made_trees(ops, name):
    edges, mcs = hand_made_trees()[name]
    want = ho.labels_from_edges(*edges, mcs)
    got = ops.hdbscan_labels_host(*edges, mcs)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("seed", SEEDS)
def test_library_labels_equal_the_oracles_on_the_blob_inputs(ops, seed):
    _, labels, edges = blob_case(seed)
    np.testing.assert_array_equal(ops.hdbscan_labels_host(*edges, 100), labels)
    for mcs in (2, 5, 30):                                                       # further selections over the same tree
        np.testing.assert_array_equal(ops.hdbscan_labels_host(*edges, mcs), ho.labels_from_edges(*edges, mcs))


def test_oracle_tree_is_the_unique_one_under_the_total_order():
    # an 4 x 4 x 4 lattice: every edge of length 1 ties; Prim from any start under the same order must give the same tree
    g = np.stack(np.meshgrid(*[np.arange(4.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    lo, hi, w2 = ho.mst(g, 2)
    w = ho.w2_matrix(g, 2)
    n = len(g)
    for start in (0, 21, 63):
        inside = {start}
        edges = set()
        while len(inside) < n:
            best = min((w[i, j], min(i, j), max(i, j)) for i in inside for j in range(n) if j not in inside)
            edges.add(best)
            inside.add(best[1] if best[1] not in inside else best[2])
        assert sorted(edges) == list(zip(w2.tolist(), lo.tolist(), hi.tolist()))


# ------------------------------------------------------------------------------------------------- the refusals that need no device
def test_host_labels_refusals(ops):
    lo, hi, w2 = sorted_edges(np.arange(5), np.arange(1, 6), np.arange(1.0, 6.0))
    for bad, text in (((lo, hi, w2[::-1].copy(), 5), "ascend"), ((hi, lo, w2, 5), "lo < hi"), ((lo, hi, w2, 1), "min_cluster_size"),
                      ((lo, hi, np.r_[w2[:4], np.nan], 5), "NaN"), ((np.zeros(5, np.int32), np.r_[1, 1, 2, 3, 4].astype(np.int32), w2, 5), "cycle")):
        with pytest.raises(RuntimeError, match=text):
            ops.hdbscan_labels_host(*bad)


def test_abi_refusals_come_before_any_launch(ops):
    from vfmreg import _lib
    lib = _lib.load()
    assert lib.vfm_mreach_mst_workspace_bytes(1000) >= 1000 * 48
    for args, text in (((1, 1, 1, 1, 1.0, 1, 1, 1, 1, None, None, 1, 1 << 30, None), b"n must be in 2"),
                       ((1, 1, 1, 10, 0.0, 1, 1, 1, 1, None, None, 1, 1 << 30, None), b"cell size"),
                       ((1, 1, 1, 10, float("nan"), 1, 1, 1, 1, None, None, 1, 1 << 30, None), b"cell size"),
                       ((1, 1, 1, 10, 1.0, None, 1, 1, 1, None, None, 1, 1 << 30, None), b"null"),
                       ((1, 1, 1, 10, 1.0, 1, 1, 1, 1, None, None, 1, 16, None), b"workspace")):
        assert lib.vfm_mreach_mst(*args) == -1 and text in lib.vfm_last_error(), text


def test_class_refusals_need_no_device():
    from vfmreg.clustering import HDBSCAN
    for kwargs in (dict(min_samples=0), dict(min_samples=65), dict(min_cluster_size=70), dict(min_cluster_size=1)):
        with pytest.raises(ValueError):
            HDBSCAN(**kwargs)
    for name, value in (("cluster_selection_epsilon", 0.5), ("max_cluster_size", 10), ("metric", "manhattan"), ("alpha", 1.5), ("p", 2),
                        ("algorithm", "boruvka_kdtree"), ("gen_min_span_tree", True), ("cluster_selection_method", "leaf"),
                        ("allow_single_cluster", True), ("prediction_data", True), ("match_reference_implementation", True),
                        ("cluster_selection_persistence", 0.1)):
        with pytest.raises(NotImplementedError, match=name):
            HDBSCAN(**{name: value})
    c = HDBSCAN(min_cluster_size=100, min_samples=25, approx_min_span_tree=False, core_dist_n_jobs=1, leaf_size=10)
    assert (c.min_cluster_size, c.min_samples) == (100, 25) and HDBSCAN(7).min_samples == 7
    with pytest.raises(ValueError, match="number of samples"):
        c.fit(np.zeros((24, 3)))
    with pytest.raises(ValueError, match="2 points"):
        HDBSCAN(5, 1).fit(np.zeros((1, 3)))
    with pytest.raises(NotImplementedError):
        c.fit(np.zeros((30, 2)))


# ------------------------------------------------------------------------------------------------- the coin per cluster
def test_remove_clusters_draws_one_coin_per_label_in_order():
    from vfmreg import utils
    rng = np.random.default_rng(3)
    del_idx = rng.permutation(500)[:200]
    labels = rng.integers(-1, 6, 200)
    for chance in (0.0, 0.3, 0.5, 1.0):
        got_del, got_keep = utils.remove_clusters(del_idx, labels, chance, np.random.RandomState(42))
        want = ho.remove_restated(del_idx, labels, chance, np.random.RandomState(42))
        np.testing.assert_array_equal(got_del, want)
        np.testing.assert_array_equal(np.sort(np.r_[got_del, got_keep]), np.sort(del_idx))
        draws = np.random.RandomState(42).standard_normal(6)
        kept = [k for k in range(6) if draws[k] > ho.norm_ppf(chance)]
        assert set(labels[np.isin(del_idx, got_del)]) == set(range(6)) - set(kept)
    assert len(utils.remove_clusters(del_idx, labels, 0.0, np.random.RandomState(1))[0]) == 0          # a chance of 0 removes nothing
    assert len(utils.remove_clusters(del_idx, labels, 1.0, np.random.RandomState(1))[0]) == np.sum(labels != -1)
    none_del, none_keep = utils.remove_clusters(del_idx, np.full(200, -1), 0.5, np.random.RandomState(1))
    assert len(none_del) == 0 and np.array_equal(none_keep, del_idx)
    try:
        from scipy.stats import norm
    except ImportError:
        return
    for p in (0.0, 1e-9, 0.25, 0.5, 0.9, 1.0):
        assert ho.norm_ppf(p) == pytest.approx(float(norm.ppf(p)), rel=1e-12)

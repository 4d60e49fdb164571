"""Exact HDBSCAN* on the GPU (csrc/hdbscan.hip ``vfm_mreach_mst``, csrc/hdbscan_host.cpp, ``vfmreg.clustering.HDBSCAN``,
``utils.filter_map_clusters``) against tests/hdbscan_oracle.py: the sorted edge list (lo, hi, w2) of the spanning tree EQUAL bit for
bit and the labels equal exactly -- on blobs at four ``min_samples``, on inputs where nearly every edge ties (a lattice, a cloud stored
three times), at the smallest sizes, on inputs that force many rounds or the scan of every point, at every extreme of the cell size, at
the clamped border of the grid, and with every output and the workspace between guard bytes."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import grid_border_cases as gb  # noqa: E402
from tests import hdbscan_oracle as ho  # noqa: E402
from tests import knn3_oracle  # noqa: E402
from tests.guarded import GuardedBuffer  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def product_tree(P, min_samples, cell=None):
    """((lo, hi, w2) sorted, rounds, fallbacks) from ops: the grid, the core distances, the tree"""
    from vfmreg import neighbors, ops
    pts = dev(P)
    grid = neighbors.choose_cell(pts) if cell is None else ops.nn3_build(pts, cell)
    _, d2, _ = ops.nn3_knn(grid, pts, min_samples)
    core2 = d2[:, min_samples - 1].contiguous()
    lo, hi, w2, rounds, fb = ops.mreach_mst(grid, core2, want_counts=True)
    assert lo.dtype == hi.dtype == torch.int32 and w2.dtype == torch.float64 and tuple(lo.shape) == tuple(w2.shape) == (len(P) - 1,)
    lo, hi, w2 = lo.cpu().numpy(), hi.cpu().numpy(), w2.cpu().numpy()
    order = np.lexsort((hi, lo, w2))
    return (lo[order], hi[order], w2[order]), int(rounds.item()), int(fb.item())


def check(P, min_samples, min_cluster_size=5, cell=None, msg=""):
    """the tree and the labels of the product against the oracle's; returns (rounds, fallbacks, labels)"""
    from vfmreg import ops
    want_labels, want = ho.hdbscan(P, min_cluster_size, min_samples)
    got, rounds, fb = product_tree(P, min_samples, cell)
    for g, w, what in zip(got, want, ("lo", "hi", "w2")):
        np.testing.assert_array_equal(g, w, err_msg=f"{msg} {what}")            # w2 bit for bit
    assert (got[2].view(np.int64) == want[2].view(np.int64)).all(), msg
    labels = ops.hdbscan_labels_host(*got, min_cluster_size)
    np.testing.assert_array_equal(labels, want_labels, err_msg=msg)
    assert 0 <= rounds <= max(1, math.ceil(math.log2(len(P))))
    return rounds, fb, labels


@pytest.mark.parametrize("min_samples", [1, 2, 25, 64])
def test_blobs(min_samples):
    P = ho.blobs(0)
    assert len(P) == 2700
    rounds, _, labels = check(P, min_samples, 100, msg=f"min_samples {min_samples}")
    assert rounds >= 2
    if min_samples == 25:
        from vfmreg.clustering import HDBSCAN
        c = HDBSCAN(min_cluster_size=100, min_samples=25)
        got = c.fit_predict(P.astype(np.float32))                               # float32 rows are widened: the same points
        assert got.dtype == np.int64 and c.labels_ is got and got.max() >= 3
        np.testing.assert_array_equal(got, labels)
        for g, w in zip(c._mst_, ho.mst(P, 25)):
            np.testing.assert_array_equal(g, w)
        np.testing.assert_array_equal(HDBSCAN(100, 25).fit(dev(P)).labels_, labels)     # a device tensor


@pytest.mark.parametrize("min_samples", [1, 2, 7])
def test_lattice_where_only_the_index_order_decides(min_samples):
    g = np.stack(np.meshgrid(*[np.arange(8.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    P = g[np.random.default_rng(5).permutation(len(g))]
    _, want = ho.hdbscan(P, 5, min_samples)
    assert len(np.unique(want[2])) <= 2                                         # nearly every edge ties
    check(P, min_samples, 5)
    check(g, min_samples, 5, msg="in lattice order")
    check(P, min_samples, 5, cell=0.5, msg="a point per cell")
    check(P, min_samples, 5, cell=3.0, msg="27 points per cell")


def test_every_point_stored_three_times():
    rng = np.random.default_rng(6)
    base = rng.uniform(-3, 3, (250, 3))
    P = np.concatenate([base, base, base])[rng.permutation(750)]
    _, want = ho.hdbscan(P, 10, 3)
    assert (ho.core2(P, 3) == 0).all() and np.sum(want[2] == 0) == 500          # core2 = 0: lambda = inf inside every triple
    check(P, 3, 10)
    check(P, 3, 3, msg="min_cluster_size 3: the triples are clusters born at lambda = inf")
    check(P, 2, 10, msg="min_samples 2")


def test_smallest_sizes():
    from vfmreg.clustering import HDBSCAN
    rng = np.random.default_rng(8)
    two = np.array([[0.0, 0, 0], [1.0, 2, 2]])
    for ms in (1, 2):
        rounds, _, labels = check(two, ms, 2)
        assert rounds == 1 and labels.tolist() == [-1, -1]
    check(np.zeros((2, 3)), 2, 2, msg="two equal points")
    for n in (3, 25, 64):                                                       # n = min_samples: every core2 is the farthest point's d2
        P = rng.normal(0, 1, (n, 3))
        check(P, n, 2, msg=f"n = min_samples = {n}")
        assert HDBSCAN(5, n).fit(P).labels_.shape == (n,)
    with pytest.raises(ValueError):
        HDBSCAN(5, 26).fit(rng.normal(0, 1, (25, 3)))
    bad = rng.normal(0, 1, (30, 3))
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        HDBSCAN(5, 3).fit(bad)
    bad[7, 1] = np.inf
    with pytest.raises(ValueError, match="infinite"):
        HDBSCAN(5, 3).fit(bad)


def test_collinear_points_whose_gaps_double_force_many_rounds():
    # gaps 1, 2, 1, 4, 1, 2, 1, 8, ...: every round joins neighbouring components in pairs, so the components only halve.  (Gaps that
    # double from one point to the next -- 1, 2, 4, 8, ... -- are the second input: each point hooks to its left neighbour and ONE round
    # joins the whole chain, which is why the first input is the one the rounds are counted on.)
    n = 64
    k = np.arange(1, n)
    gaps = (k & -k).astype(np.float64)                                          # the largest power of two that divides k
    x = np.r_[0.0, np.cumsum(gaps)]
    P = np.c_[x, np.zeros(n), np.zeros(n)]
    rounds, _, _ = check(P, 1, 2, msg="ruler gaps")
    assert rounds > 1 and rounds <= math.ceil(math.log2(n))
    assert rounds == 6
    rounds, _, _ = check(P[np.random.default_rng(9).permutation(n)] * 0.37, 2, 4, msg="ruler gaps, shuffled, min_samples 2")
    assert 1 < rounds <= math.ceil(math.log2(n))
    x = np.r_[0.0, np.cumsum(2.0 ** np.arange(39))]
    check(np.c_[np.zeros(40), x, np.zeros(40)], 1, 2, msg="gaps 1, 2, 4, ...")
    check(np.c_[np.zeros(40), x, x], 3, 2, msg="gaps 1, 2, 4, ..., min_samples 3")


def test_two_blobs_far_apart_fall_back_to_the_scan():
    rng = np.random.default_rng(10)
    P = np.concatenate([rng.normal(0, 1, (200, 3)), rng.normal(0, 1, (230, 3)) + np.array([1e6, 0, 0])])
    P = P[rng.permutation(len(P))].astype(np.float32).astype(np.float64)
    rounds, fb, labels = check(P, 5, 50)
    assert fb > 0 and rounds >= 2 and sorted(np.unique(labels).tolist()) == [0, 1]


def test_extreme_cells():
    P = ho.blobs(1, per_blob=80, n_blobs=4, n_uniform=60)
    n = len(P)
    _, fb, _ = check(P + 30.0, 5, 20, cell=1e9, msg="one cell for all points")
    assert fb == 0
    _, fb, _ = check(P, 5, 20, cell=1e-4, msg="cells of 0.1 mm")
    assert fb >= 0.9 * n                                                        # the first round's walks read every point (all but a pair that shares its 27 cells)


@pytest.mark.parametrize("cell", [0.5, 1e-7])
def test_clamped_border(cell):
    """the cloud of tests/grid_border_cases.py: sub-clouds astride and beyond the clamp of the cell index in one, two and three axes,
    with repeated points on both sides of it"""
    P, names = gb.nn3_cloud(cell, seed=3, per=200)
    c = gb.cells(P, cell, gb.NN3_L)
    assert (np.abs(c) == gb.NN3_L).any(axis=1).sum() > 300 and len(P) <= 2000
    check(P, 4, 30, cell=cell)
    check(P, 1, 30, cell=cell, msg="min_samples 1")


def test_outputs_and_workspace_stay_inside_their_buffers():
    from vfmreg import _lib, neighbors, ops
    lib = _lib.load()
    P = ho.blobs(2, per_blob=100, n_blobs=3, n_uniform=33)
    n = len(P)
    pts = dev(P)
    grid = neighbors.choose_cell(pts)
    _, d2, _ = ops.nn3_knn(grid, pts, 6)
    core2 = GuardedBuffer(n, torch.float64).set(d2[:, 5])
    core2.poison_guards("nan")
    lo, hi = GuardedBuffer(n - 1, torch.int32).fill_bytes(0xFF), GuardedBuffer(n - 1, torch.int32).fill_bytes(0xFF)
    w2 = GuardedBuffer(n - 1, torch.float64).fill_nan()
    rounds, fb = GuardedBuffer(1, torch.int32).fill_bytes(0xFF), GuardedBuffer(1, torch.int32).fill_bytes(0xFF)
    need = lib.vfm_mreach_mst_workspace_bytes(n)
    ws = GuardedBuffer(need, torch.uint8).fill_bytes(0xFF)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.vfm_mreach_mst(grid.keys.data_ptr(), grid.order.data_ptr(), grid.sorted.data_ptr(), n, grid.cell, core2.ptr(), lo.ptr(), hi.ptr(),
                              w2.ptr(), rounds.ptr(), fb.ptr(), ws.ptr(), need - 1, stream) == -1           # refused before any launch
    assert b"workspace" in lib.vfm_last_error()
    _lib.check(lib.vfm_mreach_mst(grid.keys.data_ptr(), grid.order.data_ptr(), grid.sorted.data_ptr(), n, grid.cell, core2.ptr(), lo.ptr(),
                                  hi.ptr(), w2.ptr(), rounds.ptr(), fb.ptr(), ws.ptr(), need, stream), "mreach_mst")
    torch.cuda.synchronize()
    for name, buf in (("core2", core2), ("lo", lo), ("hi", hi), ("w2", w2), ("rounds", rounds), ("fallbacks", fb), ("workspace", ws)):
        assert buf.intact(), f"{name}: {buf.intact()}"
    got = (lo.numpy(), hi.numpy(), w2.numpy())
    order = np.lexsort((got[1], got[0], got[2]))
    for g, w in zip(got, ho.mst(P, 6)):
        np.testing.assert_array_equal(g[order], w)
    assert 2 <= rounds.numpy()[0] <= 9 and fb.numpy()[0] >= 0
    # the counts are optional
    _lib.check(lib.vfm_mreach_mst(grid.keys.data_ptr(), grid.order.data_ptr(), grid.sorted.data_ptr(), n, grid.cell, core2.ptr(), lo.ptr(),
                                  hi.ptr(), w2.ptr(), None, None, ws.ptr(), need, stream), "mreach_mst")
    torch.cuda.synchronize()
    assert all(b.intact() for b in (lo, hi, w2, ws))
    np.testing.assert_array_equal(np.sort(w2.numpy()), ho.mst(P, 6)[2])


# ------------------------------------------------------------------------------------------------- the map filter
@pytest.fixture(scope="module")
def filter_scene():
    """~2500 points: five dense 'trees', a ground plane, 60 isolated candidates, a bush of 70; the oracle's grown set and labels of it, once"""
    rng = np.random.default_rng(21)
    centres = np.array([[0, 0, 3], [9, 1, 3], [-8, 4, 3], [3, -9, 3], [-5, -7, 3.0]])
    trees = np.concatenate([c + rng.normal(0, 1, (340, 3)) * np.array([0.6, 0.6, 1.2]) for c in centres])
    ground = np.c_[rng.uniform(-14, 14, (640, 2)), rng.normal(0, 0.02, 640)]
    lonely = np.c_[rng.uniform(-14, 14, (60, 2)), rng.uniform(8, 12, 60)]
    bush = np.array([12.0, -12, 1]) + rng.uniform(0, 1, (70, 3)) * np.array([2, 2, 1.5])      # dense enough to stay, too small for a cluster
    xyz = np.concatenate([trees, ground, lonely, bush]).astype(np.float32)
    perm = rng.permutation(len(xyz))
    xyz = xyz[perm]
    is_candidate = np.r_[rng.random(len(trees)) < 0.7, np.zeros(len(ground), bool), np.ones(len(lonely) + len(bush), bool)][perm]
    del_idx = rng.permutation(np.flatnonzero(is_candidate))
    grown, _ = knn3_oracle.grow_restated(xyz, del_idx)
    labels, _ = ho.hdbscan(xyz[grown, :3].astype(np.float32).astype(np.float64), 100, 25)
    assert 2000 <= len(xyz) <= 3000 and len(grown) < len(del_idx) + 1000 and labels.max() >= 2 and (labels == -1).any()
    return dict(xyz=xyz, del_idx=del_idx, grown=grown, labels=labels)


@pytest.mark.parametrize("remove_chance", [0.0, 0.5, 1.0])
def test_filter_map_clusters(filter_scene, remove_chance):
    from vfmreg import utils
    s = filter_scene
    want_del = ho.remove_restated(s["grown"], s["labels"], remove_chance, np.random.RandomState(42))
    want_keep = np.delete(np.arange(len(s["xyz"])), want_del)
    got_del, got_keep = utils.filter_map_clusters(s["xyz"], s["del_idx"], remove_chance, np.random.RandomState(42))
    np.testing.assert_array_equal(got_del, want_del)
    np.testing.assert_array_equal(got_keep, want_keep)
    if remove_chance == 0.0:
        assert len(got_del) == 0
    if remove_chance == 1.0:
        assert len(got_del) == np.sum(s["labels"] != -1)
    if remove_chance == 0.5:
        assert 0 < len(got_del) < np.sum(s["labels"] != -1)                     # RandomState(42) keeps some clusters and removes others
        full_del, full_keep = ho.filter_restated(s["xyz"], s["del_idx"], remove_chance, np.random.RandomState(42))
        np.testing.assert_array_equal(got_del, full_del)
        np.testing.assert_array_equal(got_keep, full_keep)

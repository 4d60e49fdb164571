"""CPU checks of the k-NN oracle (tests/knn3_oracle.py): anchored against sklearn's KDTree on tie-free inputs and, where faiss imports,
its restated ``FaissKNeighbors`` against the reference's own class body on inputs whose cuts have a margin; the oracle's order, cap and
padding on hand-made inputs; and the argument checks of ``KDTree.query_knn``, ``FaissKNeighbors`` and ``vfm_nn3_knn`` that need no device."""
import numpy as np
import pytest

from tests import knn3_oracle, nn3_oracle


def test_oracle_equals_sklearn_kdtree_bit_for_bit():
    neighbors = pytest.importorskip("sklearn.neighbors", reason="sklearn is absent: the oracle is not compared with KDTree.query(k)")
    rng = np.random.default_rng(0)
    for n, nq, scale, k in ((3000, 400, 30.0, 10), (1200, 300, 5.0, 50), (70, 50, 1.0, 64), (9, 20, 1.0, 9)):
        P = rng.uniform(-scale, scale, (n, 3))
        Q = np.concatenate([P[rng.integers(0, n, nq // 2)] + rng.normal(0, 1e-4, (nq // 2, 3)), rng.uniform(-2 * scale, 2 * scale, (nq - nq // 2, 3))])
        dist, ind = neighbors.KDTree(P, metric="euclidean").query(Q, k=k, return_distance=True)
        idx, d2, count = knn3_oracle.knn(P, Q, k)
        assert (count == k).all() and (np.diff(d2, axis=1) > 0).all()          # tie-free
        np.testing.assert_array_equal(idx, ind)
        np.testing.assert_array_equal(np.sqrt(d2), dist)                       # bit-equal


def test_restated_faiss_class_equals_faiss_where_the_cuts_have_a_margin():
    faiss = pytest.importorskip("faiss", reason="faiss is absent: the restated FaissKNeighbors is not compared with IndexFlatL2")
    rng = np.random.default_rng(1)
    P = rng.uniform(-4, 4, (2000, 3)).astype(np.float32)
    y = rng.permutation(5000)[:2000]
    Q = np.concatenate([P[:200], rng.uniform(-4, 4, (200, 3)).astype(np.float32)])
    ours = knn3_oracle.FaissRestated()
    ours.fit(P, y)
    index = faiss.IndexFlatL2(3)
    index.add(P)
    for k, r in ((10, .5), (50, .5)):
        d2, idx = ours.search(Q, k)
        real = d2[np.isfinite(d2)]
        assert not (np.abs(real - r) <= 1e-4 * r).any()                        # no d2 within 1e-4 relative of r
        assert not ((real != 0) & (real <= 1e-6)).any()                        # none within 1e-6 of 0 other than exact zeros
        fd, fi = index.search(Q, k)
        sel = (fd.flatten() > 0) & (fd.flatten() < r)
        np.testing.assert_array_equal(ours.query(Q, k, r), np.unique(y[fi.flatten()[sel]]))
        np.testing.assert_array_equal(ours.n_neighbors_in_radius(Q, k, r), np.sum((fd > 0) & (fd <= r) & (fi != -1), axis=1))


def test_oracle_order_cap_and_padding():
    P = np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, 0], [-1.0, 0, 0], [3.0, 0, 0], [np.nan, 0, 0]])
    Q = np.array([[0.0, 0, 0], [1.0, 0, 0], [np.nan, 0, 0]])
    idx, d2, count = knn3_oracle.knn(P, Q, 7)
    assert idx.tolist() == [[0, 1, 2, 3, 4, -1, -1], [0, 2, 1, 3, 4, -1, -1], [-1] * 7]       # equal d2: the lower index first
    assert d2[0].tolist() == [1.0, 1.0, 1.0, 1.0, 9.0, np.inf, np.inf] and d2[1, :5].tolist() == [0.0, 0.0, 2.0, 4.0, 4.0]
    assert count.tolist() == [5, 5, 0] and np.isinf(d2[2]).all()
    idx, d2, count = knn3_oracle.knn(P, Q[:2], 3, max_d2=2.0)                                 # the cap is inclusive
    assert idx.tolist() == [[0, 1, 2], [0, 2, 1]] and count.tolist() == [3, 3]
    idx, d2, count = knn3_oracle.knn(P, Q[:2], 3, max_d2=0.5)
    assert idx.tolist() == [[-1, -1, -1], [0, 2, -1]] and count.tolist() == [0, 2]
    i1, d1, _ = knn3_oracle.knn(P[:5], Q[:2], 1)                                              # k = 1 is the 1-NN oracle
    w_i, w_d = nn3_oracle.nearest(P[:5], Q[:2])
    assert i1[:, 0].tolist() == w_i.tolist() and np.sqrt(d1[:, 0]).tolist() == w_d.tolist()
    idx, d2, count = knn3_oracle.knn(P, np.zeros((0, 3)), 4)
    assert idx.shape == d2.shape == (0, 4) and count.shape == (0,)


def test_the_two_oracles_state_one_order_on_exact_ties():
    """nn3_oracle.nearest(P, Q) is knn3_oracle.knn(P, Q, 1): the same index among equal distances, the same bits of the distance"""
    g = np.arange(8, dtype=np.float64)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    P = P[np.random.default_rng(3).permutation(len(P))]
    Q = np.concatenate([P[:150], P[150:300] + 0.5])                          # lattice points and cell centres (8 equal distances)
    rng = np.random.default_rng(4)
    base = rng.uniform(-3, 3, (300, 3))
    P3 = np.concatenate([base, base, base])[rng.permutation(900)]            # every point three times
    Q3 = np.concatenate([base[:200], rng.uniform(-3, 3, (100, 3))])
    for points, queries in ((P, Q), (P3, Q3)):
        idx, d2, count = knn3_oracle.knn(points, queries, 1)
        w_i, w_d = nn3_oracle.nearest(points, queries)
        tied = (((points[None, :, :] - queries[:, None, :]) ** 2).sum(-1) == d2[:, :1]).sum(1)
        assert (tied > 1).sum() >= 140                                       # the inputs do hold ties (a centre beyond the last plane: fewer)
        assert (count == 1).all()
        np.testing.assert_array_equal(idx[:, 0], w_i)
        np.testing.assert_array_equal(np.sqrt(d2[:, 0]), w_d)                # bit-equal


def test_restated_class_keeps_the_reference_quirks():
    P = np.array([[0.0, 0, 0], [0.5, 0, 0], [0, 0.7, 0], [0, 0, 1.0], [0.0, 0, 0]])           # squared distances from the origin: 0, .25, .49, 1, 0
    y = np.array([40, 30, 20, 10, 50])
    f = knn3_oracle.FaissRestated()
    f.fit(P, y)
    o = np.zeros((1, 3))
    d2 = knn3_oracle.knn(P.astype(np.float32).astype(np.float64), o, 5)[1][0]
    assert f.query(o, 5, float(d2[3])).tolist() == [30]                      # r against the SQUARED distance, d2 < r strict, zeros dropped
    assert f.n_neighbors_in_radius(o, 5, float(d2[3])).tolist() == [2]       # ... and d2 <= r inclusive
    assert f.query(o, 2, 5.0).tolist() == []                                 # the two zero-distance hits occupy both slots
    assert f.query(o, 3, 5.0).tolist() == [30]
    assert f.n_neighbors_in_radius(o, 10, 5.0).tolist() == [3]               # padded slots are not counted
    assert f.query(np.array([[0.0, 0, 0], [0, 0, 1.0]]), 4, 5.0).tolist() == [20, 30, 40, 50]   # unique and sorted over all rows


def test_query_knn_and_faiss_stand_in_argument_checks():
    pytest.importorskip("torch")
    from vfmreg import ops, utils
    from vfmreg.neighbors import KDTree
    tree = KDTree.__new__(KDTree)                                            # no device here: the checks come before the search
    tree.grid = ops.Nn3Grid(None, None, None, 1.0, 5)
    with pytest.raises(ValueError, match="at least 1"):
        tree.query_knn(np.zeros((2, 3)), 0)
    with pytest.raises(ValueError, match="less than or equal to the number of training points"):
        tree.query_knn(np.zeros((2, 3)), 6)
    tree.grid = ops.Nn3Grid(None, None, None, 1.0, 500)
    with pytest.raises(NotImplementedError, match="64"):
        tree.query_knn(np.zeros((2, 3)), 65)
    with pytest.raises(ValueError, match="dimension"):
        tree.query_knn(np.zeros((2, 2)), 3)
    with pytest.raises(NotImplementedError):
        tree.query(np.zeros((2, 3)), k=2)                                    # k > 1 stays out of query()
    assert "query_knn" in KDTree.query.__doc__
    knn = utils.FaissKNeighbors()
    with pytest.raises(RuntimeError, match="fit"):
        knn.query(np.zeros((2, 3)), 10, .5)
    with pytest.raises(ValueError, match="Invalid shape"):
        knn.fit(np.zeros((4, 2)), np.arange(4))
    with pytest.raises(ValueError, match="labels"):
        knn.fit(np.zeros((4, 3)), np.arange(3))
    knn.fit(np.zeros((0, 3)), np.zeros(0, dtype=np.int64))                   # an empty index needs no device: faiss answers with padding
    assert knn.query(np.ones((3, 3)), 10, .5).tolist() == [] and knn.n_neighbors_in_radius(np.ones((3, 3)), 10, .5).tolist() == [0, 0, 0]
    for k in (0, 65):
        with pytest.raises(NotImplementedError):
            knn.query(np.zeros((2, 3)), k, .5)
    with pytest.raises(ValueError, match="Invalid shape"):
        knn.n_neighbors_in_radius(np.zeros((2, 4)), 10, .5)
    assert "fp32" in utils.FaissKNeighbors.__doc__ and "lower index" in utils.FaissKNeighbors.__doc__


def test_nn3_knn_entry_point_checks_its_arguments_on_the_host():
    pytest.importorskip("torch")
    from vfmreg import _lib
    lib = _lib.load()
    assert "vfm_nn3_knn" in _lib.SIGNATURES
    inf = float("inf")
    call = lambda n=10, cell=0.5, nq=5, k=10, cap=inf, keys=1: lib.vfm_nn3_knn(keys, 1, 1, n, cell, 1, nq, k, cap, 1, 1, 1, None, None)
    assert call(k=0) == -1 and b"k must be in 1..64" in lib.vfm_last_error()
    assert call(k=65) == -1 and b"k must be in 1..64" in lib.vfm_last_error()
    assert call(cap=-1e-300) == -1 and b"max_d2" in lib.vfm_last_error()
    assert call(cap=float("nan")) == -1 and b"max_d2" in lib.vfm_last_error()
    assert call(n=0) == -1 and b"empty cloud" in lib.vfm_last_error()
    assert call(n=(1 << 26) + 1) == -1
    assert call(cell=0.0) == -1 and b"cell" in lib.vfm_last_error()
    assert call(nq=-1) == -1
    assert call(keys=None) == -1 and b"null pointer" in lib.vfm_last_error()

"""The oracle of the exact 3-D k-nearest-neighbour search (csrc/nn3.hip ``nn3_knn_kernel``, ``ops.nn3_knn``, ``KDTree.query_knn``) and of
the stand-ins built on it (``vfmreg.utils.FaissKNeighbors``, ``grow_deletion_set``), in numpy fp64.

``knn`` is brute force: d2 = (dx*dx + dy*dy) + dz*dz per query, the candidates are the points whose d2 is no NaN and at most the
(inclusive) cap, their order is (d2, index), the first k are the row and the rest of it is (-1, +inf).  On tie-free inputs it gives the
indices and, after the root, the bit-equal distances of ``sklearn.neighbors.KDTree.query(Q, k)`` (tests/test_knn3_oracle.py compares
where sklearn imports).  ``FaissRestated`` restates the three methods of vfm_reg/utils.py:19-44 on top of it and ``grow_restated`` the
map filter of registration_node.py:704-717."""
from __future__ import annotations

import numpy as np


def knn(points: np.ndarray, queries: np.ndarray, k: int, max_d2: float = np.inf):
    """(idx int64[K, k], d2 fp64[K, k], count int32[K]) of the k nearest of ``points`` (n x 3) for every row of ``queries``."""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    q = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 3)
    idx = np.full((len(q), k), -1, dtype=np.int64)
    d2 = np.full((len(q), k), np.inf, dtype=np.float64)
    count = np.zeros(len(q), dtype=np.int32)
    rows = np.arange(len(p))
    with np.errstate(invalid="ignore", over="ignore"):
        for i, c in enumerate(q):
            dx, dy, dz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
            d = (dx * dx + dy * dy) + dz * dz
            ok = d <= max_d2                                  # (False for a NaN)
            cand, dc = rows[ok], d[ok]
            first = np.lexsort((cand, dc))[:k]
            count[i] = len(first)
            idx[i, :len(first)] = cand[first]
            d2[i, :len(first)] = dc[first]
    return idx, d2, count


class FaissRestated:
    """vfm_reg/utils.py:19-44 with ``knn`` for ``faiss.IndexFlatL2.search``: float32 points and queries (widened to fp64 for the
    search), ``r`` against the SQUARED distance, the cuts after the search."""

    def fit(self, X, y):
        self.points = np.asarray(X).astype(np.float32).astype(np.float64)
        self.y = np.asarray(y)

    def search(self, X, k):
        idx, d2, _ = knn(self.points, np.asarray(X).astype(np.float32).astype(np.float64), k)
        return d2, idx

    def query(self, X, k, r):                     # utils.py:30-37
        d2, idx = self.search(X, k)
        take = (d2 > 0) & (d2 < r)
        return np.unique(self.y[idx[take]])

    def n_neighbors_in_radius(self, X, k, r):     # utils.py:39-44
        d2, idx = self.search(X, k)
        return np.sum((d2 > 0) & (d2 <= r) & (idx != -1), axis=1)


def grow_restated(xyz: np.ndarray, del_idx: np.ndarray):
    """registration_node.py:704-717: (del_idx, keep_idx) after the isolated candidates are dropped and the set has grown."""
    everything = np.arange(len(xyz))
    first = FaissRestated()
    first.fit(xyz[del_idx, :3], del_idx)
    dense = first.n_neighbors_in_radius(xyz[del_idx, :3], 10, .5) >= 3
    del_idx = del_idx[dense]
    keep_idx = np.delete(everything, del_idx)
    second = FaissRestated()
    second.fit(xyz[keep_idx, :3], keep_idx)
    del_idx = np.concatenate([del_idx, second.query(xyz[del_idx, :3], 50, .5)])
    return del_idx, np.delete(everything, del_idx)

"""The oracle of the exact 3-D 1-nearest-neighbour search (csrc/nn3.hip, vfmreg/neighbors.py) and of the row filter of
registration_node.py:301-309, in numpy fp64.

``nearest`` is brute force: d2 = (dx*dx + dy*dy) + dz*dz, the arg-min with the lower index on equal d2, dist = sqrt(d2).  On tie-free
inputs it gives the indices and bit-equal distances of ``sklearn.neighbors.KDTree(P, metric="euclidean").query(Q, k=1)``
(tests/test_nn3_oracle.py makes that comparison where sklearn imports)."""
from __future__ import annotations

import numpy as np


def nearest(points: np.ndarray, queries: np.ndarray, chunk: int | None = None):
    """(idx int64[K], dist fp64[K]) of the nearest of ``points`` (n x 3) for every row of ``queries`` (K x 3)."""
    p = np.ascontiguousarray(points, dtype=np.float64)
    q = np.ascontiguousarray(queries, dtype=np.float64)
    if p.shape[0] == 0:
        raise ValueError("Found array with 0 sample(s) while a minimum of 1 is required")
    if chunk is None:
        chunk = max(1, min(1024, 4_000_000 // len(p)))   # ~32 MB per temporary
    idx = np.empty(len(q), dtype=np.int64)
    d2 = np.empty(len(q), dtype=np.float64)
    px, py, pz = p[:, 0][None, :], p[:, 1][None, :], p[:, 2][None, :]
    for s in range(0, len(q), chunk):
        c = q[s:s + chunk]
        dx, dy, dz = px - c[:, 0:1], py - c[:, 1:2], pz - c[:, 2:3]
        d = (dx * dx + dy * dy) + dz * dz
        j = np.argmin(d, axis=1)                     # numpy: the first of equal minima = the lower index
        idx[s:s + chunk] = j
        d2[s:s + chunk] = d[np.arange(len(c)), j]
    return idx, np.sqrt(d2)


def filter_pairs(src_indices, src_dist, tgt_indices, tgt_dist) -> np.ndarray:
    """RN:301-309 restated on flat arrays: the surviving (source row, target row) pairs, K' x 2 int64."""
    src_indices, src_dist, tgt_indices, tgt_dist = (np.asarray(a).reshape(-1) for a in (src_indices, src_dist, tgt_indices, tgt_dist))
    if src_dist.max() > .001 or tgt_dist.max() > .001:
        tgt_indices = tgt_indices[src_dist < .001]
        tgt_dist = tgt_dist[src_dist < .001]
        src_indices = src_indices[src_dist < .001]
        src_dist = src_dist[src_dist < .001]
        src_indices = src_indices[tgt_dist < .001]
        tgt_indices = tgt_indices[tgt_dist < .001]
    return np.stack((src_indices, tgt_indices), axis=1).astype(np.int64)

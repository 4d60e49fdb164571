"""Stand-in for ``hdbscan.HDBSCAN`` as registration_node.py:14 imports and RN:735-736 uses it: exact HDBSCAN* in 3-D.

    clusterer = HDBSCAN(min_cluster_size=100, min_samples=25)
    cluster_labels = clusterer.fit_predict(local_map[del_idx, :3])

The definition, stated so that the answer is unique: points in fp64 (float32 rows are widened),
``d2 = (dx*dx + dy*dy) + dz*dz``; ``core2[i]`` is the d2 of the ``min_samples``-th nearest point of the set, i itself included;
``w2(i, j) = max(core2[i], core2[j], d2(i, j))``; THE minimum spanning tree is the unique one under the total order
``(w2, min(i, j), max(i, j))`` on edges (csrc/hdbscan.hip, Boruvka on the grid of csrc/nn3.hip); single linkage, condensed tree,
stabilities and excess-of-mass selection as ``sklearn.cluster._hdbscan._tree`` computes them with ``allow_single_cluster=False`` and
``cluster_selection_epsilon=0`` (csrc/hdbscan_host.cpp, on the host).  Clusters are numbered 0.. in ascending condensed-tree node,
noise is -1.  Only labels are produced.

Deviations from the library the reference calls: that one builds an approximate spanning tree by default
(``approx_min_span_tree=True``) on rooted distances and leaves ties to its tree builder; here the tree is exact, every order is decided
on squares and ties go to the lower indices.  Labels therefore agree up to the points whose membership a tie decides.
"""
from __future__ import annotations

import numpy as np
import torch

from . import neighbors, ops

# the constructor of hdbscan.HDBSCAN: names and defaults.  The options in _NO_EFFECT change how that library computes, not what an
# exact computation returns, and are accepted with any value.
_DEFAULTS = dict(cluster_selection_epsilon=0.0, max_cluster_size=0, metric="euclidean", alpha=1.0, p=None, algorithm="best", leaf_size=40,
                 memory=None, approx_min_span_tree=True, gen_min_span_tree=False, core_dist_n_jobs=4, cluster_selection_method="eom",
                 allow_single_cluster=False, prediction_data=False, match_reference_implementation=False)
_NO_EFFECT = ("leaf_size", "memory", "approx_min_span_tree", "core_dist_n_jobs")


class HDBSCAN:
    def __init__(self, min_cluster_size=5, min_samples=None, cluster_selection_epsilon=0.0, max_cluster_size=0, metric="euclidean",
                 alpha=1.0, p=None, algorithm="best", leaf_size=40, memory=None, approx_min_span_tree=True, gen_min_span_tree=False,
                 core_dist_n_jobs=4, cluster_selection_method="eom", allow_single_cluster=False, prediction_data=False,
                 match_reference_implementation=False, **kwargs):
        given = dict(locals())
        for name, default in _DEFAULTS.items():
            if name not in _NO_EFFECT and given[name] != default:
                raise NotImplementedError(f"{name} = {given[name]!r}: only the default ({default!r}) is implemented (registration_node.py:735)")
        if kwargs:
            raise NotImplementedError(f"unsupported arguments: {sorted(kwargs)}")
        self.min_cluster_size = int(min_cluster_size)
        self.min_samples = self.min_cluster_size if min_samples is None else int(min_samples)
        if self.min_cluster_size < 2:
            raise ValueError(f"min_cluster_size = {min_cluster_size}: must be at least 2")
        if not 1 <= self.min_samples <= ops.NN3_KNN_MAX_K:
            raise ValueError(f"min_samples = {self.min_samples}: 1..{ops.NN3_KNN_MAX_K} are implemented (the k-nearest search's limit)")
        self.labels_ = None
        self._mst_ = None          # (lo int32[n-1], hi int32[n-1], w2 fp64[n-1]) ascending in (w2, lo, hi), numpy
        self._counts_ = None       # (Boruvka rounds that did work, searches that read every point)

    def fit(self, X, y=None):
        device_in = isinstance(X, torch.Tensor)
        shape = tuple(X.shape) if device_in else np.shape(X)
        if len(shape) != 2 or shape[1] != 3:
            raise NotImplementedError(f"shape {shape}: only N x 3 points are implemented")
        n = shape[0]
        if n < max(self.min_samples, 2):
            raise ValueError(f"min_samples ({self.min_samples}) must be at most the number of samples in X ({n}), and 2 points at least")
        pts = X.to(torch.float64).contiguous() if device_in else torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).cuda()
        if not bool(torch.isfinite(pts).all()):
            raise ValueError("X contains a NaN or an infinite coordinate")
        grid = neighbors.choose_cell(pts)
        _, d2, _ = ops.nn3_knn(grid, pts, self.min_samples)
        core2 = d2[:, self.min_samples - 1].contiguous()
        lo, hi, w2, rounds, fallbacks = ops.mreach_mst(grid, core2, want_counts=True)
        lo, hi, w2 = lo.cpu().numpy(), hi.cpu().numpy(), w2.cpu().numpy()
        order = np.lexsort((hi, lo, w2))
        self._mst_ = (lo[order], hi[order], w2[order])
        self._counts_ = (int(rounds.item()), int(fallbacks.item()))
        self.labels_ = ops.hdbscan_labels_host(*self._mst_, self.min_cluster_size).astype(np.int64)
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

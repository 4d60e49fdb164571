"""Mirror of the hot-path helpers of vfm_reg.utils: ``transform_pcl`` (vfm_reg/utils.py:47-54) and ``FaissKNeighbors``
(vfm_reg/utils.py:19-44) with the map filter that uses it (registration_node.py:684-792: the colour gate ``colour_gate``,
``grow_deletion_set``, ``remove_clusters``, both around the clustering in ``filter_map_clusters``, and the whole of it behind
``run_pca`` in ``filter_map_semantic``)."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import neighbors, ops


def transform_pcl(pcl: np.ndarray, transform: np.ndarray) -> np.ndarray:
    """xyz' = T @ [xyz; 1] in fp64 on the GPU, descriptors carried through, cast back to pcl.dtype."""
    assert transform.shape == (4, 4), "Invalid shape"
    xyz = torch.from_numpy(np.ascontiguousarray(pcl[:, :3], dtype=np.float64)).cuda()
    T = torch.from_numpy(np.ascontiguousarray(transform, dtype=np.float64)).cuda()
    out = ops.transform_xyz(xyz, T).cpu().numpy()
    pcl_out = np.c_[out, pcl[:, 3:]]
    assert pcl_out.shape == pcl.shape
    return pcl_out.astype(pcl.dtype)


class FaissKNeighbors:
    """``vfm_reg.utils.FaissKNeighbors`` (utils.py:19-44) on the exact 3-D k-NN search of csrc/nn3.hip instead of a
    ``faiss.IndexFlatL2``: numpy in, numpy out, N x 3 points, k <= 64.

    ``fit`` casts to float32 as the reference does; the search runs on those float32 coordinates widened to fp64.  The reference's
    quirks stay: ``r`` is compared with the SQUARED distance; ``query`` keeps ``0 < d2 < r`` and returns ``np.unique(y[...])``;
    ``n_neighbors_in_radius`` counts ``0 < d2 <= r``; hits at distance zero still occupy their slots among the k, because the cut
    comes after the search; rows with fewer than k points are padded as faiss pads them (index -1), and the cuts drop the padding.

    Deviation: faiss computes the distances in fp32, and for larger batches as ``|x|^2 + |y|^2 - 2 x.y``; here
    ``d2 = (dx*dx + dy*dy) + dz*dz`` in fp64.  A point within fp32 rounding of ``r``, or two points within rounding of each other
    (a ``d2`` that faiss rounds to 0 or to a negative number), may fall on the other side of a cut there.  Equal distances go to the
    lower index here; faiss leaves them open."""

    def __init__(self):
        self.index = None      # the grid of the fitted points (None: not fitted, or fitted with no points)
        self.y = None
        self._n = None

    def fit(self, X, y):
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != 3:
            raise ValueError(f"Invalid shape {X.shape}: only N x 3 points are implemented")
        y = np.asarray(y)
        if len(y) != len(X):
            raise ValueError(f"{len(X)} points but {len(y)} labels")
        self._n = len(X)
        self.y = y
        self.index = None
        if self._n:
            pts = torch.from_numpy(np.ascontiguousarray(X.astype(np.float32), dtype=np.float64)).cuda()
            self.index = neighbors.choose_cell(pts)

    def _search(self, X, k, r):
        """(idx int64[K, k], d2 fp64[K, k]) on the device: faiss's ``index.search(X.astype(np.float32), k)`` with its (-1, huge)
        padding.  A cap changes no row that passes the cuts (both cuts drop d2 > r) and ends the search sooner."""
        if self._n is None:
            raise RuntimeError("FaissKNeighbors: fit() first")
        k = int(k)
        if not 1 <= k <= ops.NN3_KNN_MAX_K:
            raise NotImplementedError(f"k = {k}: 1..{ops.NN3_KNN_MAX_K} neighbours are implemented")
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != 3:
            raise ValueError(f"Invalid shape {X.shape}: only N x 3 points are implemented")
        if self.index is None:      # an empty index: nothing but padding
            return torch.full((len(X), k), -1, dtype=torch.int64), torch.full((len(X), k), math.inf, dtype=torch.float64)
        Q = torch.from_numpy(np.ascontiguousarray(X.astype(np.float32), dtype=np.float64)).cuda()
        r = float(r)
        idx, d2, _ = ops.nn3_knn(self.index, Q, k, max_d2=r if r >= 0 else math.inf)
        return idx, d2

    def query(self, X, k, r):
        """utils.py:30-37: the labels of the points among the k nearest of any row of X with ``0 < d2 < r``, unique and sorted."""
        idx, d2 = self._search(X, k, r)
        hit = torch.unique(idx[(d2 > 0) & (d2 < float(r))]).cpu().numpy()     # (the unique of the labels is the unique over unique rows)
        return np.unique(self.y[hit])

    def n_neighbors_in_radius(self, X, k, r):
        """utils.py:39-44: per row of X, how many of its k nearest have ``0 < d2 <= r``."""
        idx, d2 = self._search(X, k, r)
        return ((d2 > 0) & (d2 <= float(r))).sum(dim=1).cpu().numpy()


def _rows_without(n: int, rows: np.ndarray) -> np.ndarray:
    mask = np.ones(n, dtype=bool)
    mask[rows] = False
    return np.flatnonzero(mask)


def grow_deletion_set(local_map_xyz: np.ndarray, del_idx: np.ndarray):
    """The map filter of registration_node.py:704-717 in one function.  ``del_idx`` are the rows of the map (N x 3, further columns
    ignored) that might be removed.  Isolated candidates go first: one with fewer than 3 other candidates at 0 < d2 <= .5 among its
    10 nearest candidates is dropped (RN:705-708).  Then the set grows: every other point of the map that is among the 50 nearest of
    a remaining candidate at 0 < d2 < .5 joins it (RN:709-715).  Returns ``(del_idx, keep_idx)`` as RN:715-717 leave them: the
    remaining candidates followed by the joined rows in ascending order, and the rows of the map in neither, ascending."""
    xyz = np.asarray(local_map_xyz)[:, :3]
    n = xyz.shape[0]
    cand = np.asarray(del_idx).astype(np.int64)
    among = FaissKNeighbors()
    among.fit(xyz[cand], cand)
    cand = cand[among.n_neighbors_in_radius(xyz[cand], 10, .5) >= 3]
    others = _rows_without(n, cand)
    rest = FaissKNeighbors()
    rest.fit(xyz[others], others)
    grown = np.concatenate([cand, rest.query(xyz[cand], 50, .5)])
    return grown, _rows_without(n, grown)


def _norm_ppf(p: float) -> float:
    try:
        from scipy.stats import norm
        return float(norm.ppf(p))
    except ImportError:
        from statistics import NormalDist
        if not 0 < p < 1:
            return -math.inf if p == 0 else math.inf if p == 1 else math.nan
        return NormalDist().inv_cdf(p)


def remove_clusters(del_idx: np.ndarray, labels: np.ndarray, remove_chance: float, rng):
    """The seeded coin per cluster of registration_node.py:740-778.  ``labels`` are the cluster labels of the rows ``del_idx``.  Noise
    rows (label -1) leave the deletion set (RN:740-741).  Then, for ``label in range(labels.max() + 1)`` IN THAT ORDER, one
    ``rng.standard_normal()`` per label is compared with ``norm.ppf(remove_chance)``: a draw above the threshold takes the cluster out
    of the deletion set, i.e. keeps it in the map (RN:769-776).  ``rng`` is anything with ``standard_normal()``
    (``np.random.RandomState``, ``np.random.Generator``).  The threshold is ``scipy.stats.norm.ppf`` where scipy imports and
    ``statistics.NormalDist().inv_cdf`` otherwise (with -inf / +inf for a chance of 0 / 1, as scipy gives them).  Returns
    ``(del_idx, keep_idx)``: the rows that remain in the deletion set and, in their input order, the given rows that stay in the map
    (noise and kept clusters); the ``keep_idx`` of RN:777-778 over the whole map needs its size: ``filter_map_clusters`` returns it.

    Deviation: with no cluster at all the reference fails on ``max()`` of an empty array; here nothing is drawn and nothing remains."""
    del_idx, labels = np.asarray(del_idx), np.asarray(labels)
    if del_idx.shape != labels.shape:
        raise ValueError(f"{len(del_idx)} rows but {len(labels)} labels")
    given = del_idx
    del_idx, labels = del_idx[labels != -1], labels[labels != -1]
    if len(labels) == 0:
        return del_idx, given
    threshold = _norm_ppf(float(remove_chance))
    for label in range(int(labels.max()) + 1):
        if rng.standard_normal() > threshold:
            del_idx, labels = del_idx[labels != label], labels[labels != label]
    return del_idx, given[~np.isin(given, del_idx)]


def filter_map_clusters(local_map_xyz: np.ndarray, del_idx: np.ndarray, remove_chance: float, rng, min_cluster_size: int = 100,
                        min_samples: int = 25):
    """registration_node.py:704-778 in one call: ``grow_deletion_set``, then ``HDBSCAN(100, 25)`` on the grown set's float32
    coordinates (vfmreg.clustering: exact, on the GPU), then ``remove_clusters``.  Starts from ``del_idx`` as ``grow_deletion_set``
    does: the colour gate in front (RN:694-702) is ``colour_gate``, and ``filter_map_semantic`` runs both.  Returns
    ``(del_idx, keep_idx)`` as RN:777-778 leave them."""
    from .clustering import HDBSCAN
    xyz = np.asarray(local_map_xyz)[:, :3]
    grown, _ = grow_deletion_set(xyz, del_idx)
    labels = HDBSCAN(min_cluster_size=min_cluster_size, min_samples=min_samples).fit_predict(xyz[grown].astype(np.float32))
    removed, _ = remove_clusters(grown, labels, remove_chance, rng)
    return removed, _rows_without(xyz.shape[0], removed)


# The "tree (broadleaf and coniferous)" class of registration_node.py:685-688: two colours of the reference's PCA image of its maps.
# They mean something only under the reference's own fit -- the arrays of its ``pca_fit.pkl`` put into ``fit_pca[3]`` (vfmreg/pca.py):
# a fit made here has other axes and, by its sign rule, possibly other signs, and its colours of a tree are whatever that fit gives.
TREE_COLOURS = np.array([[217, 60, 165], [118, 105, 57]], dtype=np.float32)


def colour_gate(colours, remove_class, radius: float = 50.) -> np.ndarray:
    """The colour gate of registration_node.py:696-702: for every colour of ``remove_class`` ([m, 3]) the rows of ``colours`` (uint8
    [n, 3], numpy or a device tensor) with ``norm(row - colour) < radius``, ascending, concatenated in the colours' order -- a row near
    two colours appears twice.  On the GPU (csrc/pca.hip): the squared distance in fp64 against ``radius * radius``, which for
    integer-valued colours decides exactly as the reference's float32 ``norm < 50`` does.  Returns int64 numpy."""
    t = colours if isinstance(colours, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(colours))
    if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"colours: expected uint8 [n, 3], got {t.dtype} {tuple(t.shape)}")
    gate = np.ascontiguousarray(np.asarray(remove_class, dtype=np.float64).reshape(-1, 3))
    if t.shape[0] == 0 or gate.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    t = t.cuda().contiguous()
    idx, counts = ops.colour_gate(t, torch.from_numpy(gate).cuda(), float(radius))
    counts = counts.cpu().numpy()
    return np.concatenate([idx[c, :int(counts[c])].cpu().numpy() for c in range(len(counts))])


def filter_map_semantic(local_map: np.ndarray, pca, remove_classes, remove_chance: float, rng):
    """registration_node.py:693-792 in one call.  ``local_map`` is N x (3 + C); ``pca`` has ``run_pca`` (an ``ImageFeatureGenerator``, a
    ``pca.DescriptorPCA``).  The map's descriptors get their RGB colours (RN:694); then, per class of ``remove_classes`` (each [m, 3]
    colours, e.g. ``[TREE_COLOURS]``), ``colour_gate`` picks the candidates, ``filter_map_clusters`` decides which of them go, and the
    map and its colours are cut down before the next class (RN:790-791).  ``rng`` is the coin's ``np.random.RandomState`` (RN:584).
    Returns ``(local_map[keep_idx], local_map_pca[keep_idx], keep_idx)``, ``keep_idx`` being rows of the map given."""
    local_map = np.asarray(local_map)
    local_map_pca = pca.run_pca(local_map[:, 3:], n_components=3)
    keep_idx = np.arange(local_map.shape[0])
    for remove_class in remove_classes:
        del_idx = colour_gate(local_map_pca, remove_class)
        _, keep = filter_map_clusters(local_map[:, :3], del_idx, remove_chance, rng)
        local_map, local_map_pca, keep_idx = local_map[keep], local_map_pca[keep], keep_idx[keep]
    return local_map, local_map_pca, keep_idx

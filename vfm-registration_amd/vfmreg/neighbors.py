"""Stand-in for ``sklearn.neighbors.KDTree`` as registration_node.py:27 imports and RN:295-298 uses it: an exact Euclidean 1-nearest
neighbour search in 3-D on the GPU (csrc/nn3.hip).

    tree = KDTree(voxel_scan, metric="euclidean")
    dist, ind = tree.query(src, k=1, return_distance=True)      # (K, 1) fp64, (K, 1) int64

numpy in, numpy out; device tensors (N x 3 fp64 on the ROCm device) are taken and returned as such.  Distances are
``sqrt((dx*dx + dy*dy) + dz*dz)`` in fp64 -- bit-equal to sklearn's on the inputs tests/test_nn3_oracle.py compares --; among points at
the same distance the lowest row wins (sklearn leaves that unspecified).  ``query`` answers k = 1; the k nearest (k <= 64) are
``query_knn`` (csrc/nn3.hip, ``nn3_knn_kernel``).  Other metrics, other widths than 3: NotImplementedError.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops

# Points per occupied cell the grid is sized for.  The value rests on the timing run of tools/time_fpfh_ransac.py
# (profiles/fpfh_ransac_timing.md: the query's time over a sweep of this number), not on a model.
POINTS_PER_CELL = 4.0
_EUCLIDEAN = ("euclidean", "l2")


def choose_cell(pts: torch.Tensor, target: float = POINTS_PER_CELL, builds: int = 3) -> ops.Nn3Grid:
    """Build the grid of ``pts`` (n x 3 fp64 on the device, n >= 1) with a cell that holds about ``target`` points per OCCUPIED cell.
    The first cell spreads the points evenly over the bounding box (over the axes that have an extent); then, up to ``builds - 1``
    times, the occupancy of the built grid is counted (distinct keys) and the cell rescaled by sqrt(target / measured) -- the clouds
    here are surfaces, whose occupancy grows with the square of the cell -- until the measured number is within a factor 2 of the
    target.  One read-back per build.  The cell never goes below max|coordinate| / 2^19, so that no cell index is clamped."""
    n = pts.shape[0]
    box = torch.stack((pts.amin(0), pts.amax(0))).cpu().numpy()
    ext = box[1] - box[0]
    live = ext[np.isfinite(ext) & (ext > 0)]
    reach = float(np.nanmax(np.abs(box))) if np.isfinite(box).any() else 0.0
    floor = max(reach / (1 << 19), 1e-300) if math.isfinite(reach) else 1.0
    cell = float((np.prod(live) * target / n) ** (1.0 / len(live))) if len(live) else 1.0
    grid = None
    for attempt in range(max(1, builds)):
        cell = max(cell, floor)
        if not (math.isfinite(cell) and cell > 0):
            cell = 1.0
        grid = ops.nn3_build(pts, cell)
        if attempt == builds - 1 or n <= target:
            break
        occupied = int((grid.keys[1:] != grid.keys[:-1]).sum().item()) + 1
        per_cell = n / occupied
        if target / 2 <= per_cell <= target * 2:
            break
        new = cell * math.sqrt(target / per_cell)
        if max(new, floor) == cell:
            break
        cell = new
    return grid


def _rows(X, training: bool = False):
    """``X``, a numpy array or a device tensor, as (contiguous fp64 N x 3 rows on the device, it was a device tensor); the shape is
    refused in sklearn's words for the tree's data (``training``) or for queries before anything is uploaded."""
    device_in = isinstance(X, torch.Tensor)
    if not device_in:
        X = np.asarray(X)
    shape = tuple(X.shape)
    if training:
        if len(shape) != 2:
            raise ValueError(f"Expected 2D array, got {len(shape)}D array instead")
        if shape[0] == 0:
            raise ValueError(f"Found array with 0 sample(s) (shape={shape}) while a minimum of 1 is required.")
        if shape[1] != 3:
            raise NotImplementedError("only 3-D points are implemented")
    elif len(shape) != 2 or shape[1] != 3:
        raise ValueError("query data dimension must match training data dimension")
    rows = X.to(torch.float64).contiguous() if device_in else torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).cuda()
    return rows, device_in


class KDTree:
    """``sklearn.neighbors.KDTree(X, leaf_size, metric)`` for N x 3 data: the grid is built here, once (``leaf_size`` has no
    counterpart and is ignored)."""

    def __init__(self, X, leaf_size: int = 40, metric: str = "euclidean", **kwargs):
        if metric not in _EUCLIDEAN:
            raise NotImplementedError(f"metric {metric!r}: only 'euclidean' is implemented (registration_node.py:295-296)")
        if kwargs:
            raise NotImplementedError(f"unsupported arguments: {sorted(kwargs)}")
        self.data, _ = _rows(X, training=True)
        self.grid = choose_cell(self.data)

    def query_device(self, Q: torch.Tensor, want_fallbacks: bool = False):
        """(idx int64[K], dist fp64[K]) on the device, no read-back; ``want_fallbacks``: see ``ops.nn3_query``."""
        return ops.nn3_query(self.grid, Q, want_fallbacks)

    def query(self, X, k: int = 1, return_distance: bool = True, **kwargs):
        """``sklearn.neighbors.KDTree.query`` for k = 1 (registration_node.py:297-298); k > 1 lives in ``query_knn``."""
        if k != 1:
            raise NotImplementedError("query answers k = 1 (registration_node.py:297-298); the k nearest are query_knn(X, k)")
        if kwargs:
            raise NotImplementedError(f"unsupported arguments: {sorted(kwargs)}")
        Q, device_in = _rows(X)
        idx, dist = ops.nn3_query(self.grid, Q)
        idx, dist = idx.reshape(-1, 1), dist.reshape(-1, 1)
        if not device_in:
            idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        return (dist, idx) if return_distance else idx

    def query_knn(self, X, k: int, return_distance: bool = True):
        """``sklearn.neighbors.KDTree.query(X, k)`` for 1 <= k <= 64: ``(dist, ind)`` of shape (K, k), fp64 distances (roots) ascending
        and int64 rows, equal distances by the lower row; numpy or device tensors as ``query``.  ``k`` above the number of points
        raises ValueError, as sklearn does."""
        k = int(k)
        if k < 1:
            raise ValueError(f"k must be at least 1, got {k}")
        if k > self.grid.n:
            raise ValueError("k must be less than or equal to the number of training points")
        if k > ops.NN3_KNN_MAX_K:
            raise NotImplementedError(f"k = {k}: at most {ops.NN3_KNN_MAX_K} neighbours are implemented")
        Q, device_in = _rows(X)
        idx, d2, _ = ops.nn3_knn(self.grid, Q, k)
        dist = torch.sqrt(d2)
        if not device_in:
            idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        return (dist, idx) if return_distance else idx

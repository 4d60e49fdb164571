"""The oracle of exact HDBSCAN* as ``vfmreg.clustering.HDBSCAN`` defines it, in numpy and plain Python, independent of
the product: nothing here imports ``vfmreg`` or sklearn.

* points in fp64, ``d2 = (dx*dx + dy*dy) + dz*dz``; every order is decided on squares;
* ``core2[i]``: the d2 of the ``min_samples``-th nearest point of the set, i itself included;
* ``w2(i, j) = max(core2[i], core2[j], d2(i, j))``; THE spanning tree is the one of Kruskal over all pairs in the total order
  ``(w2, min(i, j), max(i, j))`` (``mst``: n <= 3000 keeps the n (n - 1) / 2 pairs affordable);
* single linkage: Kruskal over the tree's edges in that order, ``lambda = 1 / sqrt(w2)``, ``+inf`` for ``w2 == 0``; the node of the
  lower endpoint's side is the left one (``sklearn.cluster._hdbscan._linkage.make_single_linkage``);
* condensed tree, stabilities, excess of mass and labels after ``sklearn.cluster._hdbscan._tree`` with allow_single_cluster=False,
  cluster_selection_epsilon=0 -- written here from its description as lists and dicts, the sums in its order.

``filter_restated`` restates registration_node.py:704-778 on top of ``knn3_oracle.grow_restated``.
"""
from __future__ import annotations

import numpy as np

from . import knn3_oracle


def d2_matrix(points: np.ndarray) -> np.ndarray:
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    dx, dy, dz = (p[:, None, a] - p[None, :, a] for a in range(3))
    return (dx * dx + dy * dy) + dz * dz


def core2(points: np.ndarray, min_samples: int) -> np.ndarray:
    return np.sort(d2_matrix(points), axis=1)[:, min_samples - 1]


def w2_matrix(points: np.ndarray, min_samples: int) -> np.ndarray:
    d2 = d2_matrix(points)
    c = np.sort(d2, axis=1)[:, min_samples - 1]
    return np.maximum(np.maximum(c[:, None], c[None, :]), d2)


def mst(points: np.ndarray, min_samples: int):
    """(lo int32[n-1], hi int32[n-1], w2 fp64[n-1]) ascending in (w2, lo, hi): Kruskal over all pairs lo < hi in that order."""
    w = w2_matrix(points, min_samples)
    n = len(w)
    lo, hi = np.triu_indices(n, 1)
    ww = w[lo, hi]
    order = np.lexsort((hi, lo, ww))
    lo, hi, ww = lo[order], hi[order], ww[order]
    up = np.arange(n)

    def find(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x

    # Kruskal, a block of edges at a time: the edges of a block that already lie inside one component are dropped together (they would
    # be refused one by one), the others are tried in their order
    took = []
    for start in range(0, len(lo), 8192):
        if len(took) == n - 1:
            break
        root = up
        while True:
            nxt = root[root]
            if np.array_equal(nxt, root):
                break
            root = nxt
        up = root.copy()
        sl = slice(start, start + 8192)
        for e in start + np.flatnonzero(up[lo[sl]] != up[hi[sl]]):
            a, b = find(lo[e]), find(hi[e])
            if a != b:
                up[a] = b
                took.append(e)
    took = np.asarray(took, dtype=np.int64)
    return lo[took].astype(np.int32), hi[took].astype(np.int32), ww[took]


def single_linkage(lo, hi, w2):
    """rows (left, right, lambda, size) of nodes n, n + 1, ... from the edges in their (sorted) order"""
    n = len(lo) + 1
    up, node, size = list(range(n)), list(range(n)), [1] * n

    def find(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x

    rows = []
    with np.errstate(divide="ignore"):
        lam = np.where(np.asarray(w2) > 0, 1.0 / np.sqrt(np.asarray(w2, dtype=np.float64)), np.inf)
    for e in range(n - 1):
        a, b = find(int(lo[e])), find(int(hi[e]))
        assert a != b, "not a spanning tree"
        rows.append((node[a], node[b], float(lam[e]), size[a] + size[b]))
        up[a] = b
        size[b] += size[a]
        node[b] = n + e
    return rows


def _bfs(tree, n, root):
    out, level = [], [root]
    while level:
        out.extend(level)
        level = [c for x in level if x >= n for c in tree[x - n][:2]]
    return out


def condense(tree, min_cluster_size: int):
    """rows (parent, child, lambda, size): points are children below n, clusters are numbered from n (the root) in breadth-first order"""
    n = len(tree) + 1
    root = 2 * (n - 1)
    relabel = {root: n}
    next_label = n + 1
    ignore = set()
    rows = []
    for x in _bfs(tree, n, root):
        if x in ignore or x < n:
            continue
        left, right, lam, _ = tree[x - n]
        lc = tree[left - n][3] if left >= n else 1
        rc = tree[right - n][3] if right >= n else 1
        if lc >= min_cluster_size and rc >= min_cluster_size:
            for side, count in ((left, lc), (right, rc)):
                relabel[side] = next_label
                next_label += 1
                rows.append((relabel[x], relabel[side], lam, count))
            continue
        for side, count in ((left, lc), (right, rc)):
            if count >= min_cluster_size:
                relabel[side] = relabel[x]
            else:
                for y in _bfs(tree, n, side):
                    if y < n:
                        rows.append((relabel[x], y, lam, 1))
                    ignore.add(y)
    return rows


def labels_from_condensed(rows, n: int) -> np.ndarray:
    birth, stability, children = {n: 0.0}, {}, {}
    for p, c, lam, _ in rows:
        stability.setdefault(p, 0.0)
        if c >= n:
            birth[c] = lam
            children.setdefault(p, []).append(c)
    with np.errstate(invalid="ignore"):
        for p, c, lam, size in rows:
            stability[p] = float(np.float64(stability[p]) + (np.float64(lam) - np.float64(birth[p])) * np.float64(size))
    is_cluster = {c: True for c in stability if c != n}
    for c in sorted(is_cluster, reverse=True):
        subtree = 0.0
        for d in children.get(c, []):
            subtree = subtree + stability[d]
        if subtree > stability[c]:
            is_cluster[c] = False
            stability[c] = subtree
        else:
            below = list(children.get(c, []))
            while below:
                d = below.pop()
                is_cluster[d] = False
                below.extend(children.get(d, []))
    chosen = sorted(c for c in is_cluster if is_cluster[c])
    number = {c: k for k, c in enumerate(chosen)}
    parent_of = {c: p for p, c, _, _ in rows if c >= n}
    labels = np.full(n, -1, dtype=np.int32)
    for p, c, _, _ in rows:
        if c >= n:
            continue
        while p != n and not is_cluster[p]:
            p = parent_of[p]
        labels[c] = -1 if p == n else number[p]
    return labels


def labels_from_edges(lo, hi, w2, min_cluster_size: int) -> np.ndarray:
    return labels_from_condensed(condense(single_linkage(lo, hi, w2), min_cluster_size), len(lo) + 1)


def hdbscan(points: np.ndarray, min_cluster_size: int, min_samples: int):
    """(labels int32[n], (lo, hi, w2))"""
    edges = mst(points, min_samples)
    return labels_from_edges(*edges, min_cluster_size), edges


def blobs(seed: int, per_blob: int = 400, n_blobs: int = 6, n_uniform: int = 300) -> np.ndarray:
    """anisotropic Gaussian blobs, sigma = (0.8, 0.8, 2.0), centres uniform in +-20, plus uniform points in +-25; float32-rounded fp64"""
    rng = np.random.RandomState(seed)
    centres = rng.uniform(-20, 20, size=(n_blobs, 3))
    parts = [c + rng.standard_normal((per_blob, 3)) * np.array([0.8, 0.8, 2.0]) for c in centres]
    parts.append(rng.uniform(-25, 25, size=(n_uniform, 3)))
    return np.concatenate(parts).astype(np.float32).astype(np.float64)


def norm_ppf(p: float) -> float:
    """the standard normal's quantile, as ``statistics.NormalDist`` gives it (0 -> -inf, 1 -> +inf as scipy.stats.norm.ppf)"""
    from statistics import NormalDist
    if p <= 0:
        return -np.inf if p == 0 else np.nan
    if p >= 1:
        return np.inf if p == 1 else np.nan
    return NormalDist().inv_cdf(p)


def remove_restated(del_idx, labels, remove_chance, rng):
    """registration_node.py:740-778 (without the map: keep_idx is left to the caller)"""
    del_idx, labels = np.asarray(del_idx), np.asarray(labels)
    del_idx = del_idx[labels != -1]
    labels = labels[labels != -1]
    if len(labels) == 0:
        return del_idx
    for label in range(labels.max() + 1):
        if rng.standard_normal() > norm_ppf(remove_chance):
            del_idx = del_idx[labels != label]
            labels = labels[labels != label]
    return del_idx


def filter_restated(xyz, del_idx, remove_chance, rng, min_cluster_size=100, min_samples=25):
    """registration_node.py:704-778: (del_idx, keep_idx)"""
    xyz = np.asarray(xyz)
    del_idx, _ = knn3_oracle.grow_restated(xyz, np.asarray(del_idx))
    pts = xyz[del_idx, :3].astype(np.float32).astype(np.float64)
    labels, _ = hdbscan(pts, min_cluster_size, min_samples)
    del_idx = remove_restated(del_idx, labels, remove_chance, rng)
    return del_idx, np.delete(np.arange(len(xyz)), del_idx)

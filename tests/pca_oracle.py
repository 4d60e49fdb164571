"""The oracle of the descriptor PCA and the colour gate as ``vfmreg.pca`` defines them, in numpy fp64, independent of the
product: nothing here imports ``vfmreg`` or reads a kernel.

* fit: ``mean = X.mean(0)``, ``S = Xc.T @ Xc``, ``eigh(S)``, the top k eigenvectors by descending eigenvalue; in every component the entry
  of largest magnitude (lowest index on a tie) is positive; ``singular_values = sqrt(eigenvalue)``;
* projection: ``y[n][j] = sum_c t_c``, ``t_c = (x[n][c] - mean[c]) * components[j][c]``, in THE order of the contract: 64 partial sums
  start from +0.0, partial l adds ``t_l, t_{l+64}, t_{l+128}, ...`` ascending; then for s = 32, 16, 8, 4, 2, 1 every partial becomes
  ``p_l + p_{l xor s}``; any partial is the value;
* normalisation: ``Y -= Y.min(0); Y /= Y.max(0)``; colours: ``(Y * 255.0)`` truncated to uint8, black where every feature is zero;
  a component whose maximum equals its minimum is NaN as a value and 0 as a colour;
* gate: registration_node.py:696-702 the reference's way, ``np.linalg.norm`` in float32.

``filter_semantic_restated`` restates registration_node.py:693-792 on top of ``hdbscan_oracle.filter_restated``.
"""
from __future__ import annotations

import numpy as np

from . import hdbscan_oracle


# ------------------------------------------------------------------------------------------------------------------------------ fit
def moments(X: np.ndarray):
    X = np.asarray(X, dtype=np.float64)
    mean = X.mean(axis=0)
    Xc = X - mean
    return mean, Xc.T @ Xc


def apply_sign_rule(components: np.ndarray) -> np.ndarray:
    out = np.array(components, dtype=np.float64)
    for row in out:
        if row[np.argmax(np.abs(row))] < 0:      # (argmax: the lowest index among equal magnitudes)
            row *= -1.0
    return out


def fit_from_scatter(S: np.ndarray, k: int):
    """(components [k, d], singular_values [k], eigenvalues descending [d])"""
    w, V = np.linalg.eigh(np.asarray(S, dtype=np.float64))
    order = np.argsort(-w, kind="stable")
    w, V = w[order], V[:, order]
    return apply_sign_rule(V[:, :k].T), np.sqrt(np.maximum(w[:k], 0.0)), w


def fit(X: np.ndarray, k: int):
    """(mean [d], components [k, d], singular_values [k])"""
    mean, S = moments(X)
    comps, sv, _ = fit_from_scatter(S, k)
    return mean, comps, sv


# ----------------------------------------------------------------------------------------------------------------------- projection
def project_ordered(X: np.ndarray, mean: np.ndarray, components: np.ndarray) -> np.ndarray:
    """y [n, k] in the contract's order of addition.  (Padding the terms with +0.0 up to a multiple of 64 changes nothing: a partial sum
    that starts from +0.0 is never -0.0, and p + 0.0 == p otherwise.)"""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    xc = X - np.asarray(mean, dtype=np.float64)
    steps = -(-d // 64)
    lanes = np.arange(64)
    out = np.empty((n, len(components)), dtype=np.float64)
    for j, comp in enumerate(np.asarray(components, dtype=np.float64)):
        t = np.zeros((n, steps * 64), dtype=np.float64)
        t[:, :d] = xc * comp
        t = t.reshape(n, steps, 64)
        p = np.zeros((n, 64), dtype=np.float64)
        for i in range(steps):
            p = p + t[:, i, :]
        for s in (32, 16, 8, 4, 2, 1):
            p = p + p[:, lanes ^ s]
        out[:, j] = p[:, 0]
    return out


def zero_rows(X: np.ndarray) -> np.ndarray:
    return np.all(np.asarray(X) == 0, axis=-1)


def normalise(Y: np.ndarray) -> np.ndarray:
    Y = np.array(Y, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        Y -= Y.min(axis=0)
        Y /= Y.max(axis=0)
    return Y


def colours(Y: np.ndarray, X: np.ndarray) -> np.ndarray:
    """uint8 [n, 3] of image_features.py:184-190; NaN (a constant component) becomes 0"""
    v = normalise(Y) * 255.0
    out = np.where(np.isnan(v), 0.0, v).astype(np.uint8)
    out[zero_rows(X)] = 0
    return out


def run_pca(X: np.ndarray, k: int = 3, fit_=None):
    """image_features.py:162-192 with the exact fit: uint8 colours for k == 3, float32 otherwise"""
    mean, comps = fit_ if fit_ is not None else fit(X, k)[:2]
    Y = project_ordered(X, mean, comps)
    return colours(Y, X) if k == 3 else normalise(Y).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------------- gate
def gate(local_map_pca: np.ndarray, remove_class: np.ndarray, radius: float = 50) -> np.ndarray:
    """registration_node.py:696-702"""
    del_idx = []
    for color in np.asarray(remove_class, dtype=np.float32):
        distance = np.linalg.norm(local_map_pca - color, axis=1)
        del_idx.append(np.flatnonzero(distance < radius))
    return np.concatenate(del_idx)


# offsets at d2 = 2498, 2499, 2500, 2501 from a colour: the gate's radius of 50 lies between the second and the third
BOUNDARY_OFFSETS = np.array([[47, 17, 0], [35, 35, 7], [30, 40, 0], [49, 10, 0]])


def filter_semantic_restated(local_map, local_map_pca, remove_classes, remove_chance, rng):
    """registration_node.py:696-792 behind run_pca: (local_map[keep], local_map_pca[keep], keep) with keep as rows of the map given"""
    local_map, local_map_pca = np.asarray(local_map), np.asarray(local_map_pca)
    keep = np.arange(len(local_map))
    for remove_class in remove_classes:
        del_idx = gate(local_map_pca, remove_class)
        _, keep_idx = hdbscan_oracle.filter_restated(local_map[:, :3], del_idx, remove_chance, rng)
        local_map, local_map_pca, keep = local_map[keep_idx], local_map_pca[keep_idx], keep[keep_idx]
    return local_map, local_map_pca, keep


# ------------------------------------------------------------------------------------------------------------------------ generator
SPECTRUM = (8.0, 4.0, 2.0, 1.0)     # standard deviations of the leading directions; 0.5 for every other one


def spectrum_data(seed: int, N: int, D: int) -> np.ndarray:
    """rows Z . diag(8, 4, 2, 1, 0.5, 0.5, ...) . Q^T + offset in float32: Z standard normal, Q a random orthogonal matrix"""
    rng = np.random.RandomState(seed)
    sigma = np.full(D, 0.5)
    sigma[:min(D, len(SPECTRUM))] = SPECTRUM[:D]
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    Z = rng.standard_normal((N, D))
    return ((Z * sigma) @ Q.T + rng.standard_normal(D)).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------------------- bounds
U = 2.0 ** -53


def scatter_bound(S: np.ndarray, n: int) -> np.ndarray:
    """|S_computed - S|_ij <= 4 n u sqrt(S_ii S_jj): the fp64 dot product's n u |a|.|b| <= n u sqrt(S_ii S_jj) (Cauchy-Schwarz), once for
    each of two computations that add in different orders, doubled for the rounded mean (a mean off by n u |mean| moves a centred entry
    by at most that, which is below the entry's own share of the first term for data whose offset is of its spread's order)."""
    dg = np.sqrt(np.clip(np.diag(S), 0.0, None))
    return 4.0 * n * U * np.outer(dg, dg)


def eigen_gap(eigenvalues: np.ndarray, k: int) -> float:
    """the smallest gap between neighbours among the k + 1 largest eigenvalues"""
    w = np.sort(np.asarray(eigenvalues))[::-1][:k + 1]
    return float(np.min(w[:-1] - w[1:]))


def fit_bound(S: np.ndarray, n: int, k: int) -> float:
    """Davis-Kahan: two symmetric matrices E apart have unit eigenvectors within 2 |E|_F / gap of each other (sin-theta <= |E| / gap,
    |v - v'| <= sqrt(2) sin-theta for equally signed unit vectors, rounded up), gap being the distance of the eigenvalue to its neighbours"""
    w = np.linalg.eigvalsh(S)
    return 2.0 * float(np.linalg.norm(scatter_bound(S, n))) / eigen_gap(w, k)


def colour_delta(X: np.ndarray, mean: np.ndarray, S: np.ndarray, Y: np.ndarray, k: int) -> float:
    """How far value * 255 of the same rows can lie apart under two fits within ``fit_bound`` of each other.  With B = fit_bound and R the
    largest centred row norm, a projection moves by at most dy = R B sqrt(d) (every entry of the component off by B) + |dmean|
    (|dmean| <= sqrt(d) n u max|x|) + 2 d u R (the sums' own rounding); a normalised value (y - min) / (max - min) with all three of y, min,
    max off by dy moves by at most 4 dy / range; times 255."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    R = float(np.sqrt(((X - mean) ** 2).sum(axis=1).max()))
    dy = R * fit_bound(S, n, k) * np.sqrt(d) + np.sqrt(d) * n * U * float(np.abs(X).max()) + 2 * d * U * R
    span = float((Y.max(axis=0) - Y.min(axis=0)).min())
    return 255.0 * 4.0 * dy / span


def near_integer(v255: np.ndarray, delta: float) -> np.ndarray:
    """where value * 255 lies within delta of an integer; the exact 0s and 255s of the minimum and maximum rows do not count"""
    r = np.abs(v255 - np.round(v255))
    return (r <= delta) & (v255 != 0.0) & (v255 != 255.0)

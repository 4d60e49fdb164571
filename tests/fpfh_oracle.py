"""numpy fp64 oracle of the FPFH path (csrc/fpfh.hip): Open3D 0.18's KDTreeFlann::SearchHybrid, EstimateNormals (fast path),
VoxelDownSample, ComputeSPFHFeature and ComputeFPFHFeature, restated in the kernels' operation order.

A restatement, not an anchor: Open3D is not available to this project's tests, so these functions repeat what the kernels were
written to, with the same conventions -- equal distances ordered by index, voxels emitted in ascending
(ix, iy, iz) order.  The pair features also report how close each value came to a bin edge (or to the swap decision) before the
floor: the device's atan2 / acos may differ from the host's by an ulp, so a histogram may legitimately differ only there.
"""
from __future__ import annotations

import numpy as np

PI = 3.14159265358979323846


def _d2(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def _rows(q: np.ndarray, j: np.ndarray, d2: np.ndarray, n: int, max_nn: int):
    """candidates (query, point, d2) -> the first max_nn per query by (d2, index), padded rows"""
    idx = np.full((n, max_nn), -1, dtype=np.int32)
    dd = np.zeros((n, max_nn), dtype=np.float64)
    o = np.lexsort((j, d2, q))
    q, j, d2 = q[o], j[o], d2[o]
    start = np.searchsorted(q, np.arange(n))
    rank = np.arange(len(q)) - start[q]
    keep = rank < max_nn
    idx[q[keep], rank[keep]] = j[keep]
    dd[q[keep], rank[keep]] = d2[keep]
    cnt = np.minimum(np.bincount(q, minlength=n), max_nn).astype(np.int32)
    return idx, dd, cnt


def hybrid_search_brute(pts: np.ndarray, radius: float, max_nn: int):
    """SearchHybrid for every point by brute force: (idx int32[n, max_nn] (-1 padded), d2 fp64[n, max_nn], cnt int32[n])."""
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    n = len(pts)
    if n == 0:
        return np.zeros((0, max_nn), np.int32), np.zeros((0, max_nn)), np.zeros(0, np.int32)
    d2 = _d2(pts[:, None, :], pts[None, :, :])
    q, j = np.nonzero(d2 < radius * radius)
    return _rows(q, j, d2[q, j], n, max_nn)


def hybrid_search(pts: np.ndarray, radius: float, max_nn: int, chunk: int = 20000):
    """SearchHybrid via scipy's cKDTree (candidates from a slightly larger ball, then the exact d2 < r^2 test in the kernels' order)."""
    from scipy.spatial import cKDTree

    pts = np.ascontiguousarray(pts, dtype=np.float64)
    n = len(pts)
    idx = np.full((n, max_nn), -1, dtype=np.int32)
    dd = np.zeros((n, max_nn))
    cnt = np.zeros(n, dtype=np.int32)
    if n == 0:
        return idx, dd, cnt
    tree = cKDTree(pts)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        lists = tree.query_ball_point(pts[s:e], radius * (1 + 1e-7), workers=-1)
        lens = np.fromiter((len(l) for l in lists), dtype=np.int64, count=e - s)
        j = np.fromiter((x for l in lists for x in l), dtype=np.int64, count=int(lens.sum()))
        q = np.repeat(np.arange(s, e), lens)
        d2 = _d2(pts[j], pts[q])
        ok = d2 < radius * radius
        i2, d2r, c2 = _rows(q[ok] - s, j[ok], d2[ok], e - s, max_nn)
        idx[s:e], dd[s:e], cnt[s:e] = i2, d2r, c2
    return idx, dd, cnt


# ------------------------------------------------------------------------------------------------ normals
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _w(c, a, b):
    return np.where(c[..., None], a, b)


def _eigenvector0(A, e):
    row0 = np.stack([A[:, 0, 0] - e, A[:, 0, 1], A[:, 0, 2]], -1)
    row1 = np.stack([A[:, 0, 1], A[:, 1, 1] - e, A[:, 1, 2]], -1)
    row2 = np.stack([A[:, 0, 2], A[:, 1, 2], A[:, 2, 2] - e], -1)
    r01, r02, r12 = _cross(row0, row1), _cross(row0, row2), _cross(row1, row2)
    d0, d1, d2 = _dot(r01, r01), _dot(r02, r02), _dot(r12, r12)
    imax = np.zeros(len(e), dtype=np.int64)
    dmax = d0.copy()
    c1 = d1 > dmax
    imax[c1], dmax[c1] = 1, d1[c1]
    imax[d2 > dmax] = 2
    v = _w(imax == 0, r01, _w(imax == 1, r02, r12))
    s = np.sqrt(np.where(imax == 0, d0, np.where(imax == 1, d1, d2)))
    return v / s[:, None]


def _eigenvector1(A, e0, eval1, want_arm: bool = False):
    big = np.abs(e0[:, 0]) > np.abs(e0[:, 1])
    il_a = 1.0 / np.sqrt(e0[:, 0] * e0[:, 0] + e0[:, 2] * e0[:, 2])
    il_b = 1.0 / np.sqrt(e0[:, 1] * e0[:, 1] + e0[:, 2] * e0[:, 2])
    z = np.zeros_like(il_a)
    U = _w(big, np.stack([-e0[:, 2] * il_a, z, e0[:, 0] * il_a], -1), np.stack([z, e0[:, 2] * il_b, -e0[:, 1] * il_b], -1))
    V = _cross(e0, U)

    def mul(X):
        return np.stack([(A[:, 0, 0] * X[:, 0] + A[:, 0, 1] * X[:, 1]) + A[:, 0, 2] * X[:, 2],
                         (A[:, 0, 1] * X[:, 0] + A[:, 1, 1] * X[:, 1]) + A[:, 1, 2] * X[:, 2],
                         (A[:, 0, 2] * X[:, 0] + A[:, 1, 2] * X[:, 1]) + A[:, 2, 2] * X[:, 2]], -1)
    AU, AV = mul(U), mul(V)
    m00 = _dot(U, AU) - eval1
    m01 = _dot(U, AV)
    m11 = _dot(V, AV) - eval1
    a00, a01, a11 = np.abs(m00), np.abs(m01), np.abs(m11)
    first = a00 >= a11
    # branch 1 (|m00| >= |m11|)
    t1 = a00 >= a01
    x01 = m01 / m00
    x00 = 1.0 / np.sqrt(1.0 + x01 * x01)
    x01 = x01 * x00
    y00 = m00 / m01
    y01 = 1.0 / np.sqrt(1.0 + y00 * y00)
    y00 = y00 * y01
    a1, b1 = np.where(t1, x01, y01), np.where(t1, x00, y00)
    ok1 = np.maximum(a00, a01) > 0
    # branch 2
    t2 = a11 >= a01
    x01 = m01 / m11
    x11 = 1.0 / np.sqrt(1.0 + x01 * x01)
    x01 = x01 * x11
    y11 = m11 / m01
    y01 = 1.0 / np.sqrt(1.0 + y11 * y11)
    y11 = y11 * y01
    a2, b2 = np.where(t2, x11, y11), np.where(t2, x01, y01)
    ok2 = np.maximum(a11, a01) > 0
    a, b = np.where(first, a1, a2), np.where(first, b1, b2)
    ok = np.where(first, ok1, ok2)
    r = a[:, None] * U - b[:, None] * V
    out = _w(ok, r, U)
    if not want_arm:
        return out
    arm = np.where(first, np.where(ok1, np.where(t1, EV1_M00_DIV, EV1_M00_INV), EV1_M00_ZERO),
                   np.where(ok2, np.where(t2, EV1_M11_DIV, EV1_M11_INV), EV1_M11_ZERO))
    return out, np.where(big, EV1_U_XZ, EV1_U_YZ), arm


# Which exit of csrc/fpfh.hip's fast_eigen3x3 a row took (``fast_eigen3x3(C, branches=True)``), next to the kernel line it mirrors:
EIG_ZERO = 0        # if (mc == 0.0): the zero vector (fpfh_normal_kernel then writes (0, 0, 1))
EIG_DIAG_X = 1      # norm == 0:  if (d0 < d1 && d0 < d2) out[0] = 1.0
EIG_DIAG_Y = 2      #             else if (d1 < d0 && d1 < d2) out[1] = 1.0
EIG_DIAG_Z = 3      #             else out[2] = 1.0, with d2 strictly the smallest
EIG_DIAG_TIE = 4    #             else out[2] = 1.0, by the tie rule: no diagonal entry is strictly the smallest
EIG_POS_EVEC = 5    # half_det >= 0: if (eval2 < eval0 && eval2 < eval1) -> eigenvector0(A, eval2)
EIG_POS_EVEC1 = 6   #                if (eval1 < eval0 && eval1 < eval2) -> eigenvector1
EIG_POS_CROSS = 7   #                cross3(e1, e0, out)
EIG_NEG_EVEC = 8    # half_det < 0:  if (eval0 < eval1 && eval0 < eval2) -> eigenvector0(A, eval0)
EIG_NEG_EVEC1 = 9   #                if (eval1 < eval0 && eval1 < eval2) -> eigenvector1
EIG_NEG_CROSS = 10  #                cross3(e0, e1, out)
EIG_EXITS = tuple(range(11))
# eigenvector1, for the rows whose exit went through it (EIG_*_EVEC1, EIG_*_CROSS; -1 elsewhere).  The U construction:
EV1_U_XZ = 0        # if (fabs(evec0[0]) > fabs(evec0[1])): U = (-e2, 0, e0) / length
EV1_U_YZ = 1        # else:                                 U = (0, e2, -e1) / length
# and the arm that normalises (m00, m01, m11):
EV1_M00_DIV = 0     # absM00 >= absM11, absM00 >= absM01: m01 /= m00
EV1_M00_INV = 1     # absM00 >= absM11, else:             m00 /= m01
EV1_M00_ZERO = 2    # absM00 >= absM11, !(mx > 0): return U
EV1_M11_DIV = 3     # else, absM11 >= absM01: m01 /= m11
EV1_M11_INV = 4     # else, else:             m11 /= m01
EV1_M11_ZERO = 5    # else, !(mx > 0): return U (absM00 >= absM11 was false with absM11 not above 0: a NaN in m00 or m11)
EV1_ARMS = tuple(range(6))


def fast_eigen3x3(C: np.ndarray, branches: bool = False):
    """Open3D 0.18 FastEigen3x3 for a stack of 3 x 3 matrices: the eigenvector of the smallest eigenvalue (0 for a zero matrix).
    With ``branches``: (vectors, exit int[M] (EIG_*), U construction int[M] (EV1_U_*, -1), eigenvector1 arm int[M] (EV1_M*, -1))."""
    C = np.asarray(C, dtype=np.float64).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        mc = C.reshape(-1, 9).max(axis=1)
        A = C / mc[:, None, None]
        norm = (A[:, 0, 1] * A[:, 0, 1] + A[:, 0, 2] * A[:, 0, 2]) + A[:, 1, 2] * A[:, 1, 2]
        q = ((A[:, 0, 0] + A[:, 1, 1]) + A[:, 2, 2]) / 3.0
        b00, b11, b22 = A[:, 0, 0] - q, A[:, 1, 1] - q, A[:, 2, 2] - q
        p = np.sqrt((((b00 * b00 + b11 * b11) + b22 * b22) + norm * 2.0) / 6.0)
        c00 = b11 * b22 - A[:, 1, 2] * A[:, 1, 2]
        c01 = A[:, 0, 1] * b22 - A[:, 1, 2] * A[:, 0, 2]
        c02 = A[:, 0, 1] * A[:, 1, 2] - b11 * A[:, 0, 2]
        det = ((b00 * c00 - A[:, 0, 1] * c01) + A[:, 0, 2] * c02) / ((p * p) * p)
        half_det = np.minimum(np.maximum(det * 0.5, -1.0), 1.0)
        angle = np.arccos(half_det) / 3.0
        beta2 = np.cos(angle) * 2.0
        beta0 = np.cos(angle + 2.09439510239319549) * 2.0
        beta1 = -(beta0 + beta2)
        ev0, ev1, ev2 = q + p * beta0, q + p * beta1, q + p * beta2
        pos = half_det >= 0
        ef = _eigenvector0(A, np.where(pos, ev2, ev0))
        c1 = np.where(pos, (ev2 < ev0) & (ev2 < ev1), (ev0 < ev1) & (ev0 < ev2))
        e1, u_id, arm = _eigenvector1(A, ef, ev1, want_arm=True)
        c2 = (ev1 < ev0) & (ev1 < ev2)
        last = _w(pos, _cross(e1, ef), _cross(ef, e1))
        off = _w(c1, ef, _w(c2, e1, last))
        d0, d1, d2 = A[:, 0, 0] * mc, A[:, 1, 1] * mc, A[:, 2, 2] * mc
        ax = np.where((d0 < d1) & (d0 < d2), 0, np.where((d1 < d0) & (d1 < d2), 1, 2))
        diag = np.eye(3)[ax]
        out = _w(norm > 0, off, diag)
        out = _w(mc == 0, np.zeros_like(out), out)
        if not branches:
            return out
        ex_off = np.where(pos, np.where(c1, EIG_POS_EVEC, np.where(c2, EIG_POS_EVEC1, EIG_POS_CROSS)),
                          np.where(c1, EIG_NEG_EVEC, np.where(c2, EIG_NEG_EVEC1, EIG_NEG_CROSS)))
        strict_z = (d2 < d0) & (d2 < d1)
        ex_diag = np.where(ax == 0, EIG_DIAG_X, np.where(ax == 1, EIG_DIAG_Y, np.where(strict_z, EIG_DIAG_Z, EIG_DIAG_TIE)))
        ex = np.where(mc == 0, EIG_ZERO, np.where(norm > 0, ex_off, ex_diag))
        used1 = (norm > 0) & (mc != 0) & ~c1
        return out, ex, np.where(used1, u_id, -1), np.where(used1, arm, -1)


def covariances(pts: np.ndarray, idx: np.ndarray, cnt: np.ndarray) -> np.ndarray:
    """ComputeCovariance's one-pass form over the neighbour rows; the identity below 3 neighbours."""
    n, kmax = idx.shape
    cu = np.zeros((n, 9))
    for k in range(kmax):
        live = k < cnt
        if not live.any():
            break
        p = pts[np.where(live, idx[:, k], 0)]
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        terms = np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], -1)
        cu = np.where(live[:, None], cu + terms, cu)
    with np.errstate(all="ignore"):
        cu = cu / cnt[:, None].astype(np.float64)
    C = np.empty((n, 3, 3))
    C[:, 0, 0] = cu[:, 3] - cu[:, 0] * cu[:, 0]
    C[:, 1, 1] = cu[:, 6] - cu[:, 1] * cu[:, 1]
    C[:, 2, 2] = cu[:, 8] - cu[:, 2] * cu[:, 2]
    C[:, 0, 1] = C[:, 1, 0] = cu[:, 4] - cu[:, 0] * cu[:, 1]
    C[:, 0, 2] = C[:, 2, 0] = cu[:, 5] - cu[:, 0] * cu[:, 2]
    C[:, 1, 2] = C[:, 2, 1] = cu[:, 7] - cu[:, 1] * cu[:, 2]
    C[cnt < 3] = np.eye(3)
    return C


def estimate_normals(pts: np.ndarray, idx: np.ndarray, cnt: np.ndarray) -> np.ndarray:
    """EstimateNormals(fast_normal_computation=True) on a cloud without normals: no orientation step, zero -> (0, 0, 1)."""
    nv = fast_eigen3x3(covariances(pts, idx, cnt))
    zero = np.sqrt(_dot(nv, nv)) == 0.0
    nv[zero] = (0.0, 0.0, 1.0)
    return nv


# ------------------------------------------------------------------------------------------------ down-sample
def voxel_down_sample(pts: np.ndarray, voxel_size: float, normals: np.ndarray | None = None):
    """VoxelDownSample: per-voxel means summed in input order (normals not renormalised), voxels ascending by (ix, iy, iz)."""
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    if len(pts) == 0:
        return np.zeros((0, 3)), (None if normals is None else np.zeros((0, 3)))
    origin = pts.min(axis=0) - voxel_size * 0.5
    v = np.floor((pts - origin) / voxel_size).astype(np.int64)
    if v.max() >= (1 << 21):
        raise ValueError("voxel index reaches 2^21")
    key = (v[:, 0] << 42) | (v[:, 1] << 21) | v[:, 2]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.r_[True, ks[1:] != ks[:-1]]
    vid = np.cumsum(head) - 1
    start = np.flatnonzero(head)
    rank = np.arange(len(ks)) - start[vid]
    m = len(start)
    count = np.diff(np.r_[start, len(ks)]).astype(np.float64)

    def average(a):
        acc = np.zeros((m, 3))
        for r in range(int(rank.max()) + 1):
            sel = rank == r
            acc[vid[sel]] = acc[vid[sel]] + a[order[sel]]
        return acc / count[:, None]
    return average(pts), (None if normals is None else average(np.asarray(normals, dtype=np.float64)))


# ------------------------------------------------------------------------------------------------ features
# Which exit of csrc/fpfh.hip's pair_features a pair took (``pair_features(..., branches=True)``):
PAIR_DN_ZERO = 0       # if (dn == 0.0) return: coincident points, all three features 0
PAIR_VN_ZERO = 1       # if (vn == 0.0) return, roles kept: n1 parallel to d (or a zero n1)
PAIR_VN_ZERO_SWAP = 2  # if (vn == 0.0) return, after the swap: n2 parallel to d
PAIR_KEPT = 3          # acos(fabs(angle1)) < acos(fabs(angle2)): roles kept
PAIR_KEPT_TIE = 4      # acos(fabs(angle1)) == acos(fabs(angle2)): the strict > keeps the roles on the exact tie
PAIR_SWAP = 5          # acos(fabs(angle1)) > acos(fabs(angle2)): a = n2, b = n1, d = -d, f2 = -angle2
PAIR_KEPT_NAN = 6      # a NaN on either side of the > (|angle| > 1 from a normal longer than 1): roles kept
PAIR_EXITS = tuple(range(7))


def pair_features(p1, n1, p2, n2, branches: bool = False, exact_ok: bool = False):
    """ComputePairFeatures for stacks of pairs: (f fp64[M, 3], margin fp64[M]).  margin: the smallest distance of a bin coordinate
    (11 (f0 + pi) / 2 pi, 11 (f1 + 1) / 2, 11 (f2 + 1) / 2) from an integer, or of the two acos values the swap compares.
    ``exact_ok``: what no rounding of a libm call can move is left out of the margin -- a feature that IS an end of its range
    (f0 = -+pi, which atan2 returns only for a zero of either sign over a negative number; f1, f2 = -+1, which come from sqrt,
    division, products and sums alone; the bin coordinate follows by products and sums too), and a swap comparison whose two arguments
    |angle1| and |angle2| are the same number.  ``branches``: also exit int[M] (PAIR_*)."""
    with np.errstate(all="ignore"):
        d = p2 - p1
        dn = np.sqrt(_dot(d, d))
        a1, a2 = _dot(n1, d) / dn, _dot(n2, d) / dn
        c1, c2 = np.arccos(np.abs(a1)), np.arccos(np.abs(a2))
        swap = c1 > c2
        a = _w(swap, n2, n1)
        b = _w(swap, n1, n2)
        d = _w(swap, d * -1.0, d)
        f2 = np.where(swap, -a2, a1)
        v = _cross(d, a)
        vn = np.sqrt(_dot(v, v))
        v = v / vn[:, None]
        w = _cross(a, v)
        f1 = _dot(v, b)
        f0 = np.arctan2(_dot(w, b), _dot(a, b))
        f = np.stack([f0, f1, f2], -1)
        zero = (dn == 0.0) | (vn == 0.0)
        f[zero] = 0.0
        x = _bin_coords(f)
        mx = np.abs(x - np.round(x))
        gap = np.abs(c1 - c2)
        if exact_ok:
            ends = np.stack([np.abs(f[:, 0]) == PI, np.abs(f[:, 1]) == 1.0, np.abs(f[:, 2]) == 1.0], -1)
            mx = np.where(ends, np.inf, mx)
            gap = np.where(np.abs(a1) == np.abs(a2), np.inf, gap)
        margin = np.min(mx, axis=1)
        margin = np.where(zero, np.inf, (np.fmin if exact_ok else np.minimum)(margin, gap))
        if not branches:
            return f, margin
        full = np.where(swap, PAIR_SWAP, np.where(c1 < c2, PAIR_KEPT, np.where(c1 == c2, PAIR_KEPT_TIE, PAIR_KEPT_NAN)))
        ex = np.where(dn == 0.0, PAIR_DN_ZERO, np.where(vn == 0.0, np.where(swap, PAIR_VN_ZERO_SWAP, PAIR_VN_ZERO), full))
    return f, margin, ex


def _bin_coords(f):
    return np.stack([11.0 * (f[:, 0] + PI) / (2.0 * PI), 11.0 * (f[:, 1] + 1.0) * 0.5, 11.0 * (f[:, 2] + 1.0) * 0.5], -1)


def spfh(pts: np.ndarray, normals: np.ndarray, idx: np.ndarray, cnt: np.ndarray, edge: float = 1e-9, exact_ok: bool = False,
         branches: bool = False):
    """ComputeSPFHFeature: (spfh fp64[n, 33], near_edge bool[n] -- some pair of the row within `edge` of a bin edge).  ``exact_ok``:
    see pair_features.  ``branches``: also int[n, len(PAIR_EXITS)], how many pairs of the row took each exit of pair_features, and
    int[n, 3, 2], how many of its pairs put feature g on or below the lower end of its range (-pi, -1, -1: clamp_bin's bin 0) and on or
    above the upper end (its bin 10, where h >= 11 is clamped)."""
    n, kmax = idx.shape
    counts = np.zeros((n, 33), dtype=np.int64)
    near = np.zeros(n, dtype=bool)
    exits = np.zeros((n, len(PAIR_EXITS)), dtype=np.int64)
    ends = np.zeros((n, 3, 2), dtype=np.int64)
    for k in range(1, kmax):
        live = k < cnt
        if not live.any():
            break
        i = np.flatnonzero(live)
        j = idx[i, k]
        f, margin, ex = pair_features(pts[i], normals[i], pts[j], normals[j], branches=True, exact_ok=exact_ok)
        np.add.at(exits, (i, ex), 1)
        with np.errstate(all="ignore"):
            x = _bin_coords(f)
        top = np.array([PI, 1.0, 1.0])
        for g in range(3):
            np.add.at(ends[:, g, 0], i, (f[:, g] <= -top[g]).astype(np.int64))
            np.add.at(ends[:, g, 1], i, (f[:, g] >= top[g]).astype(np.int64))
        h = np.clip(np.floor(x), -1, 11)
        h = np.clip(h, 0, 10).astype(np.int64) + np.array([0, 11, 22])
        for g in range(3):
            np.add.at(counts, (i, h[:, g]), 1)
        near[i] |= margin < edge
    incr = np.zeros(n)
    has = cnt > 1
    incr[has] = 100.0 / (cnt[has] - 1).astype(np.float64)
    out = np.zeros((n, 33))
    for t in range(int(counts.max()) if counts.size else 0):
        out = np.where(t < counts, out + incr[:, None], out)
    out[~has] = 0.0
    if branches:
        return out, near, exits, ends
    return out, near


def fpfh(sp: np.ndarray, idx: np.ndarray, d2: np.ndarray, cnt: np.ndarray, near_spfh: np.ndarray | None = None):
    """ComputeFPFHFeature from the SPFH rows: (fpfh fp64[n, 33], near_edge bool[n] -- own or a weighted neighbour's SPFH row near an
    edge; None if near_spfh is None)."""
    n, kmax = idx.shape
    acc = np.zeros((n, 33))
    s = np.zeros((n, 3))
    near = None if near_spfh is None else near_spfh.copy()
    for k in range(1, kmax):
        live = (k < cnt) & (d2[:, k] != 0.0)
        if not (k < cnt).any():
            break
        j = np.where(live, idx[:, k], 0)
        with np.errstate(all="ignore"):
            val = sp[j] / d2[:, k][:, None]
        acc = np.where(live[:, None], acc + val, acc)
        for g in range(3):
            for b in range(11):
                s[:, g] = np.where(live, s[:, g] + val[:, 11 * g + b], s[:, g])
        if near is not None:
            near |= live & near_spfh[j]
    with np.errstate(all="ignore"):
        scale = np.where(s != 0.0, 100.0 / s, s)
    out = acc * np.repeat(scale, 11, axis=1) + sp
    out[cnt <= 1] = 0.0
    return out, near


def extract_fpfh_features(pcl: np.ndarray, voxel_size: float, normalize: bool = False):
    """descriptors.py:19-44 on this oracle: (down-sampled points, features N x 33)."""
    pts = np.ascontiguousarray(np.asarray(pcl)[:, :3], dtype=np.float64)
    i, _, c = hybrid_search(pts, voxel_size * 2, 30)
    nv = estimate_normals(pts, i, c)
    down, dn = voxel_down_sample(pts, voxel_size, nv)
    i, d, c = hybrid_search(down, voxel_size * 5, 100)
    sp, _ = spfh(down, dn, i, c)
    f, _ = fpfh(sp, i, d, c)
    if normalize:
        f = f / (np.linalg.norm(f, axis=1, keepdims=True) + 1e-6)
    return down, f

"""TEASER++ registration as registration_node.py:91-159 calls it, restated in numpy / plain Python from DESIGN.md 7.8 (cbar2 = 1,
noise_bound = 0.2, no scale, PMC_EXACT, CHAIN, GNC_TLS): the oracle of csrc/teaser.hip, csrc/teaser_host.cpp and vfmreg/teaser.py.

Every floating-point operation below is a single correctly rounded fp64 operation in the order the specification gives (numpy's
element-wise ufuncs round once per operation and fuse nothing), so the product is asked for EQUAL bits, not near ones.
``tests/test_teaser_oracle.py`` anchors this file against networkx, numpy.linalg.svd and a brute force."""
import math

import numpy as np

NOISE_BOUND, CBAR2, GNC_FACTOR, MAX_ITERATIONS, COST_THRESHOLD = 0.2, 1.0, 1.4, 10000, 1e-16
JACOBI_SWEEPS = 6
SUM_LANES = 256


# ------------------------------------------------------------------------------------------------- 1. the consistency graph
def graph(src, tgt, noise_bound=NOISE_BOUND, cbar2=CBAR2):
    """n x n bool: edge {i, j}, i != j, iff abs(sqrt(d2s) - sqrt(d2t)) <= beta (inclusive; a NaN gives no edge)"""
    src, tgt = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(tgt, np.float64).reshape(-1, 3)
    beta = 2 * noise_bound * math.sqrt(cbar2)

    def d2(p, rows):
        d = p[rows, None, :] - p[None, :, :]       # row i, column j: p[i] - p[j]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    n = len(src)
    adj = np.zeros((n, n), bool)
    with np.errstate(invalid="ignore"):
        for lo in range(0, n, 512):                # (blocks of rows: the n x n x 3 differences of a few thousand points are gigabytes)
            rows = slice(lo, min(lo + 512, n))
            adj[rows] = np.abs(np.sqrt(d2(src, rows)) - np.sqrt(d2(tgt, rows))) <= beta
    np.fill_diagonal(adj, False)
    return adj


def pack(adj):
    """the bool matrix as n x ceil(n / 64) uint64 words, bit j of row i in word j // 64 at position j % 64; padding clear"""
    adj = np.asarray(adj, bool)
    n = adj.shape[0]
    W = (n + 63) // 64
    padded = np.zeros((n, W * 64), bool)
    padded[:, :n] = adj
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(n, W)


def unpack(words, n):
    words = np.ascontiguousarray(words, np.uint64).reshape(n, -1)
    return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


# ------------------------------------------------------------------------------------------------- 2. THE maximum clique
def _rows_as_ints(adj):
    adj = np.asarray(adj, bool)
    return [int.from_bytes(np.packbits(r, bitorder="little").tobytes(), "little") for r in adj]


def max_clique_brute(adj):
    """every clique, by extension with higher indices in ascending order and no pruning at all; the first of the largest size is the
    lexicographically smallest.  For graphs of a dozen vertices."""
    adj = np.asarray(adj, bool)
    n = len(adj)
    best = []

    def extend(clique, cands):
        nonlocal best
        if len(clique) > len(best):
            best = list(clique)
        for at, v in enumerate(cands):
            extend(clique + [v], [u for u in cands[at + 1:] if adj[v, u]])
    extend([], list(range(n)))
    return best


def max_clique(adj):
    """THE maximum clique -- of the largest size, and among those the lexicographically smallest ascending index list -- by a depth-first
    search that extends a clique by higher indices in ascending order and prunes a branch iff size + bound <= best, the bound a greedy
    colouring's number of colours.  It visits cliques in lexicographic order and never prunes a prefix of the answer while
    best < omega, so the first clique of size omega it reaches is the answer.  Exact for every graph; Python ints as bitsets."""
    rows = _rows_as_ints(adj)
    n = len(rows)
    best, record = 0, []

    def colours(P):
        used = 0
        while P:
            used += 1
            q = P
            while q:
                v = (q & -q).bit_length() - 1
                P &= ~(1 << v)
                q &= ~(1 << v) & ~rows[v]
        return used

    def expand(clique, P):
        nonlocal best, record
        if len(clique) > best:
            best, record = len(clique), list(clique)
        if not P or len(clique) + bin(P).count("1") <= best or len(clique) + colours(P) <= best:
            return
        while P:
            if len(clique) + bin(P).count("1") <= best:
                return
            v = (P & -P).bit_length() - 1
            P &= ~(1 << v)
            clique.append(v)
            expand(clique, P & rows[v])     # (P holds indices above v only)
            clique.pop()
    expand([], (1 << n) - 1)
    return record


def core(adj, h):
    """the fixpoint of "keep v iff popcount(adj[v] & kept) >= h - 1": ascending indices"""
    adj = np.asarray(adj, bool)
    alive = np.ones(len(adj), bool)
    while True:
        keep = alive & ((adj & alive[None, :]).sum(1) >= h - 1)
        if (keep == alive).all():
            return np.flatnonzero(alive)
        alive = keep


def greedy_clique_size(adj, seed_rank):
    """the size of the greedy clique the device grows from the seed_rank-th vertex in (degree descending, index ascending) order"""
    adj = np.asarray(adj, bool)
    n = len(adj)
    deg = adj.sum(1)
    order = sorted(range(n), key=lambda v: (-deg[v], v))
    if seed_rank >= n:
        return 0
    P = adj[order[seed_rank]].copy()
    size = 1
    for u in order:
        if P[u]:
            size += 1
            P &= adj[u]
    return size


# ------------------------------------------------------------------------------------------------- the project's 3x3 rotation
def rot_from_sigma(S):
    """csrc/rot3.h restated: one-sided Jacobi, six fixed sweeps, only + - * / sqrt.  (ok, R 3x3)"""
    S = np.asarray(S, np.float64).reshape(3, 3)
    G = [[float(S[r, c]) for c in range(3)] for r in range(3)]
    V = [[1.0 if r == c else 0.0 for c in range(3)] for r in range(3)]
    sq = math.sqrt
    for _ in range(JACOBI_SWEEPS):
        for e in range(3):
            p = 1 if e == 2 else 0
            q = 1 if e == 0 else 2
            alpha = (G[0][p] * G[0][p] + G[1][p] * G[1][p]) + G[2][p] * G[2][p]
            beta = (G[0][q] * G[0][q] + G[1][q] * G[1][q]) + G[2][q] * G[2][q]
            gamma = (G[0][p] * G[0][q] + G[1][p] * G[1][q]) + G[2][p] * G[2][q]
            if gamma == 0.0:
                continue
            zeta = (beta - alpha) / (2.0 * gamma)
            tt = 1.0 / (abs(zeta) + sq(1.0 + zeta * zeta))
            if zeta < 0.0:
                tt = -tt
            c = 1.0 / sq(1.0 + tt * tt)
            s = c * tt
            for r in range(3):
                gp, gq = G[r][p], G[r][q]
                G[r][p] = c * gp - s * gq
                G[r][q] = s * gp + c * gq
                vp, vq = V[r][p], V[r][q]
                V[r][p] = c * vp - s * vq
                V[r][q] = s * vp + c * vq
    nn = [(G[0][c] * G[0][c] + G[1][c] * G[1][c]) + G[2][c] * G[2][c] for c in range(3)]
    i1 = 0
    if nn[1] > nn[0]:
        i1 = 1
    if nn[2] > nn[i1]:
        i1 = 2
    ca = 1 if i1 == 0 else 0
    cb = 1 if i1 == 2 else 2
    i2 = cb if nn[cb] > nn[ca] else ca
    n1, n2 = nn[i1], nn[i2]
    if not n1 > 0.0 or not n2 > n1 * 1e-20:
        return False, np.eye(3)
    s1, s2 = sq(n1), sq(n2)
    u1 = [G[r][i1] / s1 for r in range(3)]
    u2 = [G[r][i2] / s2 for r in range(3)]
    v1 = [V[r][i1] for r in range(3)]
    v2 = [V[r][i2] for r in range(3)]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    u3, v3 = cross(u1, u2), cross(v1, v2)
    R = np.array([[(u1[r] * v1[c] + u2[r] * v2[c]) + u3[r] * v3[c] for c in range(3)] for r in range(3)])
    return True, R


# ------------------------------------------------------------------------------------------------- THE order of summation
def fixed_sum(terms):
    """256 partials p_l = sum of terms[i], i = l, l + 256, ... ascending, from +0.0; then p_l = p_l + p_{l+s}, s = 128, ..., 1"""
    terms = np.asarray(terms, np.float64)
    p = np.zeros(SUM_LANES)
    for base in range(0, len(terms), SUM_LANES):
        chunk = terms[base:base + SUM_LANES]
        p[:len(chunk)] = p[:len(chunk)] + chunk
    s = SUM_LANES // 2
    while s >= 1:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    return float(p[0])


# ------------------------------------------------------------------------------------------------- 3 + 4. chain TIMs, GNC-TLS
def _residuals(R, x, y):
    e = [y[:, a] - ((R[a, 0] * x[:, 0] + R[a, 1] * x[:, 1]) + R[a, 2] * x[:, 2]) for a in range(3)]
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


def gnc_tls(src, tgt, clique, noise_bound=NOISE_BOUND, factor=GNC_FACTOR, max_iterations=MAX_ITERATIONS,
            cost_threshold=COST_THRESHOLD):
    """(R 3x3, weights [k - 1], iterations, v [k x 3] = tgt - R src over the clique)"""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    c = np.asarray(clique, np.int64)
    x, y = src[c[1:]] - src[c[:-1]], tgt[c[1:]] - tgt[c[:-1]]
    m = len(x)
    nb2 = noise_bound * noise_bound
    if nb2 < 1e-16:
        nb2 = 1e-2
    w = np.ones(m)
    R = np.eye(3)
    mu, prev, iterations = 1.0, math.inf, 0
    for it in range(max_iterations):
        H = np.array([[fixed_sum((w * y[:, r]) * x[:, cc]) for cc in range(3)] for r in range(3)])
        ok, R = rot_from_sigma(H)
        if not ok:
            R = np.eye(3)
        r = _residuals(R, x, y)
        cost = fixed_sum(w * r)
        if it == 0:
            with np.errstate(divide="ignore"):
                mu = float(np.float64(1.0) / (np.float64(2.0 * r.max()) / nb2 - 1.0))
            if not mu > 0.0 or not mu < math.inf:
                break
        th1, th2 = (mu + 1.0) / mu * nb2, mu / (mu + 1.0) * nb2
        with np.errstate(divide="ignore", invalid="ignore"):
            mid = np.sqrt(nb2 * mu * (mu + 1.0) / r) - mu
        w = np.where(r >= th1, 0.0, np.where(r <= th2, 1.0, mid))
        iterations = it + 1
        diff = abs(cost - prev)
        mu = mu * factor
        prev = cost
        if diff < cost_threshold:
            break
    s = src[c]
    v = np.stack([tgt[c][:, a] - ((R[a, 0] * s[:, 0] + R[a, 1] * s[:, 1]) + R[a, 2] * s[:, 2]) for a in range(3)], axis=1)
    return R, w, iterations, v


# ------------------------------------------------------------------------------------------------- 5. TLS translation
def tls_scalar(v, rng_):
    """TEASER's scalar TLS estimator for one axis: the x_hat of the smallest cost over the sweep, first on ties"""
    k = len(v)
    ends = sorted([(float(v[i]) - rng_, i + 1) for i in range(k)] + [(float(v[i]) + rng_, -(i + 1)) for i in range(k)])
    wt = 1.0 / (rng_ * rng_)
    card, dot_w, dot_vw, sum_v, sum_sq, outside = 0, 0.0, 0.0, 0.0, 0.0, 0.0
    for _ in range(k):
        outside = outside + rng_
    best = None
    for value, tag in ends:
        i, eps = abs(tag) - 1, (1.0 if tag > 0 else -1.0)
        xi = float(v[i])
        card += 1 if tag > 0 else -1
        dot_w = dot_w + eps * wt
        dot_vw = dot_vw + (eps * wt) * xi
        outside = outside - eps * rng_
        sum_v = sum_v + eps * xi
        sum_sq = sum_sq + (eps * xi) * xi
        if card == 0:
            continue
        x_hat = dot_vw / dot_w
        cost = ((card * (x_hat * x_hat) + sum_sq) - (2.0 * sum_v) * x_hat) + outside
        if best is None or cost < best[0]:
            best = (cost, x_hat)
    return best[1]


def tls_translation(v, noise_bound=NOISE_BOUND, cbar2=CBAR2):
    """(t [3], inlier mask [k]) over ALL rows of v"""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    rng_ = noise_bound * math.sqrt(cbar2)
    t = np.array([tls_scalar(v[:, a], rng_) for a in range(3)])
    return t, (np.abs(v - t[None, :]) <= rng_).all(1)


def tls_scalar_brute(v, rng_):
    """the same estimate without the sweep, for values whose 2k endpoints are all different: every consensus set the sweep meets is
    the set of intervals [v_i - range, v_i + range] that cover the midpoint of two consecutive endpoints; its cost is
    sum (v_i - x_hat)^2 inside + range per point outside, x_hat the mean (all weights are equal).  Returns (smallest cost, its x_hat)
    in ordinary floating point: near, not equal, to the sweep's."""
    v = np.asarray(v, np.float64)
    pts = np.sort(np.r_[v - rng_, v + rng_])
    assert (np.diff(pts) > 0).all()
    best = None
    for x in (pts[1:] + pts[:-1]) / 2:
        inside = np.abs(v - x) < rng_
        if not inside.any():
            continue
        x_hat = v[inside].mean()
        cost = ((v[inside] - x_hat) ** 2).sum() + rng_ * (~inside).sum()
        if best is None or cost < best[0]:
            best = (cost, x_hat)
    return best


# ------------------------------------------------------------------------------------------------- 6. the whole solve
def max_clique_reduced(adj):
    """``max_clique`` on the (h - 1)-core, h the size of the greedy clique grown from the vertex of highest degree: every clique of h
    members or more lies inside that core, so the answer is the same; for graphs of thousands of vertices, where the plain search in
    Python takes minutes.  (tests/test_teaser_oracle.py compares the two.)"""
    adj = np.asarray(adj, bool)
    if len(adj) == 0:
        return []
    kept = core(adj, greedy_clique_size(adj, 0))
    return [int(kept[i]) for i in max_clique(adj[np.ix_(kept, kept)])]


def solve(src, tgt, noise_bound=NOISE_BOUND, cbar2=CBAR2, factor=GNC_FACTOR, max_iterations=MAX_ITERATIONS,
          cost_threshold=COST_THRESHOLD, reduce=False):
    """dict(valid, rotation 3x3, translation [3], clique, weights, iterations, rotation_inliers, translation_inliers) on n x 3 inputs"""
    src, tgt = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(tgt, np.float64).reshape(-1, 3)
    clique = (max_clique_reduced if reduce else max_clique)(graph(src, tgt, noise_bound, cbar2)) if len(src) else []
    if len(clique) <= 1:
        return dict(valid=False, rotation=np.eye(3), translation=np.zeros(3), clique=np.array(clique, np.int64), weights=np.zeros(0),
                    iterations=0, rotation_inliers=np.zeros(0, bool), translation_inliers=np.zeros(0, bool))
    R, w, iterations, v = gnc_tls(src, tgt, clique, noise_bound, factor, max_iterations, cost_threshold)
    t, t_in = tls_translation(v, noise_bound, cbar2)
    return dict(valid=True, rotation=R, translation=t, clique=np.array(clique, np.int64), weights=w, iterations=iterations,
                rotation_inliers=w >= 0.5, translation_inliers=t_in)


def pose_of(solution):
    T = np.eye(4)
    T[:3, :3] = solution["rotation"]
    T[:3, 3] = solution["translation"]
    return T


# ------------------------------------------------------------------------------------------------- planted scenes
def planted_scene(n, inliers, seed):
    """src ~ U([-60, 60]^2 x [-3, 12]); yaw ~ U(+-pi); t ~ (N(0, 10), N(0, 10), N(0, 1)); inlier noise N(0, 0.05) per axis; the
    outliers' targets redrawn uniformly in the same box.  (src, tgt, T 4x4, the inlier indices ascending)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-60.0, -60.0, -3.0]), np.array([60.0, 60.0, 12.0])
    src = rng.uniform(lo, hi, (n, 3))
    yaw = rng.uniform(-math.pi, math.pi)
    t = rng.normal(0.0, 1.0, 3) * np.array([10.0, 10.0, 1.0])
    R = np.array([[math.cos(yaw), -math.sin(yaw), 0.0], [math.sin(yaw), math.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
    tgt = src @ R.T + t + rng.normal(0.0, 0.05, (n, 3))
    inl = np.sort(rng.choice(n, inliers, replace=False))
    out = np.setdiff1d(np.arange(n), inl)
    tgt[out] = rng.uniform(lo, hi, (len(out), 3))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return src, tgt, T, inl


PLANTED = [(65, 20), (130, 13), (400, 160), (700, 70)]


def errors(R, t, T):
    """(RRE in degrees, RTE in m) of (R, t) against the 4x4 truth"""
    c = (np.trace(R.T @ T[:3, :3]) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1)))), float(np.linalg.norm(t - T[:3, 3]))

"""Seeded inputs for the narrow-row Euclidean search (VFM_MATCH_NARROW, csrc/match_l2_narrow.hip).  Shared by
tests/test_l2_narrow_cases.py (CPU: the generators have the properties claimed here, checked with the oracle alone) and
tests/test_gpu_l2_narrow.py (GPU: the library returns the oracle's answer on them, bit for bit).  Every generator returns float32
arrays; nothing here touches a device.

The kernel's geometry the cases aim at (include/vfmreg.h, match_l2_narrow.hip): map rows are screened in tiles of 32; inside a tile the
two halves of a wavefront hold rows r and r + 4 (mod 8) of the same query; the map is cut into slices at tile edges; the screened
quantity is c = |b~|^2 - 2 a~.b~ in f32 on rows scaled by a common power of two so that every norm is <= 1, inside a window of
(8 Kp + 16) 2^-24, Kp = d rounded up to even.
"""
from __future__ import annotations

import numpy as np

NARROW = 2
NARROW_MAX_D = 64
WIDTHS = (1, 2, 7, 32, 33, 34, 63, 64)
SHAPES = ((1, 1), (1, 257), (31, 33), (33, 31), (65, 1025), (129, 4099))
TIE_WIDTHS = (7, 33, 64)


def window(d: int) -> float:
    """the kernel's window on c, in scaled units"""
    return (8 * ((d + 1) & ~1) + 16) * 2.0 ** -24


def common_scale(a: np.ndarray, b: np.ndarray) -> float:
    """a power of two s with every row norm of s a and s b in (0.24, 1] (the library's own choice may differ by a factor of two)"""
    mx = max(float(np.sqrt((a.astype(np.float64) ** 2).sum(1).max())), float(np.sqrt((b.astype(np.float64) ** 2).sum(1).max())))
    if mx == 0.0:
        return 1.0
    return 2.0 ** -int(np.ceil(np.log2(mx * 1.01)))


# ------------------------------------------------------------------------------------------------------------------ 1. shapes
def random_pair(n: int, m: int, d: int, seed: int = 0):
    """random rows, half the queries planted near map rows (as _l2_pair of tests/test_gpu_bounds.py)"""
    rng = np.random.default_rng(1000 * d + 7 * n + m + seed)
    b = rng.standard_normal((m, d)).astype(np.float32)
    a = rng.standard_normal((n, d)).astype(np.float32)
    k = n // 2
    a[:k] = b[rng.integers(0, m, k)] + 0.05 * rng.standard_normal((k, d)).astype(np.float32)
    return a, b


# ------------------------------------------------------------------------------------------------------------------ 2. exact ties
def tie_cases(d: int):
    """{name: (a, b, pairs)}: ``pairs`` lists (query, lower copy, upper copy) -- two identical map rows that are the query's nearest."""
    rng = np.random.default_rng(50 + d)
    out = {}

    def near(row):
        return (row + 1e-4 * rng.standard_normal(d)).astype(np.float32)

    # rows 31 | 32: the two copies sit in neighbouring tiles
    b = rng.standard_normal((100, d)).astype(np.float32)
    b[32] = b[31]
    out["tile edge"] = (np.stack([near(b[31]), rng.standard_normal(d).astype(np.float32)]), b, [(0, 31, 32)])
    # rows r and r + 4 of one tile: the two halves of a wavefront
    b = rng.standard_normal((100, d)).astype(np.float32)
    b[45] = b[41]
    b[13] = b[9]
    out["lane halves"] = (np.stack([near(b[41]), near(b[9])]), b, [(0, 41, 45), (1, 9, 13)])
    # a pair across EVERY tile edge of a map that is searched in several slices: whatever the slicing rule, every slice boundary
    # has a pair on either side of it
    m = 4099
    b = rng.standard_normal((m, d)).astype(np.float32)
    edges = list(range(32, m, 32))
    a = np.empty((len(edges), d), np.float32)
    pairs = []
    for i, e in enumerate(edges):
        b[e] = b[e - 1]
        a[i] = near(b[e])
        pairs.append((i, e - 1, e))
    out["every tile edge"] = (a, b, pairs)
    return out


def zero_distance_case(d: int):
    """queries that ARE map rows (d^2 = 0), some of them twice in the map: (a, b)"""
    rng = np.random.default_rng(60 + d)
    b = rng.standard_normal((300, d)).astype(np.float32)
    b[200] = b[17]
    a = b[[17, 0, 299, 150]].copy()
    return a, b


def all_zero_case(d: int):
    """all-zero rows on both sides, as FPFH gives isolated points, among ordinary ones: (a, b)"""
    rng = np.random.default_rng(70 + d)
    b = np.abs(rng.standard_normal((200, d))).astype(np.float32)
    b[[3, 40, 41, 199]] = 0.0
    a = np.abs(rng.standard_normal((6, d))).astype(np.float32)
    a[[1, 4]] = 0.0
    return a, b


def only_zero_case(d: int):
    return np.zeros((5, d), np.float32), np.zeros((70, d), np.float32)


def identical_map_case(d: int):
    """a map of 300 identical rows: (a, b)"""
    rng = np.random.default_rng(80 + d)
    row = rng.standard_normal(d).astype(np.float32)
    return rng.standard_normal((9, d)).astype(np.float32), np.tile(row, (300, 1))


# ------------------------------------------------------------------------------------------------------------------ 3. near-ties
def fpfh_like_row(rng) -> np.ndarray:
    """33 columns, three 11-bin blocks each summing to 100, the first bin of every block in [64, 128) (one f32 ulp there is 2^-17)"""
    x = np.zeros(33, np.float64)
    for blk in range(3):
        big = rng.integers(64 * 8, 90 * 8) / 8.0
        rest = rng.dirichlet(np.ones(10)) * (100.0 - big)
        rest = np.round(rest * 8) / 8.0
        rest[-1] = 100.0 - big - rest[:-1].sum()
        x[11 * blk] = big
        x[11 * blk + 1:11 * blk + 11] = rest
    return x.astype(np.float32)


def near_tie_case(seed: int = 3):
    """query x; map rows x + j 2^-17 e_0 for j = 1 .. 6 in shuffled order: (a [1, 33], b [6, 33], j per map row).  The squared distances
    are j^2 2^-34 -- about 6e-11 apart --, far below what f32 resolves of c; only the fp64 decision separates the rows."""
    rng = np.random.default_rng(seed)
    x = fpfh_like_row(rng)
    assert np.isclose(x[:11].sum(), 100.0) and 64 <= x[0] < 127
    order = np.array([4, 2, 6, 1, 5, 3])
    b = np.tile(x, (6, 1))
    b[:, 0] = x[0] + order.astype(np.float32) * np.float32(2.0 ** -17)
    return x[None, :].copy(), b, order


# ------------------------------------------------------------------------------------------------------------------ 4. scale
def _fpfh_like_pair(n, m, seed):
    rng = np.random.default_rng(seed)
    b = np.stack([fpfh_like_row(rng) for _ in range(m)])
    a = np.stack([fpfh_like_row(rng) for _ in range(n)])
    k = n // 2
    a[:k] = b[rng.integers(0, m, k)]
    a[:k, 1:5] += rng.integers(-4, 5, (k, 4)).astype(np.float32) / 8.0
    return a, b


def scale_cases():
    """{name: (a, b)} on FPFH-like rows (d = 33): both sets times 2^40 and 2^-40 (exact), one map row 1e4 times longer than the rest,
    and both sets times 2^62 -- there the f32 products a_k b_k overflow, and are finite only on the commonly scaled rows."""
    a, b = _fpfh_like_pair(40, 700, 90)
    out = {"x 2^40": (a * np.float32(2.0 ** 40), b * np.float32(2.0 ** 40)),
           "x 2^-40": (a * np.float32(2.0 ** -40), b * np.float32(2.0 ** -40)),
           "x 2^62": (a * np.float32(2.0 ** 62), b * np.float32(2.0 ** 62))}
    bl = b.copy()
    bl[123] *= np.float32(1e4)
    out["one long map row"] = (a.copy(), bl)
    return out


# ------------------------------------------------------------------------------------------------------------------ 5. real features
FPFH_SEEDS = (2, 5)


def fpfh_scene(seed: int):
    from vfmreg import synth
    return synth.make_structured_scene(1500, 8000, seed=seed)

"""Clouds and queries at the clamped border of the sorted-key grid (csrc/grid3.h), shared by tests/test_grid_border_cases.py (CPU: the
inputs are tie-free, so the brute-force oracles' answers are unambiguous) and tests/test_gpu_grid_border.py (GPU).

Coordinates are (cell index + fraction) * cell with indices around +-L, L the quantiser's clamp (nn3: 2^20 - 16, FPFH: 2^20 - 2): cells
below L keep their own index, cells at and beyond it share the border cell."""
import numpy as np

NN3_L = (1 << 20) - 16
FPFH_L = (1 << 20) - 2


def _block(rng, n, lo, hi):
    """n points, axis a uniform over cells [lo[a], hi[a]) (in cells)"""
    return np.stack([rng.uniform(lo[a], hi[a], n) for a in range(3)], -1)


def nn3_cloud(cell: float, seed: int = 0, per: int = 330):
    """(points <= 3000 x 3, names of the sub-clouds per row).  x straddles +L, y straddles -L, z straddles both ends, one sub-cloud has
    all three axes beyond the clamp (and one beyond -L), and points of both sides of the clamp are repeated (equal distances: the lower
    index wins)."""
    rng = np.random.default_rng(seed)
    L = NN3_L
    blocks = [
        ("x+", _block(rng, per, (L - 12, 0, 0), (L + 12, 10, 10))),
        ("y-", _block(rng, per, (0, -L - 12, 0), (10, -L + 12, 10))),
        ("z+", _block(rng, per, (0, 0, L - 12), (10, 10, L + 12))),
        ("z-", _block(rng, per, (0, 0, -L - 12), (10, 10, -L + 12))),
        ("xyz+", _block(rng, per, (L + 1, L + 1, L + 1), (L + 12, L + 12, L + 12))),
        ("xyz-", _block(rng, per, (-L - 12, -L - 12, -L - 12), (-L - 1, -L - 1, -L - 1))),
        ("corner", _block(rng, per, (L - 3, -L - 3, L - 3), (L + 3, -L + 3, L + 3))),
    ]
    pts = np.concatenate([b for _, b in blocks])
    names = np.concatenate([[nm] * len(b) for nm, b in blocks])
    xs = pts[:per]
    inside = xs[xs[:, 0] < L - 1][:40]
    beyond = xs[xs[:, 0] > L + 1][:40]
    assert len(inside) == 40 and len(beyond) == 40
    dup = np.concatenate([inside, beyond, inside[:10]])
    pts = np.concatenate([pts, dup]) * cell
    names = np.concatenate([names, ["dup"] * len(dup)])
    order = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[order]), names[order]


def nn3_queries(P: np.ndarray, cell: float, seed: int = 1):
    """dict name -> queries.  'rows': every row of the cloud; 'near': rows moved by < 1 mm (and by less than half a cell); 'border': up to 8
    cells either side of +-L in one axis, the others inside the sub-cloud of that axis; 'far': 3e6 cells out and 1e12 (with cell = 1e-7
    the product with 1 / cell is beyond 2^63); 'opposite': the corners opposite to the sub-clouds."""
    rng = np.random.default_rng(seed)
    L = NN3_L
    step = min(5e-4, 0.4 * cell)
    border = []
    for axis, sign in ((0, 1), (1, -1), (2, 1), (2, -1)):
        q = rng.uniform(0, 10, (120, 3))
        q[:, axis] = sign * (L + rng.uniform(-8, 8, 120))
        border.append(q)
    q = np.stack([L + rng.uniform(-8, 8, 120), -L + rng.uniform(-8, 8, 120), L + rng.uniform(-8, 8, 120)], -1)
    border.append(q)
    border.append(L + rng.uniform(-8, 12, (120, 3)))
    border.append(-L - rng.uniform(-8, 12, (120, 3)))
    far = np.concatenate([
        rng.uniform(0, 10, (40, 3)) * cell + np.array([3e6 * cell, 0, 0]),
        rng.uniform(0, 10, (40, 3)) * cell + np.array([0, -3e6 * cell, 3e6 * cell]),
        rng.uniform(-1, 1, (20, 3)) + np.array([1e12, 0.0, 0.0]),
        rng.uniform(-1, 1, (20, 3)) + np.array([-1e12, 1e12, -1e12]),
    ])
    opposite = np.stack([s * (L + rng.uniform(-4, 20, 60)) for s in (-1, 1, -1)], -1)
    return {
        "rows": P.copy(),
        "near": P + rng.uniform(-step, step, P.shape),
        "border": np.concatenate(border) * cell,
        "far": far,
        "opposite": opposite * cell,
    }


def fpfh_cloud(r: float, sign: int, seed: int = 0, per: int = 260):
    """<= 2000 points for ops.fpfh_search(radius r) whose cells (edge r (1 + 1e-6)) lie around sign * L in one, two and three axes, with
    pairs less than r apart in the cells (L - 1, L), (L, clamped L + 1) and (clamped, clamped).  sign = -1 mirrors everything."""
    rng = np.random.default_rng(seed)
    L = FPFH_L
    cell = r * (1.0 + 1e-6)
    blocks = [
        _block(rng, per, (L - 3, 0, 0), (L + 4, 3, 3)),
        _block(rng, per, (0, L - 3, 0), (3, L + 4, 3)),
        _block(rng, per, (0, 0, L - 3), (3, 3, L + 4)),
        _block(rng, per, (L - 2, L - 2, 0), (L + 3, L + 3, 3)),
        _block(rng, 2 * per, (L - 2, L - 2, L - 2), (L + 3, L + 3, L + 3)),     # queries in the cell (L, L, L): the last key of all
        _block(rng, per, (L + 1, L + 1, L + 1), (L + 3, L + 3, L + 3)),         # all three axes beyond the clamp
    ]
    pairs = []
    for axis in range(3):
        for edge in (L, L + 1, L + 3):           # a pair astride the face `edge`: cells (edge - 1, edge)
            base = np.array([1.5, 1.5, 1.5]) + rng.uniform(-0.2, 0.2, 3)
            for off in (-0.11, 0.13):
                p = base.copy()
                p[axis] = edge + off + rng.uniform(-0.01, 0.01)
                pairs.append(p)
        a = np.full(3, L + 2.5) + rng.uniform(-0.2, 0.2, 3)      # both clamped in every axis
        pairs += [a, a + rng.uniform(-0.2, 0.2, 3)]
    pts = np.concatenate(blocks + [np.array(pairs)]) * cell * sign
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


def cells(pts: np.ndarray, cell: float, lim: int) -> np.ndarray:
    """grid3::cell for every coordinate"""
    with np.errstate(invalid="ignore"):
        c = np.floor(pts * (1.0 / cell))
    return np.where(np.isnan(c), -lim, np.clip(c, -lim, lim)).astype(np.int64)

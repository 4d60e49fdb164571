"""Hand-made neighbour rows that drive csrc/fpfh.hip through the exits its structured-scene test never takes, shared by the census
in tests/test_fpfh_oracle.py (CPU: which exit every row takes, by the oracle's branch ids) and tests/test_gpu_fpfh_branches.py (GPU).

Rows are fed straight into ops.fpfh_normals / fpfh_spfh / fpfh_fpfh as idx / d2 / count, so a case dictates its own neighbourhood.
Most coordinates are small dyadic numbers: sums, products and the division by a power-of-two count are then exact, and a covariance
is exactly diagonal, exactly singular or exactly isotropic where the case wants it so."""
import numpy as np

SHIFT = np.array([3.0e5, -6.0e5, 75.0])      # UTM-like: the one-pass covariance loses digits here
WIDTH = 32                                   # max_nn of the normals' rows
E = 2.0 ** -52


def _frames():
    return [np.array(f, dtype=np.float64) for f in (
        [(3, 4, 0), (-4, 3, 0), (0, 0, 5)], [(1, 1, 0), (1, -1, 0), (0, 0, 1)], [(0, 1, 1), (0, 1, -1), (1, 0, 0)],
        [(1, 0, 1), (1, 0, -1), (0, 1, 0)], [(1, 2, 2), (2, 1, -2), (2, -2, 1)], [(2, 3, 6), (3, -6, 2), (6, 2, -3)])]


def _axes_points(F, a, b, c, dup=0):
    """+-a F0, +-b F1, +-c F2 (covariance: exact, principal axes F), one pair repeated to make 8 points"""
    pts = [a * F[0], -a * F[0], b * F[1], -b * F[1], c * F[2], -c * F[2]]
    if dup:
        pts += [pts[2 * dup - 2], pts[2 * dup - 1]]
    return np.array(pts)


def normal_cases():
    """dict(pts n x 3, idx int32 n x WIDTH, count int32 n, kind str[n], axis n x 3 (the dominant axis of a row whose normal is not
    unique, else 0)).  The row of a case's first point holds the case; the rows of its other points hold 0, 1 or 2 neighbours."""
    rng = np.random.default_rng(11)
    cases = []   # (kind, points, dominant axis or None)

    def add(kind, pts, axis=None):
        cases.append((kind, np.asarray(pts, dtype=np.float64), axis))

    # zero covariance: all neighbours the same point (dyadic coordinates: every sum is exact)
    for k, p in ((4, (1.5, -2.25, 0.75)), (8, (0.0, 0.0, 0.0)), (5, (3.0, 1.0, -2.0)), (16, tuple(SHIFT))):
        add("zero", np.tile(p, (k, 1)))
    # grids in the axis planes: diagonal covariance, the normal is the axis of the zero entry
    g = np.stack(np.meshgrid(np.arange(4.0), np.arange(4.0), indexing="ij"), -1).reshape(-1, 2)
    for scale, off in ((0.25, (1.0, -3.0, 0.5)), (1.0, (0.0, 0.0, 0.0)), (0.5, (-8.0, 2.0, 4.0)), (2.0, tuple(SHIFT))):
        u, v = g[:, 0] * scale, g[:, 1] * scale * 2.0          # unequal extents: no tie
        z = np.zeros(len(g))
        add("diag_z", np.stack([u, v, z], -1) + off)
        add("diag_x", np.stack([z, u, v], -1) + off)
        add("diag_y", np.stack([u, z, v], -1) + off)
    # ties of the diagonal entries: lines along an axis (two zero entries), a square grid's two equal entries below / above the
    # third, the octahedron and the cube (three equal entries)
    t = np.arange(-2.0, 2.0)[:, None]
    for ax in range(3):
        add("diag_tie", t * np.eye(3)[ax] * 0.5)
    octa = np.concatenate([np.eye(3), -np.eye(3), np.eye(3)[:1], -np.eye(3)[:1]])
    add("diag_tie", np.concatenate([np.eye(3), -np.eye(3)]))
    add("diag_tie", octa[:, [1, 2, 0]] * 0.5)                   # y doubled: d0 = d2 < d1
    add("diag_tie", octa[:, [2, 0, 1]] * 2.0)                   # z doubled: d0 = d1 < d2 -- the rule still says z
    add("diag_tie", np.array([(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64))
    # tilted planes: smallest eigenvalue exactly 0 (integer combinations of two integer vectors), and nearly 0
    uv = np.array([(i, j) for i in range(-2, 2) for j in range(-2, 2)], dtype=np.float64)
    for a, b in (((1, 0, 1), (0, 1, 1)), ((2, 1, 0), (0, 1, 3)), ((1, 1, 1), (1, -1, 0)), ((1, 2, 2), (2, 1, -2)), ((3, 4, 0), (0, 1, 2))):
        a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
        plane = uv[:, :1] * a * 0.25 + uv[:, 1:] * b * 0.5
        n = np.cross(a, b) / np.linalg.norm(np.cross(a, b))
        add("plane", plane)
        add("plane", plane + rng.uniform(-1e-9, 1e-9, (16, 1)) * n)
        add("plane", plane + rng.uniform(-1e-4, 1e-4, (16, 1)) * n)
        add("plane_shifted", plane + rng.uniform(-1e-4, 1e-4, (16, 1)) * n + SHIFT)
    # needles: one large eigenvalue, two small ones that are equal or nearly so; dominant axis with |x| > |y| (U built from x, z) and
    # with |x| <= |y| (U built from y, z)
    tt = np.arange(-8.0, 8.0)[:, None] * 0.125
    for d in ((1, 0, 0), (2, 1, 0), (3, -1, 2), (0, 1, 0), (0, 0, 1), (1, 2, 0), (1, -3, 1), (0, 1, 1), (1, 1, 1), (-1, 1, 0)):
        d = np.array(d, dtype=np.float64)
        axis = d / np.linalg.norm(d)
        if np.count_nonzero(d) > 1:
            add("needle", tt * d, axis)                                       # exactly collinear
        add("needle", tt * d + rng.uniform(-1e-7, 1e-7, (16, 3)), axis)
        add("needle", tt * d + rng.uniform(-1e-3, 1e-3, (16, 3)), axis)
    # ellipsoid axes +-a F0, +-b F1, +-c F2 in rotated frames: oblate (half_det < 0), prolate (half_det > 0), and equal pairs
    for fi, F in enumerate(_frames()):
        for a, b, c in ((3, 2, 1), (1, 2, 3), (2, 3, 1), (5, 4, 1), (1, 4, 5)):
            add("gapped", _axes_points(F, a, b, c, dup=1 + fi % 3) * 0.25)
        add("gapped", _axes_points(F, 2, 2, 1) * 0.5)                          # oblate: the small eigenvalue is simple
        add("gapped", _axes_points(F, 1, 3, 3, dup=1) * 0.5)
        add("gapped_shifted", _axes_points(F, 3, 2, 1, dup=2) * 0.25 + SHIFT)
        add("gapped_shifted", _axes_points(F, 2, 2, 1, dup=3) * 0.5 + SHIFT)
        big = F[0] / np.linalg.norm(F[0])
        add("prolate", _axes_points(F, 2, 1, 1), big)                          # two equal small eigenvalues
        add("prolate", _axes_points(F, 1.25, 1, 1), big)
        add("prolate", _axes_points(F, 5, 4, 4), big)
        add("prolate", _axes_points(F[[1, 0, 2]], 5, 4, 4), F[1] / np.linalg.norm(F[1]))
    # blobs isotropic to the last bit but for off-diagonal entries of 2^-55 .. 2^-100: the three computed eigenvalues are the SAME
    # number, so neither "smallest" test holds and both signs of half_det end in their cross product
    for m in ((55, 55, 58), (55, 60, 100), (55, 58, 100), (55, 55, 55), (55, 70, 70), (55, 58, 58)):
        for s in ((1, 1, 1), (1, 1, -1), (-1, 1, 1), (1, -1, -1)):
            h = [s[k] * 2.0 ** -m[k] for k in range(3)]
            add("isotropic", [(1, h[0], 0), (-1, -h[0], 0), (0, 1, h[1]), (0, -1, -h[1]), (h[2], 0, 1), (-h[2], 0, -1)])
    # near-isotropic blobs with a last-bit spread of the axes (the trigonometric branch at its worst conditioning)
    F = _frames()[0]
    for a, b, c in ((1 + E, 1 + E, 1), (1, 1 + 2 * E, 1 + E), (1 + 2.0 ** -26, 1, 1 - E / 2), (1, 1 - E / 2, 1 + 2.0 ** -27)):
        add("isotropic", _axes_points(F, a, b, c, dup=2))
        add("isotropic", _axes_points(F[[2, 0, 1]], a, b, c, dup=1))

    # pairs of nearly equal axes in a frame with no zero entry: the m11 / m01 arm of eigenvector1
    F = _frames()[4]
    for a, b, c in ((1, 1, 1 + 2.0 ** -26), (1, 2, 1 + 2.0 ** -27), (1, 3, 2), (1, 1 + 2.0 ** -26, 1)):
        add("blob", _axes_points(F, a, b, c, dup=2 if (a, b, c) != (1, 3, 2) else 0))

    n = sum(len(p) for _, p, _ in cases)
    pts = np.concatenate([p for _, p, _ in cases])
    idx = np.full((n, WIDTH), -1, dtype=np.int32)
    cnt = np.zeros(n, dtype=np.int32)
    kind = np.empty(n, dtype=object)
    axis = np.zeros((n, 3))
    s = 0
    for name, p, ax in cases:
        k = len(p)
        assert 3 <= k <= WIDTH
        idx[s, :k] = np.arange(s, s + k)
        cnt[s] = k
        kind[s] = name
        if ax is not None:
            axis[s] = ax
        for t_ in range(1, k):                   # the other points of the case: 0, 1 and 2 neighbours (the identity covariance)
            c = (t_ - 1) % 3
            idx[s + t_, :c] = np.arange(s, s + c)
            cnt[s + t_] = c
            kind[s + t_] = f"cnt{c}"
        s += k
    return dict(pts=np.ascontiguousarray(pts), idx=idx, count=cnt, kind=kind.astype(str), axis=axis)


# ---------------------------------------------------------------------------------------------------- pair features, SPFH, FPFH
FEATURE_WIDTH = 1024


def feature_cases():
    """dict(pts, normals n x 3, idx int32 n x 1024, d2 n x 1024, count int32 n, kind str[n]).  Position 0 of a row is the point itself
    (the kernels skip it); d2 is the oracle's own squared distance, so a coincident neighbour has d2 == 0 exactly."""
    rng = np.random.default_rng(12)
    P, N, rows = [], [], []        # rows: (kind, centre index, [neighbour indices])

    def point(p, n):
        P.append(np.asarray(p, dtype=np.float64))
        N.append(np.asarray(n, dtype=np.float64))
        return len(P) - 1

    def unit(v):
        v = np.asarray(v, dtype=np.float64)
        return v / np.linalg.norm(v)

    def star(kind, p, n, nbrs):
        """a centre and its neighbours [(point, normal)]"""
        c = point(p, n)
        rows.append((kind, c, [point(q, m) for q, m in nbrs]))
        return c

    def generic(k, centre=(0.0, 0.0, 0.0), spread=0.3):
        return [(np.asarray(centre) + rng.uniform(-spread, spread, 3), unit(rng.normal(0, 1, 3))) for _ in range(k)]

    X, Y, Z = np.eye(3)
    for rep in range(3):
        o = np.array([4.0 * rep, 0.0, 0.0])
        nz = unit(rng.normal(0, 1, 3))
        # coincident neighbours: dn == 0 in the SPFH pair, dist == 0 skipped in the FPFH sum
        star("coincident", o, nz, [(o, unit(rng.normal(0, 1, 3))), (o, nz)] + generic(4 + rep, o))
        # n1 parallel to d (exact: axis-aligned): vn == 0 with the roles kept; n2 parallel to d with n1 not: the swap, then vn == 0
        star("n1_parallel", o + Y, X, [(o + Y + 0.5 * X, unit((1, 2, 2))), (o + Y - 0.25 * X, Z)] + generic(3, o + Y))
        star("n2_parallel", o + 2 * Y, unit((3, 4, 0)), [(o + 2 * Y + 0.5 * X, X), (o + 2 * Y - 2.0 * Z, -Z)] + generic(3, o + 2 * Y))
        # symmetric pairs: angle1 == -angle2 exactly (n2 = n1 mirrored in the plane across d): |angle1| == |angle2|, no swap
        for d, n1, n2 in ((X, (0.6, 0.8, 0.0), (-0.6, 0.8, 0.0)), (Z, (0.0, 0.28, 0.96), (0.28, 0.0, -0.96)), (Y, (0.8, -0.6, 0.0), (0.0, 0.6, 0.8))):
            star("symmetric", o + 3 * Y, n1, [(o + 3 * Y + 0.5 * (1 + rep) * d, n2)] + generic(2, o + 3 * Y))
        # each side of the swap, far from the decision
        star("kept", o + 4 * Y, unit((0.9, 0.1, 0.42)), [(o + 4 * Y + 0.5 * X, unit((0.1, 0.9, 0.42)))] + generic(2, o + 4 * Y))
        star("swapped", o + 5 * Y, unit((0.1, 0.9, 0.42)), [(o + 5 * Y + 0.5 * X, unit((0.9, 0.1, 0.42)))] + generic(2, o + 5 * Y))
        # zero-length normals (a down-sampled voxel can average to one): v = d x 0 = 0
        star("zero_normal", o + 6 * Y, (0.0, 0.0, 0.0), generic(3, o + 6 * Y))
        star("zero_normal_nbr", o + 7 * Y, nz, [(o + 7 * Y + 0.5 * X, (0.0, 0.0, 0.0))] + generic(3, o + 7 * Y))
        # features ON the ends of their ranges, exact in fp64 (no libm call decides the bin):
        #   f2 = angle1 = -+1 with n1 = (-+1, 1, 0) (not a unit vector -- neither is a down-sampled normal): d x n1 is not 0
        #   f1 = v . n2 = -+1 with n2 = -+v
        #   f0 = atan2(+-0, negative) = +-pi with n2 = -n1 (w . n2 = +-0, n1 . n2 = -1)
        e = o + 8 * Y
        star("f2_plus", e, (1.0, 1.0, 0.0), [(e + 0.5 * X, Z), (e + 0.25 * X, unit((0.0, 0.6, 0.8)))])
        star("f2_minus", e + Y, (-1.0, 1.0, 0.0), [(e + Y + 0.5 * X, Z), (e + Y + 0.25 * X, unit((0.0, 0.6, 0.8)))])
        star("f1_minus", e + 2 * Y, Z, [(e + 2 * Y + 0.5 * X, Y), (e + 2 * Y + 0.25 * Y, -X)])      # v = d x n1 = -y | x: n2 = -v
        star("f1_plus", e + 3 * Y, Z, [(e + 3 * Y + 0.5 * X, -Y), (e + 3 * Y + 0.25 * Y, X)])
        star("f0_pi", e + 4 * Y, Z, [(e + 4 * Y + 0.5 * X, -Z), (e + 4 * Y - 0.5 * Y, -Z)])
        star("f0_pi", e + 5 * Y, -Z, [(e + 5 * Y + 0.5 * X, Z), (e + 5 * Y + 0.5 * Y, Z)])
        # a normal longer than 1: |angle| > 1, acos is a NaN on one side of the >, the roles stay; f2 = 2 is clamped into bin 10
        star("long_normal", e + 6 * Y, (2.0, 1.0, 0.0), [(e + 6 * Y + 0.5 * X, unit((0.0, 0.6, 0.8))), (e + 6 * Y - 0.5 * X, Z)])
        # counts 0, 1 and 2
        c = point(e + 7 * Y, nz)
        rows.append(("cnt0", c, None))
        c = point(e + 7.5 * Y, nz)
        rows.append(("cnt1", c, []))
        star("cnt2", e + 8 * Y, nz, generic(1, e + 8 * Y))
    # 64, 65 and 1024 entries: the lane-stride edges of the SPFH loop (pairs 63, 64 and 1023)
    for k in (64, 65, 1024, 64, 65, 64, 65):
        o = np.array([0.0, 40.0 + k + len(rows), 0.0])
        star(f"row{k}", o, unit(rng.normal(0, 1, 3)), generic(k - 1, o, spread=0.45))
    # a point whose neighbours all have all-zero SPFH rows (their own rows hold one entry): s == 0 in the FPFH group sum
    for rep in range(3):
        o = np.array([-10.0 - rep, 0.0, 0.0])
        star("zero_spfh_nbrs", o, unit(rng.normal(0, 1, 3)), generic(3 + rep, o))
    lonely = {j for kind, _, nb in rows if kind == "zero_spfh_nbrs" for j in nb}

    pts, nrm = np.array(P), np.array(N)
    n = len(pts)
    idx = np.full((n, FEATURE_WIDTH), -1, dtype=np.int32)
    d2 = np.zeros((n, FEATURE_WIDTH))
    cnt = np.zeros(n, dtype=np.int32)
    kind = np.array(["leaf"] * n, dtype=object)
    owner = np.full(n, -1)
    for name, c, nb in rows:
        kind[c] = name
        if nb is None:
            continue
        row = [c] + nb
        idx[c, :len(row)] = row
        cnt[c] = len(row)
        owner[nb] = c
    for j in range(n):                 # a neighbour's own row: itself, its centre and its fellow neighbours (nothing for the lonely)
        if owner[j] < 0:
            continue
        if j in lonely:
            idx[j, 0], cnt[j], kind[j] = j, 1, "lonely"
            continue
        c = owner[j]
        fellows = [t for t in idx[c, 1:cnt[c]] if t != j][:40]
        row = [j, c] + fellows
        idx[j, :len(row)] = row
        cnt[j] = len(row)
    for i in range(n):
        k = cnt[i]
        d = pts[idx[i, :k]] - pts[i]
        d2[i, :k] = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return dict(pts=np.ascontiguousarray(pts), normals=np.ascontiguousarray(nrm), idx=idx, d2=d2, count=cnt, kind=kind.astype(str))

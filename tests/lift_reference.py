"""Descriptor lifting restated on the CPU in long double / fp64 -- an independent check of csrc/project.hip.

The reference lifts ViT patch features onto LiDAR points in three steps (prepare_scenes.py:50-107):
  1. project every point into every camera (nclt.py:311-366, oxford_robotcar.py:330-363, kitti_odometry.py:110-125);
  2. sample the bilinearly upsampled patch grid at the point's pixel (image_features.py:104-110), zero where the raw
     image is black (prepare_scenes.py:57-62), with the features turned by rot90 for NCLT (prepare_scenes.py:80-81);
  3. let the first camera in dict order win (np.unique(return_index=True), prepare_scenes.py:96-101).

This module states the same thing again, without the oracle's or the kernels' operation order:

* The projection is evaluated in ``np.longdouble``.  A point is *undecided* when fp64 in another operation order may
  legitimately land on either side of a truncation or a filter: its depth lies within ``TOL`` of 0, or a pixel
  coordinate of a point in front of the camera and near the image lies within ``TOL * max(1, |x|)`` of an integer
  (the integers include the bounds 0 / W / H, the inclusive RobotCar / KITTI bound and the NCLT window edges).  For
  such points every admissible answer is listed; everywhere else the answer is unique.
* The upsample is never materialised.  ``interp_matrix`` runs ``F.interpolate`` on an identity matrix, which yields
  torch's own source indices and lambdas as an [out, in] weight matrix; a descriptor is ``Ah[row] . G . Aw[col]^T``
  evaluated in fp64 at the needed pixels only (two taps per axis).

Two documented deviations from the reference are encoded here (and named in the tests):
* RobotCar / KITTI keep pixels with ``u == W`` or ``v == H`` (inclusive bound); the reference's ``feat[v, u]`` raises
  IndexError there, the product writes a zero row for them (csrc/project.hip, gather_point).
* A cloud no camera sees gives all-zero descriptors; the reference fails on ``pcl_indices is None``.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

LD = np.longdouble
TOL = 1e-9               # distance to a truncation / filter edge below which fp64 may land on either side
DESC_RTOL = 2.0 ** -20   # |gpu - ref| <= DESC_RTOL * max |four corner rows| per point

NCLT, ROBOTCAR, KITTI = "nclt", "robotcar", "kitti"
X_BODY_LB3_T = (0.035, 0.002, -1.23)          # NCLT dataset SDK: body -> Ladybug
X_BODY_LB3_RPY_DEG = (-179.93, -0.23, 0.50)


# ------------------------------------------------------------------------------------------------- cameras
def nclt_extrinsic(x_lb3) -> np.ndarray:
    """T_c_body = inv(x_lb3_c) @ inv(x_body_lb3), formed in fp64 as the NCLT dataset class forms it."""
    from scipy.spatial.transform import Rotation
    x_body = np.eye(4)
    x_body[:3, 3] = X_BODY_LB3_T
    x_body[:3, :3] = Rotation.from_euler("xyz", X_BODY_LB3_RPY_DEG, degrees=True).as_matrix()
    return np.linalg.inv(np.asarray(x_lb3, dtype=np.float64)) @ np.linalg.inv(x_body)


def nclt_camera(T_c_body, K, coords, subsample, raw=None):
    """``raw``: the camera image as read (turned clockwise); the projection sees it turned back (rot90 CCW)."""
    return dict(mode=NCLT, T=np.asarray(T_c_body, np.float64), K=np.asarray(K, np.float64),
                win=np.asarray(coords, dtype=np.int64) // int(subsample), s=float(subsample), raw=raw)


def robotcar_camera(lidar_in_ego, cam_in_ego, G, fc, subsample, raw=None):
    return dict(mode=ROBOTCAR, L=np.asarray(lidar_in_ego, np.float64), M=np.asarray(cam_in_ego, np.float64),
                G=np.asarray(G, np.float64), fc=[float(x) for x in fc], s=float(subsample), raw=raw)


def kitti_camera(P2, Tr, subsample, raw=None):
    return dict(mode=KITTI, P2=np.asarray(P2, np.float64), Tr=np.asarray(Tr, np.float64), s=float(subsample), raw=raw)


def projection_image(cam):
    """the image project_pcl_to_image receives: NCLT's is the raw image turned 90 degrees counter-clockwise"""
    return np.rot90(cam["raw"], 1) if cam["mode"] == NCLT else cam["raw"]


# ------------------------------------------------------------------------------------------------- long double algebra
def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def _inv_ld(A):
    """Gauss-Jordan with partial pivoting in long double (numpy's LAPACK has no long double)."""
    A = _ld(A).copy()
    n = A.shape[0]
    X = np.eye(n, dtype=LD)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]], X[[k, p]] = A[[p, k]], X[[p, k]]
        d = A[k, k]
        A[k] /= d
        X[k] /= d
        for r in range(n):
            if r != k and A[r, k] != 0:
                f = A[r, k]
                A[r] -= f * A[k]
                X[r] -= f * X[k]
    return X


def _near_int(x):
    with np.errstate(invalid="ignore"):
        return np.abs(x - np.rint(x)) <= TOL * np.maximum(LD(1), np.abs(x))


def _near_zero(z):
    with np.errstate(invalid="ignore"):
        return np.abs(z) <= TOL


def _trunc_int(x):
    """astype(int) of a finite value; non-finite and far-out values land far outside every image"""
    with np.errstate(invalid="ignore"):
        y = np.where(np.isfinite(x), np.clip(x, LD(-2.0 ** 40), LD(2.0 ** 40)), LD(-2.0 ** 40))
    return np.trunc(y).astype(np.int64)


# ------------------------------------------------------------------------------------------------- projection
@dataclass
class Projection:
    """one camera's project_pcl_to_image over all N points: ``keep`` / ``u`` / ``v`` per point (u = v = 0 where
    dropped); ``alts[i]``: the admissible (keep, u, v) answers of an undecided point i."""
    keep: np.ndarray
    u: np.ndarray
    v: np.ndarray
    decided: np.ndarray
    alts: dict = field(default_factory=dict)

    def indices(self):
        idx = np.flatnonzero(self.keep)
        return idx, self.u[idx], self.v[idx]

    def head(self, n):
        return Projection(self.keep[:n], self.u[:n], self.v[:n], self.decided[:n],
                          {i: a for i, a in self.alts.items() if i < n})


def _projective(cam, p):
    """(front, depth, x, y) of the mode; x, y: the pixel coordinates before truncation"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if cam["mode"] == NCLT:
            pc = _ld(cam["T"])[:3] @ p                              # nclt.py:328
            q = _ld(cam["K"]) @ pc                                  # :331
            z = q[2]
            x = q[0] / z / LD(cam["s"])                             # :334-336
            y = q[1] / z / LD(cam["s"])
            front = z > 0
        elif cam["mode"] == ROBOTCAR:
            e = _ld(cam["L"]) @ p                                   # oxford_robotcar.py:335
            c = _ld(cam["M"]) @ e                                   # :338
            g = _inv_ld(cam["G"]) @ c                               # :341 (solve)
            z = g[2]
            fx, fy, cx, cy = (LD(t) for t in cam["fc"])
            x = (fx * g[0] / z + cx) / LD(cam["s"])                 # :350-353
            y = (fy * g[1] / z + cy) / LD(cam["s"])
            front = z >= 0                                          # :344
        else:
            q = (_ld(cam["P2"]) @ _ld(cam["Tr"])) @ p               # kitti_odometry.py:112-113
            z = q[2]
            x = q[0] / z / LD(cam["s"])                             # :116
            y = q[1] / z / LD(cam["s"])
            front = z > 0                                           # :114
    return front, z, x, y


def _outcome(cam, image, front, x, y):
    """(keep, u, v) of the mode's filters for given depth signs and real pixel coordinates (vectorised)"""
    with np.errstate(invalid="ignore"):
        if cam["mode"] == NCLT:
            r0, c0, h, w = (int(t) for t in cam["win"])
            xi, yi = _trunc_int(x), _trunc_int(y)                   # nclt.py:342-343
            keep = front & (xi >= c0) & (xi < c0 + w) & (yi >= r0) & (yi < r0 + h)   # :344-349
            u, v = xi - c0, yi - r0                                 # :350-351
            k = np.flatnonzero(keep)
            keep[k] = np.any(image[v[k], u[k]] != 0, axis=-1)       # :353-359 black pixels of the projection image
        else:
            H, W = image.shape[0], image.shape[1]
            keep = front & (x >= 0) & (x <= W) & (y >= 0) & (y <= H)   # inclusive bound (oxford_robotcar.py:356-357)
            u, v = _trunc_int(x), _trunc_int(y)
    return keep, np.where(keep, u, 0), np.where(keep, v, 0)


def _reach(cam, image, x, y):
    """pixel coordinates within a pixel of the region the filters test: only there can a truncation flip matter"""
    with np.errstate(invalid="ignore"):
        if cam["mode"] == NCLT:
            r0, c0, h, w = (int(t) for t in cam["win"])
            return (x >= c0 - 1) & (x <= c0 + w + 1) & (y >= r0 - 1) & (y <= r0 + h + 1)
        H, W = image.shape[0], image.shape[1]
        return (x >= -1) & (x <= W + 1) & (y >= -1) & (y <= H + 1)


def _candidates(x):
    """just below, at and just above the integer a coordinate sits on (half a pixel stands for 'just')"""
    k = np.rint(x)
    return [k - LD(0.5), k, k + LD(0.5)]


def project(cam, pcl4xn, image=None) -> Projection:
    """project_pcl_to_image of one camera in long double.  ``pcl4xn``: homogeneous [4, N] (fp64 or fp32 values);
    ``image``: what the projection receives (NCLT: black pixels are filtered there; the others use its shape)."""
    image = projection_image(cam) if image is None else image
    front, z, x, y = _projective(cam, _ld(pcl4xn))
    keep, u, v = _outcome(cam, image, front, x, y)
    und_z = _near_zero(z)
    undecided = und_z | ((_near_int(x) | _near_int(y)) & _reach(cam, image, x, y) & front)
    alts = {}
    for i in np.flatnonzero(undecided):
        fs = [False, True] if und_z[i] else [bool(front[i])]
        xs = _candidates(x[i]) if _near_int(x[i]) else [x[i]]
        ys = _candidates(y[i]) if _near_int(y[i]) else [y[i]]
        F_, X_, Y_ = np.meshgrid(np.array(fs), np.array(xs, dtype=LD), np.array(ys, dtype=LD), indexing="ij")
        kk, uu, vv = _outcome(cam, image, F_.ravel(), X_.ravel(), Y_.ravel())
        alts[int(i)] = frozenset(zip(kk.tolist(), uu.tolist(), vv.tolist())) | {(bool(keep[i]), int(u[i]), int(v[i]))}
    return Projection(keep, u, v, ~undecided, alts)


# ------------------------------------------------------------------------------------------------- first camera wins
@dataclass
class Lift:
    """the lifting decisions over all N points: ``seen`` = winning camera (-1: none) and its pixel ``u``, ``v``;
    ``alts[i]``: the admissible (seen, u, v) of an undecided point; ``projs``: every camera's Projection"""
    projs: list
    seen: np.ndarray
    u: np.ndarray
    v: np.ndarray
    decided: np.ndarray
    alts: dict

    @property
    def n(self):
        return len(self.seen)

    @property
    def filled(self):
        return self.seen >= 0

    def head(self, n):
        """the decisions of the first n points (every point is decided on its own)"""
        return Lift([p.head(n) for p in self.projs], self.seen[:n], self.u[:n], self.v[:n], self.decided[:n],
                    {i: a for i, a in self.alts.items() if i < n})


def lift(cams, pcl) -> Lift:
    """create_descriptors' decisions for ``pcl`` [N, 3+] and ``cams`` in priority (dict) order"""
    pcl = np.asarray(pcl)[:, :3]
    projs = [project(c, np.insert(pcl, 3, values=1, axis=1).T) for c in cams]   # prepare_scenes.py:69
    n = pcl.shape[0]
    seen = np.full(n, -1, dtype=np.int64)
    u = np.zeros(n, dtype=np.int64)
    v = np.zeros(n, dtype=np.int64)
    decided = np.ones(n, dtype=bool)
    resolved = np.zeros(n, dtype=bool)          # an earlier camera decidedly took the point
    for k, pr in enumerate(projs):              # np.unique(return_index=True) keeps the first camera's entry
        decided &= resolved | pr.decided
        resolved |= pr.decided & pr.keep
        take = pr.keep & (seen < 0)
        seen[take], u[take], v[take] = k, pr.u[take], pr.v[take]
    alts = {}
    for i in np.flatnonzero(~decided):
        i = int(i)
        options = set()

        def walk(k):
            if k == len(projs):
                options.add((-1, 0, 0))
                return
            pr = projs[k]
            for keep, uu, vv in pr.alts.get(i, {(bool(pr.keep[i]), int(pr.u[i]), int(pr.v[i]))}):
                if keep:
                    options.add((k, uu, vv))
                else:
                    walk(k + 1)
        walk(0)
        alts[i] = frozenset(options)
    return Lift(projs, seen, u, v, decided, alts)


# ------------------------------------------------------------------------------------------------- bilinear sampling
@functools.lru_cache(maxsize=64)
def interp_matrix(n_in: int, n_out: int, dtype: str = "float32") -> np.ndarray:
    """[n_out, n_in]: torch's upsample_bilinear2d(align_corners=False) weights along one axis, read off F.interpolate
    of an identity (channel i = unit impulse at i; the other axis goes 1 -> 1 with weight exactly 1)."""
    import torch
    import torch.nn.functional as F
    eye = torch.eye(n_in, dtype=getattr(torch, dtype)).reshape(1, n_in, n_in, 1)
    A = F.interpolate(eye, size=(n_out, 1), mode="bilinear", align_corners=False)
    return A[0, :, :, 0].T.contiguous().numpy()


@functools.lru_cache(maxsize=64)
def taps(n_in: int, n_out: int):
    """the (at most two, adjacent) non-zero entries of every row of interp_matrix: (i0, i1, w0, w1), weights in fp64;
    i1 = i0 and w1 = 0 where a row has one"""
    A = interp_matrix(n_in, n_out)
    nz = A != 0
    i0 = np.argmax(nz, axis=1)
    i1 = n_in - 1 - np.argmax(nz[:, ::-1], axis=1)
    assert (nz.sum(1) >= 1).all() and (nz.sum(1) <= 2).all() and ((i1 - i0) <= 1).all()
    r = np.arange(n_out)
    w0 = A[r, i0].astype(np.float64)
    w1 = np.where(i1 != i0, A[r, i1], 0).astype(np.float64)
    return i0, i1, w0, w1


@functools.lru_cache(maxsize=8)
def _rot_index(H: int, W: int) -> np.ndarray:
    """np.rot90(features, k=1) as an index map: flat raw-pixel index of what the turned features hold at [v, u]"""
    return np.rot90(np.arange(H * W, dtype=np.int64).reshape(H, W), k=1)


def sample(cam, grid, u, v, _col_shift: int = 0):
    """descriptor rows (fp64 [k, C]) of camera ``cam`` at projected pixels (u, v), the per-point tolerance scale
    max |four corner rows|, and which rows are zero (black raw pixel, or a pixel outside the feature map)."""
    raw = cam["raw"]
    Hup, Wup = raw.shape[0], raw.shape[1]
    u = np.asarray(u, dtype=np.int64)
    v = np.asarray(v, dtype=np.int64)
    if cam["mode"] == NCLT:                                         # prepare_scenes.py:80-81
        rot = _rot_index(Hup, Wup)
        ok = (v >= 0) & (v < rot.shape[0]) & (u >= 0) & (u < rot.shape[1])
        row, col = np.divmod(rot[np.where(ok, v, 0), np.where(ok, u, 0)], Wup)
        row = np.where(ok, row, -1)
    else:
        row, col = v, u
    col = col + _col_shift
    inside = (row >= 0) & (row < Hup) & (col >= 0) & (col < Wup)   # u == W / v == H: zero row (documented deviation)
    row, col = np.where(inside, row, 0), np.where(inside, col, 0)
    zero = ~inside | ~np.any(raw[row, col] != 0, axis=-1)           # prepare_scenes.py:57-62
    G = np.asarray(grid, dtype=np.float32)
    gh, gw, _ = G.shape
    h0, h1, a0, a1 = (t[row] for t in taps(gh, Hup))
    w0, w1, b0, b1 = (t[col] for t in taps(gw, Wup))
    G64 = G.astype(np.float64)
    out = ((a0 * b0)[:, None] * G64[h0, w0] + (a0 * b1)[:, None] * G64[h0, w1]
           + (a1 * b0)[:, None] * G64[h1, w0] + (a1 * b1)[:, None] * G64[h1, w1])
    amax = np.abs(G64).max(axis=2)
    scale = np.maximum.reduce([amax[h0, w0], amax[h0, w1], amax[h1, w0], amax[h1, w1]])
    out[zero] = 0.0
    return out, scale, zero


def rows(cams, grids, seen, u, v, _col_shift: int = 0):
    """expected descriptor rows and scales for (winning camera, pixel) triples; seen == -1 gives a zero row"""
    seen, u, v = (np.asarray(t, dtype=np.int64) for t in (seen, u, v))
    C = np.asarray(grids[0]).shape[2]
    out = np.zeros((len(seen), C), dtype=np.float64)
    scale = np.zeros(len(seen), dtype=np.float64)
    for k, cam in enumerate(cams):
        s = np.flatnonzero(seen == k)
        if len(s):
            out[s], scale[s], _ = sample(cam, grids[k], u[s], v[s], _col_shift if cam["mode"] == NCLT else 0)
    return out, scale


def render(L: Lift, cams, grids, _col_shift: int = 0):
    """the reference's own output as the product returns it: (desc float32 [N, C], filled uint8 [N])"""
    d, _ = rows(cams, grids, L.seen, L.u, L.v, _col_shift)
    return d.astype(np.float32), L.filled.astype(np.uint8)


# ------------------------------------------------------------------------------------------------- comparison
def _rows_ok(got, exp, scale):
    """per row: exactly zero where the reference row is empty, else within DESC_RTOL * scale"""
    empty = ~np.any(exp != 0, axis=1)
    with np.errstate(invalid="ignore"):
        close = np.all(np.abs(got.astype(np.float64) - exp) <= DESC_RTOL * scale[:, None], axis=1)
    return np.where(empty, ~np.any(got != 0, axis=1), close)


def check_lift(L: Lift, cams, grids, desc, filled, chunk: int = 4096):
    """assert that (desc, filled) of the product are the reference's lifting: exact ``filled`` and rows within
    DESC_RTOL on decided points, one of the admissible answers on undecided ones."""
    desc = np.asarray(desc)
    filled = np.asarray(filled).astype(bool)
    n = L.n
    assert desc.shape[0] == n and filled.shape == (n,), (desc.shape, filled.shape, n)
    bad = np.flatnonzero(L.decided & (filled != L.filled))
    assert len(bad) == 0, f"filled differs from the reference at {len(bad)} decided points, e.g. {bad[:8].tolist()}"
    for s0 in range(0, n, chunk):
        sel = np.arange(s0, min(n, s0 + chunk))
        sel = sel[L.decided[sel]]
        exp, scale = rows(cams, grids, L.seen[sel], L.u[sel], L.v[sel])
        ok = _rows_ok(desc[sel], exp, scale)
        if not ok.all():
            j = int(np.flatnonzero(~ok)[0])
            i = int(sel[j])
            err = np.abs(desc[i].astype(np.float64) - exp[j]).max()
            raise AssertionError(f"descriptor of decided point {i} (camera {L.seen[i]}, pixel {L.u[i]}, {L.v[i]}) differs "
                                 f"from the reference: max err {err:.3g}, allowed {DESC_RTOL * scale[j]:.3g} "
                                 f"({int((~ok).sum())} rows of this chunk)")
    for i, options in L.alts.items():
        matches = False
        for s, uu, vv in options:
            if filled[i] != (s >= 0):
                continue
            exp, scale = rows(cams, grids, [s], [uu], [vv])
            if _rows_ok(desc[i:i + 1], exp, scale)[0]:
                matches = True
                break
        assert matches, f"undecided point {i}: the answer is none of the admissible {sorted(options)}"


def check_projection(P: Projection, idx, u, v, name=""):
    """a product projection (surviving indices, u, v) against one camera's reference projection"""
    idx, u, v = (np.asarray(t, dtype=np.int64) for t in (idx, u, v))
    n = len(P.keep)
    assert np.all(np.diff(idx) > 0), f"{name}: surviving indices are not ascending"
    got = np.zeros(n, dtype=bool)
    gu = np.zeros(n, dtype=np.int64)
    gv = np.zeros(n, dtype=np.int64)
    got[idx], gu[idx], gv[idx] = True, u, v
    bad = np.flatnonzero(P.decided & ((got != P.keep) | (gu != P.u) | (gv != P.v)))
    if len(bad):
        b = int(bad[0])
        raise AssertionError(f"{name}: projection differs from the reference at {len(bad)} decided points, e.g. point {b}: "
                             f"{(bool(got[b]), int(gu[b]), int(gv[b]))} vs {(bool(P.keep[b]), int(P.u[b]), int(P.v[b]))}")
    for i, options in P.alts.items():
        a = (bool(got[i]), int(gu[i]), int(gv[i]))
        assert a in options, f"{name}: undecided point {i}: {a} is none of {sorted(options)}"


# ------------------------------------------------------------------------------------------------- planting points
def from_projective(cam, q) -> np.ndarray:
    """world points [k, 3] (fp64) with projective coordinates ``q`` [k, 3], solved in long double: NCLT / KITTI
    (q0, q1, q2) with pixel = q0 / q2 / s; RobotCar the image-frame point (g0, g1, g2) before the focal lengths"""
    q = _ld(q).T
    one = np.ones((1, q.shape[1]), dtype=LD)
    if cam["mode"] == NCLT:
        p = _inv_ld(cam["T"]) @ np.vstack([_inv_ld(cam["K"]) @ q, one])
    elif cam["mode"] == ROBOTCAR:
        p = _inv_ld(cam["L"]) @ (_inv_ld(cam["M"]) @ (_ld(cam["G"]) @ np.vstack([q, one])))
    else:
        P = _ld(cam["P2"]) @ _ld(cam["Tr"])
        p = _inv_ld(P[:, :3]) @ (q - P[:, 3:4])
    return np.asarray(p[:3].T, dtype=np.float64)


def backproject(cam, x, y, depth) -> np.ndarray:
    """world points whose pixel coordinates (before truncation) are (x, y) at camera depth ``depth``"""
    x, y, depth = np.broadcast_arrays(*(np.atleast_1d(_ld(t)) for t in (x, y, depth)))
    s = LD(cam["s"])
    if cam["mode"] == ROBOTCAR:
        fx, fy, cx, cy = (LD(t) for t in cam["fc"])
        q = np.stack([(x * s - cx) / fx * depth, (y * s - cy) / fy * depth, depth], 1)
    else:
        q = np.stack([x * s * depth, y * s * depth, depth], 1)
    return from_projective(cam, q)

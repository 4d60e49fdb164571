"""Synthetic scan/map pairs of SURVEY.md section 8 D.2 (the benchmark's and the tests' inputs).

map : M points, xyz ~ U([-60,60]^2 x [-3,12]) fp32, descriptors randn(M, D) row-normalised.
scan: N points = random subset of the map moved into the scan frame by T_gt^-1 plus N(0, 0.02 m)
      noise; descriptor = matched map descriptor + sigma * randn, renormalised (inlier cosine
      ~ 0.9); a fraction rho of the rows is replaced by fresh random unit vectors (cosine ~ 0,
      rejected by the 0.8 threshold of registration_node.py:418).
T_gt: yaw ~ U(+-180 deg), roll/pitch ~ N(0, 2 deg), t_xy ~ N(0, 10 m), t_z ~ N(0, 1 m)
      (mirrors registration_node.py:847-853).  Pair p uses seed 42 + p.
"""
from __future__ import annotations

import math

import numpy as np


def random_pose(rng: np.random.Generator) -> np.ndarray:
    yaw = rng.uniform(-math.pi, math.pi)
    roll, pitch = np.deg2rad(rng.normal(0.0, 2.0, 2))
    cr, sr, cp, sp, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = [rng.normal(0, 10), rng.normal(0, 10), rng.normal(0, 1)]
    return T


def make_pair(n: int, m: int, d: int = 384, seed: int = 42, outlier: float = 0.5, inlier_cos: float = 0.9,
              noise_m: float = 0.02):
    """numpy generator (CPU). Returns dict(q_desc [n,d] f32, q_xyz [n,3] f64, b_desc [m,d] f32,
    b_xyz [m,3] f64, T_gt [4,4], match [n] int64 (-1 for outlier rows))."""
    rng = np.random.default_rng(seed)
    b_xyz = np.c_[rng.uniform(-60, 60, m), rng.uniform(-60, 60, m), rng.uniform(-3, 12, m)].astype(np.float32)
    b_desc = rng.standard_normal((m, d), dtype=np.float32)
    b_desc /= np.linalg.norm(b_desc, axis=1, keepdims=True)
    T = random_pose(rng)
    pick = rng.choice(m, size=n, replace=(n > m))
    R, t = T[:3, :3], T[:3, 3]
    q_xyz = (b_xyz[pick].astype(np.float64) - t) @ R  # R^T (p - t)
    q_xyz = q_xyz + rng.normal(0, noise_m, q_xyz.shape)
    sigma = math.sqrt((1.0 / inlier_cos ** 2 - 1.0) / d)
    q_desc = b_desc[pick] + sigma * rng.standard_normal((n, d), dtype=np.float32)
    is_out = rng.random(n) < outlier
    q_desc[is_out] = rng.standard_normal((int(is_out.sum()), d), dtype=np.float32)
    q_desc /= np.linalg.norm(q_desc, axis=1, keepdims=True)
    match = np.where(is_out, -1, pick).astype(np.int64)
    return dict(q_desc=np.ascontiguousarray(q_desc, dtype=np.float32), q_xyz=np.ascontiguousarray(q_xyz),
                b_desc=np.ascontiguousarray(b_desc, dtype=np.float32),
                b_xyz=np.ascontiguousarray(b_xyz.astype(np.float64)), T_gt=T, match=match)


def make_pair_device(n: int, m: int, d: int = 384, seed: int = 42, device="cuda", outlier: float = 0.5,
                     inlier_cos: float = 0.9, noise_m: float = 0.02):
    """Same distribution generated on the device with torch (the 20k x 200k x 384 benchmark pair is
    230 M floats; the host is not the bottleneck).  Returns torch tensors + T_gt (numpy)."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    rng = np.random.default_rng(seed)
    T = random_pose(rng)
    b_xyz = torch.rand((m, 3), generator=g, device=device, dtype=torch.float32)
    b_xyz = b_xyz * torch.tensor([120.0, 120.0, 15.0], device=device) + torch.tensor([-60.0, -60.0, -3.0], device=device)
    b_desc = torch.randn((m, d), generator=g, device=device, dtype=torch.float32)
    b_desc /= b_desc.norm(dim=1, keepdim=True)
    pick = torch.randint(0, m, (n,), generator=g, device=device) if n > m else torch.randperm(m, generator=g, device=device)[:n]
    Tt = torch.tensor(T, device=device, dtype=torch.float64)
    q_xyz = (b_xyz[pick].double() - Tt[:3, 3]) @ Tt[:3, :3]
    q_xyz = q_xyz + noise_m * torch.randn(q_xyz.shape, generator=g, device=device, dtype=torch.float64)
    sigma = math.sqrt((1.0 / inlier_cos ** 2 - 1.0) / d)
    q_desc = b_desc[pick] + sigma * torch.randn((n, d), generator=g, device=device, dtype=torch.float32)
    is_out = torch.rand(n, generator=g, device=device) < outlier
    fresh = torch.randn((n, d), generator=g, device=device, dtype=torch.float32)
    q_desc = torch.where(is_out[:, None], fresh, q_desc)
    q_desc /= q_desc.norm(dim=1, keepdim=True)
    match = torch.where(is_out, torch.full_like(pick, -1), pick)
    return dict(q_desc=q_desc.contiguous(), q_xyz=q_xyz.contiguous(), b_desc=b_desc.contiguous(),
                b_xyz=b_xyz.double().contiguous(), T_gt=T, match=match)


def lifted_map(m: int, d: int, clouds: int, cams: int, gh: int, gw: int, seed: int, view_noise: float, device="cuda",
               revisit: int = 0):
    """Map descriptors that look like LIFTED ones (prepare_scenes.py:50-107 + image_features.py:104-108): row r belongs to
    (cloud, camera) image k and is the bilinear sample of that image's gh x gw patch grid at a random position.  Images of
    different clouds that look at the same place share a smooth scene field: grid(k) = scene_grid(camera) + view_noise *
    randn.  ``revisit`` > 0: the same physical points are seen again by every cloud (that many pixel positions per camera)."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    scene = torch.randn((cams, gh, gw, d), generator=g, device=device)
    K = clouds * cams
    img = torch.randint(0, K, (m,), generator=g, device=device)
    cam = img % cams
    noise_seed = torch.randn((K, gh, gw, d), generator=g, device=device) * view_noise
    if revisit:
        py = torch.rand((cams, revisit), generator=g, device=device) * (gh - 1 - 1e-3)
        px = torch.rand((cams, revisit), generator=g, device=device) * (gw - 1 - 1e-3)
        which = torch.randint(0, revisit, (m,), generator=g, device=device)
        y, x = py[cam, which], px[cam, which]
    else:
        y = torch.rand(m, generator=g, device=device) * (gh - 1 - 1e-3)
        x = torch.rand(m, generator=g, device=device) * (gw - 1 - 1e-3)
    i, j = y.long(), x.long()
    fy, fx = (y - i)[:, None], (x - j)[:, None]

    def at(ii, jj):
        return scene[cam, ii, jj] + noise_seed[img, ii, jj]
    out = at(i, j) * (1 - fy) * (1 - fx) + at(i + 1, j) * fy * (1 - fx) + at(i, j + 1) * (1 - fy) * fx + at(i + 1, j + 1) * fy * fx
    return out.float().contiguous()


def make_lifted_pair_device(n: int, m: int, d: int = 384, seed: int = 42, device="cuda", clouds: int = 10,
                            view_noise: float = 0.1, common: float = 0.0, revisit: int = 0):
    """A D.2 pair (same geometry, same planted matches, same outlier rows) whose MAP descriptors are lifted ones
    (``lifted_map``) and whose scan descriptors are the matched map rows + 0.3 rms noise.  ``common`` > 0 adds one shared
    vector of that many rms to every row (scan and map): descriptors that are all alike, as a ViT's patch tokens are."""
    import torch
    base = make_pair_device(n, m, d, seed=seed, device=device)
    b = lifted_map(m, d, clouds, 6, 16, 21, seed + 7, view_noise, device, revisit)
    g = torch.Generator(device=device)
    g.manual_seed(seed + 1)
    rms = b.pow(2).mean().sqrt()
    pick = base["match"].clamp(min=0)
    q = b[pick] + 0.3 * rms * torch.randn((n, d), generator=g, device=device)
    q = torch.where((base["match"] < 0)[:, None], rms * torch.randn((n, d), generator=g, device=device), q)
    if common > 0:
        mu = common * rms * torch.randn((1, d), generator=g, device=device)
        b, q = b + mu, q + mu
    base["b_desc"], base["q_desc"] = b.contiguous(), q.contiguous()
    return base


_VIT_GRIDS = {}


def _vit_grids(seed: int, device):
    """(images, patch grids) of the repository's ViT-S/14 with random weights on 6 seeded 1200 x 1600 camera images (kept: the
    forward is the same for every pair of a seed)"""
    key = (int(seed), str(device))
    if key not in _VIT_GRIDS:
        import torch
        from . import vit as V
        rng = np.random.default_rng(seed)
        imgs = torch.from_numpy(rng.integers(1, 255, (6, 1200, 1600, 3), dtype=np.uint8)).to(device)
        model = V.ViTS14(V.random_weights(seed), 1200, 1600, device=device)
        _VIT_GRIDS.clear()
        _VIT_GRIDS[key] = (imgs, model.forward(imgs))
    return _VIT_GRIDS[key]


def lift_vit_features(points: int, seed: int = 0, device="cuda", vit_seed: int = 0):
    """``points`` rows of the ViT's own features lifted (ops.LiftPlan, prepare_scenes.py:85-104) from a 6-camera rig (90 x 74 deg
    each, 60 deg apart) onto points 6 - 45 m around it: every returned row was seen by a camera (non-zero)."""
    import torch
    from . import ops
    imgs, grids = _vit_grids(vit_seed, device)
    H, W = imgs.shape[1], imgs.shape[2]
    K = np.array([[800.0, 0, 800], [0, 800, 600], [0, 0, 1]])
    cams = []
    for c in range(6):
        y = np.deg2rad(60 * c)
        R = np.stack([[np.sin(y), -np.cos(y), 0], [0, 0, -1], [np.cos(y), np.sin(y), 0]])
        cams.append(dict(mode=ops.PROJ_KITTI, mats=[K @ np.c_[R, np.zeros(3)]], fc=None, subsample=1.0, win=None, H=H, W=W,
                         proj_image=None, grid=grids[c], Hup=H, Wup=W, rot_mode=0, raw_image=imgs[c]))
    plan = ops.LiftPlan(cams, grids.shape[-1])
    rng = np.random.default_rng(seed + 1)
    total = points + points // 4 + 64            # (the few points no camera sees are dropped)
    r, az = rng.uniform(6.0, 45.0, total), rng.uniform(-np.pi, np.pi, total)
    xyz = np.c_[r * np.cos(az), r * np.sin(az), rng.uniform(-2.0, 3.0, total)]
    pcl = torch.from_numpy(np.ascontiguousarray(np.insert(xyz, 3, 1, axis=1).T)).to(device)
    desc = torch.zeros((total, grids.shape[-1]), dtype=torch.float32, device=device)
    filled = torch.zeros(total, dtype=torch.uint8, device=device)
    plan(pcl, desc, filled)
    seen = torch.nonzero((filled != 0) & (desc != 0).any(dim=1)).flatten()
    if len(seen) < points:
        raise RuntimeError(f"lift_vit_features: {len(seen)} of {total} points seen, {points} wanted")
    return desc[seen[:points]].contiguous()


def make_all_lifted_pair_device(n: int, m: int, d: int = 384, seed: int = 42, device="cuda", views: int = 10, view_noise: float = 0.05,
                                scan_noise: float = 0.05, zero_rows: float = 0.0, outlier: float = 0.5):
    """A D.2 pair (``make_pair_device``'s geometry: b_xyz, q_xyz, match, T_gt) whose descriptors are ALL lifted ViT features, as the
    reference's maps are (registration_node.py:562 keeps only rows with a descriptor; prepare_scenes.py:85-104 lifts every one of them
    from the same ViT): ``lift_vit_features`` on ceil(m / views) points; every map row is one of those rows + ``view_noise`` rms of
    noise per view (``views`` near-duplicates per point, spread over the map); a matched scan row is its planted map row +
    ``scan_noise`` rms; an outlier scan row is the lifted row of a point the map does not hold (+ the same noise).  A ``zero_rows``
    fraction of the scan rows carries the all-zero descriptor of a point no camera saw (their ``match`` is -1); map rows never do.
    The rows share the large common component of the ViT's patch tokens: |mean of the normalised rows| ~ 0.7.  One ViT (random weights
    and images of seed 0) serves every pair; the ViT is only a data source -- tests compare against the oracle on the rows it gives."""
    import torch
    if d != 384:
        raise ValueError("the ViT-S/14 features are 384 wide")
    base = make_pair_device(n, m, d, seed=seed, device=device, outlier=outlier)
    pts = -(-m // views)
    n_out = max(1, min(n, pts))
    lifted = lift_vit_features(pts + n_out, seed=seed, device=device)
    g = torch.Generator(device=device)
    g.manual_seed(seed + 5)
    rms = lifted.pow(2).mean().sqrt()
    point = torch.randperm(m, generator=g, device=device) % pts
    b = lifted[point] + view_noise * rms * torch.randn((m, d), generator=g, device=device)
    match = base["match"]
    q = b[match.clamp(min=0)] + scan_noise * rms * torch.randn((n, d), generator=g, device=device)
    other = lifted[pts + torch.randint(0, n_out, (n,), generator=g, device=device)]
    other = other + scan_noise * rms * torch.randn((n, d), generator=g, device=device)
    q = torch.where((match < 0)[:, None], other, q)
    if zero_rows > 0:
        z = torch.rand(n, generator=g, device=device) < zero_rows
        q[z] = 0.0
        base["match"] = torch.where(z, torch.full_like(match, -1), match)
    base["b_desc"], base["q_desc"] = b.contiguous(), q.contiguous()
    return base


def make_structured_scene(n_scan: int = 20000, n_map: int = 200000, seed: int = 0, extent: float = 30.0, scan_range: float = 15.0,
                          boxes: int = 24, cylinders: int = 16, noise_m: float = 0.01, yaw_deg: float = 30.0, shift_m: float = 2.0):
    """A seeded scene with surfaces (the FPFH baseline needs real normals; Gaussian blobs have none): a ground plane over
    [-extent, extent]^2, axis-aligned boxes (four walls and a roof) and vertical cylinders (mantle and top), sampled uniformly by area.
    The map samples the whole scene; the scan is an independent sample of the surfaces within ``scan_range`` (in x / y) of the origin,
    moved into the scan frame: map = T_gt (scan) + noise.  Both get N(0, noise_m) noise.  T_gt: yaw ~ U(+-yaw_deg), roll / pitch
    ~ N(0, 1 deg), t ~ U(+-shift_m) in x / y, N(0, 0.1 m) in z.  Returns dict(scan [n_scan, 3] f64, map [n_map, 3] f64, T_gt)."""
    rng = np.random.default_rng(seed)
    surf = []   # (kind, params, area)
    surf.append(("plane", (-extent, extent, -extent, extent), (2 * extent) ** 2))
    for _ in range(boxes):
        cx, cy = rng.uniform(-extent + 3, extent - 3, 2)
        sx, sy = rng.uniform(0.8, 4.0, 2)
        h = rng.uniform(1.0, 5.0)
        surf.append(("box", (cx, cy, sx, sy, h), 2 * h * (sx + sy) + sx * sy))
    for _ in range(cylinders):
        cx, cy = rng.uniform(-extent + 2, extent - 2, 2)
        r = rng.uniform(0.2, 1.2)
        h = rng.uniform(1.5, 6.0)
        surf.append(("cyl", (cx, cy, r, h), 2 * math.pi * r * h + math.pi * r * r))

    def sample(count, region):
        out = []
        area = np.array([s[2] for s in surf])
        got = 0
        while got < count:
            want = int((count - got) * 1.3) + 64
            k = rng.choice(len(surf), size=want, p=area / area.sum())
            pts = np.empty((want, 3))
            for si in np.unique(k):
                sel = np.flatnonzero(k == si)
                kind, prm, _ = surf[si]
                u, v, w = rng.random(len(sel)), rng.random(len(sel)), rng.random(len(sel))
                if kind == "plane":
                    x0, x1, y0, y1 = prm
                    pts[sel] = np.c_[x0 + u * (x1 - x0), y0 + v * (y1 - y0), np.zeros(len(sel))]
                elif kind == "box":
                    cx, cy, sx, sy, h = prm
                    face_area = np.array([sx * h, sx * h, sy * h, sy * h, sx * sy])
                    f = rng.choice(5, size=len(sel), p=face_area / face_area.sum())
                    x = cx + (u - 0.5) * sx
                    y = cy + (v - 0.5) * sy
                    z = w * h
                    x = np.where(f == 2, cx - sx / 2, np.where(f == 3, cx + sx / 2, x))
                    y = np.where(f == 0, cy - sy / 2, np.where(f == 1, cy + sy / 2, y))
                    z = np.where(f == 4, h, z)
                    pts[sel] = np.c_[x, y, z]
                else:
                    cx, cy, r, h = prm
                    top = rng.random(len(sel)) < (math.pi * r * r) / (2 * math.pi * r * h + math.pi * r * r)
                    th = 2 * math.pi * u
                    rr = np.where(top, r * np.sqrt(v), r)
                    pts[sel] = np.c_[cx + rr * np.cos(th), cy + rr * np.sin(th), np.where(top, h, w * h)]
            if region is not None:
                pts = pts[(np.abs(pts[:, 0]) <= region) & (np.abs(pts[:, 1]) <= region)]
            out.append(pts)
            got += len(pts)
        pts = np.concatenate(out)[:count]
        return pts + rng.normal(0.0, noise_m, pts.shape)

    world_map = sample(n_map, None)
    world_scan = sample(n_scan, scan_range)
    yaw = math.radians(rng.uniform(-yaw_deg, yaw_deg))
    roll, pitch = np.deg2rad(rng.normal(0.0, 1.0, 2))
    cr, sr, cp, sp, cy_, sy_ = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    R = np.array([[cy_, -sy_, 0], [sy_, cy_, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]]) @ \
        np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = [rng.uniform(-shift_m, shift_m), rng.uniform(-shift_m, shift_m), rng.normal(0.0, 0.1)]
    scan = (world_scan - T[:3, 3]) @ R   # R^T (p - t)
    return dict(scan=np.ascontiguousarray(scan), map=np.ascontiguousarray(world_map), T_gt=T)

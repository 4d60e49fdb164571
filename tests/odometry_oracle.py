"""CPU oracle of the odometry front end (vfmreg.preprocess / deskew / threshold / mapping.VoxelHashMap.update / kiss_icp), restated in
numpy and composed from ``oracle.oracle`` (``voxel_down_sample``, ``register_frame``, ``transform_pcl``).

  range_crop              Preprocess (Preprocessing.cpp:139-197): min_range < sqrt((x x + y y) + z z) < max_range, both strict
  se3_log                 Sophus SE3::log: the rotation vector through the quaternion, V^-1 with its small-angle branch
  deskew / deskew_ld      DeSkewScan (Deskew.cpp:40-68) with oracle.se3_exp's formulas, in fp64 / in np.longdouble
  deskew_bound            B_i of the de-skew test: eps (|p_i| + |tau_i| + c)
  AdaptiveThreshold       Threshold.cpp:29-50; ``get_threshold`` adds a sample at every call
  VoxelMap                a dict of voxels with the stated update rule: cap with old points first, then EVERY voxel whose first point is
                          far goes; ``grid()`` is the sorted-key CSR (keys, start, pts) in (voxel key, insertion) order
  KissICP                 kiss_icp.py:35-138 on top of these
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

EPS = float(np.finfo(np.float64).eps)


def load_config(max_range=100.0, deskew=False, fixed_threshold=None):
    """the constants of vfmreg.config.load_config, restated"""
    max_range = float(max_range)
    return SimpleNamespace(
        data=SimpleNamespace(max_range=max_range, min_range=5.0, deskew=bool(deskew), preprocess=True),
        mapping=SimpleNamespace(voxel_size=float(max_range / 100.0), max_points_per_voxel=20),
        adaptive_threshold=SimpleNamespace(fixed_threshold=fixed_threshold, initial_threshold=2.0, min_motion_th=0.1))


# ------------------------------------------------------------------------------------------------------------------ crop
def range_norm(xyz: np.ndarray) -> np.ndarray:
    x, y, z = (np.asarray(xyz[:, k], dtype=np.float64) for k in range(3))
    return np.sqrt((x * x + y * y) + z * z)


def range_crop(points: np.ndarray, min_range: float, max_range: float) -> np.ndarray:
    """ascending indices of the rows Preprocess keeps"""
    points = np.asarray(points)
    if len(points) == 0:
        return np.zeros(0, dtype=np.int64)
    norm = range_norm(points)
    return np.flatnonzero((norm < max_range) & (norm > min_range)).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ SE(3)
def hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.asarray(w).dtype)


def se3_exp(dx: np.ndarray, dtype=np.float64) -> np.ndarray:
    """oracle.se3_exp's formulas (Sophus::SE3::exp, first-order branch below theta = 1e-10) in ``dtype``"""
    dx = np.asarray(dx, dtype=dtype)
    ups, om = dx[:3], dx[3:]
    th = np.sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2])
    Om = hat(om)
    eye = np.eye(3, dtype=dtype)
    if th < 1e-10:
        R = eye + Om
        V = eye + dtype(0.5) * Om
    else:
        O2 = Om @ Om
        R = eye + np.sin(th) / th * Om + (1 - np.cos(th)) / (th * th) * O2
        V = eye + (1 - np.cos(th)) / (th * th) * Om + (th - np.sin(th)) / (th * th * th) * O2
    T = np.eye(4, dtype=dtype)
    T[:3, :3] = R
    T[:3, 3] = V @ ups
    return T


def quaternion_of(Rm: np.ndarray):
    """Eigen's matrix -> quaternion (w, vec): the trace branch, else the branch of the largest diagonal element"""
    Rm = np.asarray(Rm, dtype=np.float64)
    t = Rm[0, 0] + Rm[1, 1] + Rm[2, 2]
    q = np.zeros(3)
    if t > 0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        q[0] = (Rm[2, 1] - Rm[1, 2]) * t
        q[1] = (Rm[0, 2] - Rm[2, 0]) * t
        q[2] = (Rm[1, 0] - Rm[0, 1]) * t
    else:
        i = 0
        if Rm[1, 1] > Rm[0, 0]:
            i = 1
        if Rm[2, 2] > Rm[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(Rm[i, i] - Rm[j, j] - Rm[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        w = (Rm[k, j] - Rm[j, k]) * t
        q[j] = (Rm[j, i] + Rm[i, j]) * t
        q[k] = (Rm[k, i] + Rm[i, k]) * t
    return float(w), q


def rotation_angle(Rm: np.ndarray) -> float:
    """Eigen::AngleAxisd(R).angle(): 2 atan2(|vec|, |w|)"""
    w, q = quaternion_of(Rm)
    n = float(np.sqrt(q @ q))
    return 2.0 * float(np.arctan2(n, abs(w))) if n != 0.0 else 0.0


def se3_log(T: np.ndarray) -> np.ndarray:
    """Sophus SE3::log of a 4 x 4 pose: [upsilon, omega]"""
    T = np.asarray(T, dtype=np.float64)
    w, q = quaternion_of(T[:3, :3])
    sq = float(q @ q)
    if sq < 1e-10 * 1e-10:
        two_atan = 2.0 / w - (2.0 / 3.0) * sq / (w * w * w)
    else:
        n = np.sqrt(sq)
        atan = np.arctan2(-n, -w) if w < 0 else np.arctan2(n, w)
        two_atan = 2.0 * atan / n
    om = two_atan * q
    theta = float(np.sqrt(om @ om))
    Om = hat(om)
    if abs(theta) < 1e-10:
        Vinv = np.eye(3) - 0.5 * Om + (1.0 / 12.0) * (Om @ Om)
    else:
        half = 0.5 * theta
        Vinv = np.eye(3) - 0.5 * Om + (1.0 - theta * np.cos(half) / (2.0 * np.sin(half))) / (theta * theta) * (Om @ Om)
    return np.r_[Vinv @ T[:3, 3], om]


# ------------------------------------------------------------------------------------------------------------------ de-skew
def _deskew(xyz, stamps, delta, dtype):
    xyz = np.asarray(xyz, dtype=dtype)
    delta = np.asarray(delta, dtype=dtype)
    out = np.empty((len(xyz), 3), dtype=dtype)
    tau = np.empty((len(xyz), 3), dtype=dtype)
    for i in range(len(xyz)):
        M = se3_exp((dtype(stamps[i]) - dtype(0.5)) * delta, dtype)
        out[i] = M[:3, :3] @ xyz[i] + M[:3, 3]
        tau[i] = M[:3, 3]
    return out, tau


def deskew(xyz, stamps, delta) -> np.ndarray:
    return _deskew(np.asarray(xyz)[:, :3], stamps, delta, np.float64)[0]


def deskew_ld(xyz, stamps, delta):
    """(points, the motions' translations) in np.longdouble"""
    return _deskew(np.asarray(xyz)[:, :3], stamps, delta, np.longdouble)


def deskew_bound(xyz, stamps, delta, tau) -> np.ndarray:
    """B_i = eps (|p_i| + |tau_i| + c), c = |upsilon| / |omega| where the scaled angle is >= 1e-10, else 0: the conditioning of Sophus'
    own (1 - cos theta) / theta^2 and (theta - sin theta) / theta^3 terms"""
    xyz = np.asarray(xyz, dtype=np.float64)[:, :3]
    delta = np.asarray(delta, dtype=np.float64)
    s = np.abs(np.asarray(stamps, dtype=np.float64) - 0.5)
    nu, nw = np.linalg.norm(delta[:3]), np.linalg.norm(delta[3:])
    c = np.where(s * nw >= 1e-10, nu / nw if nw > 0 else 0.0, 0.0)
    return EPS * (np.linalg.norm(xyz, axis=1) + np.linalg.norm(np.asarray(tau, dtype=np.float64), axis=1) + c)


# ------------------------------------------------------------------------------------------------------------------ threshold
class AdaptiveThreshold:
    def __init__(self, initial_threshold: float, min_motion_th: float, max_range: float):
        self.initial_threshold, self.min_motion_th, self.max_range = float(initial_threshold), float(min_motion_th), float(max_range)
        self.model_error_sse2 = 0.0
        self.num_samples = 0
        self.model_deviation = np.eye(4)

    def model_error(self) -> float:
        theta = rotation_angle(self.model_deviation[:3, :3])
        delta_rot = 2.0 * self.max_range * np.sin(theta / 2.0)
        t = self.model_deviation[:3, 3]
        return float(np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) + delta_rot)

    def get_threshold(self) -> float:
        e = self.model_error()
        if e > self.min_motion_th:
            self.model_error_sse2 += e * e
            self.num_samples += 1
        if self.num_samples < 1:
            return self.initial_threshold
        return float(np.sqrt(self.model_error_sse2 / self.num_samples))

    def update_model_deviation(self, model_deviation):
        self.model_deviation = np.array(model_deviation, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------ map
def voxel_keys(xyz: np.ndarray, voxel_size: float) -> np.ndarray:
    v = np.trunc(np.asarray(xyz, dtype=np.float64) / voxel_size).astype(np.int64)
    bad = np.abs(v) >= (1 << 20) - 1
    v = np.where(bad, 0, v) + (1 << 20)
    return (v[:, 0] << 42) | (v[:, 1] << 21) | v[:, 2], bool(bad.any())


class VoxelMap:
    """dict: voxel key -> list of points in insertion order"""

    def __init__(self, voxel_size: float, max_distance: float, max_points_per_voxel: int):
        self.voxel_size, self.max_distance, self.cap = float(voxel_size), float(max_distance), int(max_points_per_voxel)
        self.voxels = {}
        self.status = 0
        self.last = dict(points_added=0, voxels_removed=0, points_removed=0)

    def add_points(self, xyz: np.ndarray) -> int:
        xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64)[:, :3])
        added = 0
        if len(xyz):
            keys, bad = voxel_keys(xyz, self.voxel_size)
            self.status |= int(bad)
            for k, p in zip(keys.tolist(), xyz):
                block = self.voxels.get(k)
                if block is None:
                    self.voxels[k] = [p]
                    added += 1
                elif self.cap <= 0 or len(block) < self.cap:
                    block.append(p)
                    added += 1
        self.last = dict(points_added=added, voxels_removed=0, points_removed=0)
        return added

    def remove_far(self, origin) -> None:
        o = np.asarray(origin, dtype=np.float64)
        md2 = self.max_distance * self.max_distance
        gone = []
        for k, block in self.voxels.items():
            d = block[0] - o
            if ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) > md2:
                gone.append(k)
        self.last["voxels_removed"] = len(gone)
        self.last["points_removed"] = sum(len(self.voxels[k]) for k in gone)
        for k in gone:
            del self.voxels[k]

    def update(self, xyz: np.ndarray, pose=None, origin="pose") -> None:
        """pose None: the points as they are; origin "pose": the pose's translation, None: no removal"""
        from oracle import oracle
        xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64)[:, :3])
        if pose is not None and len(xyz):
            xyz = oracle.transform_pcl(xyz, np.asarray(pose, dtype=np.float64))
        self.add_points(xyz)
        if isinstance(origin, str):
            origin = np.asarray(pose, dtype=np.float64)[:3, 3] if pose is not None else None
        if origin is not None:
            self.remove_far(origin)

    def grid(self):
        keys = np.array(sorted(self.voxels), dtype=np.int64)
        sizes = np.array([len(self.voxels[k]) for k in keys.tolist()], dtype=np.int64)
        start = np.r_[0, np.cumsum(sizes)].astype(np.int32)
        pts = np.array([p for k in keys.tolist() for p in self.voxels[k]], dtype=np.float64).reshape(-1, 3)
        return keys, start, pts

    def points(self) -> np.ndarray:
        return self.grid()[2]

    def info(self):
        keys, start, pts = self.grid()
        return [len(keys), len(pts), self.status, self.last["points_added"], self.last["voxels_removed"], self.last["points_removed"]]

    def empty(self) -> bool:
        return not self.voxels


# ------------------------------------------------------------------------------------------------------------------ pipeline
class KissICP:
    """kiss_icp.py:35-138; ``deskewed``: per frame the de-skewed coordinates to use instead of this oracle's own (the device's, where the
    test feeds them: de-skew is bounded, not bit-equal)"""

    def __init__(self, config, map_update_threshold=0.0):
        self.config = config
        self.poses = []
        at = config.adaptive_threshold
        self.adaptive_threshold = None if at.fixed_threshold is not None else AdaptiveThreshold(at.initial_threshold, at.min_motion_th,
                                                                                                config.data.max_range)
        self.local_map = VoxelMap(config.mapping.voxel_size, config.data.max_range, config.mapping.max_points_per_voxel)
        self.map_update_threshold = map_update_threshold
        self.thresholds = []
        self.stats = []

    def get_adaptive_threshold(self):
        if not self.has_moved():
            return self.config.adaptive_threshold.initial_threshold
        if self.adaptive_threshold is None:
            return self.config.adaptive_threshold.fixed_threshold
        return self.adaptive_threshold.get_threshold()

    def get_prediction_model(self):
        if len(self.poses) < 2:
            return np.eye(4)
        return np.linalg.inv(self.poses[-2]) @ self.poses[-1]

    def has_moved(self):
        if len(self.poses) < 1:
            return False
        motion = np.linalg.norm((np.linalg.inv(self.poses[0]) @ self.poses[-1])[:3, -1])
        return motion > 5 * self.config.adaptive_threshold.min_motion_th

    def register_frame(self, frame, timestamps, deskewed=None):
        from oracle import oracle
        frame = np.asarray(frame, dtype=np.float64)
        if self.config.data.deskew and len(self.poses) >= 2:
            if deskewed is None:
                delta = se3_log(np.linalg.inv(self.poses[-2]) @ self.poses[-1])
                deskewed = deskew(frame, timestamps, delta)
            frame = np.c_[deskewed, frame[:, 3:]]
        if self.config.data.preprocess:
            frame = frame[range_crop(frame, self.config.data.min_range, self.config.data.max_range)]
        vs = self.config.mapping.voxel_size
        frame_downsample = oracle.voxel_down_sample(frame, vs * 0.5)
        source = oracle.voxel_down_sample(frame_downsample, vs * 1.5)
        sigma = self.get_adaptive_threshold()
        self.thresholds.append(sigma)
        prediction = self.get_prediction_model()
        last_pose = self.poses[-1] if self.poses else np.eye(4)
        initial_guess = last_pose @ prediction
        if self.local_map.empty() or len(source) == 0:
            new_pose = np.ascontiguousarray(initial_guess, dtype=np.float64)
        else:
            new_pose = oracle.register_frame(source[:, :3], self.local_map.points(), vs, initial_guess, 3 * sigma, sigma / 3)
        motion = np.linalg.inv(last_pose) @ new_pose
        if np.linalg.norm(motion[:3, -1]) < self.map_update_threshold and len(self.poses) > 1:
            return new_pose, frame_downsample, False
        if self.adaptive_threshold is not None:
            self.adaptive_threshold.update_model_deviation(np.linalg.inv(initial_guess) @ new_pose)
        self.local_map.update(frame_downsample[:, :3], new_pose)
        self.stats.append(dict(self.local_map.last, offered=len(frame_downsample)))
        self.poses.append(new_pose)
        return new_pose, frame_downsample, True


# ------------------------------------------------------------------------------------------------------------------ the drive
def synthetic_drive(frames: int = 40, points: int = 6000, seed: int = 7, width: int = 3):
    """The seeded drive of the pipeline tests: a 150 x 24 m ground strip, two wavy walls and 120 pillars of 1.4 x 1.4 x 3 m; ``points``
    points per scan within 21 m of the sensor with 0.01 m noise; the sensor advances 0.6 m per frame, 0.9 m from frame 20 on, and yaws
    0.012 rad per frame.  Returns (scans in the sensor frame, ground-truth poses, timestamps)."""
    rng = np.random.default_rng(seed)
    n_world = 900000
    kind = rng.integers(0, 10, n_world)
    x = rng.uniform(-25.0, 125.0, n_world)
    world = np.empty((n_world, 3))
    ground = kind < 5
    wall = (kind >= 5) & (kind < 7)
    pillar = kind >= 7
    world[ground] = np.c_[x[ground], rng.uniform(-12.0, 12.0, ground.sum()), np.zeros(ground.sum())]
    side = np.where(rng.random(wall.sum()) < 0.5, -1.0, 1.0)
    world[wall] = np.c_[x[wall], side * (11.0 + 0.8 * np.sin(0.35 * x[wall] + side)), rng.uniform(0.0, 4.0, wall.sum())]
    cx, cy = rng.uniform(-25.0, 125.0, 120), rng.uniform(-9.5, 9.5, 120)
    which = rng.integers(0, 120, pillar.sum())
    face = rng.integers(0, 4, pillar.sum())
    u = rng.uniform(-0.7, 0.7, pillar.sum())
    px = np.where(face < 2, np.where(face == 0, -0.7, 0.7), u)
    py = np.where(face < 2, u, np.where(face == 2, -0.7, 0.7))
    world[pillar] = np.c_[cx[which] + px, cy[which] + py, rng.uniform(0.0, 3.0, pillar.sum())]
    scans, poses, stamps = [], [], []
    pos, yaw = np.array([0.0, 0.0, 1.8]), 0.0
    for f in range(frames):
        if f:
            step = 0.6 if f < 20 else 0.9
            yaw += 0.012
            pos = pos + step * np.array([np.cos(yaw), np.sin(yaw), 0.0])
        T = np.eye(4)
        T[:3, :3] = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
        T[:3, 3] = pos
        near = np.flatnonzero(np.linalg.norm(world - pos, axis=1) < 21.0)
        pick = rng.choice(near, size=min(points, len(near)), replace=False)
        local = (world[pick] - pos) @ T[:3, :3] + rng.normal(0.0, 0.01, (len(pick), 3))
        if width > 3:
            local = np.c_[local, rng.normal(size=(len(local), width - 3))]
        scans.append(np.ascontiguousarray(local))
        poses.append(T)
        stamps.append(rng.uniform(0.0, 1.0, len(local)))
    return scans, poses, stamps

"""CPU oracle of the descriptor-carrying odometry (``KissICP.register_frame(use_descriptors=True)``, ``VoxelHashMap.update`` on 387-column
rows), composed from tests/odometry_oracle.py and ``oracle.oracle``.

  RowVoxelMap        odometry_oracle.VoxelMap holding 387-column rows: the same cap (old points first) and the same removal (EVERY voxel whose
                     first point's xyz is far goes); ``rows()`` in (voxel key, insertion) order -- the row numbering of the searches
  KissICPDesc        the loop of odometry_oracle.KissICP with the descriptor-seeded RegisterFrame (oracle.register_frame_nd) against
                     ``rows()`` and ``update`` on the rows; ``history`` keeps every frame's iterations
  descriptor_drive   odometry_oracle.synthetic_drive with a descriptor per point that is a smooth function of its WORLD position: the same
                     surface point matches across frames at cosine >= 0.8, points 2 m apart do not
"""
from __future__ import annotations

import numpy as np

from tests import odometry_oracle as oo

DESCRIPTOR_SIZE = 384
POINT_SIZE = 3 + DESCRIPTOR_SIZE


class RowVoxelMap(oo.VoxelMap):
    """dict: voxel key -> list of rows (fp64 [387]: xyz in the map frame, then the descriptor as given) in insertion order"""

    def add_points(self, rows: np.ndarray) -> int:
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float64))
        added = 0
        if len(rows):
            keys, bad = oo.voxel_keys(rows[:, :3], self.voxel_size)
            self.status |= int(bad)
            for k, r in zip(keys.tolist(), rows):
                block = self.voxels.get(k)
                if block is None:
                    self.voxels[k] = [r]
                    added += 1
                elif self.cap <= 0 or len(block) < self.cap:
                    block.append(r)
                    added += 1
        self.last = dict(points_added=added, voxels_removed=0, points_removed=0)
        return added

    def remove_far(self, origin) -> None:
        o = np.asarray(origin, dtype=np.float64)
        md2 = self.max_distance * self.max_distance
        gone = []
        for k, block in self.voxels.items():
            d = block[0][:3] - o
            if ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) > md2:
                gone.append(k)
        self.last["voxels_removed"] = len(gone)
        self.last["points_removed"] = sum(len(self.voxels[k]) for k in gone)
        for k in gone:
            del self.voxels[k]

    def update(self, rows: np.ndarray, pose=None, origin="pose") -> None:
        from oracle import oracle
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float64))
        if pose is not None and len(rows):
            rows = oracle.transform_pcl(rows, np.asarray(pose, dtype=np.float64))     # xyz moved, the other columns as they are
        self.add_points(rows)
        if isinstance(origin, str):
            origin = np.asarray(pose, dtype=np.float64)[:3, 3] if pose is not None else None
        if origin is not None:
            self.remove_far(origin)

    def rows(self) -> np.ndarray:
        width = next(iter(self.voxels.values()))[0].shape[0] if self.voxels else POINT_SIZE
        return np.array([r for k in sorted(self.voxels) for r in self.voxels[k]], dtype=np.float64).reshape(-1, width)

    def grid(self):
        keys = np.array(sorted(self.voxels), dtype=np.int64)
        sizes = np.array([len(self.voxels[k]) for k in keys.tolist()], dtype=np.int64)
        return keys, np.r_[0, np.cumsum(sizes)].astype(np.int32), self.rows()[:, :3]

    def full_voxels(self) -> int:
        return sum(len(b) == self.cap for b in self.voxels.values())


class KissICPDesc(oo.KissICP):
    def __init__(self, config, map_update_threshold=0.0):
        super().__init__(config, map_update_threshold)
        self.local_map = RowVoxelMap(config.mapping.voxel_size, config.data.max_range, config.mapping.max_points_per_voxel)
        self.history = []     # per registered frame: the (kind, system, dx, count) tuples of oracle.register_frame_nd

    def register_frame(self, frame, timestamps, deskewed=None):
        from oracle import oracle
        frame = np.asarray(frame, dtype=np.float64)
        if self.config.data.preprocess:
            frame = frame[oo.range_crop(frame, self.config.data.min_range, self.config.data.max_range)]
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
            new_pose, _, _, hist = oracle.register_frame_nd(source, self.local_map.rows(), vs, initial_guess, 3 * sigma, sigma / 3,
                                                            return_history=True)
            self.history.append(hist)
        motion = np.linalg.inv(last_pose) @ new_pose
        if np.linalg.norm(motion[:3, -1]) < self.map_update_threshold and len(self.poses) > 1:
            return new_pose, frame_downsample, False
        if self.adaptive_threshold is not None:
            self.adaptive_threshold.update_model_deviation(np.linalg.inv(initial_guess) @ new_pose)
        self.local_map.update(frame_downsample, new_pose)
        self.stats.append(dict(self.local_map.last, offered=len(frame_downsample)))
        self.poses.append(new_pose)
        return new_pose, frame_downsample, True


def descriptor_of(world: np.ndarray, P: np.ndarray, phase: np.ndarray) -> np.ndarray:
    return np.cos(np.asarray(world, dtype=np.float64) @ P + phase)


def descriptor_drive(frames: int = 14, points: int = 2500, seed: int = 11):
    """(387-column fp64 scans in the sensor frame, ground-truth poses, timestamps): descriptor = cos(w @ P + phase) + N(0, 0.02), w the
    point's world position, P ~ N(0, 0.6) [3, 384] and phase ~ U(0, 2 pi) from default_rng(seed + 1)"""
    scans, poses, stamps = oo.synthetic_drive(frames, points, seed, width=3)
    rng = np.random.default_rng(seed + 1)
    P = rng.normal(0.0, 0.6, (3, DESCRIPTOR_SIZE))
    phase = rng.uniform(0.0, 2.0 * np.pi, DESCRIPTOR_SIZE)
    wide = []
    for local, T in zip(scans, poses):
        world = local @ T[:3, :3].T + T[:3, 3]
        desc = descriptor_of(world, P, phase) + rng.normal(0.0, 0.02, (len(local), DESCRIPTOR_SIZE))
        wide.append(np.ascontiguousarray(np.c_[local, desc]))
    return wide, poses, stamps


def drive_config(load_config, **kw):
    """the configuration of the descriptor drive's tests from either ``load_config``: max_range 12, voxel 1.0, cap 20, sigma fixed at 2"""
    cfg = load_config(max_range=12, **kw)
    cfg.mapping.voxel_size = 1.0
    cfg.mapping.max_points_per_voxel = 20
    cfg.adaptive_threshold.fixed_threshold = 2.0
    return cfg

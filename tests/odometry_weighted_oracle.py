"""CPU oracle of the descriptor-weighted odometry (``KissICP(descriptor_mode="weighted").register_frame(use_descriptors=True)``, a
``VoxelHashMap(descriptor_mode="weighted")`` under ``update``), composed from tests/odometry_desc_oracle.py and ``oracle.oracle``.

  KissICPWeighted    odometry_desc_oracle.KissICPDesc with RegisterFrame(VectorXd ...) (oracle.register_frame_xd) against ``rows()`` of its
                     RowVoxelMap -- rows of any width --; ``history`` keeps every registered frame's (source, map rows, initial guess,
                     3 sigma, sigma / 3, iterations) so a test can replay a frame's search
  weighted_drive     odometry_desc_oracle.descriptor_drive's recipe with the descriptor width as a parameter
  first_targets      the first iteration's (tgt, valid) of a recorded frame, with its descriptors or with all of them zeroed (every weight
                     is then 1: the plain nearest neighbour of the same loop)
  map_stats          orc_icp_desc_stats of descriptor rows
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import odometry_desc_oracle as do
from tests import odometry_oracle as oo


class KissICPWeighted(do.KissICPDesc):
    def register_frame(self, frame, timestamps, deskewed=None):
        from oracle import oracle
        frame = np.asarray(frame, dtype=np.float64)
        if self.config.data.deskew and len(self.poses) >= 2:
            if deskewed is None:
                deskewed = oo.deskew(frame, timestamps, oo.se3_log(np.linalg.inv(self.poses[-2]) @ self.poses[-1]))
            frame = np.c_[deskewed, frame[:, 3:]]
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
        if self.local_map.empty() or len(source) == 0:                              # Registration.cpp:389
            new_pose = np.ascontiguousarray(initial_guess, dtype=np.float64)
        else:
            rows = self.local_map.rows()
            new_pose, hist = oracle.register_frame_xd(source, rows, vs, initial_guess, 3 * sigma, sigma / 3, return_history=True)
            self.history.append(dict(source=source, rows=rows, voxel_size=vs, guess=np.array(initial_guess), max_dist=3 * sigma,
                                     kernel=sigma / 3, hist=hist))
        motion = np.linalg.inv(last_pose) @ new_pose
        if np.linalg.norm(motion[:3, -1]) < self.map_update_threshold and len(self.poses) > 1:
            return new_pose, frame_downsample, False
        if self.adaptive_threshold is not None:
            self.adaptive_threshold.update_model_deviation(np.linalg.inv(initial_guess) @ new_pose)
        self.local_map.update(frame_downsample, new_pose)
        self.stats.append(dict(self.local_map.last, offered=len(frame_downsample)))
        self.poses.append(new_pose)
        return new_pose, frame_downsample, True


def weighted_drive(width: int, frames: int = 10, points: int = 2500, seed: int = 11, dtype=np.float64):
    """(scans of 3 + ``width`` columns in the sensor frame, ground-truth poses, timestamps): descriptor_drive's recipe -- descriptor =
    cos(w @ P + phase) + N(0, 0.02), w the point's world position, P ~ N(0, 0.6) [3, width], phase ~ U(0, 2 pi) from
    default_rng(seed + 1) -- at any width, the scans in ``dtype``"""
    scans, poses, stamps = oo.synthetic_drive(frames, points, seed, width=3)
    rng = np.random.default_rng(seed + 1)
    P = rng.normal(0.0, 0.6, (3, width))
    phase = rng.uniform(0.0, 2.0 * np.pi, width)
    wide = []
    for local, T in zip(scans, poses):
        world = local @ T[:3, :3].T + T[:3, 3]
        desc = do.descriptor_of(world, P, phase) + rng.normal(0.0, 0.02, (len(local), width))
        wide.append(np.ascontiguousarray(np.c_[local, desc].astype(dtype)))
    return wide, poses, stamps


def run(frames, stamps, load_config=oo.load_config, threshold=0.0, **config):
    k = KissICPWeighted(do.drive_config(load_config, **config), threshold)
    return k, [k.register_frame(f, t) for f, t in zip(frames, stamps)]


def first_targets(record, zero_descriptors: bool = False):
    """(tgt [n, 3], valid uint8[n]) of the first iteration of a frame ``KissICPWeighted.history`` recorded"""
    from oracle import oracle
    source, rows = record["source"], record["rows"]
    if zero_descriptors:
        source, rows = source.copy(), rows.copy()
        source[:, 3:] = 0.0
        rows[:, 3:] = 0.0
    _, hist = oracle.register_frame_xd(source, rows, record["voxel_size"], record["guess"], record["max_dist"], record["kernel"], max_iter=1,
                                       return_history=True)
    return hist[0][2], hist[0][3]


def map_stats(desc: np.ndarray):
    """(norm fp64[n], has uint8[n]) = orc_icp_desc_stats of the rows' fp64 image"""
    from oracle import oracle
    d = np.ascontiguousarray(desc, dtype=np.float64)
    n, f = d.shape
    norm, has = np.empty(n), np.empty(n, np.uint8)
    oracle.lib().orc_icp_desc_stats(d.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(n), C.c_int32(f),
                                    norm.ctypes.data_as(C.POINTER(C.c_double)), has.ctypes.data_as(C.POINTER(C.c_uint8)))
    return norm, has

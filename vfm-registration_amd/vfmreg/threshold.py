"""Mirror of kiss_icp.threshold (src/kiss-icp/python/kiss_icp/threshold.py:28-59) with the estimator of Threshold.cpp:29-50 restated on
the host in fp64: sigma = sqrt(mean of the squared model errors), model error = |t| + 2 max_range sin(theta / 2) of the deviation
between the predicted and the estimated pose, theta as Eigen::AngleAxisd(R).angle() computes it (matrix -> quaternion,
2 atan2(|vec|, |w|)).

``get_threshold()`` ADDS A SAMPLE EVERY TIME IT IS CALLED while the stored deviation's error exceeds ``min_motion_th``
(AdaptiveThreshold::ComputeThreshold does); a frame whose map update is skipped leaves the deviation in place, so the next call counts
it a second time -- the reference's behaviour, kept."""
from __future__ import annotations

import numpy as np

from .icp import quaternion_of


def get_threshold_estimator(config):
    if config.adaptive_threshold.fixed_threshold is not None:
        return FixedThreshold(config.adaptive_threshold.fixed_threshold)
    return AdaptiveThreshold(config)


class FixedThreshold:

    def __init__(self, fixed_threshold: float):
        self.fixed_threshold = fixed_threshold

    def get_threshold(self):
        return self.fixed_threshold

    def update_model_deviation(self, model_deviation):
        pass


def rotation_angle(R: np.ndarray) -> float:
    """Eigen::AngleAxisd(R).angle()"""
    w, q = quaternion_of(R)
    n = float(np.sqrt(q @ q))
    return 2.0 * float(np.arctan2(n, abs(w))) if n != 0.0 else 0.0


class AdaptiveThreshold:

    def __init__(self, config):
        self.initial_threshold = float(config.adaptive_threshold.initial_threshold)
        self.min_motion_th = float(config.adaptive_threshold.min_motion_th)
        self.max_range = float(config.data.max_range)
        self.model_error_sse2 = 0.0
        self.num_samples = 0
        self.model_deviation = np.eye(4)

    def compute_model_error(self) -> float:
        theta = rotation_angle(self.model_deviation[:3, :3])
        delta_rot = 2.0 * self.max_range * np.sin(theta / 2.0)
        t = self.model_deviation[:3, 3]
        delta_trans = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
        return float(delta_trans + delta_rot)

    def get_threshold(self):
        model_error = self.compute_model_error()
        if model_error > self.min_motion_th:
            self.model_error_sse2 += model_error * model_error
            self.num_samples += 1
        if self.num_samples < 1:
            return self.initial_threshold
        return float(np.sqrt(self.model_error_sse2 / self.num_samples))

    def update_model_deviation(self, model_deviation: np.ndarray):
        self.model_deviation = np.array(model_deviation, dtype=np.float64)

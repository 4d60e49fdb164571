"""Mirror of kiss_icp.deskew (src/kiss-icp/python/kiss_icp/deskew.py:28-49): ``MotionCompensator.deskew_scan`` moves every point of a
scan by the share of the last inter-frame motion that its timestamp asks for (DeSkewScan, Deskew.cpp:40-68):
``out_i = exp((t_i - 0.5) * log(poses[-2]^-1 poses[-1])) * p_i``.  The twist is taken on the host (``icp.se3_log``), the per-point
exponential and product run on the GPU (csrc/odometry.hip ``vfm_deskew_scan``).  Rows wider than 3 keep their other columns, as the
C++ ``VectorXd`` overload does."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .icp import se3_log


def get_motion_compensator(config):
    return MotionCompensator() if config.data.deskew else StubCompensator()


class StubCompensator:

    def deskew_scan(self, frame, poses, timestamps):
        return frame


class MotionCompensator:

    @staticmethod
    def delta(poses) -> np.ndarray:
        """(start_pose.inverse() * finish_pose).log() of the last two poses (Deskew.cpp:44)"""
        return se3_log(np.linalg.inv(poses[-2]) @ poses[-1])

    def deskew_device(self, rows: torch.Tensor, poses, timestamps: torch.Tensor) -> torch.Tensor:
        """the de-skewed coordinates (fp64 [n, 3]) of device-resident rows; needs two poses"""
        return ops.deskew_scan(rows, timestamps, self.delta(poses))

    def deskew_scan(self, frame, poses, timestamps):
        if len(poses) < 2:
            return frame
        frame = np.asarray(frame)
        if frame.ndim != 2 or frame.shape[1] < 3:
            raise ValueError("Invalid shape")
        if len(frame) == 0:
            return np.zeros((0, frame.shape[1]), dtype=np.float64)
        rows = torch.from_numpy(np.ascontiguousarray(frame, dtype=np.float64)).cuda()
        stamps = torch.from_numpy(np.ascontiguousarray(timestamps, dtype=np.float64)).cuda()
        out = np.array(frame, dtype=np.float64)
        out[:, :3] = self.deskew_device(rows, poses, stamps).cpu().numpy()
        return out

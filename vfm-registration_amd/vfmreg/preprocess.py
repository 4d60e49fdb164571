"""Mirror of kiss_icp.preprocess (src/kiss-icp/python/kiss_icp/preprocess.py:28-60): ``Preprocessor`` keeps the rows whose range lies
strictly between ``config.data.min_range`` and ``config.data.max_range`` (Preprocess, Preprocessing.cpp:139-197), in input order.
The crop runs on the GPU (csrc/odometry.hip ``vfm_range_crop``: an ordered compaction in one launch); rows of any width >= 3 are taken,
the columns behind xyz ride along."""
from __future__ import annotations

import numpy as np
import torch

from . import ops


def get_preprocessor(config):
    return Preprocessor(config) if config.data.preprocess else Stubcessor()


class Stubcessor:

    def __call__(self, frame: np.ndarray):
        return frame


class Preprocessor(Stubcessor):

    def __init__(self, config):
        self.config = config

    def crop_device(self, rows: torch.Tensor):
        """(idx int64[n], count int64[1]) of the surviving rows of device-resident fp64 rows -- no read-back"""
        return ops.range_crop(rows, self.config.data.min_range, self.config.data.max_range)

    def __call__(self, frame: np.ndarray):
        frame = np.asarray(frame)
        if frame.ndim != 2 or frame.shape[1] < 3:
            raise ValueError("Invalid shape")   # preprocess.py:53
        if len(frame) == 0:
            return np.zeros((0, frame.shape[1]), dtype=np.float64)
        rows = torch.from_numpy(np.ascontiguousarray(frame, dtype=np.float64)).cuda()
        idx, count = self.crop_device(rows)
        return rows[idx[:int(count.item())]].cpu().numpy()

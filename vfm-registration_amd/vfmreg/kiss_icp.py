"""Mirror of kiss_icp.kiss_icp.KissICP (src/kiss-icp/python/kiss_icp/kiss_icp.py:35-138): LiDAR odometry over a stream of scans with
a local map that grows and forgets.

A frame is uploaded once.  On the device: the optional de-skew (``vfm_deskew_scan``), the range crop (``vfm_range_crop``), the two
voxel levels at 0.5 and 1.5 x the map's voxel size (``vfm_voxel_robin_level``, chained on indices without a read-back, as
``RegistrationNode._voxel_chain``), the ICP loop against the map's kept grid (``icp.register_frame_on_grid``) and the map update
(``VoxelHashMap.update`` -> ``vfm_icp_grid_update``).  On the host: the pose algebra in the reference's expressions
(``np.linalg.inv(a) @ b``), the adaptive threshold and the 6 x 6 solves.  Descriptor columns ride along by index and come back in
``original_frame_downsample``.

The reference's class has its de-skew line commented out; here it runs when ``config.data.deskew`` is true (default false: the
reference's behaviour), as the C++ pipeline (KissICP.cpp:69-103) and upstream do.

``use_descriptors=True`` (kiss_icp.py:47-113, the paper's VFM-seeded odometry) takes frames of 387 columns: ``source`` and
``frame_downsample`` keep their 384 descriptor columns, the pose comes from the descriptor-seeded RegisterFrame
(``icp._register_frame_nd_device``) against a local map that carries descriptors, and ``VoxelHashMap.update`` moves the map's descriptor
rows along with its points (``vfm_icp_grid_update_src`` + ``vfm_rows_merge``).  The map's search operand is prepared again for the whole
map every frame.  In this mode (``descriptor_mode="seeded"``, the default) frames of another width are refused.

``KissICP(config, map_update_threshold, descriptor_mode="weighted")`` is the reference's ``VectorXd`` local map (``map_x_``) and the paper's
descriptor-weighted ICP: ``use_descriptors=True`` then takes frames of 3 + D columns, D >= 1 (387 included), through the same stages, keeps
them in a local map of that width (``VoxelHashMap(descriptor_mode="weighted")``) and registers with RegisterFrame(VectorXd ...)
(Registration.cpp:384-423; ``icp.register_frame_weighted_device``, csrc/icp_rows.hip), whose search picks the neighbour that minimises
``|dxyz|^2 * clamp(0.5 (1 - cos), 0.01, 1)``; the initial guess is returned while ``empty_x()`` (Registration.cpp:389).  The first frame
fixes the width.  ``use_descriptors=False`` is the same in both modes."""
from __future__ import annotations

import time

import numpy as np
import torch

from . import icp, ops
from .deskew import get_motion_compensator
from .mapping import check_descriptor_mode, get_voxel_hash_map
from .preprocess import get_preprocessor
from .threshold import get_threshold_estimator


class KissICP:
    CHAIN_MAX = 1 << 18   # the one-launch voxel level's limit (vfm_voxel_robin_level)

    def __init__(self, config, map_update_threshold=0.0, descriptor_mode="seeded"):
        self.descriptor_mode = check_descriptor_mode(descriptor_mode)     # what ``use_descriptors=True`` runs (the module docstring)
        self.poses = []
        self.config = config
        self.compensator = get_motion_compensator(config)
        self.adaptive_threshold = get_threshold_estimator(self.config)
        self.local_map = get_voxel_hash_map(self.config, descriptor_mode)
        self.preprocess = get_preprocessor(self.config)
        self.map_update_threshold = map_update_threshold
        self.profile = False      # True: synchronise between the stages and keep their wall-clock times in ``timings``
        self.timings = {}
        self._host = None         # pinned int64: the frame's one read-back of counts and level infos

    # ------------------------------------------------------------------ stages
    def _tick(self, name, t0):
        if self.profile:
            torch.cuda.synchronize()
            now = time.perf_counter()
            self.timings[name] = self.timings.get(name, 0.0) + (now - t0)
            return now
        return t0

    def _levels(self, pts: torch.Tensor, idx, count):
        """(rows of ``pts`` behind frame_downsample, behind source): VoxelDownsample at 0.5 x then 1.5 x the voxel size on the rows
        ``idx[:count]`` of ``pts`` (None: all of them), each level in the order the one before left (kiss_icp.py:115-122)."""
        vs = self.config.mapping.voxel_size
        n = pts.shape[0]
        dev = pts.device
        if self._host is None:
            self._host = torch.zeros(17, dtype=torch.int64).pin_memory()
        if 1 <= n <= self.CHAIN_MAX:
            l1 = ops.voxel_robin_level(pts, vs * 0.5, idx=idx, n_dev=count, n_max=n)
            l2 = ops.voxel_robin_level(pts, vs * 1.5, idx=l1["keep"], n_dev=l1["count"], n_max=n)
            cnt = count if count is not None else torch.full((1,), n, dtype=torch.int64, device=dev)
            self._host.copy_(torch.cat((cnt, l1["info"], l2["info"])), non_blocking=True)
            torch.cuda.current_stream().synchronize()
            h = self._host.numpy()
            if h[0] == 0:
                empty = torch.zeros(0, dtype=torch.int64, device=dev)
                return empty, empty
            if all(h[1 + 8 * k + 5] == 1 and h[1 + 8 * k + 1] > 0 for k in range(2)):
                return l1["keep"][:int(h[2])], l2["keep"][:int(h[10])]
            kept = idx[:int(h[0])] if idx is not None else None
        else:
            kept = idx[:int(count.item())] if idx is not None else None
        # level by level (a scan beyond the one-launch kernel's size, or a level it does not reproduce): the same answers
        xyz = pts[:, :3] if kept is None else pts[kept, :3]
        if xyz.shape[0] == 0:
            empty = torch.zeros(0, dtype=torch.int64, device=dev)
            return empty, empty
        o1 = ops.voxel_robin(xyz.contiguous(), vs * 0.5)
        down = o1 if kept is None else kept[o1]
        o2 = ops.voxel_robin(pts[down, :3].contiguous(), vs * 1.5)
        return down, down[o2]

    # ------------------------------------------------------------------ kiss_icp.py:47-113
    def register_frame(self, frame, timestamps, use_descriptors=False):
        if use_descriptors:
            return self._register_frame_desc(frame, timestamps)
        frame = np.asarray(frame)
        if frame.ndim != 2 or frame.shape[1] < 3:
            raise ValueError("Invalid shape")
        t0 = time.perf_counter() if self.profile else 0.0
        rows = torch.from_numpy(np.ascontiguousarray(frame, dtype=np.float64)).cuda()     # the frame's one upload
        n = rows.shape[0]
        # de-skew (kiss_icp.py:50 has the call commented out; KissICP.cpp:69-103 makes it)
        pts = rows
        deskewed = self.config.data.deskew and len(self.poses) >= 2 and n > 0
        if deskewed:
            stamps = torch.from_numpy(np.ascontiguousarray(timestamps, dtype=np.float64)).cuda()
            pts = self.compensator.deskew_device(rows, self.poses, stamps)
        t0 = self._tick("upload_deskew", t0)
        # range crop (kiss_icp.py:54-60)
        idx = count = None
        if self.config.data.preprocess and n > 0:
            idx, count = self.preprocess.crop_device(pts)
        t0 = self._tick("crop", t0)
        # the two voxel levels (kiss_icp.py:65-79); the rows' other columns follow by index
        if n > 0:
            down_idx, source_idx = self._levels(pts, idx, count)
        else:
            down_idx = source_idx = torch.zeros(0, dtype=torch.int64, device=rows.device)
        frame_downsample = pts[down_idx, :3].contiguous()
        source = pts[source_idx, :3].contiguous()
        t0 = self._tick("voxel_chain", t0)

        # kiss_icp.py:83-88: sigma, then the constant-velocity guess
        sigma = self.get_adaptive_threshold()
        prediction = self.get_prediction_model()
        last_pose = self.poses[-1] if self.poses else np.eye(4)
        initial_guess = last_pose @ prediction

        # kiss_icp.py:94-100
        if source.shape[0] == 0 or self.local_map.empty():
            new_pose = np.ascontiguousarray(initial_guess, dtype=np.float64)   # Registration.cpp:150
        else:
            new_pose = icp.register_frame_on_grid(source, icp._grid_of(self.local_map), initial_guess, 3 * sigma, sigma / 3)
        t0 = self._tick("icp", t0)

        original_frame_downsample = rows[down_idx].cpu().numpy()    # (all columns: kiss_icp.py:76)
        if deskewed:
            original_frame_downsample[:, :3] = frame_downsample.cpu().numpy()

        # kiss_icp.py:104-113: a frame that moved less than the threshold leaves map, deviation and poses as they were
        motion = np.linalg.inv(last_pose) @ new_pose
        if np.linalg.norm(motion[:3, -1]) < self.map_update_threshold and len(self.poses) > 1:
            return new_pose, original_frame_downsample, False

        self.adaptive_threshold.update_model_deviation(np.linalg.inv(initial_guess) @ new_pose)
        self.local_map.update(frame_downsample, new_pose)
        self.poses.append(new_pose)
        self._tick("update", t0)
        return new_pose, original_frame_downsample, True

    def _register_frame_desc(self, frame, timestamps):
        """register_frame(use_descriptors=True): the stages of ``register_frame`` with the descriptor columns kept on ``source`` and
        ``frame_downsample`` (kiss_icp.py:65-79), the descriptor-seeded RegisterFrame (Registration.cpp:197-382) and the 387-column map"""
        frame = np.asarray(frame)
        if frame.ndim != 2 or frame.shape[1] < 3:
            raise ValueError("Invalid shape")
        weighted = self.descriptor_mode == "weighted"
        if weighted:                             # (before anything is uploaded) xyz + D >= 1 descriptor columns, the width of the map's rows
            held = self.local_map.width_n()
            if frame.shape[1] < 4 or (held is not None and held != frame.shape[1]):
                raise ValueError("Invalid shape")
        elif frame.shape[1] != icp.POINT_SIZE:   # (before anything is uploaded)
            raise NotImplementedError(f"use_descriptors=True: descriptor odometry takes frames of {icp.POINT_SIZE} columns (xyz + "
                                      f"{icp.POINT_SIZE - 3} descriptor columns), got {frame.shape[1]}; the VectorXd local map of other "
                                      "widths is not built")
        t0 = time.perf_counter() if self.profile else 0.0
        rows = torch.from_numpy(np.ascontiguousarray(frame)).cuda()                # the frame's one upload, in its own dtype
        if rows.dtype not in (torch.float32, torch.float64):
            rows = rows.double()
        n = rows.shape[0]
        xyz = rows[:, :3].double().contiguous()                                     # (fp32 -> fp64 is exact: what pybind's cast gives)
        deskewed = self.config.data.deskew and len(self.poses) >= 2 and n > 0
        if deskewed:
            stamps = torch.from_numpy(np.ascontiguousarray(timestamps, dtype=np.float64)).cuda()
            xyz = self.compensator.deskew_device(xyz, self.poses, stamps)
        t0 = self._tick("upload_deskew", t0)
        idx = count = None
        if self.config.data.preprocess and n > 0:
            idx, count = self.preprocess.crop_device(xyz)
        t0 = self._tick("crop", t0)
        if n > 0:
            down_idx, source_idx = self._levels(xyz, idx, count)
        else:
            down_idx = source_idx = torch.zeros(0, dtype=torch.int64, device=rows.device)
        down_rows = rows[down_idx]                                                  # frame_downsample, all columns
        if deskewed:
            down_rows = down_rows.double()
            down_rows[:, :3] = xyz[down_idx]
        source_rows, source_xyz = rows[source_idx], xyz[source_idx].contiguous()   # (the search reads the descriptor columns only)
        t0 = self._tick("voxel_chain", t0)

        sigma = self.get_adaptive_threshold()
        prediction = self.get_prediction_model()
        last_pose = self.poses[-1] if self.poses else np.eye(4)
        initial_guess = last_pose @ prediction

        if weighted:
            if source_rows.shape[0] == 0 or self.local_map.empty_x():
                new_pose = np.ascontiguousarray(initial_guess, dtype=np.float64)   # Registration.cpp:389
            else:
                new_pose = icp.register_frame_weighted_device(source_rows[:, 3:].contiguous(), source_xyz, self.local_map, initial_guess,
                                                              3 * sigma, sigma / 3)
        elif source_rows.shape[0] == 0 or self.local_map.empty_n():
            new_pose = np.ascontiguousarray(initial_guess, dtype=np.float64)       # Registration.cpp:204
        else:
            new_pose, _, _ = icp._register_frame_nd_device(source_rows, source_xyz, self.local_map, initial_guess, 3 * sigma, sigma / 3)
        t0 = self._tick("icp", t0)

        original_frame_downsample = down_rows.double().cpu().numpy()
        t0 = self._tick("download", t0)

        motion = np.linalg.inv(last_pose) @ new_pose
        if np.linalg.norm(motion[:3, -1]) < self.map_update_threshold and len(self.poses) > 1:
            return new_pose, original_frame_downsample, False

        self.adaptive_threshold.update_model_deviation(np.linalg.inv(initial_guess) @ new_pose)
        self.local_map.update(down_rows, new_pose)
        self.poses.append(new_pose)
        self._tick("update", t0)
        return new_pose, original_frame_downsample, True

    def voxelize(self, iframe):
        """kiss_icp.py:115-122 on a host array: (source, frame_downsample)"""
        iframe = np.asarray(iframe)
        if iframe.ndim != 2 or iframe.shape[1] < 3:
            raise ValueError("Invalid shape")
        if len(iframe) == 0:
            empty = np.zeros((0, iframe.shape[1]), dtype=np.float64)
            return empty, empty
        rows = torch.from_numpy(np.ascontiguousarray(iframe, dtype=np.float64)).cuda()
        down_idx, source_idx = self._levels(rows, None, None)
        return rows[source_idx].cpu().numpy(), rows[down_idx].cpu().numpy()

    def get_adaptive_threshold(self):
        """sigma of this frame (kiss_icp.py:124-126): the initial threshold until the sensor has moved, then the estimator's -- whose
        ``get_threshold`` adds a sample at every call (vfmreg/threshold.py)"""
        if self.has_moved():
            return self.adaptive_threshold.get_threshold()
        return self.config.adaptive_threshold.initial_threshold

    def get_prediction_model(self):
        """constant velocity (kiss_icp.py:128-131): the last inter-frame motion, the identity before there are two poses"""
        if len(self.poses) >= 2:
            return np.linalg.inv(self.poses[-2]) @ self.poses[-1]
        return np.eye(4)

    def has_moved(self):
        """kiss_icp.py:133-138: the translation between the first and the last pose exceeds 5 min_motion_th"""
        if not self.poses:
            return False
        travelled = np.linalg.inv(self.poses[0]) @ self.poses[-1]
        return np.linalg.norm(travelled[:3, -1]) > 5 * self.config.adaptive_threshold.min_motion_th

"""Mirror of the hot-path methods of ``RegistrationNode`` (src/vfm-reg/src/registration_node.py):

  compute_vfm_correspondences  RN:396-425      ransac_registration('vfm')  RN:273-357
  find_correspondences         RN:482-538      compute_errors              RN:997-1019
  compute_correspondences      RN:427-547 (the FPFH baseline; the learned baselines raise NotImplementedError)
  rotation re-orthogonalisation RN:331-336     icp_registration            RN:359-394
  ransac_registration('fpfh')  RN:282-357 (opt-in: ``baseline_methods``; the row recovery of RN:295-310 is vfmreg.neighbors)

  teaser_registration('vfm' | 'fpfh')  RN:91-159 (vfmreg/teaser.py stands in for teaserpp_python; 'fpfh' opt-in like the RANSAC row)

Same names, argument meaning and return values; numpy in / numpy out.  The ROS node, the learned baseline
descriptors and PointDSC are out of scope.  ``run_icp=True`` runs the point-to-point ICP
refinement of registration_node.py:338-344 / 133-157 (row F2, vfmreg/icp.py).
"""
from __future__ import annotations

import weakref
import zlib
from typing import Optional, Tuple

import numpy as np
import torch

from . import o3d, ops
from .config import load_config
from .descriptors import extract_fpfh_features_device
from .icp import register_frame
from .mapping import get_voxel_hash_map
from .utils import transform_pcl
from .voxelization import down_sample_device, to_device_rows, voxel_down_sample


def orthogonalize_rotation(pose: np.ndarray) -> np.ndarray:
    """RN:331-336: Newton iteration towards the closest rotation (3x3 fp64, host)."""
    pose = np.array(pose, dtype=np.float64, copy=True)
    R = pose[:3, :3]
    while np.abs(1 - np.linalg.det(R)) > 1e-12:
        R = 3 / 2 * R - 1 / 2 * R @ R.T @ R
    pose[:3, :3] = R
    return pose


def compute_errors(pose: np.ndarray, gt_pose: np.ndarray) -> Tuple[float, float]:
    """RN:997-1019: (RTE in m, RRE in degrees)."""
    rte = float(np.linalg.norm(pose[:3, 3] - gt_pose[:3, 3]))
    c = (np.trace(pose[:3, :3].T @ gt_pose[:3, :3]) - 1) / 2
    rre = float(np.abs(np.arccos(np.clip(c, -1, 1))) * 180 / np.pi)
    return rte, rre


def find_correspondences(feats0: np.ndarray, feats1: np.ndarray, n_points: int = 5000, mutual_filter: bool = True):
    """RN:482-538 (adapted from TEASER++): exact Euclidean 1-NN on the GPU instead of cKDTree.

    The rows are searched as float32 (the descriptors of this path are float32 -- image_features.py:101 --; the reference's
    cKDTree works in the caller's dtype, so float64 inputs that differ only beyond float32 precision may resolve exact ties and
    near-ties differently); the decision among float32 rows is the oracle's fp64 distance, ties to the lowest index."""
    f0 = torch.from_numpy(np.ascontiguousarray(feats0, dtype=np.float32)).cuda()
    f1 = torch.from_numpy(np.ascontiguousarray(feats1, dtype=np.float32)).cuda()
    i0, i1 = find_correspondences_device(f0, f1, n_points, mutual_filter)
    return i0.cpu().numpy(), i1.cpu().numpy()


# Rows of at most 64 columns have a search of their own on the f32 matrix cores (ops.NARROW).  On FPFH features it beats the fp16 search
# (ops.FAST) at every size measured -- 2x at 275 x 2751, 33x at 17 651 x 176 073 --, on well-separated random rows it ties up to 2000 x
# 2000 and loses from 5000 x 5000 on (profiles/l2_narrow_timing.md).  The forward search takes it from this many rows on:
# the first power of two above the random shape that lost.
NARROW_MIN_ROWS = 8192


def l2_search_mode(n: int, m: int, d: int) -> int:
    """The precision mode ``find_correspondences_device`` passes to ``ops.match_mutual_l2`` for n queries among m rows of d columns."""
    return ops.NARROW if d <= ops.NARROW_MAX_D and max(n, m) >= NARROW_MIN_ROWS else ops.FAST


def find_correspondences_device(f0: torch.Tensor, f1: torch.Tensor, n_points: int = 5000, mutual_filter: bool = True):
    """``find_correspondences`` on float32 rows that are on the device: the two index lists as device tensors, in the same order."""
    if mutual_filter:   # RN:520-532 in one call: the reverse direction is searched only at the matched rows of feats1
        i0, i1, count = ops.match_mutual_pairs(f0, f1)
        k = int(count.item())
        return i0[:k], i1[:k]
    # RN:505-518: the n_points pairs with the smallest distance (numpy's argpartition decides which and in what order: on the host)
    # (same indices and distances in every mode; ops.match_mutual_pairs above runs rows of at most 64 columns in NARROW at every size)
    nn01, d2, _ = ops.match_mutual_l2(f0, f1, mutual=False, prec=l2_search_mode(f0.shape[0], f1.shape[0], f0.shape[1]))
    dists = np.sqrt(d2.cpu().numpy())
    n = min(n_points, len(dists) - 1)
    top = torch.from_numpy(np.argpartition(dists, n)[:n]).to(nn01.device)
    return top, nn01[top]


def filter_recovered_rows(src_idx: torch.Tensor, src_dist: torch.Tensor, tgt_idx: torch.Tensor, tgt_dist: torch.Tensor) -> torch.Tensor:
    """RN:301-310 on the two ``KDTree.query`` results (K-element tensors, any device): if no distance of either side is above 1 mm
    every pair is kept (a distance of exactly 0.001 included); otherwise the pairs with ``src_dist < .001`` survive and of those the
    ones with ``tgt_dist < .001`` (exactly 0.001 is dropped), order preserved.  Returns the surviving (source row, target row) pairs
    as K' x 2 int64 -- in BOTH branches: the (K, 1) arrays sklearn returns make the reference's unfiltered branch stack to (K, 2, 1),
    which Vector2iVector flattens to the same pairs.  One read-back (the count).  K = 0 gives 0 pairs (the reference's ``.max()`` of
    an empty array raises)."""
    src_idx, src_dist, tgt_idx, tgt_dist = (t.reshape(-1) for t in (src_idx, src_dist, tgt_idx, tgt_dist))
    pairs = torch.stack((src_idx, tgt_idx), dim=1)
    if pairs.shape[0] == 0:
        return pairs
    over = (src_dist.max() > .001) | (tgt_dist.max() > .001)                        # RN:301
    keep = ~over | ((src_dist < .001) & (tgt_dist < .001))                          # RN:302-308
    return pairs[keep]


def _fingerprint(a: np.ndarray) -> Optional[int]:
    """A cheap host-side fingerprint of a C-contiguous array: CRC of ~4096 evenly spaced elements plus its first and last rows
    (microseconds for a 600 MB map).  None for arrays whose flat view would be a copy."""
    if not a.flags.c_contiguous or a.size == 0:
        return None
    flat = a.reshape(-1)
    step = max(1, flat.size // 4096)
    return zlib.crc32(np.ascontiguousarray(flat[::step]).tobytes() + a[0].tobytes() + a[-1].tobytes())


class MapHandle:
    """A scene's map, built once (``RegistrationNode.set_map``): the VoxelHashMap of RN:402-403 with its kept rows in the container's
    order on the device, cast and prepared for the search.  Pass it wherever a method takes ``voxel_map``: the scene loop of
    RN:556-589 builds ``local_map`` once and registers every scan of the scene against it -- with a handle nothing is rebuilt and
    nothing is guessed (no fingerprint of a 600 MB array: the caller says which map it means)."""

    __slots__ = ("voxel_hash_map", "rows", "cols", "dtype")

    def __init__(self, voxel_hash_map, shape, dtype):
        self.voxel_hash_map = voxel_hash_map
        self.rows, self.cols = int(shape[0]), int(shape[1])
        self.dtype = dtype

    def __repr__(self):
        return f"MapHandle({self.rows} x {self.cols} {self.dtype})"


class RegistrationNode:
    """The registration methods of the reference's node, without ROS (RN:44-89).

    ``cache_map`` (default OFF = the reference's behaviour, a fresh map per call): the reference registers every scan of a scene against the same ``local_map`` (built once,
    RN:556-580, used at RN:587-589), and re-builds its ``VoxelHashMap`` from that array in every call (RN:402-403).  Here the built
    map -- the kept rows in the container's order, uploaded and cast for the search -- is kept for as long as the caller passes the
    SAME array object (identity, shape, dtype) with the same fingerprint (``_fingerprint``: a CRC of ~4096 sampled elements and the
    first / last rows); a 200 000 x 387 fp64 map is 619 MB of PCIe upload and ~4 ms of container replay per call otherwise.  An
    in-place edit that misses every sampled element goes unnoticed (tests/test_gpu_api.py documents one): a caller that opts in
    promises not to edit the array in place between calls, or calls ``invalidate_map()`` after doing so.  ``evaluate_scene`` -- which
    builds the scene's map itself and never edits it -- opts in."""

    def __init__(self, config=None, ransac_iterations: int = 50000, max_correspondence_distance: float = 10000.0,
                 min_cosine_similarity: float = 0.8, cache_map: bool = False, baseline_methods=(), vfm_candidates: int = 1):
        self.config = config or load_config(None, None)  # RN:85
        self.ransac_iterations = ransac_iterations       # RN:326
        self.max_correspondence_distance = max_correspondence_distance  # RN:323
        self.min_cosine_similarity = min_cosine_similarity              # RN:418
        self.cache_map = bool(cache_map)
        self.baseline_methods = tuple(baseline_methods)   # the baseline rows of RN:867-874 ransac_registration answers to (opt-in)
        for m in self.baseline_methods:
            if m != "fpfh" and m not in self._LEARNED:
                raise ValueError(f"Invalid method: {m}")
        # map candidates per scan point of the VFM correspondences (the k of VoxelHashMap.cpp:491; the reference sets 1).  1: today's
        # search, the same code path; more: the k-best search -- among alike descriptors the best cosine is often a twin of the
        # right row -- and RANSAC / TEASER receive up to k pairs per scan point
        self.vfm_candidates = int(vfm_candidates)
        if not 1 <= self.vfm_candidates <= ops.MATCH_TOPK_MAX_K:
            raise ValueError(f"vfm_candidates must be in 1 .. {ops.MATCH_TOPK_MAX_K}, got {vfm_candidates}")
        self._map_cache = None   # (weakref to the array, (shape, dtype, fingerprint), VoxelHashMap)
        self._pose_cache = None  # (bytes of the last initial pose, its device copy): the node passes the identity in every call
        self._chain_host = None  # page-locked landing area of the voxel chain's one read-back
        self.map_descriptor_cache = {}   # RN:67: method -> (down_map, feats_map)
        self._map_descriptor_keys = {}   # method -> (shape, dtype, fingerprint) of the map those features were computed from
        self._map_descriptor_device = {}  # method -> (that key, down_map fp64, feats_map fp32) on the device

    def clear_map_descriptors(self) -> None:
        """RN:876-877: forget the maps' baseline features (the evaluation loop does at the first scan of a scene)."""
        self.map_descriptor_cache = {}
        self._map_descriptor_keys = {}
        self._map_descriptor_device = {}

    def invalidate_map(self) -> None:
        """Forget the kept map (``cache_map=True``): the next call rebuilds it from the array it is handed."""
        self._map_cache = None

    def set_map(self, voxel_map) -> MapHandle:
        """Build the scene's map ONCE (RN:402-403 + the upload and the search operand) and return a handle to pass in place of the array
        -- the explicit form of what ``cache_map=True`` infers from a sampled CRC.  The array may be edited or freed
        afterwards: the handle owns device copies."""
        vm = np.asarray(voxel_map)
        if vm.ndim != 2 or vm.shape[1] < 3:
            raise ValueError("Invalid shape")
        voxel_hash_map = get_voxel_hash_map(self.config)
        voxel_hash_map.add_points(vm)
        if not voxel_hash_map.empty_n():
            voxel_hash_map._device_map()
        return MapHandle(voxel_hash_map, vm.shape, vm.dtype.str)

    def _hash_map_for(self, voxel_map):
        """The VoxelHashMap of RN:402-403 for this map array -- built, or the one built for the same array before."""
        if isinstance(voxel_map, MapHandle):
            return voxel_map.voxel_hash_map
        vm = np.asarray(voxel_map)
        key = None
        if self.cache_map and isinstance(vm, np.ndarray) and vm.ndim == 2:
            fp = _fingerprint(vm)
            key = (vm.shape, vm.dtype.str, fp) if fp is not None else None
        c = self._map_cache
        if key is not None and c is not None and c[0]() is vm and c[1] == key:
            return c[2]
        voxel_hash_map = get_voxel_hash_map(self.config)                # RN:402-403
        voxel_hash_map.add_points(vm)
        if key is not None:
            if not voxel_hash_map.empty_n():
                voxel_hash_map._device_map()                            # ordered rows + fp32 descriptors, once
            try:
                self._map_cache = (weakref.ref(vm), key, voxel_hash_map)
            except TypeError:                                            # (an array-like that cannot be weakly referenced)
                self._map_cache = None
        return voxel_hash_map

    # The steps below are registration_node.py:396-425 and 288-344 line for line, but on device-resident rows: the
    # clouds are uploaded once, every voxelisation / transform / search works on the device copies, and only what the
    # caller receives (coordinates, poses) comes back.  The numpy-level mirrors (voxel_down_sample, transform_pcl,
    # VoxelHashMap.get_vfm_correspondences) give the same values; chaining THEM re-uploads 387-column fp64 rows at every
    # step (85 ms for a 6 000-point scan against a 30 000-point map, against 6 ms this way).
    def _correspond(self, voxel_map, raw_scan, initial_pose):
        vs = self.config.mapping.voxel_size
        # Only the scan's COORDINATES go to the device up front (N x 3): the three chained voxelisations key on them alone, and of
        # the N x 387 rows only the few hundred to ~2000 that survive the 5 m grid (RN:414) are ever searched -- their descriptor
        # columns are gathered on the host by the composed index chain and uploaded then (1 - 3 MB instead of 31 MB at C2 size).
        scan = np.asarray(raw_scan)
        if scan.ndim != 2 or scan.shape[1] < 3:
            raise ValueError("Invalid shape")
        raw_xyz = torch.from_numpy(np.ascontiguousarray(scan[:, :3], dtype=np.float64)).cuda()
        pose = np.ascontiguousarray(initial_pose, dtype=np.float64)
        key = pose.tobytes()
        if self._pose_cache is None or self._pose_cache[0] != key:
            self._pose_cache = (key, torch.from_numpy(pose).cuda())
        T = self._pose_cache[1]
        chain = self._voxel_chain(raw_xyz, T, vs) if 1 <= len(raw_xyz) <= (1 << 18) else None
        if chain is not None:
            # RN:399-400 + 414 in three launches and ONE read-back (round 5): every level takes the survivors of the one before as rows of
            # the raw scan, on the device
            xyz, raw_of_voxel_scan, order5, raw_idx5 = chain
        else:
            o1 = ops.voxel_robin(raw_xyz, vs * 0.5)                     # RN:399
            xyz = raw_xyz[o1]
            o2 = ops.voxel_robin(xyz, vs * 1.0)                         # RN:400  -> voxel_scan
            xyz = xyz[o2]
            raw_of_voxel_scan = o1[o2]                                  # rows of raw_scan behind voxel_scan, in its order
            order5 = raw_idx5 = None
        voxel_hash_map = self._hash_map_for(voxel_map)                  # RN:402-403 (kept across the scans of a scene)
        pcl_xyz = ops.transform_xyz(xyz, T)                             # RN:408 (descriptors carried through)
        out = None
        for voxel in (5.0, 1.0):                                        # RN:414, retry RN:420-423
            if voxel == 5.0 and order5 is not None:
                order, raw_idx = order5, raw_idx5
            else:
                order = ops.voxel_robin(pcl_xyz, voxel)
                raw_idx = raw_of_voxel_scan[order].cpu().numpy()
            sub_xyz = pcl_xyz[order]
            q_desc = self._upload_rows(scan, raw_idx)                   # VoxelHashMap.cpp:478-481
            if self.vfm_candidates == 1:
                qi, mi, _ = voxel_hash_map.search_device(None, self.min_cosine_similarity, q_desc=q_desc)       # RN:418
            else:   # up to k pairs per scan point, query-major (a scan point may appear several times: legal in both solvers)
                qi, mi, _, _ = voxel_hash_map.search_device_topk(None, self.min_cosine_similarity, self.vfm_candidates, q_desc=q_desc)
            out = dict(src_rows=order[qi], tgt_rows=mi, src_xyz=sub_xyz[qi])
            if len(qi) >= 75:
                break
            if voxel == 5.0:
                print("[WARNING] Voxelized too sparse, retrying with a larger voxel size")
        out.update(voxel_scan_xyz=xyz, voxel_hash_map=voxel_hash_map, map_xyz=voxel_hash_map.point_cloud_device())
        return out

    def _voxel_chain(self, raw_xyz: torch.Tensor, T: torch.Tensor, vs: float):
        """The three chained VoxelDownsample()s of RN:399-400 and 414 (voxel sizes vs / 2, vs, 5 m; the third on the points moved by the
        initial pose) as three kernel launches and one read-back: (voxel_scan xyz, its rows of the raw scan, the 5 m level's positions in
        voxel_scan, their rows of the raw scan on the host) -- or None where a level is not the one-launch kernel's (the caller then takes
        the level-by-level path: the same answers)."""
        n = raw_xyz.shape[0]
        l1 = ops.voxel_robin_level(raw_xyz, vs * 0.5)
        l2 = ops.voxel_robin_level(raw_xyz, vs * 1.0, idx=l1["keep"], n_dev=l1["count"], n_max=n)
        l3 = ops.voxel_robin_level(raw_xyz, 5.0, idx=l2["keep"], n_dev=l2["count"], n_max=n, T=T, want_local=True)
        head = min(n, self._CHAIN_HEAD)
        if self._chain_host is None:
            self._chain_host = torch.empty(24 + self._CHAIN_HEAD, dtype=torch.int64).pin_memory()
        packed = torch.cat((l1["info"], l2["info"], l3["info"], l3["keep"][:head]))
        self._chain_host[:packed.numel()].copy_(packed, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        h = self._chain_host.numpy()
        if any(h[8 * k + 5] != 1 or h[8 * k + 1] < 0 for k in range(3)):
            return None
        n2, n3 = int(h[9]), int(h[17])
        if n2 == 0 or n3 == 0:
            return None
        raw_of_voxel_scan = l2["keep"][:n2]
        raw_idx5 = h[24:24 + n3].copy() if n3 <= head else l3["keep"][:n3].cpu().numpy()
        return raw_xyz[raw_of_voxel_scan], raw_of_voxel_scan, l3["local"][:n3], raw_idx5

    def _voxel_scan(self, raw_xyz: torch.Tensor, vs: float) -> torch.Tensor:
        """RN:361-362 / 399-400 on device-resident 3-D points: VoxelDownsample at vs / 2, then at vs on its survivors in ITS order --
        two launches of the chain's kernel and one read-back, or level by level where that kernel does not reproduce a level."""
        n = raw_xyz.shape[0]
        if n == 0:
            return raw_xyz
        if n <= (1 << 18):
            l1 = ops.voxel_robin_level(raw_xyz, vs * 0.5)
            l2 = ops.voxel_robin_level(raw_xyz, vs * 1.0, idx=l1["keep"], n_dev=l1["count"], n_max=n)
            if self._chain_host is None:
                self._chain_host = torch.empty(24 + self._CHAIN_HEAD, dtype=torch.int64).pin_memory()
            self._chain_host[:16].copy_(torch.cat((l1["info"], l2["info"])), non_blocking=True)
            torch.cuda.current_stream().synchronize()
            h = self._chain_host.numpy()
            if all(h[8 * k + 5] == 1 and h[8 * k + 1] > 0 for k in range(2)):
                return raw_xyz[l2["keep"][:int(h[9])]]
        xyz = raw_xyz[ops.voxel_robin(raw_xyz, vs * 0.5)]
        return xyz[ops.voxel_robin(xyz, vs * 1.0)]

    _CHAIN_HEAD = 8192   # rows of the 5 m level read back together with the levels' infos (more: a second read-back)

    @staticmethod
    def _upload_rows(scan: np.ndarray, raw_idx: np.ndarray) -> torch.Tensor:
        """scan[raw_idx, 3:] as float32 on the device.  (Measured and dropped in round 5: gathering into a page-locked staging buffer
        and an asynchronous copy from there -- 180 us against 135 for this form at 1 700 rows x 384: numpy's row gather into
        page-locked memory is slower than into pageable memory by more than the driver's staging copy costs.)"""
        return torch.from_numpy(np.ascontiguousarray(scan[raw_idx, 3:], dtype=np.float32)).cuda()

    def compute_vfm_correspondences(self, voxel_map, raw_scan, initial_pose=np.eye(4)):
        c = self._correspond(voxel_map, raw_scan, initial_pose)
        return c["src_xyz"].cpu().numpy(), c["map_xyz"][c["tgt_rows"]].cpu().numpy()

    def ransac_registration(self, voxel_map, raw_scan, method: str = "vfm", run_icp: bool = False):
        """RN:273-357.  ``'vfm'`` always; the baseline names of RN:281 only on a node created with ``baseline_methods`` (default
        ``()``: they raise ValueError as every unknown name does): then ``'fpfh'`` runs where it is listed, and the learned names
        raise NotImplementedError as ``compute_correspondences`` does."""
        if method != "vfm":
            if self.baseline_methods and method in self._LEARNED:
                raise NotImplementedError(f"{method}: the learned baselines need their trained weights and are out of scope")
            if method == "fpfh" and method in self.baseline_methods:
                return self._ransac_registration_baseline(voxel_map, raw_scan, method, run_icp)
            raise ValueError(f"Invalid method: {method}")
        c = self._correspond(voxel_map, raw_scan, np.eye(4))
        # correspondence indices (RN:288-317).  The reference re-voxelises the scan and the map in 3-D and recovers the
        # rows with two KD-trees (distance < 1e-3); the containers are the same ones (same hash, same order), so the rows
        # are the ones the search already produced.
        # (the clouds and the index pairs stay on the device: o3d.utility.DeviceArray -- np.asarray() of one downloads it on demand;
        # the map's 200 000 points used to go down and up again, 4.8 MB each way, in every call)
        pcd_src = o3d.geometry.PointCloud()
        pcd_src.points = o3d.utility.Vector3dVector(o3d.utility.DeviceArray(c["voxel_scan_xyz"]))
        pcd_tgt = o3d.geometry.PointCloud()
        pcd_tgt.points = o3d.utility.Vector3dVector(o3d.utility.DeviceArray(c["map_xyz"]))
        coors = o3d.utility.Vector2iVector(o3d.utility.DeviceArray(torch.stack((c["src_rows"], c["tgt_rows"]), dim=1).to(torch.int32)))
        result = o3d.pipelines.registration.registration_ransac_based_on_correspondence(
            pcd_src, pcd_tgt, coors, self.max_correspondence_distance,
            o3d.pipelines.registration.TransformationEstimationPointToPoint(False), ransac_n=3,
            criteria=o3d.pipelines.registration.RANSACConvergenceCriteria(self.ransac_iterations, 1))
        ransac_pose = np.array(result.transformation)
        if run_icp:
            ransac_pose = orthogonalize_rotation(ransac_pose)                 # RN:331-336
            sigma = self.config.adaptive_threshold.initial_threshold          # RN:339
            # RN:290-293 builds the 3-D hash map from voxel_map[:, :3]: the same kept points in the same container
            vhm = c["voxel_hash_map"]
            voxel_scan = np.asarray(pcd_src.points)
            pose = register_frame(points=voxel_scan, voxel_map=vhm if not vhm.empty() else vhm.xyz_map(), initial_guess=ransac_pose,
                                  max_correspondance_distance=3 * sigma, kernel=sigma / 3)   # RN:340-344
            return ransac_pose, pose
        return ransac_pose, None

    def teaser_registration(self, voxel_map, raw_scan, method: str, run_icp: bool = False):
        """RN:91-159: TEASER++ on the correspondences of ``compute_vfm_correspondences`` (``'vfm'``) or of
        ``compute_correspondences(..., 'fpfh', mutual_filter=True)`` (``'fpfh'``: only on a node created with ``baseline_methods``
        that lists it, as ``ransac_registration('fpfh')``); every other name raises ValueError.  Returns (teaser_pose, pose after ICP or
        None).  An invalid solution (fewer than two consistent correspondences) is the identity, as the reference's ``np.eye(4)`` filled
        from an aborted solve.  ``voxel_map`` may be a ``MapHandle`` for ``'vfm'``."""
        from . import teaser
        if method == "vfm":
            c = self._correspond(voxel_map, raw_scan, np.eye(4))                                   # RN:104
            src, tgt = c["src_xyz"], c["map_xyz"][c["tgt_rows"]]
        elif method == "fpfh" and method in self.baseline_methods:
            vm, scan = np.asarray(voxel_map), np.asarray(raw_scan)
            if vm.ndim != 2 or vm.shape[1] < 3 or scan.ndim != 2 or scan.shape[1] < 3:
                raise ValueError("Invalid shape")
            map_xyz = np.ascontiguousarray(vm[:, :3])
            raw_xyz = torch.from_numpy(np.ascontiguousarray(scan[:, :3], dtype=np.float64)).cuda()
            src, tgt = self._baseline_correspondences_device(map_xyz, raw_xyz, method, True)       # RN:98-101
        else:
            raise ValueError(f"Invalid method: {method}")
        solver_params = teaser.RobustRegistrationSolver.Params()                                   # RN:112-124
        solver_params.cbar2 = 1.0
        solver_params.noise_bound = 0.2
        solver_params.estimate_scaling = False
        solver_params.inlier_selection_mode = teaser.RobustRegistrationSolver.INLIER_SELECTION_MODE.PMC_EXACT
        solver_params.rotation_tim_graph = teaser.RobustRegistrationSolver.INLIER_GRAPH_FORMULATION.CHAIN
        solver_params.rotation_estimation_algorithm = teaser.RobustRegistrationSolver.ROTATION_ESTIMATION_ALGORITHM.GNC_TLS
        solver_params.rotation_gnc_factor = 1.4
        solver_params.rotation_max_iterations = 10000
        solver_params.rotation_cost_threshold = 1e-16
        solver = teaser.RobustRegistrationSolver(solver_params)                                    # RN:125
        solution = solver.solve_rows(src.to(torch.float64).contiguous(), tgt.to(torch.float64).contiguous())   # RN:127-128
        teaser_pose = np.eye(4)                                                                    # RN:129-131
        teaser_pose[:3, :3] = solution.rotation
        teaser_pose[:3, 3] = solution.translation
        if not run_icp:
            return teaser_pose, None
        teaser_pose = orthogonalize_rotation(teaser_pose)                                          # RN:145-148
        sigma = self.config.adaptive_threshold.initial_threshold                                   # RN:150
        if method == "vfm":
            vhm = c["voxel_hash_map"]                                                              # RN:135-136: the same kept points
            voxel_scan = c["voxel_scan_xyz"].cpu().numpy()                                         # RN:139-141
            pose = register_frame(points=voxel_scan, voxel_map=vhm if not vhm.empty() else vhm.xyz_map(), initial_guess=teaser_pose,
                                  max_correspondance_distance=3 * sigma, kernel=sigma / 3)         # RN:151-155
        else:
            from .icp import _grid_of, register_frame_on_grid
            voxel_hash_map = get_voxel_hash_map(self.config)                                       # RN:135-136
            voxel_hash_map.add_points(map_xyz)
            voxel_scan = self._voxel_scan(raw_xyz, self.config.mapping.voxel_size)                 # RN:139-141
            pose = register_frame_on_grid(voxel_scan, _grid_of(voxel_hash_map), teaser_pose, 3 * sigma, sigma / 3)   # RN:151-155
        return teaser_pose, pose

    def baseline_row_pairs(self, voxel_map, raw_scan, method: str = "fpfh") -> dict:
        """RN:282-310 on the device: the baseline's correspondences, the scan's two voxel levels, the 3-D hash map of
        ``voxel_map[:, :3]`` in its ``point_cloud()`` order, the two 1-NN queries and the 1 mm filter.  Returns dict(voxel_scan [S, 3],
        voxel_map_3d [M, 3], pairs [K', 2] int64 (rows of the two), voxel_hash_map) -- device tensors."""
        from .neighbors import KDTree
        vm, scan = np.asarray(voxel_map), np.asarray(raw_scan)
        if vm.ndim != 2 or vm.shape[1] < 3 or scan.ndim != 2 or scan.shape[1] < 3:
            raise ValueError("Invalid shape")
        vs = self.config.mapping.voxel_size
        map_xyz = np.ascontiguousarray(vm[:, :3])
        raw_xyz = torch.from_numpy(np.ascontiguousarray(scan[:, :3], dtype=np.float64)).cuda()
        src, tgt = self._baseline_correspondences_device(map_xyz, raw_xyz, method, False)         # RN:282
        voxel_scan = self._voxel_scan(raw_xyz, vs)                                                 # RN:289-290
        voxel_hash_map = get_voxel_hash_map(self.config)                                           # RN:291-292
        voxel_hash_map.add_points(map_xyz)
        voxel_map_3d = voxel_hash_map.point_cloud_device()                                         # RN:293
        if voxel_map_3d is None or voxel_scan.shape[0] == 0:
            raise ValueError("Found array with 0 sample(s) while a minimum of 1 is required")      # (sklearn's, from RN:295-296)
        src_idx, src_dist = KDTree(voxel_scan, metric="euclidean").query_device(src)               # RN:295, 297
        tgt_idx, tgt_dist = KDTree(voxel_map_3d, metric="euclidean").query_device(tgt)             # RN:296, 298
        pairs = filter_recovered_rows(src_idx, src_dist, tgt_idx, tgt_dist)                        # RN:301-310
        return dict(voxel_scan=voxel_scan, voxel_map_3d=voxel_map_3d, pairs=pairs, voxel_hash_map=voxel_hash_map)

    def _ransac_registration_baseline(self, voxel_map, raw_scan, method: str, run_icp: bool):
        """RN:282-357 for a baseline descriptor, line for line, with the clouds on the device between the steps.  The correspondence
        points are voxel MEANS (``extract_fpfh_features``), so the row recovery of RN:295-310 does real work here: only a mean over a
        single point is a row of the voxelised cloud.  Fewer than 3 surviving pairs give Open3D's default result (the identity)."""
        from .icp import _grid_of, register_frame_on_grid
        r = self.baseline_row_pairs(voxel_map, raw_scan, method)
        voxel_scan, voxel_map_3d, voxel_hash_map, pairs = r["voxel_scan"], r["voxel_map_3d"], r["voxel_hash_map"], r["pairs"]
        pcd_src = o3d.geometry.PointCloud()
        pcd_src.points = o3d.utility.Vector3dVector(o3d.utility.DeviceArray(voxel_scan))
        pcd_tgt = o3d.geometry.PointCloud()
        pcd_tgt.points = o3d.utility.Vector3dVector(o3d.utility.DeviceArray(voxel_map_3d))
        coors = o3d.utility.Vector2iVector(o3d.utility.DeviceArray(pairs.to(torch.int32)))
        result = o3d.pipelines.registration.registration_ransac_based_on_correspondence(
            pcd_src, pcd_tgt, coors, self.max_correspondence_distance,
            o3d.pipelines.registration.TransformationEstimationPointToPoint(False), ransac_n=3,
            criteria=o3d.pipelines.registration.RANSACConvergenceCriteria(self.ransac_iterations, 1))      # RN:319-327
        ransac_pose = np.array(result.transformation)
        if run_icp:
            ransac_pose = orthogonalize_rotation(ransac_pose)                                      # RN:331-336
            sigma = self.config.adaptive_threshold.initial_threshold                               # RN:339
            pose = register_frame_on_grid(voxel_scan, _grid_of(voxel_hash_map), ransac_pose, 3 * sigma, sigma / 3)   # RN:340-344
            return ransac_pose, pose
        return ransac_pose, None

    def icp_registration(self, voxel_map, raw_scan, initial_pose=None, dist=3):
        """RN:359-394: point-to-point ICP of a scan against a map, both voxelised the way the node does it -- the ground truth of the
        evaluation loop (RN:646) and its vanilla-ICP row (RN:929, ``dist=7``).  The scan is down-sampled at 0.5 x and then 1.0 x the
        map's voxel size (RN:361-362); the map is a fresh ``get_voxel_hash_map(config)`` filled with ``voxel_map`` (RN:364-365).

        3-column clouds never build that container: the map goes from the upload into ``vfm_icp_grid_build`` with the config's
        points-per-voxel cap (the grid ``register_frame`` would build from the container's ``point_cloud()``: same voxels, same kept
        points, same order inside a voxel), the scan's two levels run on the device, and the 3-D loop of ``vfmreg.icp`` does the rest.
        Other widths call ``register_frame`` with ``src_`` / ``tgt_`` as RN:382-389 does and return the pose (the correspondence
        publisher of RN:392 is out of scope).  A ``MapHandle`` is taken wherever an array is; its grid stays with it between calls."""
        from .icp import VoxelGridDevice, _grid_of, register_frame_on_grid
        from .mapping import VoxelHashMap
        vs = self.config.mapping.voxel_size
        scan = np.asarray(raw_scan)
        if scan.ndim != 2 or scan.shape[1] < 3:
            raise ValueError("Invalid shape")
        handle = voxel_map if isinstance(voxel_map, MapHandle) else None
        vm = None if handle is not None else np.asarray(voxel_map)
        if vm is not None and (vm.ndim != 2 or vm.shape[1] < 3):
            raise ValueError("Invalid shape")
        map_cols = handle.cols if handle is not None else vm.shape[1]
        sigma = self.config.adaptive_threshold.initial_threshold                          # RN:372
        if initial_pose is None:
            initial_pose = np.eye(4)                                                      # RN:373-374
        initial_pose = np.ascontiguousarray(initial_pose, dtype=np.float64)
        if scan.shape[1] == 3 and map_cols == 3:
            raw_xyz = torch.from_numpy(np.ascontiguousarray(scan, dtype=np.float64)).cuda()
            xyz = self._voxel_scan(raw_xyz, vs)                                           # RN:361-362
            if handle is not None:
                grid = _grid_of(handle.voxel_hash_map)
            else:                                                                         # RN:364-365 without the container
                m_xyz = torch.from_numpy(np.ascontiguousarray(vm, dtype=np.float64)).cuda()
                grid = VoxelGridDevice.from_device(m_xyz, vs, self.config.mapping.max_points_per_voxel)
            if not VoxelHashMap.quiet:
                print(f"Map size: {grid.n_kept}, Scan size: {xyz.shape[0]}")             # RN:368
            return register_frame_on_grid(xyz, grid, initial_pose, dist * sigma, sigma / dist)   # RN:376-380
        downsample_scan = voxel_down_sample(scan, vs * 0.5)                               # RN:361
        voxel_scan = voxel_down_sample(downsample_scan, vs * 1.0)                         # RN:362
        if handle is not None:
            voxel_hash_map = handle.voxel_hash_map
        else:
            voxel_hash_map = get_voxel_hash_map(self.config)                              # RN:364-365
            voxel_hash_map.add_points(vm)
        if not VoxelHashMap.quiet:
            kept = sum(len(x) for _, x in (voxel_hash_map._chunks.get("3") or voxel_hash_map._chunks.get("n") or []))
            print(f"Map size: {kept}, Scan size: {voxel_scan.shape[0]}")                  # RN:367-368 (the kept rows: no download)
        if scan.shape[1] == 3:
            return register_frame(points=voxel_scan, voxel_map=voxel_hash_map, initial_guess=initial_pose,
                                  max_correspondance_distance=dist * sigma, kernel=sigma / dist)     # RN:376-380
        src_, tgt_ = np.array([[0, 0, 0]]), np.array([[0, 0, 0]])                         # RN:382
        out = register_frame(points=voxel_scan, voxel_map=voxel_hash_map, initial_guess=initial_pose,
                             max_correspondance_distance=dist * sigma, kernel=sigma / dist, src_=src_, tgt_=tgt_)   # RN:383-389
        return out[0] if isinstance(out, tuple) else out

    _LEARNED = ("dip", "gedi", "fcgf", "gcl", "spinnet")

    def compute_correspondences(self, voxel_map, raw_scan, method: str, mutual_filter: bool = False):
        """RN:427-547: baseline descriptors of the scan and of the map, matched by find_correspondences(n_points=5000); returns
        (down_scan[i0], down_map[i1]).  'fpfh' runs extract_fpfh_features(., 0.1) on the GPU (csrc/fpfh.hip).  The map's features
        are kept in ``map_descriptor_cache[method]`` as in the reference, and reused only for a map of the same shape, dtype and
        ``_fingerprint`` (a non-contiguous map is not cached)."""
        vm = np.asarray(voxel_map)
        if method == "fpfh" and (vm.ndim != 2 or vm.shape[1] < 3):
            raise ValueError("Invalid shape")
        scan = np.asarray(raw_scan)
        raw_xyz = torch.from_numpy(np.ascontiguousarray(scan[:, :3], dtype=np.float64)).cuda() if method == "fpfh" else None
        src, tgt = self._baseline_correspondences_device(vm, raw_xyz, method, mutual_filter)
        return src.cpu().numpy(), tgt.cpu().numpy()

    def _baseline_correspondences_device(self, vm: np.ndarray, raw_xyz: torch.Tensor, method: str, mutual_filter: bool):
        """``compute_correspondences`` with the scan's coordinates (n x 3 fp64) on the device and both results left there.  The map's
        features are kept twice: as numpy in ``map_descriptor_cache`` (the reference's attribute) and on the device for the matching."""
        if method in self._LEARNED:
            raise NotImplementedError(f"{method}: the learned baselines need their trained weights and are out of scope")
        if method != "fpfh":
            raise ValueError(f"Invalid method: {method}")
        fp = _fingerprint(vm)
        key = (vm.shape, vm.dtype.str, fp) if fp is not None else None
        kept = self._map_descriptor_device.get(method)
        if not (key is not None and kept is not None and kept[0] == key and method in self.map_descriptor_cache
                and self._map_descriptor_keys.get(method) == key):
            kept = None
        down_scan, feats_scan = extract_fpfh_features_device(raw_xyz, .1)
        if kept is None:
            m_xyz = torch.from_numpy(np.ascontiguousarray(vm[:, :3], dtype=np.float64)).cuda()
            down_map, feats_map = extract_fpfh_features_device(m_xyz, .1)
            kept = (key, down_map, feats_map.float())
            if key is not None:
                self.map_descriptor_cache[method] = (down_map.cpu().numpy(), feats_map.cpu().numpy())
                self._map_descriptor_keys[method] = key
                self._map_descriptor_device[method] = kept
        if key is None:
            self.map_descriptor_cache.pop(method, None)
            self._map_descriptor_keys.pop(method, None)
            self._map_descriptor_device.pop(method, None)
        corrs_scan, corrs_map = find_correspondences_device(feats_scan.float(), kept[2], n_points=5000, mutual_filter=mutual_filter)
        return down_scan[corrs_scan], kept[1][corrs_map]

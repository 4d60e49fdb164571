"""Row F4: the evaluation harness around the accelerated path -- map accumulation, error and recall
bookkeeping of ``RegistrationNode.make_step`` (registration_node.py:548-989), ``compute_errors`` /
``compute_success_rate`` (RN:997-1025) and the summary of print_errors.py:8-36.  Pure host
orchestration (as in the reference); the heavy steps it calls (voxel_down_sample, transform_pcl,
ransac_registration, register_frame) run on the GPU.

Scenes (row F3): the reference stores processed scenes as HDF5 (prepare_scenes.py:16-47, read_h5.py:17-49):
``/map/<seq>/pose/<jjj>`` f64[4,4], ``/map/<seq>/point_cloud/<jjj>`` f32[n, 3+C], ``/scans/<seq>/{pose, point_cloud}``,
rows = [x, y, z, d0..dC-1].  ``save_scene`` / ``read_scenes`` write and read that file format itself (``vfmreg.h5lite``:
h5py is not installed; the subset of HDF5 those h5py calls produce, verified against libhdf5's own tools and files);
a path ending in ``.npz`` selects a numpy container with the same key paths instead (cache format of round 1).
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import h5lite
from .registration import RegistrationNode
from .utils import TREE_COLOURS, filter_map_semantic, transform_pcl
from .voxelization import voxel_down_sample

SUCCESS_THRESHOLDS = [(.3, 15), (.6, 1.5), (2, 5)]  # (RTE m, RRE deg): PointDSC, GCL, D3Feat/SpinNet (RN:973-977)


def save_scene(filename, sequences: List[str], map_poses, map_point_clouds, seq_poses, seq_point_clouds) -> None:
    """prepare_scenes.save_scene (PS:16-47): the same groups and datasets, as an HDF5 file."""
    filename = Path(filename)
    filename.parent.mkdir(parents=True, exist_ok=True)
    data = {}
    for j in range(len(map_poses)):
        data[f"map/{sequences[0]}/pose/{j:03}"] = np.asarray(map_poses[j])
        data[f"map/{sequences[0]}/point_cloud/{j:03}"] = np.asarray(map_point_clouds[j])
    for j in range(len(seq_poses)):
        if seq_poses[j] is None:  # this sequence has no hits (PS:41-42)
            continue
        data[f"scans/{sequences[j + 1]}/pose"] = np.asarray(seq_poses[j])
        data[f"scans/{sequences[j + 1]}/point_cloud"] = np.asarray(seq_point_clouds[j])
    if filename.suffix == ".npz":
        np.savez(filename, **data)
        return
    tree: dict = {"map": {sequences[0]: {"pose": {}, "point_cloud": {}}}, "scans": {}}   # PS:30-38: groups exist even when empty
    for key, arr in data.items():
        node = tree
        parts = key.split("/")
        for part in parts[:-1]:
            node = node.setdefault(part, {})
        node[parts[-1]] = arr
    h5lite.write_h5(filename, tree)


def read_scenes(filename) -> Dict[str, list]:
    """read_h5.read_scenes (read_h5.py:17-49): dict(map_poses, map_point_clouds, map_clip, scene_poses,
    scene_point_clouds) + scene_sequences (the scan group names, in the order the arrays are listed)."""
    filename = Path(filename)
    if filename.suffix == ".npz":
        z = np.load(filename)
        tree: dict = {}
        for key in sorted(z.files):
            node = tree
            parts = key.split("/")
            for part in parts[:-1]:
                node = node.setdefault(part, {})
            node[parts[-1]] = z[key]
    else:
        tree = h5lite.read_h5(filename)
    map_poses, map_point_clouds, map_clip = [], [], []
    for key in tree["map"]:  # there should be only one key corresponding to the sequence name (read_h5.py:22-24)
        g = tree["map"][key]
        for pose, cloud in zip(g["pose"].values(), g["point_cloud"].values()):
            map_poses.append(pose)
            map_point_clouds.append(cloud)
        if "clip" in g:
            map_clip.extend(g["clip"].values())
    scans = tree.get("scans", {})
    return {
        "map_poses": map_poses,
        "map_point_clouds": map_point_clouds,
        "map_clip": map_clip,
        "scene_poses": [scans[s]["pose"] for s in scans],
        "scene_point_clouds": [scans[s]["point_cloud"] for s in scans],
        "scene_sequences": list(scans),
    }


def build_local_map(map_poses, map_point_clouds, voxel_size: float = .25, n_descriptors: int = 384) -> np.ndarray:
    """RN:556-580: drop rows without descriptors (sum <= 0, RN:562), voxelise each cloud, move it into
    the map frame, concatenate, voxelise again (split in two halves above 1e6 points, RN:568-578)."""
    local = []
    for pose, pcl in zip(map_poses, map_point_clouds):
        pcl = pcl[np.sum(pcl[:, 3:], axis=1) > 0]
        pcl = voxel_down_sample(pcl, voxel_size).astype(pcl.dtype)
        local.append(transform_pcl(pcl, pose))
    m = np.concatenate(local, axis=0).astype(np.float32)
    if m.shape[0] > 1000000:
        mean_3d = np.mean(m[:, :3], axis=0)
        a = voxel_down_sample(m[m[:, 0] > mean_3d[0]], voxel_size).astype(m.dtype)
        b = voxel_down_sample(m[m[:, 0] <= mean_3d[0]], voxel_size).astype(m.dtype)
        m = np.concatenate([a, b], axis=0)
    else:
        m = voxel_down_sample(m, voxel_size).astype(m.dtype)
    return m[:, :3 + n_descriptors]


class Evaluation:
    """Error lists per method + the recall table (RN:86-89, 961-1025)."""

    def __init__(self):
        self.rot_errors: Dict[str, List[float]] = {}
        self.trans_errors: Dict[str, List[float]] = {}
        self.points_in_map: List[int] = []

    def compute_errors(self, pose: np.ndarray, gt_pose: np.ndarray, method: str) -> Tuple[float, float]:
        R, R_gt = pose[:3, :3], gt_pose[:3, :3]
        rot_error = abs(np.arccos(min(max(((R.T @ R_gt).trace() - 1) / 2, -1.0), 1.0)))
        rot_error = float(np.rad2deg(rot_error))
        trans_error = float(np.linalg.norm(pose[:3, 3] - gt_pose[:3, 3]))
        self.rot_errors.setdefault(method, []).append(rot_error)
        self.trans_errors.setdefault(method, []).append(trans_error)
        return trans_error, rot_error

    def compute_success_rate(self, method: str, translation_threshold, rotation_threshold) -> float:
        ok_t = np.array(self.trans_errors[method]) < translation_threshold
        ok_r = np.array(self.rot_errors[method]) < rotation_threshold
        return float(np.mean(ok_t & ok_r))

    def error_string(self) -> str:
        """The rows print_errors.main writes to error.txt (print_errors.py:27-56): per method
        ``RTE mean+-std & RRE mean+-std & recall & recall after ICP`` at the (0.6 m, 1.5 deg) threshold; ``*_icp`` rows
        are listed only for the vfm methods."""
        rot = {k: np.array(v) for k, v in self.rot_errors.items()}
        trans = {k: np.array(v) for k, v in self.trans_errors.items()}
        success = {m: np.logical_and(trans[m] < .6, rot[m] < 1.5) for m in rot}
        out = ""
        for method, rot_error in rot.items():
            if 'icp' in method and 'vfm' not in method:
                continue
            trans_error = trans[method]
            recall = success[method]
            out += f"{method}\t{np.round(np.mean(trans_error), 2):.2f}$\\pm${np.round(np.std(trans_error), 2):.2f}"
            out += f" & {np.round(np.mean(rot_error), 2):.2f}$\\pm${np.round(np.std(rot_error), 2):.2f}"
            out += f" & {np.round(np.mean(recall) * 100, 2):.2f}"
            recall = success.get(f"{method}_icp", recall)
            out += f" & {np.round(np.mean(recall) * 100, 2):.2f}"
            out += "\n"
        return out

    def summary(self) -> str:
        lines = ["=" * 80]
        for method, e in self.rot_errors.items():
            lines.append(f"Rotation error ({method:<20}): {np.mean(e):.3f} ± {np.std(e):.3f}")
        lines.append("-" * 80)
        for method, e in self.trans_errors.items():
            lines.append(f"Translat error ({method:<20}): {np.mean(e):.3f} ± {np.std(e):.3f}")
        lines.append("-" * 80)
        head = f"{'':<20}: " + "".join(f"{t[0]:>3}, {t[1]:<3} | " for t in SUCCESS_THRESHOLDS)
        lines.append(head[:-2])
        for method in self.rot_errors:
            row = f"{method:<20}: " + "".join(f"{100 * self.compute_success_rate(method, *t):>8.2f} | "
                                              for t in SUCCESS_THRESHOLDS)
            lines.append(row[:-2])
        lines.append("=" * 80)
        return "\n".join(lines)


def evaluate_scene(scene: Dict[str, list], node: Optional[RegistrationNode] = None,
                   evaluation: Optional[Evaluation] = None, run_icp: bool = True, icp_ground_truth: bool = False,
                   icp_baseline: bool = False, baselines=(), cluster_removal_prob: float = 0.0, remove_classes=None,
                   pca=None, teaser: bool = False, vfm_candidates: int = 1) -> Evaluation:
    """The VFM + RANSAC (+ ICP) branch of make_step for one scene (RN:587-589, 593, 860-882, 943-951):
    every scan is registered against the accumulated map with the identity as initial guess and
    compared with its ground-truth pose.  ``icp_ground_truth``: that pose is the stored one refined by ICP against the map, as the
    reference does it (RN:645-646), for every row; ``icp_baseline``: the vanilla-ICP row ``icp`` of RN:929 (``dist=7``) joins the
    table.  Both are off by default (the stored pose, no ``icp`` row).  ``baselines`` (default ``()``): the baseline descriptors of
    RN:867-874 to run before ``vfm`` -- ``("fpfh",)`` adds the rows ``fpfh_ransac`` and, with ``run_icp``, ``fpfh_ransac_icp``; the node
    must have been created with the same ``baseline_methods``.  The map's baseline features are computed at the first scan of the
    scene and kept for the others (RN:876-877).

    ``cluster_removal_prob`` (default 0.0: nothing changes): above 0 the seasonal-change experiment of RN:684-792 runs in front of every
    scan's registration -- ``utils.filter_map_semantic`` on the scene's map with ``remove_classes`` (default ``[utils.TREE_COLOURS]``),
    this chance and one ``np.random.RandomState(42)`` per scene shared by its scans (RN:584); the scan is registered against the
    filtered map, the map's baseline features are dropped at every scan (RN:876-877) and ``points_in_map`` records the filtered size
    (RN:792).  ``pca``: what has ``run_pca`` (an ``ImageFeatureGenerator`` or a ``pca.DescriptorPCA``, e.g. one whose ``fit_pca[3]`` holds
    the reference's fit); default a fresh ``pca.DescriptorPCA``, fitted on the first scan's map.

    ``teaser`` (default False: the result set is unchanged): the TEASER rows of RN:895-904 behind the RANSAC rows -- ``fpfh_teaser`` /
    ``fpfh_teaser_icp`` if ``"fpfh"`` is among ``baselines``, ``vfm_teaser`` / ``vfm_teaser_icp`` always (``*_icp`` with ``run_icp``).

    ``vfm_candidates`` (default 1: the rows are unchanged): map candidates per scan point of the VFM rows, passed to the node this
    function creates (``RegistrationNode(vfm_candidates=...)``; a ``node`` that is handed in keeps its own)."""
    node = node or RegistrationNode(cache_map=True, baseline_methods=tuple(baselines),   # local_map below is built here and never edited: one map per scene (RN:556-589)
                                    vfm_candidates=vfm_candidates)
    ev = evaluation or Evaluation()
    n_desc = scene["map_point_clouds"][0].shape[1] - 3
    local_map = build_local_map(scene["map_poses"], scene["map_point_clouds"], n_descriptors=n_desc)
    # the 3-D map both ICP calls register against: built once per scene and kept with the handle (the reference rebuilds it per call)
    icp_map = node.set_map(np.ascontiguousarray(local_map[:, :3])) if (icp_ground_truth or icp_baseline) else None
    filtering = cluster_removal_prob > 0                                             # RN:684
    if filtering:
        from .pca import DescriptorPCA
        pca = pca if pca is not None else DescriptorPCA()
        remove_classes = [TREE_COLOURS] if remove_classes is None else remove_classes
        rng_cluster_removal = np.random.RandomState(seed=42)                         # RN:584
        scene_local_map = local_map
    for i, (gt_pose, point_cloud) in enumerate(zip(scene["scene_poses"], scene["scene_point_clouds"])):
        point_cloud = voxel_down_sample(point_cloud, .1).astype(point_cloud.dtype)   # RN:593
        if icp_ground_truth:
            gt_pose = node.icp_registration(icp_map, point_cloud[:, :3], np.asarray(gt_pose))   # RN:645-646
        initial_pose = np.eye(4)                                                     # RN:858
        point_cloud = transform_pcl(point_cloud, initial_pose)                       # RN:863
        results = {}
        if filtering:                                                                # RN:693-792, from the whole map at every scan (RN:673)
            local_map, _, _ = filter_map_semantic(scene_local_map, pca, remove_classes, cluster_removal_prob, rng_cluster_removal)
            node.invalidate_map()                                                    # (the kept map is another one at every scan)
        if i == 0 or filtering:
            node.clear_map_descriptors()                                             # RN:876-877
        for method in baselines:                                                     # RN:867-883, in the reference's order
            results[f"{method}_ransac"], results[f"{method}_ransac_icp"] = node.ransac_registration(local_map, point_cloud, method, run_icp)
        results["vfm_ransac"], results["vfm_ransac_icp"] = node.ransac_registration(local_map, point_cloud, "vfm", run_icp)
        if teaser:                                                                   # RN:895-904
            for method in (("fpfh",) if "fpfh" in baselines else ()) + ("vfm",):
                results[f"{method}_teaser"], results[f"{method}_teaser_icp"] = node.teaser_registration(local_map, point_cloud, method, run_icp)
        if icp_baseline:
            results["icp"] = node.icp_registration(icp_map, point_cloud[:, :3], dist=7)          # RN:929
        for k, v in results.items():
            if v is None:
                continue
            ev.compute_errors(np.asarray(gt_pose), v @ initial_pose, k)              # RN:943-947
        ev.points_in_map.append(local_map.shape[0])
    return ev

"""The FPFH baseline descriptor of the reference (src/vfm-reg/src/vfm_reg/descriptors.py:19-44), on the GPU.

``extract_fpfh_features`` is the reference's function body on the Open3D stand-ins of ``vfmreg.o3d`` (numpy in, numpy out);
``extract_fpfh_features_device`` is the same chain on device tensors.  Both run csrc/fpfh.hip: normals from a hybrid search of
radius 2 voxel_size / 30 neighbours, an averaging voxel down-sample, FPFH from a hybrid search of radius 5 voxel_size / 100
neighbours.  The learned baselines of that module (DIP, GeDi, FCGF, GCL, SpinNet) need weights and are out of scope.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from . import o3d, ops


def extract_fpfh_features(pcl, voxel_size: float, normalize: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """descriptors.py:19-44: (down-sampled points M x 3, FPFH features M x 33), fp64 numpy."""
    pcd = o3d.geometry.PointCloud()
    pcd.points = o3d.utility.Vector3dVector(np.asarray(pcl)[:, :3])

    # Compute normals
    radius_normal = voxel_size * 2
    pcd.estimate_normals(o3d.geometry.KDTreeSearchParamHybrid(radius=radius_normal, max_nn=30))

    # Voxelize
    pcd = pcd.voxel_down_sample(voxel_size)

    # Compute FPFH features
    radius_feature = voxel_size * 5
    features = o3d.pipelines.registration.compute_fpfh_feature(
        pcd, o3d.geometry.KDTreeSearchParamHybrid(radius=radius_feature, max_nn=100))

    features = np.array(features.data).T

    if normalize:
        features = features / (np.linalg.norm(features, axis=1, keepdims=True) + 1e-6)

    return np.array(pcd.points), features


def extract_fpfh_features_device(xyz: torch.Tensor, voxel_size: float, normalize: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """The same on an N x 3 fp64 device tensor: (down-sampled points M x 3, features M x 33), both on the device.  One read-back
    (the voxel count of the down-sample)."""
    if xyz.dim() != 2 or xyz.shape[1] < 3:
        raise ValueError("Invalid shape")
    pts = xyz[:, :3].to(torch.float64).contiguous()
    if pts.shape[0] == 0:
        return pts, torch.zeros((0, 33), dtype=torch.float64, device=pts.device)
    nbrs = ops.fpfh_search(pts, voxel_size * 2, 30)
    normals = ops.fpfh_normals(pts, nbrs)
    down, dn = ops.fpfh_voxel_down_sample(pts, voxel_size, normals)
    nbrs = ops.fpfh_search(down, voxel_size * 5, 100)
    feats = ops.fpfh_fpfh(ops.fpfh_spfh(down, dn, nbrs), nbrs)
    if normalize:
        feats = feats / (torch.linalg.norm(feats, dim=1, keepdim=True) + 1e-6)
    return down, feats

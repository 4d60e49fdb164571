"""Seeded inputs shared by the ICP-grid tests (tests/test_icp_registration_host.py, tests/test_gpu_icp_registration.py)."""
import numpy as np


def crowded_cloud(n: int, voxel_size: float, seed: int) -> np.ndarray:
    """n points over ~n / 12 cells of which a fifth are five times as likely as the rest (~33 points each), negative coordinates,
    and a share of the points exactly on voxel faces (whole multiples of the voxel size, -0.0 included), in random order."""
    rng = np.random.default_rng(seed)
    if n == 0:
        return np.zeros((0, 3))
    cells = max(n // 12, 1)
    side = max(int(round(cells ** (1 / 3))), 1)
    centres = rng.integers(-side, side + 1, (cells, 3))
    w = np.where(np.arange(cells) < max(cells // 5, 1), 5.0, 1.0)
    pick = rng.choice(cells, n, p=w / w.sum())
    p = (centres[pick] + rng.uniform(0, 1, (n, 3))) * voxel_size
    face = np.flatnonzero(rng.random(n) < 0.1)
    p[face, rng.integers(0, 3, len(face))] = centres[pick[face], 0] * voxel_size
    p[::97, 1] = -0.0
    return np.ascontiguousarray(p[rng.permutation(n)])


def keys_of(p: np.ndarray, voxel_size: float) -> np.ndarray:
    v = np.trunc(p / voxel_size).astype(np.int64) + (1 << 20)
    return (v[:, 0] << 42) | (v[:, 1] << 21) | v[:, 2]


def crowded_share(p: np.ndarray, voxel_size: float, cap: int) -> float:
    """share of the voxels that hold more than ``cap`` points"""
    _, counts = np.unique(keys_of(p, voxel_size), return_counts=True)
    return float((counts > cap).mean())


def oracle_grid(p: np.ndarray, voxel_size: float, cap: int):
    """(keys, start, pts) of the grid register_frame builds from VoxelHashMap(cap).add_points(p).point_cloud(), from the oracle's pieces
    (cap 0 = no cap: the oracle's container with a cap no voxel reaches)."""
    from oracle import oracle as orc
    if len(p) == 0:
        return np.zeros(0, np.int64), np.zeros(1, np.int32), np.zeros((0, 3))
    cloud = p[orc.voxel_hash_map_points(p, voxel_size, cap if cap else len(p))]
    return orc.voxel_grid_csr(cloud, voxel_size)

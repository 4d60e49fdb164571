"""CPU checks for ``RegistrationNode.icp_registration`` and the device-built ICP grid (``vfm_icp_grid_build``): what the library
exports, the Python signatures, and -- numpy and the oracle only -- the identity the grid build rests on:

    cap to the first K points per voxel, then stable-sort by key  ==  stable-sort by key, then the first K of every run
    ==  oracle.voxel_grid_csr of the cloud in VoxelHashMap.point_cloud() order (oracle.voxel_hash_map_points)
"""
import inspect
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.icp_grid_cases import crowded_cloud, crowded_share, keys_of, oracle_grid  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def built():
    subprocess.run([sys.executable, str(ROOT / "vfm-registration_amd" / "build.py")], check=True, stdout=subprocess.DEVNULL)
    from vfmreg import _lib
    return _lib


def test_library_exports_the_grid_build(built):
    out = subprocess.run(["nm", "-D", "--defined-only", str(built.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split()}
    assert {"vfm_icp_grid_build", "vfm_icp_grid_workspace_bytes"} <= exported
    lib = built.load()
    # sized on the host, no device needed; grows with n; argument checks come before any launch
    assert lib.vfm_icp_grid_workspace_bytes(200000) > lib.vfm_icp_grid_workspace_bytes(1000) > 0
    assert lib.vfm_icp_grid_workspace_bytes(200000) >= 200000 * (8 + 4 + 8 + 4 + 4 * 4)
    assert lib.vfm_icp_grid_build(None, -1, 1.0, 0, None, None, None, None, None, 0, None) == -1
    assert lib.vfm_icp_grid_build(None, 10, 0.0, 0, None, 1, None, 1, None, 0, None) == -1
    assert lib.vfm_icp_grid_build(1, 10, 1.0, 20, 1, 1, 1, 1, 1, 16, None) == -1 and b"workspace" in lib.vfm_last_error()


def test_signatures():
    from vfmreg.evaluation import evaluate_scene
    from vfmreg.icp import VoxelGridDevice
    from vfmreg.registration import RegistrationNode
    sig = inspect.signature(RegistrationNode.icp_registration)
    assert list(sig.parameters) == ["self", "voxel_map", "raw_scan", "initial_pose", "dist"]      # RN:359
    assert sig.parameters["initial_pose"].default is None and sig.parameters["dist"].default == 3
    ev = inspect.signature(evaluate_scene).parameters
    assert ev["icp_ground_truth"].default is False and ev["icp_baseline"].default is False
    fd = inspect.signature(VoxelGridDevice.from_device).parameters
    assert list(fd) == ["xyz64", "voxel_size", "max_points_per_voxel"] and fd["max_points_per_voxel"].default == 0
    assert list(inspect.signature(VoxelGridDevice.__init__).parameters) == ["self", "points", "voxel_size"]


def cap_then_sort(p, vs, K):
    """VoxelHashMap::AddPoints' rule (the first K points of every voxel, in input order), then the stable sort"""
    keys = keys_of(p, vs)
    seen = {}
    kept = []
    for i, k in enumerate(keys.tolist()):
        c = seen.get(k, 0)
        if K == 0 or c < K:
            kept.append(i)
            seen[k] = c + 1
    kept = np.asarray(kept, dtype=np.int64)
    order = np.argsort(keys[kept], kind="stable")
    return kept[order]


def sort_then_cap(p, vs, K):
    """what vfm_icp_grid_build does: stable sort, then the first K positions of every run of equal keys"""
    keys = keys_of(p, vs)
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    i = np.arange(len(ks))
    keep = np.ones(len(ks), dtype=bool) if K == 0 else (i < K) | (ks[np.maximum(i - K, 0)] != ks)
    return order[keep]


@pytest.mark.parametrize("n,vs,K,seed", [(1000, 1.0, 20, 1), (1000, 0.5, 1, 2), (20000, 0.5, 20, 3), (20000, 1.0, 1, 4), (5000, 1.0, 0, 5),
                                         (1, 1.0, 20, 6)])
def test_cap_then_sort_equals_sort_then_cap_equals_the_grid_of_the_map(n, vs, K, seed):
    p = crowded_cloud(n, vs, seed)
    if K == 20 and n >= 1000:
        assert crowded_share(p, vs, 20) >= 0.05              # the cap is really at work
    a, b = cap_then_sort(p, vs, K), sort_then_cap(p, vs, K)
    np.testing.assert_array_equal(a, b)
    assert K == 0 or len(b) < n or n < 1000
    # the grid register_frame builds from the container's point_cloud()
    keys, start, pts = oracle_grid(p, vs, K)
    np.testing.assert_array_equal(pts, p[b])
    ks = keys_of(p[b], vs)
    uniq, first = np.unique(ks, return_index=True)
    np.testing.assert_array_equal(keys, uniq)
    np.testing.assert_array_equal(start, np.r_[first, len(ks)].astype(np.int32))

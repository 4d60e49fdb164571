"""FPFH on the GPU (csrc/fpfh.hip) against the numpy oracle (tests/fpfh_oracle.py): neighbour rows exactly, normals to 1e-9 with
the sign, the down-sample bit-equal, SPFH / FPFH to 1e-9 except where a pair feature sits within 1e-9 of a bin edge; the
reference-shaped API (o3d stand-ins, descriptors, RegistrationNode.compute_correspondences) and an end-to-end registration."""
import numpy as np
import pytest
import torch

from tests import fpfh_oracle as fo

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def gpu_search(pts, r, k):
    from vfmreg import ops
    out = ops.fpfh_search(dev(pts).reshape(-1, 3), r, k)
    torch.cuda.synchronize()
    return out["idx"].cpu().numpy(), out["d2"].cpu().numpy(), out["count"].cpu().numpy()


def assert_rows_equal(pts, r, k, brute=False):
    ref = (fo.hybrid_search_brute if brute else fo.hybrid_search)(pts, r, k)
    got = gpu_search(pts, r, k)
    np.testing.assert_array_equal(got[2], ref[2])
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(got[1], ref[1])
    return ref


@pytest.fixture(scope="module")
def scene():
    from vfmreg import synth
    return synth.make_structured_scene(20000, 200000, seed=5)


@pytest.mark.parametrize("which", ["scan", "map"])
def test_search_rows_exact_on_structured_scenes(scene, which):
    pts = scene[which]
    assert_rows_equal(pts, 0.2, 30)                   # the normals' search
    down, _ = fo.voxel_down_sample(pts, 0.1)
    assert_rows_equal(down, 0.5, 100)                 # the features' search


@pytest.mark.parametrize("r", [2.0, 2.01, 1.0])
def test_search_rows_exact_on_a_lattice_with_ties(r):
    g = np.stack(np.meshgrid(*(np.arange(12.0),) * 3, indexing="ij"), -1).reshape(-1, 3) * 0.25 - 1.0
    assert_rows_equal(g, r * 0.25, 30, brute=True)


@pytest.mark.parametrize("n,k", [(5000, 30), (5000, 100), (600, 100), (1024, 1024), (1100, 1000)])
def test_search_rows_exact_in_one_dense_ball(n, k):
    rng = np.random.default_rng(n + k)
    pts = rng.uniform(-0.05, 0.05, (n, 3))
    pts[n // 2:n // 2 + n // 5] = pts[:n // 5]          # duplicates: equal distances, ordered by index
    pts[-10:] = pts[0]
    assert_rows_equal(pts, 0.5, k, brute=True)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_search_tiny_clouds(n):
    pts = np.arange(3 * n, dtype=np.float64).reshape(n, 3) * 0.01
    ref = assert_rows_equal(pts, 0.5, 30, brute=True)
    assert (ref[2] == n).all()


def test_normals_down_sample_and_features(scene):
    from vfmreg import ops
    pts = scene["scan"]
    idx, d2, cnt = fo.hybrid_search(pts, 0.2, 30)
    nv_ref = fo.estimate_normals(pts, idx, cnt)
    P = dev(pts)
    nb = ops.fpfh_search(P, 0.2, 30)
    nv = ops.fpfh_normals(P, nb).cpu().numpy()
    assert np.abs(nv - nv_ref).max() <= 1e-9
    big = np.abs(nv_ref) > 1e-6
    np.testing.assert_array_equal(np.sign(nv[big]), np.sign(nv_ref[big]))
    # the down-sample on the same normals: bit-equal
    down_ref, dn_ref = fo.voxel_down_sample(pts, 0.1, nv_ref)
    down, dn = ops.fpfh_voxel_down_sample(P, 0.1, dev(nv_ref))
    np.testing.assert_array_equal(down.cpu().numpy(), down_ref)
    np.testing.assert_array_equal(dn.cpu().numpy(), dn_ref)
    # SPFH / FPFH on the same points, normals and rows
    i, d, c = fo.hybrid_search(down_ref, 0.5, 100)
    sp_ref, near = fo.spfh(down_ref, dn_ref, i, c)
    f_ref, fnear = fo.fpfh(sp_ref, i, d, c, near)
    D, DN = dev(down_ref), dev(dn_ref)
    nb = ops.fpfh_search(D, 0.5, 100)
    sp = ops.fpfh_spfh(D, DN, nb)
    f = ops.fpfh_fpfh(sp, nb).cpu().numpy()
    sp = sp.cpu().numpy()
    for got, ref, nr in ((sp, sp_ref, near), (f, f_ref, fnear)):
        bad = (np.abs(got - ref) > 1e-9 * np.maximum(np.abs(ref), 1.0)).any(1)
        assert not (bad & ~nr).any(), np.flatnonzero(bad & ~nr)[:10]
        assert bad.mean() < 1e-3
    # the Open3D-shaped chain gives the device chain's values
    from vfmreg import descriptors
    dp, fp_ = descriptors.extract_fpfh_features(pts, 0.1)
    dd, fd = descriptors.extract_fpfh_features_device(P, 0.1)
    np.testing.assert_array_equal(dp, dd.cpu().numpy())
    np.testing.assert_array_equal(fp_, fd.cpu().numpy())
    assert fp_.shape == (len(dp), 33)


def test_o3d_stand_ins():
    from vfmreg import o3d
    rng = np.random.default_rng(0)
    pcd = o3d.geometry.PointCloud()
    pcd.points = o3d.utility.Vector3dVector(rng.uniform(-1, 1, (3000, 3)))
    pcd.estimate_normals(o3d.geometry.KDTreeSearchParamHybrid(radius=0.2, max_nn=30))
    assert pcd.has_normals() and np.asarray(pcd.normals).shape == (3000, 3)
    down = pcd.voxel_down_sample(0.1)
    assert down.has_normals() and len(down.points) == len(down.normals) <= 3000
    feat = o3d.pipelines.registration.compute_fpfh_feature(down, o3d.geometry.KDTreeSearchParamHybrid(radius=0.5, max_nn=100))
    assert feat.dimension() == 33 and feat.num() == len(down.points)
    assert feat.data.shape == (33, feat.num())
    empty = o3d.geometry.PointCloud().voxel_down_sample(0.1)
    assert len(empty.points) == 0


@pytest.mark.parametrize("mutual", [False, True])
def test_compute_correspondences_equal_the_oracle_matcher(mutual):
    from oracle import oracle as orc
    from vfmreg import descriptors, synth
    from vfmreg.registration import RegistrationNode
    sc = synth.make_structured_scene(6000, 30000, seed=3, extent=10.0, scan_range=6.0, boxes=6, cylinders=4)
    node = RegistrationNode()
    src, tgt = node.compute_correspondences(sc["map"], sc["scan"], "fpfh", mutual_filter=mutual)
    ds, fs = descriptors.extract_fpfh_features(sc["scan"], 0.1)
    dm, fm = descriptors.extract_fpfh_features(sc["map"], 0.1)
    i0, i1 = orc.find_correspondences(fs, fm, n_points=5000, mutual_filter=mutual)
    np.testing.assert_array_equal(src, ds[i0])
    np.testing.assert_array_equal(tgt, dm[i1])


def test_map_features_are_cached_per_map():
    from vfmreg import synth
    from vfmreg.registration import RegistrationNode
    sc = synth.make_structured_scene(3000, 12000, seed=4, extent=6.0, scan_range=4.0, boxes=3, cylinders=2)
    node = RegistrationNode()
    node.compute_correspondences(sc["map"], sc["scan"], "fpfh")
    first = node.map_descriptor_cache["fpfh"][1]
    node.compute_correspondences(sc["map"], sc["scan"], "fpfh")
    assert node.map_descriptor_cache["fpfh"][1] is first                 # reused
    other = sc["map"] + np.array([0.05, 0.0, 0.0])
    node.compute_correspondences(other, sc["scan"], "fpfh")
    assert node.map_descriptor_cache["fpfh"][1] is not first             # a different map: recomputed
    np.testing.assert_array_equal(node.map_descriptor_cache["fpfh"][0], np.asarray(
        __import__("vfmreg.descriptors", fromlist=["x"]).extract_fpfh_features(other, 0.1)[0]))
    node.compute_correspondences(np.asfortranarray(sc["map"]), sc["scan"], "fpfh")   # no fingerprint: nothing kept
    assert "fpfh" not in node.map_descriptor_cache


def test_fpfh_ransac_icp_recovers_the_pose():
    from vfmreg import o3d, synth
    from vfmreg.config import load_config
    from vfmreg.icp import register_frame
    from vfmreg.mapping import get_voxel_hash_map
    from vfmreg.registration import RegistrationNode, compute_errors, orthogonalize_rotation
    sc = synth.make_structured_scene(30000, 100000, seed=2, extent=12.0, scan_range=8.0, boxes=10, cylinders=8)
    node = RegistrationNode()
    src, tgt = node.compute_correspondences(sc["map"], sc["scan"], "fpfh", mutual_filter=True)
    pcd_src, pcd_tgt = o3d.geometry.PointCloud(), o3d.geometry.PointCloud()
    pcd_src.points = o3d.utility.Vector3dVector(src)
    pcd_tgt.points = o3d.utility.Vector3dVector(tgt)
    coors = o3d.utility.Vector2iVector(np.stack([np.arange(len(src)), np.arange(len(src))], 1))
    res = o3d.pipelines.registration.registration_ransac_based_on_correspondence(
        pcd_src, pcd_tgt, coors, 0.3, o3d.pipelines.registration.TransformationEstimationPointToPoint(False), ransac_n=3,
        criteria=o3d.pipelines.registration.RANSACConvergenceCriteria(50000, 1))
    pose = orthogonalize_rotation(np.array(res.transformation))
    cfg = load_config(None, None)
    vhm = get_voxel_hash_map(cfg)
    vhm.add_points(sc["map"])
    sigma = cfg.adaptive_threshold.initial_threshold
    pose = register_frame(points=sc["scan"], voxel_map=vhm, initial_guess=pose, max_correspondance_distance=3 * sigma, kernel=sigma / 3)
    rte, rre = compute_errors(pose, sc["T_gt"])
    assert rte < 0.3 and rre < 1.5, (rte, rre, compute_errors(np.array(res.transformation), sc["T_gt"]))

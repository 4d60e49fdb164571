"""``RegistrationNode(baseline_methods=("fpfh",)).ransac_registration(map, scan, "fpfh", run_icp)`` (registration_node.py:282-357) and
``evaluate_scene(baselines=("fpfh",))`` against a re-enactment from the oracles.

The re-enactment takes the FPFH features from the GPU (``descriptors.extract_fpfh_features``, downloaded: tests/test_gpu_fpfh.py pins
them to tests/fpfh_oracle.py bit for bit; the numpy oracle needs minutes at 200 000 points) and everything after them from the CPU
oracles: ``oracle.find_correspondences``, ``oracle.voxel_down_sample`` / ``voxel_hash_map_points``, ``tests/nn3_oracle.py`` (the two
KD-tree queries and the 1 mm filter), ``oracle.ransac_corr`` with the same seed, ``oracle.orthogonalize_rotation`` and
``oracle.register_frame`` (the ICP oracle of tests/test_gpu_icp_registration.py).  Compared: the surviving pair list (equal), the
RANSAC pose (bit-equal), the refined pose (bit-equal, as that file compares the same loop)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import nn3_oracle  # noqa: E402

N_ITER = 5000


def _reenact(orc, cfg, map_xyz, scan, run_icp):
    from vfmreg import descriptors
    vs, sigma = cfg.mapping.voxel_size, cfg.adaptive_threshold.initial_threshold
    ds, fs = descriptors.extract_fpfh_features(scan, 0.1)
    dm, fm = descriptors.extract_fpfh_features(map_xyz, 0.1)
    i0, i1 = orc.find_correspondences(fs, fm, n_points=5000, mutual_filter=False)              # RN:282
    src, tgt = ds[i0], dm[i1]
    voxel_scan = orc.voxel_down_sample(orc.voxel_down_sample(scan, vs * 0.5), vs * 1.0)        # RN:289-290
    mp = np.asarray(map_xyz, dtype=np.float64)[orc.voxel_hash_map_points(map_xyz, vs, cfg.mapping.max_points_per_voxel)]   # RN:291-293
    si, sd = nn3_oracle.nearest(voxel_scan, src)                                               # RN:295-298
    ti, td = nn3_oracle.nearest(mp, tgt)
    pairs = nn3_oracle.filter_pairs(si, sd, ti, td)                                            # RN:301-309
    stats = dict(pairs=len(src), src_ok=int((sd < .001).sum()), tgt_ok=int((td < .001).sum()), both=len(pairs),
                 between=int(((sd > 0) & (sd < .001)).sum() + ((td > 0) & (td < .001)).sum()))
    if len(pairs) < 3:
        return pairs, np.eye(4), None, voxel_scan, mp, stats
    pose = orc.ransac_corr(voxel_scan, mp, pairs.astype(np.int32), 10000.0, N_ITER, seed=42).transformation   # RN:319-328
    refined = None
    if run_icp:
        pose = orc.orthogonalize_rotation(pose)                                                # RN:331-336
        refined = orc.register_frame(voxel_scan, mp, vs, pose, 3 * sigma, sigma / 3)          # RN:340-344
    return pairs, pose, refined, voxel_scan, mp, stats


@pytest.mark.parametrize("n_scan,n_map,seed", [(6000, 30000, 0), (20000, 60000, 1), (20000, 200000, 2)])
def test_fpfh_ransac_registration_equals_the_oracle_composition(n_scan, n_map, seed):
    from oracle import oracle as orc
    from vfmreg import o3d, synth
    from vfmreg.config import load_config
    from vfmreg.mapping import VoxelHashMap
    from vfmreg.registration import RegistrationNode
    VoxelHashMap.quiet = True
    cfg = load_config(None, None)
    sc = synth.make_structured_scene(n_scan, n_map, seed=seed)
    scan = orc.voxel_down_sample(sc["scan"], .1)                                               # RN:593
    map_xyz = sc["map"]
    node = RegistrationNode(cfg, ransac_iterations=N_ITER, baseline_methods=("fpfh",))
    o3d.utility.random.seed(42)
    pairs, want_ransac, want_icp, voxel_scan, mp, stats = _reenact(orc, cfg, map_xyz, scan, True)
    print(f"scene {n_scan}/{n_map} seed {seed}: {stats}")
    assert stats["both"] >= 30, stats                # a condition on the ORACLE's count: RANSAC on a handful of pairs shows nothing
    got = node.baseline_row_pairs(map_xyz, scan, "fpfh")
    np.testing.assert_array_equal(got["voxel_scan"].cpu().numpy(), voxel_scan)
    np.testing.assert_array_equal(got["voxel_map_3d"].cpu().numpy(), mp)
    np.testing.assert_array_equal(got["pairs"].cpu().numpy(), pairs)                           # the surviving pair list
    pose, pose_icp = node.ransac_registration(map_xyz, scan, "fpfh", run_icp=True)
    np.testing.assert_array_equal(pose, want_ransac)                                           # orthogonalised RANSAC pose, bit-equal
    np.testing.assert_array_equal(pose_icp, want_icp)
    raw, none = node.ransac_registration(map_xyz, scan, "fpfh", run_icp=False)
    assert none is None
    np.testing.assert_array_equal(raw, _reenact(orc, cfg, map_xyz, scan, False)[1])            # RANSAC pose as it leaves RANSAC
    # 387-column rows: the baseline reads the coordinates only (RN:282, 289, 292)
    wide_map = np.c_[map_xyz, np.ones((len(map_xyz), 4))]
    wide_scan = np.c_[scan, np.ones((len(scan), 4))]
    np.testing.assert_array_equal(node.ransac_registration(wide_map, wide_scan, "fpfh")[0], raw)
    # a default node still refuses (tests/test_gpu_api.py pins it)
    with pytest.raises(ValueError, match="Invalid method: fpfh"):
        RegistrationNode(cfg).ransac_registration(map_xyz, scan, "fpfh")


def test_fewer_than_three_surviving_pairs_give_the_identity():
    """A dense scan that is NOT pre-voxelised: every 0.1 m voxel of the FPFH down-sample averages many points, so almost no
    correspondence point is a row of the voxelised scan.  Open3D's RANSAC returns its default result below 3 pairs."""
    from oracle import oracle as orc
    from vfmreg import synth
    from vfmreg.config import load_config
    from vfmreg.mapping import VoxelHashMap
    from vfmreg.registration import RegistrationNode
    VoxelHashMap.quiet = True
    cfg = load_config(None, None)
    sc = synth.make_structured_scene(60000, 30000, seed=7, extent=10.0, scan_range=2.0, boxes=6, cylinders=4)
    pairs, want, _, _, _, stats = _reenact(orc, cfg, sc["map"], sc["scan"], False)
    print(f"dense scan: {stats}")
    assert stats["both"] < 3 and stats["pairs"] >= 1000, stats      # (condition on the oracle)
    node = RegistrationNode(cfg, ransac_iterations=N_ITER, baseline_methods=("fpfh",))
    got = node.baseline_row_pairs(sc["map"], sc["scan"], "fpfh")["pairs"]
    np.testing.assert_array_equal(got.cpu().numpy(), pairs)
    pose, pose_icp = node.ransac_registration(sc["map"], sc["scan"], "fpfh", run_icp=False)
    np.testing.assert_array_equal(pose, np.eye(4))
    assert pose_icp is None


def test_evaluate_scene_with_the_fpfh_baseline(monkeypatch):
    from tests.test_gpu_icp_registration import _errors, _synthetic_scene
    from vfmreg import registration
    from vfmreg.evaluation import Evaluation, build_local_map, evaluate_scene
    from vfmreg.mapping import VoxelHashMap
    from vfmreg.registration import RegistrationNode
    from vfmreg.utils import transform_pcl
    from vfmreg.voxelization import voxel_down_sample
    VoxelHashMap.quiet = True
    scene = _synthetic_scene()
    calls = []
    real = registration.extract_fpfh_features_device
    monkeypatch.setattr(registration, "extract_fpfh_features_device", lambda xyz, vs: (calls.append(len(xyz)), real(xyz, vs))[1])
    node = RegistrationNode(ransac_iterations=4000, cache_map=True, baseline_methods=("fpfh",))
    ev = evaluate_scene(scene, node, Evaluation(), baselines=("fpfh",))
    assert list(ev.rot_errors) == ["fpfh_ransac", "fpfh_ransac_icp", "vfm_ransac", "vfm_ransac_icp"]      # RN:867-874's order
    local_map = build_local_map(scene["map_poses"], scene["map_point_clouds"], n_descriptors=128)
    assert len(calls) == 3 and calls.count(len(local_map)) == 1             # the map's features once per scene (RN:876-877)
    plain = evaluate_scene(scene, RegistrationNode(ransac_iterations=4000, cache_map=True), Evaluation())
    assert list(plain.rot_errors) == ["vfm_ransac", "vfm_ransac_icp"]       # the default is what it was
    for k in plain.rot_errors:
        assert ev.rot_errors[k] == plain.rot_errors[k] and ev.trans_errors[k] == plain.trans_errors[k]
    direct = RegistrationNode(ransac_iterations=4000, baseline_methods=("fpfh",))
    want_t, want_r = {"fpfh_ransac": [], "fpfh_ransac_icp": []}, {"fpfh_ransac": [], "fpfh_ransac_icp": []}
    for gt, cloud in zip(scene["scene_poses"], scene["scene_point_clouds"]):
        cloud = voxel_down_sample(cloud, .1).astype(cloud.dtype)
        cloud = transform_pcl(cloud, np.eye(4))
        p0, p1 = direct.ransac_registration(local_map, cloud, "fpfh", True)
        assert p1 is not None
        for k, v in (("fpfh_ransac", p0), ("fpfh_ransac_icp", p1)):
            rte, rre = _errors(v @ np.eye(4), gt)
            want_t[k].append(rte)
            want_r[k].append(rre)
    for k in want_t:
        assert ev.trans_errors[k] == want_t[k] and ev.rot_errors[k] == want_r[k], k
    # without run_icp only the RANSAC row joins
    ev = evaluate_scene(scene, node, Evaluation(), run_icp=False, baselines=("fpfh",))
    assert list(ev.rot_errors) == ["fpfh_ransac", "vfm_ransac"]

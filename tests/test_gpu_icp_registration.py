"""``RegistrationNode.icp_registration`` (registration_node.py:359-394) and the ICP grid built on the device (``vfm_icp_grid_build``,
``VoxelGridDevice.from_device``) against the CPU oracle.  Every expected value is composed from ``oracle.oracle`` inside the test
(``voxel_hash_map_points`` -> ``voxel_grid_csr``, ``voxel_down_sample``, ``register_frame``, ``register_frame_nd``,
``build_local_map``); everything that is compared is compared bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.guarded import GuardedBuffer  # noqa: E402
from tests.icp_grid_cases import crowded_cloud, crowded_share, oracle_grid  # noqa: E402

OUT_OF_RANGE = "voxel coordinate outside"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _assert_grid(g, ref):
    keys, start, pts = ref
    assert g.n_voxels == len(keys) and g.n_kept == len(pts)
    np.testing.assert_array_equal(g.keys.cpu().numpy(), keys)
    np.testing.assert_array_equal(g.start.cpu().numpy(), start)
    np.testing.assert_array_equal(g.pts.cpu().numpy().reshape(-1, 3), pts.reshape(-1, 3))
    assert g.keys.dtype == torch.int64 and g.start.dtype == torch.int32 and g.pts.dtype == torch.float64


# ------------------------------------------------------------------------------------------------------------------ grid
@pytest.mark.parametrize("cap", [0, 1, 20])
@pytest.mark.parametrize("vs", [0.5, 1.0])
@pytest.mark.parametrize("n", [0, 1, 1000, 200000])
def test_grid_build_equals_the_grid_of_the_map(n, vs, cap):
    from vfmreg.icp import VoxelGridDevice
    p = crowded_cloud(n, vs, seed=n + int(10 * vs) + cap)
    if n >= 1000:
        assert (p < 0).any() and (p / vs == np.trunc(p / vs)).any()       # negative coordinates, points on voxel faces
        assert crowded_share(p, vs, 20) >= 0.05                             # with cap 20 the cap path is taken
    ref = oracle_grid(p, vs, cap)
    g = VoxelGridDevice.from_device(dev(p), vs, cap)
    _assert_grid(g, ref)
    if cap == 20 and n >= 1000:
        assert g.n_kept < n
    if cap == 0:
        assert g.n_kept == n
        if n:                                                               # the host constructor's grid, unchanged
            h = VoxelGridDevice(p, vs)
            _assert_grid(g, (h.keys.cpu().numpy(), h.start.cpu().numpy(), h.pts.cpu().numpy()))


def test_grid_of_a_map_added_in_three_calls():
    from vfmreg.icp import _grid_of
    from vfmreg.mapping import VoxelHashMap
    for vs in (0.5, 1.0):
        p = crowded_cloud(30000, vs, seed=77)
        assert crowded_share(p, vs, 20) >= 0.05
        vhm = VoxelHashMap(vs, 100.0, 20)
        for block in (p[:9000], p[9000:9001], p[9001:]):
            vhm.add_points(block)
        g = _grid_of(vhm)
        _assert_grid(g, oracle_grid(p, vs, 20))
        assert g.n_kept < len(p)
        assert _grid_of(vhm) is g                                            # kept with the map ...
        vhm.add_points(p[:10] + 1000.0)
        assert _grid_of(vhm) is not g                                        # ... until points are added


def test_out_of_range_coordinate_raises_the_existing_error():
    from vfmreg.icp import VoxelGridDevice
    p = crowded_cloud(1000, 1.0, seed=3)
    for bad in ((1 << 20) - 1.0, -((1 << 20) - 1.0), 3.0e9, float("inf")):
        q = p.copy()
        q[517, 1] = bad
        with pytest.raises(ValueError, match=OUT_OF_RANGE) as e_dev:
            VoxelGridDevice.from_device(dev(q), 1.0, 20)
        if np.isfinite(bad):
            with pytest.raises(ValueError, match=OUT_OF_RANGE) as e_host:
                VoxelGridDevice(q, 1.0)
            assert str(e_dev.value) == str(e_host.value)
    q = p.copy()
    q[517, 1] = (1 << 20) - 2.5                                             # the largest voxel the key holds
    _assert_grid(VoxelGridDevice.from_device(dev(q), 1.0, 0), oracle_grid(q, 1.0, 0))


# ------------------------------------------------------------------------------------------------------- buffer contract
@pytest.mark.parametrize("n,cap", [(0, 20), (1, 20), (255, 1), (256, 20), (257, 0), (1000, 20), (5000, 20), (5000, 0)])
def test_grid_build_stays_inside_the_callers_buffers(n, cap):
    """include/vfmreg.h: outputs sized for n by the caller, the workspace at exactly vfm_icp_grid_workspace_bytes(n); written are
    keys_out[0, n_voxels), start_out[0, n_voxels], pts_out[0, n_kept) and info_out -- nothing else, whatever the buffers held before."""
    from vfmreg import _lib, ops
    lib = _lib.load()
    vs = 1.0
    p = crowded_cloud(n, vs, seed=100 + n)
    keys_r, start_r, pts_r = oracle_grid(p, vs, cap)
    nv, nk = len(keys_r), len(pts_r)
    ws_bytes = lib.vfm_icp_grid_workspace_bytes(n)
    assert ws_bytes > 0
    xyz = GuardedBuffer((n, 3), torch.float64, seed=1).set(p) if n else GuardedBuffer((0, 3), torch.float64, seed=1)
    keys = GuardedBuffer(n, torch.int64, seed=2)
    start = GuardedBuffer(n + 1, torch.int32, seed=3)
    pts = GuardedBuffer((n, 3), torch.float64, seed=4)
    info = GuardedBuffer(3, torch.int32, seed=5)
    ws = GuardedBuffer(ws_bytes, torch.uint8, seed=6)
    bufs = dict(xyz=xyz, keys=keys, start=start, pts=pts, info=info, ws=ws)
    for fill, poison in ((0x00, None), (0xFF, None), (0xFF, "nan")):
        for b in (keys, start, pts, info, ws):
            b.fill_bytes(fill)
        if poison:
            xyz.poison_guards(poison)        # a read past the end of the input would meet a NaN: status, or another key
        _lib.check(lib.vfm_icp_grid_build(xyz.ptr(), n, vs, cap, keys.ptr(), start.ptr(), pts.ptr(), info.ptr(), ws.ptr(), ws_bytes,
                                          ops._stream()), "icp_grid_build")
        torch.cuda.synchronize()
        for name, b in bufs.items():
            assert b.intact(), f"{name}: {b.intact()!r}"
        if n:
            np.testing.assert_array_equal(xyz.numpy(), p)                  # the input is not written
        assert info.numpy().tolist() == [nv, nk, 0]
        k, s, q = keys.numpy(), start.numpy(), pts.numpy()
        np.testing.assert_array_equal(k[:nv], keys_r)
        np.testing.assert_array_equal(s[:nv + 1], start_r)
        np.testing.assert_array_equal(q[:nk], pts_r)
        # past the defined prefixes nothing is written
        assert (keys.body_bytes()[8 * nv:] == fill).all() and (start.body_bytes()[4 * (nv + 1):] == fill).all()
        assert (pts.body_bytes()[24 * nk:] == fill).all()
        if poison:
            xyz.restore_guards()
    # a workspace too small by one byte is refused on the host
    assert lib.vfm_icp_grid_build(xyz.ptr(), n, vs, cap, keys.ptr(), start.ptr(), pts.ptr(), info.ptr(), ws.ptr(), ws_bytes - 1,
                                  ops._stream()) == (0 if n == 0 else -1)


# ------------------------------------------------------------------------------------------------------- same grid, either way
def test_grid_of_is_the_same_with_and_without_the_container_order(monkeypatch):
    from vfmreg import ops
    from vfmreg.config import load_config
    from vfmreg.icp import _grid_of
    from vfmreg.mapping import VoxelHashMap, get_voxel_hash_map
    from vfmreg.registration import RegistrationNode
    VoxelHashMap.quiet = True
    cfg = load_config(None, None)
    p = crowded_cloud(30000, cfg.mapping.voxel_size, seed=21)
    a, b = get_voxel_hash_map(cfg), get_voxel_hash_map(cfg)
    a.add_points(p)
    b.add_points(p)
    cloud = a.point_cloud()                                                   # a: the container's order has been computed
    assert "3" in a._ordered and "3" not in b._ordered
    ga, gb = _grid_of(a), _grid_of(b)
    assert "3" not in b._ordered                                              # ... and building b's grid did not compute it
    for x, y in ((ga.keys, gb.keys), (ga.start, gb.start), (ga.pts, gb.pts)):
        assert torch.equal(x, y)
    assert (ga.n_voxels, ga.n_kept) == (gb.n_voxels, gb.n_kept) == (ga.n_voxels, len(cloud))
    _assert_grid(gb, oracle_grid(p, cfg.mapping.voxel_size, cfg.mapping.max_points_per_voxel))
    # icp_registration on a 3-column map never replays the container
    from oracle import oracle as orc
    scan, guess, T = _scan_of(p, seed=22)
    want = _oracle_icp(orc, cfg, p, scan, guess, 3)

    def refuse(*args, **kwargs):
        raise AssertionError("ops.voxel_robin called")
    monkeypatch.setattr(ops, "voxel_robin", refuse)
    node = RegistrationNode(cfg)
    np.testing.assert_array_equal(node.icp_registration(p, scan, guess), want)


# ------------------------------------------------------------------------------------------------------------------ method
def _scan_of(map_xyz, seed, n=3000, shift=0.25):
    """a scan of the map: a planted pose, 0.02 m of noise, and a guess near the planted pose"""
    from vfmreg import synth
    rng = np.random.default_rng(seed)
    T = synth.random_pose(rng)
    T[:3, 3] *= 0.1
    pick = rng.choice(len(map_xyz), n, replace=False)
    scan = (map_xyz[pick] - T[:3, 3]) @ T[:3, :3] + rng.normal(0, 0.02, (n, 3))
    guess = T.copy()
    guess[:3, 3] += rng.normal(0, shift, 3)
    return np.ascontiguousarray(scan), guess, T


def _oracle_icp(orc, cfg, map_xyz, raw_scan, initial_pose, dist):
    """RN:359-394 from the oracle's pieces"""
    vs, sigma = cfg.mapping.voxel_size, cfg.adaptive_threshold.initial_threshold
    scan = orc.voxel_down_sample(orc.voxel_down_sample(raw_scan, vs * 0.5), vs * 1.0)
    mp = np.asarray(map_xyz, dtype=np.float64)[orc.voxel_hash_map_points(map_xyz, vs, cfg.mapping.max_points_per_voxel)]
    guess = np.eye(4) if initial_pose is None else initial_pose
    return orc.register_frame(scan[:, :3], mp[:, :3], vs, guess, dist * sigma, sigma / dist)


@pytest.mark.parametrize("dist", [3, 7])
def test_icp_registration_equals_the_oracle_composition(dist, capsys):
    from oracle import oracle as orc
    from vfmreg import synth
    from vfmreg.config import load_config
    from vfmreg.mapping import VoxelHashMap
    from vfmreg.registration import MapHandle, RegistrationNode
    cfg = load_config(None, None)
    node = RegistrationNode(cfg)
    # (a) the scene shape of tests/test_gpu_icp.py (a sparse map), with an initial pose
    pr = synth.make_pair(3000, 30000, 128, seed=8)
    rng = np.random.default_rng(1)
    guess = pr["T_gt"].copy()
    guess[:3, 3] += rng.normal(0, 0.25, 3)
    VoxelHashMap.quiet = False
    pose = node.icp_registration(pr["b_xyz"], pr["q_xyz"], guess, dist=dist)
    printed = capsys.readouterr().out
    VoxelHashMap.quiet = True
    want = _oracle_icp(orc, cfg, pr["b_xyz"], pr["q_xyz"], guess, dist)
    np.testing.assert_array_equal(pose, want)
    vs = cfg.mapping.voxel_size
    n_map = len(orc.voxel_hash_map_points(pr["b_xyz"], vs, cfg.mapping.max_points_per_voxel))
    n_scan = len(orc.voxel_down_sample(orc.voxel_down_sample(pr["q_xyz"], vs * 0.5), vs))
    assert f"Map size: {n_map}, Scan size: {n_scan}" in printed                # RN:368
    # (b) a crowded map (the per-voxel cap drops points), float32 clouds as the scene files hold them, no initial pose: the scan is
    # moved into the map's frame first, as make_step does before its vanilla-ICP row (RN:861, 929)
    p = crowded_cloud(30000, vs, seed=31).astype(np.float32)
    assert crowded_share(p, vs, 20) >= 0.05
    scan, near, T = _scan_of(p.astype(np.float64), seed=32)
    scan_in_place = orc.transform_pcl(scan, near).astype(np.float32)
    pose = node.icp_registration(p, scan_in_place, dist=dist)
    want = _oracle_icp(orc, cfg, p, scan_in_place, None, dist)
    np.testing.assert_array_equal(pose, want)
    assert not np.array_equal(pose, np.eye(4))
    # ... and with the initial pose instead
    np.testing.assert_array_equal(node.icp_registration(p, scan, near, dist), _oracle_icp(orc, cfg, p, scan, near, dist))
    # a MapHandle gives the same pose, and keeps its grid between calls
    h = node.set_map(p)
    assert isinstance(h, MapHandle)
    np.testing.assert_array_equal(node.icp_registration(h, scan_in_place, dist=dist), want)
    g = h.voxel_hash_map._icp_grid[1]
    np.testing.assert_array_equal(node.icp_registration(h, scan, near, dist), _oracle_icp(orc, cfg, p, scan, near, dist))
    assert h.voxel_hash_map._icp_grid[1] is g
    # an empty map hands the initial pose back (Registration.cpp:150); bad widths are loud
    np.testing.assert_array_equal(node.icp_registration(np.zeros((0, 3)), scan, near, dist), near)
    with pytest.raises(ValueError, match="Invalid shape"):
        node.icp_registration(p, np.zeros((4, 2)))


def test_icp_registration_387_columns_takes_the_descriptor_seeded_loop():
    """RN:381-389: rows of 3 + 384 columns call register_frame with src_ / tgt_; the pose is oracle.register_frame_nd's on the same
    inputs (the scan after both down-sampling levels, the map in the container's order), bit for bit."""
    from oracle import oracle as orc
    from vfmreg import synth
    from vfmreg.config import load_config
    from vfmreg.mapping import VoxelHashMap
    from vfmreg.registration import RegistrationNode
    VoxelHashMap.quiet = True
    cfg = load_config(None, None)
    vs, sigma = cfg.mapping.voxel_size, cfg.adaptive_threshold.initial_threshold
    pr = synth.make_pair(6000, 30000, 384, seed=9)
    voxel_map = np.c_[pr["b_xyz"], pr["b_desc"]]
    scan = np.c_[pr["q_xyz"], pr["q_desc"]]
    rng = np.random.default_rng(9)
    guess = pr["T_gt"].copy()
    guess[:3, 3] += rng.normal(0, 0.4, 3)
    node = RegistrationNode(cfg)
    for dist in (3, 7):
        pose = node.icp_registration(voxel_map, scan, guess, dist=dist)
        voxel_scan = orc.voxel_down_sample(orc.voxel_down_sample(scan, vs * 0.5), vs * 1.0)
        mp = np.asarray(voxel_map, dtype=np.float64)[orc.voxel_hash_map_points(voxel_map, vs, cfg.mapping.max_points_per_voxel)]
        ref, _, _, hist = orc.register_frame_nd(voxel_scan, mp, vs, guess, dist * sigma, sigma / dist, return_history=True)
        assert any(h[0] == "vfm" for h in hist)
        assert pose.shape == (4, 4)
        np.testing.assert_array_equal(pose, ref)
    np.testing.assert_array_equal(node.icp_registration(node.set_map(voxel_map), scan, guess), node.icp_registration(voxel_map, scan, guess))


def test_icp_registration_moves_a_perturbed_pose_towards_the_planted_one():
    """relative only: from a perturbed pose the result is closer to the planted pose than the start was"""
    from vfmreg.config import load_config
    from vfmreg.mapping import VoxelHashMap
    from vfmreg.registration import RegistrationNode, compute_errors
    VoxelHashMap.quiet = True
    cfg = load_config(None, None)
    node = RegistrationNode(cfg)
    rng = np.random.default_rng(41)
    m = np.c_[rng.uniform(-40, 40, (60000, 2)), rng.uniform(-2, 6, 60000)]
    for seed in (42, 43, 44):
        scan, guess, T = _scan_of(m, seed=seed, n=5000, shift=0.3)
        for dist in (3, 7):
            pose = node.icp_registration(m, scan, guess, dist=dist)
            e0, e1 = compute_errors(guess, T), compute_errors(pose, T)
            assert e1[0] < e0[0], (seed, dist, e0, e1)
            assert np.linalg.norm(pose - T) < np.linalg.norm(guess - T)


# -------------------------------------------------------------------------------------------------------------- evaluation
def _synthetic_scene(d=128):
    """the scene of tests/test_gpu_api.py::test_evaluation_harness_on_a_synthetic_scene"""
    from vfmreg import synth
    rng = np.random.default_rng(2)
    world = np.c_[rng.uniform(-40, 40, (40000, 2)), rng.uniform(-2, 6, 40000)]
    desc = np.abs(rng.standard_normal((40000, d))).astype(np.float32)
    desc[::50] = 0.0
    map_poses, map_clouds = [], []
    for j in range(3):
        T = synth.random_pose(rng)
        sel = np.arange(j, 40000, 3)
        local = (world[sel] - T[:3, 3]) @ T[:3, :3]
        map_poses.append(T)
        map_clouds.append(np.c_[local, desc[sel]].astype(np.float32))
    scan_poses, scan_clouds = [], []
    for s in range(2):
        T = synth.random_pose(rng)
        sel = rng.permutation(40000)[:6000]
        sel = sel[desc[sel].sum(1) > 0]
        local = (world[sel] - T[:3, 3]) @ T[:3, :3] + rng.normal(0, 0.01, (len(sel), 3))
        noisy = desc[sel] + 0.05 * np.abs(rng.standard_normal((len(sel), d))).astype(np.float32)
        # the stored pose is a little off, as a dataset's is: the ICP ground truth moves it
        stored = T.copy()
        stored[:3, 3] += rng.normal(0, 0.1, 3)
        scan_poses.append(stored)
        scan_clouds.append(np.c_[local, noisy].astype(np.float32))
    return dict(map_poses=map_poses, map_point_clouds=map_clouds, map_clip=[], scene_poses=scan_poses, scene_point_clouds=scan_clouds,
                scene_sequences=["scanA", "scanB"])


def _errors(pose, gt_pose):
    """RN:997-1011 literally, as oracle.evaluate_scene states it"""
    R, R_gt = np.asarray(gt_pose)[:3, :3], pose[:3, :3]
    rre = float(np.rad2deg(abs(np.arccos(min(max(((R.T @ R_gt).trace() - 1) / 2, -1.0), 1.0)))))
    rte = float(np.linalg.norm(np.asarray(gt_pose)[:3, 3] - pose[:3, 3]))
    return rte, rre


def test_evaluate_scene_with_icp_ground_truth_and_icp_baseline():
    from oracle import oracle as orc
    from vfmreg.config import load_config
    from vfmreg.evaluation import Evaluation, evaluate_scene
    from vfmreg.mapping import VoxelHashMap
    from vfmreg.registration import RegistrationNode
    VoxelHashMap.quiet = True
    cfg = load_config(None, None)
    scene = _synthetic_scene()
    ref = orc.evaluate_scene(scene, n_iter=4000)
    # both flags off: today's output, the oracle's harness (as tests/test_gpu_api.py checks it)
    ev = evaluate_scene(scene, RegistrationNode(ransac_iterations=4000), Evaluation())
    assert set(ev.rot_errors) == {"vfm_ransac", "vfm_ransac_icp"}
    for k in ("vfm_ransac", "vfm_ransac_icp"):
        assert ev.rot_errors[k] == ref["rot_errors"][k] and ev.trans_errors[k] == ref["trans_errors"][k], k
    # both flags on: every row against the ICP ground truth (RN:645-646), plus the vanilla-ICP row (RN:929)
    ev = evaluate_scene(scene, RegistrationNode(ransac_iterations=4000), Evaluation(), icp_ground_truth=True, icp_baseline=True)
    local_map = ref["local_map"]
    want_t, want_r = {}, {}
    for (p0, p1), stored, cloud in zip(ref["poses"], scene["scene_poses"], scene["scene_point_clouds"]):
        cloud = orc.voxel_down_sample(cloud, .1).astype(cloud.dtype)                                   # RN:593
        gt = _oracle_icp(orc, cfg, local_map[:, :3], cloud[:, :3], np.asarray(stored), 3)              # RN:646
        assert not np.array_equal(gt, np.asarray(stored))
        cloud = orc.transform_pcl(cloud, np.eye(4))                                                    # RN:861
        icp = _oracle_icp(orc, cfg, local_map[:, :3], cloud[:, :3], None, 7)                           # RN:929
        for k, v in (("vfm_ransac", p0), ("vfm_ransac_icp", p1), ("icp", icp)):
            rte, rre = _errors(v @ np.eye(4), gt)
            want_t.setdefault(k, []).append(rte)
            want_r.setdefault(k, []).append(rre)
    assert list(ev.rot_errors) == ["vfm_ransac", "vfm_ransac_icp", "icp"]
    for k in want_t:
        assert ev.trans_errors[k] == want_t[k] and ev.rot_errors[k] == want_r[k], k
    assert ev.points_in_map == [len(local_map)] * 2
    assert "icp" in ev.summary()

"""The local map that carries descriptors of any width (``VoxelHashMap(descriptor_mode="weighted")``) and the descriptor-weighted odometry
(``KissICP(descriptor_mode="weighted")``) on the GPU against tests/odometry_weighted_oracle.py: rows, grid, update statistics, the kept
norms and flags, every pose and every ``frame_downsample`` bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import odometry_desc_oracle as do  # noqa: E402
from tests import odometry_oracle as oo  # noqa: E402
from tests import odometry_weighted_oracle as wo  # noqa: E402

MAP_VS, MAP_CAP, MAP_MD = 1.0, 3, 6.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(autouse=True)
def _quiet():
    from vfmreg.mapping import VoxelHashMap
    VoxelHashMap.quiet, was = True, VoxelHashMap.quiet
    yield
    VoxelHashMap.quiet = was


# ------------------------------------------------------------------------------------------------------------------ the map
def _blocks(width, dtype, seed=31):
    """six blocks of 600 rows of 3 + ``width`` columns in the sensor frame + their poses: about 3 points a voxel (the cap of 3 refuses
    some), the sensor advances 1.5 m a block (voxels fall behind max_distance 6); some rows have no descriptor or a zero element sum"""
    from oracle import oracle
    rng = np.random.default_rng(seed + width)
    blocks, poses = [], []
    T = np.eye(4)
    for _ in range(6):
        xyz = np.c_[rng.uniform(-5.0, 5.0, (600, 2)), rng.uniform(-1.0, 1.0, 600)]
        desc = rng.normal(size=(600, width))
        desc[::50] = 0.0
        desc[7::50, :2] = [1.0, -1.0]
        desc[7::50, 2:] = 0.0
        T = oracle.se3_exp(np.array([1.5, 0.1, 0.0, 0.0, 0.0, 0.04])) @ T
        blocks.append(np.ascontiguousarray(np.c_[xyz, desc].astype(dtype)))
        poses.append(T)
    return blocks, poses


def _assert_same_map(vhm, ref, stats=True):
    want = ref.rows()
    if ref.empty():
        assert vhm.empty_n() and vhm.empty_x() and vhm.point_cloud_n().shape == (0, 3) and vhm.weighted_operand() is None
    else:
        assert not vhm.empty_x() and not vhm.empty_n() and vhm.width_n() == want.shape[1]
        np.testing.assert_array_equal(vhm.point_cloud_n(), want)
        np.testing.assert_array_equal(vhm.point_cloud(), want[:, :3])           # map_ is empty: the wide rows' heads
        g, desc, norm, has = vhm.weighted_operand()
        keys, start, pts = ref.grid()
        np.testing.assert_array_equal(g.keys.cpu().numpy(), keys)
        np.testing.assert_array_equal(g.start.cpu().numpy(), start)
        np.testing.assert_array_equal(g.pts.cpu().numpy(), pts)
        np.testing.assert_array_equal(desc.double().cpu().numpy(), want[:, 3:])
        want_norm, want_has = wo.map_stats(want[:, 3:])                         # afresh from the rows
        np.testing.assert_array_equal(norm.cpu().numpy(), want_norm)
        np.testing.assert_array_equal(has.cpu().numpy(), want_has)
        assert vhm.weighted_operand()[2] is norm                                # kept until the map changes
        assert vhm.xyz_map()._icp_grid[1] is g
    assert vhm.empty()
    if stats:
        assert vhm.last_update == ref.last


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("width,dtype", [(5, np.float32), (64, np.float64)])
def test_a_weighted_map_under_update_add_points_and_removal(width, dtype, on_device):
    from vfmreg.mapping import VoxelHashMap
    blocks, poses = _blocks(width, dtype)
    vhm, ref = VoxelHashMap(MAP_VS, MAP_MD, MAP_CAP, descriptor_mode="weighted"), do.RowVoxelMap(MAP_VS, MAP_MD, MAP_CAP)
    assert vhm.empty_x()
    give = dev if on_device else (lambda a: a)
    refused = removed = 0
    for rows, T in zip(blocks[:3], poses[:3]):
        vhm.update(give(rows), T)
        ref.update(rows, T)
        _assert_same_map(vhm, ref)
        refused += len(rows) - ref.last["points_added"]
        removed += ref.last["voxels_removed"]
    assert refused > 50 and removed > 10 and ref.full_voxels() > 20              # rows overflowed the cap, far voxels went
    stats_before = vhm.weighted_operand()[2]
    # an empty update: the removal alone
    vhm.update(give(np.zeros((0, 3 + width), dtype=dtype)), poses[3])
    ref.update(np.zeros((0, 3 + width)), poses[3])
    _assert_same_map(vhm, ref)
    assert ref.last["points_added"] == 0 and ref.last["voxels_removed"] > 0 and vhm.weighted_operand()[2] is not stats_before
    # add_points on an updated map: plain AddPoints, the grid's order kept
    vhm.add_points(blocks[3])
    ref.update(blocks[3], None, None)
    _assert_same_map(vhm, ref)
    # remove_far_away_points alone
    origin = poses[3][:3, 3] + [3.0, 0.0, 0.0]
    vhm.remove_far_away_points(origin)
    ref.remove_far(origin)
    assert ref.last["voxels_removed"] > 0 and vhm.last_update["voxels_removed"] == ref.last["voxels_removed"]
    assert vhm.last_update["points_removed"] == ref.last["points_removed"]
    _assert_same_map(vhm, ref, stats=False)
    # mixed precision: everything to double
    other = np.float64 if dtype == np.float32 else np.float32
    vhm.update(give(blocks[4].astype(other)), poses[4])
    ref.update(blocks[4].astype(other), poses[4])
    _assert_same_map(vhm, ref)
    assert vhm._chunks["n"][0][0].dtype == torch.float64
    # another width: refused, the map as it was
    with pytest.raises(ValueError, match="Invalid shape"):
        vhm.update(give(np.zeros((4, 3 + width + 1), dtype=dtype)), poses[4])
    _assert_same_map(vhm, ref)
    # a removal that empties the map, then rows again; 3-column points go to the 3-D map
    vhm.remove_far_away_points([1000.0, 0.0, 0.0])
    ref.remove_far([1000.0, 0.0, 0.0])
    assert ref.empty()
    _assert_same_map(vhm, ref, stats=False)
    vhm.update(give(blocks[5]), poses[5])
    ref.update(blocks[5], poses[5])
    _assert_same_map(vhm, ref)
    vhm.update(np.ascontiguousarray(blocks[0][:, :3], dtype=np.float64), poses[0])
    assert not vhm.empty() and not vhm.empty_x()
    np.testing.assert_array_equal(vhm.point_cloud_n(), ref.rows())


def test_a_weighted_map_takes_387_columns_and_converts_at_its_first_update():
    from vfmreg.mapping import VoxelHashMap
    blocks, poses = _blocks(384, np.float32)
    vhm, ref = VoxelHashMap(MAP_VS, MAP_MD, MAP_CAP, descriptor_mode="weighted"), do.RowVoxelMap(MAP_VS, MAP_MD, MAP_CAP)
    vhm.add_points(blocks[0])                                                   # filled by add_points: the container's order until ...
    ref.update(blocks[0], None, None)
    assert not vhm.empty_x() and vhm._wide_grid is None
    vhm.update(blocks[1], poses[1])                                             # ... its first update makes it a grid
    ref.update(blocks[1], poses[1])
    _assert_same_map(vhm, ref)


# ------------------------------------------------------------------------------------------------------------------ registration
def test_register_frame_on_an_updated_weighted_map_equals_the_oracle(capsys):
    from oracle import oracle
    from vfmreg import icp
    from vfmreg.mapping import VoxelHashMap
    rng = np.random.default_rng(5)
    for width, dtype in ((5, np.float32), (64, np.float64)):
        blocks, poses = _blocks(width, dtype)
        vhm, ref = VoxelHashMap(MAP_VS, MAP_MD, MAP_CAP, descriptor_mode="weighted"), do.RowVoxelMap(MAP_VS, MAP_MD, MAP_CAP)
        guess0 = oracle.se3_exp(np.array([0.05, -0.04, 0.02, 0.0, 0.0, 0.01]))
        got = icp.register_frame(blocks[0][:50], vhm, guess0, 1.5, 0.2)        # an empty map: the guess (Registration.cpp:389)
        np.testing.assert_array_equal(got, guess0)
        for rows, T in zip(blocks[:3], poses[:3]):
            vhm.update(rows, T)
            ref.update(rows, T)
        map_rows = ref.rows()
        T = poses[2]
        scan = map_rows[rng.permutation(len(map_rows))[:200]].copy()
        scan[:, :3] = (scan[:, :3] - T[:3, 3]) @ T[:3, :3] + rng.normal(0.0, 0.01, (200, 3))
        scan[:, 3:] += rng.normal(0.0, 0.05, (200, width))
        scan = np.ascontiguousarray(scan.astype(dtype))
        guess = guess0 @ T
        grid = vhm._wide_grid
        VoxelHashMap.quiet = False
        got = icp.register_frame(scan, vhm, guess, 1.5, 0.2)
        VoxelHashMap.quiet = True
        want, hist = oracle.register_frame_xd(scan, map_rows, MAP_VS, guess, 1.5, 0.2, return_history=True)
        np.testing.assert_array_equal(got, want)
        assert len(hist) > 1 and not np.array_equal(got, guess) and vhm._wide_grid is grid      # nothing rebuilt
        assert f"[XD] [0] correspondences {int(hist[0][0][42])}" in capsys.readouterr().out
        icp.register_frame(scan, vhm, guess, 1.5, 0.2)
        assert "[XD]" not in capsys.readouterr().out                             # the line follows VoxelHashMap.quiet
        # the other precision of the scan: the same values, the same pose
        other = np.float64 if dtype == np.float32 else np.float32
        np.testing.assert_array_equal(icp.register_frame(scan.astype(other), vhm, guess, 1.5, 0.2),
                                      oracle.register_frame_xd(scan.astype(other), map_rows, MAP_VS, guess, 1.5, 0.2))
        with pytest.raises(ValueError, match="Invalid shape"):
            icp.register_frame(np.zeros((5, 3 + width + 2)), vhm, guess, 1.5, 0.2)
        # a map of the same rows filled by add_points alone: it becomes a grid at its first registration
        filled = VoxelHashMap(MAP_VS, MAP_MD, MAP_CAP, descriptor_mode="weighted")
        filled.add_points(map_rows)
        np.testing.assert_array_equal(icp.register_frame(scan, filled, guess, 1.5, 0.2), want)


def test_a_refilled_map_is_not_searched_through_the_old_statistics():
    """as many rows as before, other descriptors: the norms and flags of the rows that are there"""
    from vfmreg.mapping import VoxelHashMap
    blocks, poses = _blocks(5, np.float32)
    vhm = VoxelHashMap(MAP_VS, MAP_MD, MAP_CAP, descriptor_mode="weighted")
    vhm.update(blocks[0], poses[0])
    first = vhm.weighted_operand()[2].cpu().numpy()
    again = blocks[0].copy()
    again[:, 3:] *= 2.0
    vhm.clear()
    vhm.update(again, poses[0])
    np.testing.assert_array_equal(vhm.weighted_operand()[2].cpu().numpy(), 2.0 * first)
    vhm.clear()
    vhm.add_points(blocks[0])
    vhm.add_points(blocks[1])
    ref = do.RowVoxelMap(MAP_VS, MAP_MD, MAP_CAP)
    ref.update(blocks[0], None, None)
    ref.update(blocks[1], None, None)
    np.testing.assert_array_equal(vhm.weighted_operand()[2].cpu().numpy(), wo.map_stats(ref.rows()[:, 3:])[0])


# ------------------------------------------------------------------------------------------------------------------ the odometry
# (descriptor width, frames, dtype of the frames)
DRIVES = [(5, 10, np.float32), (16, 10, np.float32), (384, 6, np.float64)]
_DRIVES = {}


def _drive(width, frames, dtype):
    if width not in _DRIVES:
        _DRIVES[width] = wo.weighted_drive(width, frames, 2500, 11, dtype=dtype)
    return _DRIVES[width]


@pytest.mark.parametrize("deskew", [False, True], ids=["plain", "deskew"])
@pytest.mark.parametrize("width,frames,dtype", DRIVES, ids=["D5", "D16", "D384"])
def test_weighted_kiss_icp_equals_the_oracle_loop(width, frames, dtype, deskew):
    from vfmreg.config import load_config
    from vfmreg.kiss_icp import KissICP
    scans, _, stamps = _drive(width, frames, dtype)
    k = KissICP(do.drive_config(load_config, deskew=deskew), descriptor_mode="weighted")
    ref_k = wo.KissICPWeighted(do.drive_config(oo.load_config, deskew=deskew), 0.0)
    used = 0
    for f, (frame, t) in enumerate(zip(scans, stamps)):
        fed = None
        if deskew and len(k.poses) >= 2:        # de-skew is bounded, not bit-equal (tests/test_gpu_odometry.py): the oracle is fed the device's
            fed = k.compensator.deskew_device(dev(frame[:, :3].astype(np.float64)), k.poses, dev(t)).cpu().numpy()
            assert not np.array_equal(fed, frame[:, :3])
            used += 1
        pose, down, upd = k.register_frame(frame, t, use_descriptors=True)
        rpose, rdown, rupd = ref_k.register_frame(frame, t, fed)
        np.testing.assert_array_equal(pose, rpose, err_msg=f"pose of frame {f}")
        np.testing.assert_array_equal(down, rdown, err_msg=f"rows of frame {f}")
        assert upd and rupd and down.shape[1] == 3 + width and down.dtype == np.float64
    assert used == (frames - 2 if deskew else 0)
    assert len(ref_k.history) == frames - 1 and all(len(rec["hist"]) >= 1 for rec in ref_k.history)
    assert k.local_map.empty() and not k.local_map.empty_x()
    np.testing.assert_array_equal(k.local_map.point_cloud_n(), ref_k.local_map.rows())
    assert k.local_map.last_update == ref_k.local_map.last
    want_dtype = torch.float64 if (deskew or dtype == np.float64) else torch.float32     # (de-skewed rows are double rows)
    assert k.local_map._chunks["n"][0][0].dtype == want_dtype


def test_weighted_kiss_icp_without_descriptors_and_small_frames():
    from vfmreg.config import load_config
    from vfmreg.kiss_icp import KissICP
    scans, _, stamps = _drive(5, 10, np.float32)
    k = KissICP(do.drive_config(load_config), descriptor_mode="weighted")
    plain = KissICP(do.drive_config(load_config))
    for frame, t in zip(scans[:3], stamps[:3]):                                 # use_descriptors=False is unchanged: the 3-D odometry
        a, b = k.register_frame(frame, t), plain.register_frame(frame, t)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    assert k.local_map.empty_x() and not k.local_map.empty()
    k = KissICP(do.drive_config(load_config), descriptor_mode="weighted")
    pose, down, upd = k.register_frame(np.zeros((0, 8), dtype=np.float32), np.zeros(0), use_descriptors=True)      # an empty scan
    assert np.array_equal(pose, np.eye(4)) and down.shape == (0, 8) and upd and k.local_map.empty_x()


def test_default_mode_objects_still_refuse():
    from vfmreg import icp
    from vfmreg.config import load_config
    from vfmreg.kiss_icp import KissICP
    from vfmreg.mapping import VoxelHashMap
    blocks, poses = _blocks(5, np.float32)
    vhm = VoxelHashMap(MAP_VS, MAP_MD, MAP_CAP)
    with pytest.raises(NotImplementedError, match="only 3-column points and 387-column rows"):
        vhm.update(blocks[0], poses[0])
    with pytest.raises(NotImplementedError, match="only 3-column points and 387-column rows"):
        vhm.update(dev(blocks[0]), poses[0])
    assert vhm.empty_n() and vhm.empty_x()
    with pytest.raises(NotImplementedError, match="VectorXd local map of other widths is not built"):
        KissICP(do.drive_config(load_config)).register_frame(blocks[0], np.zeros(600), use_descriptors=True)
    vhm.add_points(blocks[0])                                                   # a static map of another width: searched as before
    with pytest.raises(NotImplementedError, match="only 3-column points and 387-column rows"):
        vhm.update(blocks[1], poses[1])
    with pytest.raises(RuntimeError, match="weighted"):
        vhm.weighted_operand()
    assert icp.POINT_SIZE == 387

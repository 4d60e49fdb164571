"""The descriptor-weighted odometry without a device: the oracle loop of tests/odometry_weighted_oracle.py on drives of several widths, the
check that the weighting changes what the search picks, and the argument rules of ``descriptor_mode`` that are decided before anything is
uploaded."""
import numpy as np
import pytest

from tests import odometry_desc_oracle as do
from tests import odometry_weighted_oracle as wo

# (descriptor width, frames): float32 drives of 2500 points, drive_config, P ~ N(0, 0.6), noise 0.02
DRIVES = [(5, 10), (16, 10), (384, 6)]


@pytest.fixture(scope="module", params=DRIVES, ids=lambda p: f"D{p[0]}")
def oracle_run(request):
    width, frames = request.param
    scans, gt, stamps = wo.weighted_drive(width, frames, 2500, 11, dtype=np.float32)
    k, out = wo.run(scans, stamps)
    return dict(width=width, frames=frames, scans=scans, gt=gt, k=k, out=out)


def test_the_oracle_loop_follows_the_drive(oracle_run):
    k, out, gt = oracle_run["k"], oracle_run["out"], oracle_run["gt"]
    assert len(k.history) == oracle_run["frames"] - 1 and all(upd for _, _, upd in out)      # every frame but the first is registered
    assert all(len(rec["hist"]) >= 1 for rec in k.history)
    assert out[-1][1].shape[1] == 3 + oracle_run["width"]
    assert k.local_map.rows().shape[1] == 3 + oracle_run["width"]
    # an odometry: the sensor advances 0.6 m a frame, and every estimated step is nearer to that than to standing still or to two steps
    steps = [np.linalg.norm(b[0][:3, 3] - a[0][:3, 3]) for a, b in zip(out, out[1:])]
    true = [np.linalg.norm(b[:3, 3] - a[:3, 3]) for a, b in zip(gt, gt[1:])]
    print(f"D = {oracle_run['width']}: steps {np.round(steps, 3).tolist()}")
    assert all(abs(s - t) < 0.3 for s, t in zip(steps, true))


def test_the_weighting_changes_the_first_iterations_targets(oracle_run):
    """pooled over the frames of a drive, the weighted search's first-iteration target differs from the plain nearest neighbour's (the same
    loop on zeroed descriptors) for at least 5 % of the pairs both accept"""
    both = differ = 0
    for rec in oracle_run["k"].history:
        tgt, valid = rec["hist"][0][2], rec["hist"][0][3]
        plain_tgt, plain_valid = wo.first_targets(rec, zero_descriptors=True)
        ok = (valid != 0) & (plain_valid != 0)
        both += int(ok.sum())
        differ += int((tgt[ok] != plain_tgt[ok]).any(axis=1).sum())
    print(f"D = {oracle_run['width']}: {differ} of {both} accepted pairs differ ({100.0 * differ / both:.1f} %)")
    assert both > 1000 and differ >= 0.05 * both


def test_first_targets_replays_the_recorded_iteration(oracle_run):
    rec = oracle_run["k"].history[2]
    tgt, valid = wo.first_targets(rec)
    np.testing.assert_array_equal(tgt, rec["hist"][0][2])
    np.testing.assert_array_equal(valid, rec["hist"][0][3])


# ------------------------------------------------------------------------------------------------------------------ argument rules
def test_the_mode_is_one_of_two():
    from vfmreg.config import load_config
    from vfmreg.kiss_icp import KissICP
    from vfmreg.mapping import VoxelHashMap, get_voxel_hash_map
    cfg = do.drive_config(load_config)
    for bad in ("Weighted", "", None, 1):
        with pytest.raises(ValueError, match="descriptor_mode"):
            VoxelHashMap(1.0, 12.0, 20, descriptor_mode=bad)
        with pytest.raises(ValueError, match="descriptor_mode"):
            get_voxel_hash_map(cfg, descriptor_mode=bad)
        with pytest.raises(ValueError, match="descriptor_mode"):
            KissICP(cfg, descriptor_mode=bad)
    assert VoxelHashMap(1.0, 12.0, 20).descriptor_mode == "seeded" and KissICP(cfg).local_map.descriptor_mode == "seeded"
    k = KissICP(cfg, 0.5, "weighted")
    assert k.descriptor_mode == k.local_map.descriptor_mode == "weighted" and k.map_update_threshold == 0.5
    assert get_voxel_hash_map(cfg, "weighted").descriptor_mode == "weighted"
    m = VoxelHashMap(1.0, 12.0, 20, "weighted")
    assert m.empty() and m.empty_n() and m.empty_x() and m.width_n() is None
    assert VoxelHashMap(1.0, 12.0, 20).empty_x()                                # a "seeded" map has no map_x_


def test_weighted_frames_need_a_descriptor_column():
    from vfmreg.config import load_config
    from vfmreg.kiss_icp import KissICP
    k = KissICP(do.drive_config(load_config), descriptor_mode="weighted")
    for shape in ((10, 3), (10, 2), (10,), (0, 3)):
        with pytest.raises(ValueError, match="Invalid shape"):
            k.register_frame(np.zeros(shape), np.zeros(10), use_descriptors=True)


def _holding(width, mode="weighted"):
    """a map that holds two rows of ``width`` columns, put there without a device (the container's own layout)"""
    import torch
    from vfmreg.mapping import VoxelHashMap
    m = VoxelHashMap(1.0, 12.0, 20, descriptor_mode=mode)
    m._chunks["n"] = [(torch.zeros((2, width)), torch.zeros((2, 3), dtype=torch.float64))]
    return m


def test_the_first_wide_rows_fix_the_width():
    from vfmreg import icp
    from vfmreg.config import load_config
    from vfmreg.kiss_icp import KissICP
    m = _holding(8)
    assert m.width_n() == 8 and not m.empty_x() and not m.empty_n()
    for width in (4, 9, 387):
        with pytest.raises(ValueError, match="Invalid shape"):
            m.update(np.zeros((5, width)), np.eye(4))
        with pytest.raises(ValueError, match="Invalid shape"):
            m.add_points(np.zeros((5, width)))
        with pytest.raises(ValueError, match="Invalid shape"):
            icp.register_frame(np.zeros((5, width)), m, np.eye(4), 1.0, 0.3)
    with pytest.raises(ValueError, match="4 x 4"):
        m.update(np.zeros((5, 8)), np.eye(3))
    k = KissICP(do.drive_config(load_config), descriptor_mode="weighted")
    k.local_map = m
    with pytest.raises(ValueError, match="Invalid shape"):
        k.register_frame(np.zeros((10, 9)), np.zeros(10), use_descriptors=True)


def test_the_default_mode_refuses_as_before():
    from vfmreg.config import load_config
    from vfmreg.kiss_icp import KissICP
    from vfmreg.mapping import VoxelHashMap
    m = VoxelHashMap(1.0, 12.0, 20)
    for width in (4, 8, 771):
        with pytest.raises(NotImplementedError, match="only 3-column points and 387-column rows"):
            m.update(np.zeros((5, width)), np.eye(4))
        with pytest.raises(NotImplementedError, match="VectorXd local map of other widths is not built"):
            KissICP(do.drive_config(load_config)).register_frame(np.zeros((10, width)), np.zeros(10), use_descriptors=True)
    with pytest.raises(RuntimeError, match="weighted"):
        m.weighted_operand()

"""The oracle of the descriptor-carrying odometry (tests/odometry_desc_oracle.py) is not vacuous on the drive the GPU test compares
against -- descriptor pairs are found, MAD pruning drops some, the cap fills voxels and the removal takes some --, its map obeys the
stated rules, and the new ``ops`` wrappers refuse CPU tensors.  No GPU."""
import numpy as np
import pytest

from tests import odometry_desc_oracle as do
from tests import odometry_oracle as oo


@pytest.fixture(scope="module")
def run():
    frames, gt, stamps = do.descriptor_drive(14, 2500, 11)
    k = do.KissICPDesc(do.drive_config(oo.load_config), 0.0)
    out = [k.register_frame(f, t) for f, t in zip(frames, stamps)]
    return dict(k=k, out=out, gt=gt, frames=frames)


def test_the_descriptor_drive_is_not_vacuous(run):
    k, out = run["k"], run["out"]
    assert len(k.history) == 13 and all(upd for _, _, upd in out)
    first_pairs, dropped, vfm_iters = [], [], []
    for hist in k.history:
        vfm = [h for h in hist if h[0] == "vfm"]
        assert vfm and any(h[0] == "icp" for h in hist)
        first_pairs.append(int(vfm[0][1][42]))
        dropped.append(int(vfm[0][1][42]) - vfm[-1][3])
        vfm_iters.append(len(vfm))
    removed = [s["voxels_removed"] for s in k.stats[1:]]
    print("descriptor pairs at the first VFM iteration:", first_pairs)
    print("pairs dropped by MAD pruning:", dropped)
    print("VFM iterations:", vfm_iters)
    print("voxels removed per update:", removed, "full voxels at the end:", k.local_map.full_voxels())
    assert min(first_pairs) >= 100
    assert sum(d > 0 for d in dropped) * 2 >= len(dropped)
    assert sum(r > 0 for r in removed) * 2 >= len(removed)
    assert k.local_map.full_voxels() >= 50
    T0 = run["gt"][0]
    err = [np.linalg.norm((T0 @ pose)[:3, 3] - gt[:3, 3]) for (pose, _, _), gt in zip(out, run["gt"])]
    print("trajectory error: worst %.4f m, at the end %.4f m" % (max(err), err[-1]))    # (a figure, not a check: 2 500 points a scan)


def test_descriptors_match_the_same_surface_point_only():
    rng = np.random.default_rng(12)
    P = rng.normal(0.0, 0.6, (3, do.DESCRIPTOR_SIZE))
    phase = rng.uniform(0.0, 2.0 * np.pi, do.DESCRIPTOR_SIZE)
    w = rng.uniform(-20.0, 20.0, (200, 3))
    step = rng.normal(size=(200, 3))
    step /= np.linalg.norm(step, axis=1, keepdims=True)

    def cosine(a, b):
        return (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    a = do.descriptor_of(w, P, phase) + rng.normal(0.0, 0.02, (200, do.DESCRIPTOR_SIZE))
    near = do.descriptor_of(w + 0.02 * step, P, phase) + rng.normal(0.0, 0.02, (200, do.DESCRIPTOR_SIZE))   # the scan noise: 0.01 m a point
    far = do.descriptor_of(w + 2.0 * step, P, phase) + rng.normal(0.0, 0.02, (200, do.DESCRIPTOR_SIZE))
    assert cosine(a, near).min() >= 0.8 and cosine(a, far).max() < 0.8


def test_row_voxel_map_rules():
    m = do.RowVoxelMap(1.0, 5.0, 2)
    rows = np.zeros((5, do.POINT_SIZE))
    rows[:, :3] = [[0.5, 0.5, 0.5], [0.6, 0.5, 0.5], [0.7, 0.5, 0.5], [-1.5, 0.5, 0.5], [9.5, 0.5, 0.5]]
    rows[:, 3] = np.arange(5)
    m.update(rows, None, None)
    assert m.last == dict(points_added=4, voxels_removed=0, points_removed=0)
    assert m.rows()[:, 3].tolist() == [3.0, 0.0, 1.0, 4.0]                     # (voxel key, insertion); the cap refused row 2
    T = np.eye(4)
    T[0, 3] = 1.0
    m.update(rows[2:3], T)                                                      # lands in voxel 1: (1.7, 0.5, 0.5); the far voxel goes
    assert m.last == dict(points_added=1, voxels_removed=1, points_removed=1)
    assert m.rows()[:, 3].tolist() == [3.0, 0.0, 1.0, 2.0] and abs(m.rows()[-1, 0] - 1.7) < 1e-12
    keys, start, pts = m.grid()
    assert start.tolist() == [0, 1, 3, 4] and pts.shape == (4, 3) and m.full_voxels() == 1


def test_the_new_wrappers_refuse_cpu_tensors_and_other_widths():
    torch = pytest.importorskip("torch")
    from vfmreg import icp, ops
    from vfmreg.kiss_icp import KissICP
    from vfmreg.mapping import VoxelHashMap
    assert icp.POINT_SIZE == do.POINT_SIZE
    src = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rows_merge(torch.zeros(2, 4), torch.zeros(2, 4), src, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.icp_grid_update(None, None, None, torch.zeros(4, 3, dtype=torch.float64), None, 1.0, 20, None, 10.0,
                            rows_new=torch.zeros(4, 384))
    with pytest.raises(RuntimeError, match="no CPU path"):
        VoxelHashMap(1.0, 100.0, 20).update(torch.zeros(4, do.POINT_SIZE))
    with pytest.raises(NotImplementedError, match="width 771"):
        VoxelHashMap(1.0, 100.0, 20).update(np.zeros((4, 771)))
    k = KissICP(do.drive_config(oo.load_config))
    for width in (3, 7, 771):
        with pytest.raises(NotImplementedError, match="387 columns"):
            k.register_frame(np.zeros((4, width)), np.zeros(4), use_descriptors=True)
    with pytest.raises(ValueError, match="Invalid shape"):
        k.register_frame(np.zeros((4, 2)), np.zeros(4), use_descriptors=True)

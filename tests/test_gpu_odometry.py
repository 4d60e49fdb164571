"""The odometry front end on the GPU against tests/odometry_oracle.py: the range crop, the de-skew, the in-place update of the ICP
grid, ``VoxelHashMap.update`` and the ``KissICP`` loop.  Index lists, grids and poses are compared bit for bit; the de-skew is held to
8 B_i against the longdouble oracle (B_i = eps (|p_i| + |tau_i| + c): the factor 8 is the 4-ulp limit of the device's sin / cos times
two for the remaining roundings; the numpy fp64 form stays below 1.2 B on these inputs, tests/test_odometry_oracle.py, and the kernel
was measured at 1.07 B at most: each case prints its figure).  Outputs and
workspaces live in guarded buffers of exactly the documented sizes."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import odometry_oracle as oo  # noqa: E402
from tests.guarded import GuardedBuffer  # noqa: E402
from tests.icp_grid_cases import crowded_cloud  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _intact(bufs):
    for name, b in bufs.items():
        assert b.intact(), f"{name}: {b.intact()!r}"


# ------------------------------------------------------------------------------------------------------------------ crop
def _crop_rows(n, width, lo, hi, seed):
    rng = np.random.default_rng(seed)
    up, down = (lambda v: np.nextafter(v, np.inf)), (lambda v: np.nextafter(v, -np.inf))
    special = []
    for b in (lo, hi):
        for v in (b, up(b), down(b)):
            special += [[v, 0, 0], [0, -v, 0], [0, 0, v]]
        special += [[0.6 * b, 0.8 * b, 0.0], [0.0, -0.6 * b, 0.8 * b]]        # norms that round to the bound or next to it
    special += [[3.0, 4.0, 0.0], [0.0, 12.0, 16.0], [np.nan, 1.0, 1.0], [np.inf, 0, 0], [0, 0, 0]]
    special = np.array(special, dtype=np.float64)
    d = rng.normal(size=(max(n, 1), 3))
    xyz = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.0, 1.3 * hi, (max(n, 1), 1))
    near = rng.random(len(xyz)) < 0.2
    xyz[near] *= (rng.choice([lo, hi], near.sum()) / np.linalg.norm(xyz[near], axis=1))[:, None]       # a fifth of them next to a bound
    xyz = xyz[:n]
    k = min(n, len(special))
    xyz[rng.permutation(n)[:k]] = special[:k]
    return np.ascontiguousarray(np.c_[xyz, rng.normal(size=(n, width - 3))])


@pytest.mark.parametrize("width", [3, 7])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 66000])
def test_range_crop_equals_the_oracle(n, width):
    from vfmreg import _lib, ops
    lib = _lib.load()
    lo, hi = 5.0, 20.0
    rows_h = _crop_rows(n, width, lo, hi, seed=n + width)
    want = oo.range_crop(rows_h, lo, hi)
    if n >= 255:
        norm = oo.range_norm(rows_h)
        assert 0 < len(want) < n and (norm == lo).any() and (norm == hi).any()
        assert (norm == np.nextafter(lo, np.inf)).any() and (norm == np.nextafter(hi, -np.inf)).any()
    rows = GuardedBuffer((n, width), torch.float64, seed=1)
    if n:
        rows.set(rows_h)
    rows.poison_guards("nan")
    idx = GuardedBuffer(n, torch.int64, seed=2).fill_bytes(0xFF)
    count = GuardedBuffer(1, torch.int64, seed=3).fill_bytes(0xFF)
    _lib.check(lib.vfm_range_crop(rows.ptr() if n else None, n, width, lo, hi, idx.ptr() if n else None, count.ptr(), ops._stream()), "range_crop")
    torch.cuda.synchronize()
    _intact(dict(rows=rows, idx=idx, count=count))
    assert count.numpy().tolist() == [len(want)]
    got = idx.numpy()
    np.testing.assert_array_equal(got[:len(want)], want)
    assert (got[len(want):] == -1).all()                                       # nothing behind the count is written
    if n:
        i2, c2 = ops.range_crop(dev(rows_h), lo, hi)                           # the wrapper; the Preprocessor on top of it
        np.testing.assert_array_equal(i2[:int(c2.item())].cpu().numpy(), want)
        from vfmreg.preprocess import get_preprocessor
        cfg = oo.load_config(max_range=hi)
        kept = get_preprocessor(cfg)(rows_h)
        np.testing.assert_array_equal(kept, rows_h[want])


# ------------------------------------------------------------------------------------------------------------------ de-skew
@pytest.mark.parametrize("omega", [0.0, 1e-9, 1e-5, 1e-3, 0.3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_deskew_is_within_the_bound_of_the_longdouble_oracle(n, omega):
    from vfmreg import _lib, ops
    lib = _lib.load()
    rng = np.random.default_rng(n + int(omega * 1e9) % 977)
    width = 3 if n % 2 else 7
    d = rng.normal(size=(n, 3))
    xyz = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.choice([0.5, 10.0, 100.0], (n, 1))
    rows_h = np.ascontiguousarray(np.c_[xyz, rng.normal(size=(n, width - 3))])
    ax, ups = rng.normal(size=3), rng.normal(size=3)
    delta = np.r_[ups / np.linalg.norm(ups) * (3.0 if n == 5000 else rng.uniform(0, 3)), omega * ax / np.linalg.norm(ax)]
    t = rng.uniform(0.0, 1.0, n)
    if n >= 63:
        t[:2] = [0.0, 1.0]
    t[-1] = 0.5
    ref, tau = oo.deskew_ld(xyz, t, delta)
    B = oo.deskew_bound(xyz, t, delta, tau)
    rows = GuardedBuffer((n, width), torch.float64, seed=1).set(rows_h)
    stamps = GuardedBuffer(n, torch.float64, seed=2).set(t)
    rows.poison_guards("nan")
    stamps.poison_guards("nan")
    out = GuardedBuffer((n, 3), torch.float64, seed=3).fill_nan()
    _lib.check(lib.vfm_deskew_scan(rows.ptr(), n, width, stamps.ptr(), delta.ctypes.data, out.ptr(), ops._stream()), "deskew_scan")
    torch.cuda.synchronize()
    _intact(dict(rows=rows, stamps=stamps, out=out))
    got = out.numpy()
    err = np.abs(got.astype(np.longdouble) - ref).max(axis=1).astype(np.float64)
    print(f"n {n} omega {omega}: worst error / B = {(err / B).max():.3f}")
    assert np.isfinite(got).all() and (err <= 8 * B).all(), (err / B).max()
    np.testing.assert_array_equal(got[t == 0.5], xyz[t == 0.5])                # mid-scan: the identity, exactly
    np.testing.assert_array_equal(rows.numpy(), rows_h)                        # the input is not written
    # the module on top of it: other columns ride along; fewer than two poses: the frame as it is
    from oracle import oracle
    from vfmreg.deskew import MotionCompensator
    poses = [np.eye(4), oracle.se3_exp(delta)]
    moved = MotionCompensator().deskew_scan(rows_h, poses, t)
    np.testing.assert_array_equal(moved[:, 3:], rows_h[:, 3:])
    ref2, tau2 = oo.deskew_ld(xyz, t, MotionCompensator.delta(poses))
    err2 = np.abs(moved[:, :3].astype(np.longdouble) - ref2).max(axis=1).astype(np.float64)
    assert (err2 <= 8 * oo.deskew_bound(xyz, t, MotionCompensator.delta(poses), tau2)).all()


# ------------------------------------------------------------------------------------------------------------------ grid update
VS, CAP = 1.0, 20
_OLD = {}


def _old_map(n_old):
    """(the old points, the oracle map built from them) -- built once per size, never changed (callers copy the map)"""
    if n_old not in _OLD:
        p = crowded_cloud(n_old, VS, seed=11)
        if n_old > 1000:      # a voxel one short of the cap and one at the cap, away from the crowd
            p = np.r_[p, np.c_[30.0 + np.linspace(0.1, 0.9, CAP - 1), np.full(CAP - 1, 0.5), np.full(CAP - 1, 0.5)],
                      np.c_[31.0 + np.linspace(0.1, 0.9, CAP), np.full(CAP, 0.5), np.full(CAP, 0.5)]]
        m = oo.VoxelMap(VS, 15.0, CAP)
        m.update(p, None, None)
        _OLD[n_old] = (p, m)
    return _OLD[n_old]


def _pose():
    from oracle import oracle
    return oracle.se3_exp(np.array([0.7, -1.1, 0.4, 0.02, -0.03, 0.25]))


def _new_points(m, T, seed=12):
    """m points in the sensor frame; from 257 on their posed images hold three points for the voxel one short of the cap, two for the
    full one, and voxels before, after and between all old keys"""
    local = crowded_cloud(m, VS, seed=seed) * 1.2
    if m >= 257:
        world = np.array([[30.5, 0.5, 0.5], [30.25, 0.5, 0.5], [30.75, 0.5, 0.5], [31.5, 0.5, 0.5], [31.25, 0.5, 0.5],
                          [-40.5, 0.5, 0.5], [50.5, 0.5, 0.5], [29.5, 0.5, 0.5], [-40.5, -3.5, 0.5]])
        local[5:5 + len(world)] = (world - T[:3, 3]) @ T[:3, :3]
    return np.ascontiguousarray(local)


def _device_grid(p):
    from vfmreg.icp import VoxelGridDevice
    return VoxelGridDevice.from_device(dev(p.reshape(-1, 3)), VS, CAP)


def _rebuild_form(g, new_d, T, origin, max_distance):
    """the update made only of entry points the project had before: move, build the grid of (old points, new points) with the cap, drop the
    voxels whose first point is far with a torch mask"""
    from vfmreg import ops
    from vfmreg.icp import VoxelGridDevice
    moved = new_d if T is None or len(new_d) == 0 else ops.transform_xyz(new_d, dev(T))
    r = VoxelGridDevice.from_device(torch.cat((g.pts.reshape(-1, 3), moved)).contiguous(), VS, CAP)
    keys, start, pts = r.keys, r.start.long(), r.pts.reshape(-1, 3)
    if origin is not None and r.n_voxels:
        d = pts[start[:-1]] - dev(np.asarray(origin, dtype=np.float64))
        far = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) > max_distance * max_distance
        size = start[1:] - start[:-1]
        pts = pts[torch.repeat_interleave(~far, size)]
        keys = keys[~far]
        start = torch.cat((torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(size[~far], 0)))
    return keys.cpu().numpy(), start.cpu().numpy().astype(np.int32), pts.cpu().numpy()


def _run_update(n_old, m, T, origin, max_distance, new_h=None, expect_status=0):
    from vfmreg import _lib, ops
    lib = _lib.load()
    old_p, old_map = _old_map(n_old)
    ref = copy.deepcopy(old_map)
    ref.max_distance = max_distance
    g = _device_grid(old_p)
    ok, os_, op = old_map.grid()
    np.testing.assert_array_equal(g.keys.cpu().numpy(), ok)                     # the old grid IS the oracle's
    np.testing.assert_array_equal(g.start.cpu().numpy(), os_)
    np.testing.assert_array_equal(g.pts.cpu().numpy().reshape(-1, 3), op)
    if new_h is None:
        new_h = _new_points(m, T if T is not None else np.eye(4))
    nv, nk = g.n_voxels, g.n_kept
    ref.update(new_h, T, origin)
    new = GuardedBuffer((m, 3), torch.float64, seed=1)
    if m:
        new.set(new_h)
    new.poison_guards("nan")
    keys = GuardedBuffer(nv + m, torch.int64, seed=2).fill_bytes(0xFF)
    start = GuardedBuffer(nv + m + 1, torch.int32, seed=3).fill_bytes(0xFF)
    pts = GuardedBuffer((nk + m, 3), torch.float64, seed=4).fill_bytes(0xFF)
    info = GuardedBuffer(6, torch.int32, seed=5).fill_bytes(0xFF)
    ws_bytes = lib.vfm_icp_grid_update_workspace_bytes(nv, nk, m)
    assert ws_bytes > 0
    ws = GuardedBuffer(ws_bytes, torch.uint8, seed=6).fill_bytes(0xFF)
    Th = None if T is None else np.ascontiguousarray(T, dtype=np.float64)
    oh = None if origin is None else np.ascontiguousarray(origin, dtype=np.float64)
    _lib.check(lib.vfm_icp_grid_update(g.keys.data_ptr() if nv else None, g.start.data_ptr() if nv else None, g.pts.data_ptr() if nv else None,
                                       nv, nk, new.ptr() if m else None, m, None if Th is None else Th.ctypes.data, VS, CAP,
                                       None if oh is None else oh.ctypes.data, max_distance, keys.ptr(), start.ptr(), pts.ptr(), info.ptr(),
                                       ws.ptr(), ws_bytes, ops._stream()), "icp_grid_update")
    torch.cuda.synchronize()
    _intact(dict(new=new, keys=keys, start=start, pts=pts, info=info, ws=ws))
    got_info = info.numpy().tolist()
    rk, rs, rp = ref.grid()
    assert ref.status == expect_status
    assert got_info == ref.info(), (got_info, ref.info())
    n_voxels, n_kept = got_info[:2]
    k, s, q = keys.numpy(), start.numpy(), pts.numpy()
    np.testing.assert_array_equal(k[:n_voxels], rk)
    np.testing.assert_array_equal(s[:n_voxels + 1], rs)
    np.testing.assert_array_equal(q[:n_kept], rp)
    assert (k[n_voxels:] == -1).all() and (s[n_voxels + 1:] == -1).all()       # nothing behind the stated ranges is written
    assert (pts.body_bytes()[24 * n_kept:] == 0xFF).all()
    if m:
        np.testing.assert_array_equal(new.numpy(), new_h)                      # the inputs are not written
    np.testing.assert_array_equal(g.pts.cpu().numpy().reshape(-1, 3), op)
    if not expect_status:
        bk, bs, bp = _rebuild_form(g, dev(new_h.reshape(-1, 3)), T, origin, max_distance)
        np.testing.assert_array_equal(bk, rk)
        np.testing.assert_array_equal(bs, rs)
        np.testing.assert_array_equal(bp.reshape(-1, 3), rp)
    return ref, old_map, new_h


@pytest.mark.parametrize("m", [0, 1, 257, 5000])
@pytest.mark.parametrize("n_old", [0, 1, 70000])
def test_grid_update_equals_the_oracle_and_the_rebuild(n_old, m):
    T = _pose()
    ref, old_map, new_h = _run_update(n_old, m, T, T[:3, 3], 15.0)
    if n_old == 70000 and m >= 257:
        from oracle import oracle
        moved = oracle.transform_pcl(new_h, T)
        nk_, _ = oo.voxel_keys(moved, VS)
        uk, cnt = np.unique(nk_, return_counts=True)
        old_cnt = np.array([len(old_map.voxels.get(k, ())) for k in uk.tolist()])
        assert (moved < 0).any()
        assert ((old_cnt == CAP) & (cnt > 0)).any()                             # a full voxel takes nothing
        assert ((old_cnt < CAP) & (old_cnt > 0) & (old_cnt + cnt > CAP)).any()  # a partial take
        assert ((old_cnt == CAP - 1) & (cnt == 3)).any()                        # ... of the voxel one short of the cap
        ok = np.array(sorted(old_map.voxels))
        new_only = uk[old_cnt == 0]
        assert (new_only < ok[0]).any() and (new_only > ok[-1]).any() and ((new_only > ok[0]) & (new_only < ok[-1])).any()
        assert ref.last["voxels_removed"] > 100 and 0 < ref.last["points_added"] < m
        assert len(ref.voxels) > 100


def test_grid_update_without_removal_and_without_a_pose():
    ref, _, _ = _run_update(70000, 5000, None, None, 15.0)                      # plain AddPoints
    assert ref.last["voxels_removed"] == 0
    _run_update(70000, 257, _pose(), None, 15.0)
    _run_update(70000, 0, None, np.array([1.0, 2.0, 3.0]), 15.0)               # RemovePointsFarFromLocation alone


def test_grid_update_that_removes_every_voxel():
    for n_old, m in ((70000, 5000), (1, 1), (0, 257)):
        ref, _, _ = _run_update(n_old, m, _pose(), np.array([500.0, 0.0, 0.0]), 15.0)
        assert ref.info()[:2] == [0, 0] and ref.last["voxels_removed"] > 0


def test_grid_update_distance_is_strict():
    """a voxel whose first point is at exactly max_distance stays; one ulp beyond, it goes"""
    new_h = np.array([[6.0, 8.0, 0.0], [np.nextafter(10.0, 11.0), 0.0, 0.0], [0.0, 0.0, -10.0], [7.5, 8.0, 0.0]])
    ref, _, _ = _run_update(0, len(new_h), None, np.zeros(3), 10.0, new_h=np.ascontiguousarray(new_h))
    assert sorted(ref.points()[:, 0].tolist()) == [0.0, 6.0]


def test_grid_update_reports_a_coordinate_the_key_cannot_hold():
    new_h = _new_points(257, np.eye(4))
    new_h[100, 1] = float(1 << 20)
    _run_update(70000, 257, None, None, 15.0, new_h=new_h, expect_status=1)
    from vfmreg.mapping import VoxelHashMap
    vhm = VoxelHashMap(VS, 15.0, CAP)
    vhm.update(new_h[:50])
    before = vhm.point_cloud()
    with pytest.raises(ValueError, match="voxel coordinate outside"):
        vhm.update(new_h)
    np.testing.assert_array_equal(vhm.point_cloud(), before)                    # the map is left as it was


# ------------------------------------------------------------------------------------------------------------------ the map
def test_voxel_hash_map_update_then_register_frame():
    from oracle import oracle
    from vfmreg import icp
    from vfmreg.mapping import VoxelHashMap
    vs, cap, md = 0.5, 10, 8.0
    vhm, ref = VoxelHashMap(vs, md, cap), oo.VoxelMap(vs, md, cap)
    rng = np.random.default_rng(21)
    T = np.eye(4)
    for k in range(3):
        cloud = crowded_cloud(9000, vs, seed=30 + k) * 1.5
        T = oracle.se3_exp(np.array([0.8, 0.1, 0.0, 0.0, 0.0, 0.05])) @ T
        vhm.update(cloud, T)
        ref.update(cloud, T)
        assert vhm.last_update == ref.last
    assert ref.last["voxels_removed"] > 0 and ref.last["points_added"] < 9000
    rk, rs, rp = ref.grid()
    np.testing.assert_array_equal(vhm.point_cloud(), rp)                        # the set of points, in (voxel key, insertion) order
    g = icp._grid_of(vhm)
    np.testing.assert_array_equal(g.keys.cpu().numpy(), rk)
    np.testing.assert_array_equal(g.start.cpu().numpy(), rs)
    assert icp._grid_of(vhm) is g and not vhm.empty()                           # kept with the map: no rebuild
    scan = (rp[rng.permutation(len(rp))[:3000]] - T[:3, 3]) @ T[:3, :3] + rng.normal(0, 0.02, (3000, 3))
    guess = oracle.se3_exp(np.array([0.05, -0.04, 0.02, 0.0, 0.0, 0.01])) @ T
    got = icp.register_frame(scan, vhm, guess, 1.5, 0.2)
    want = oracle.register_frame(scan, rp, vs, guess, 1.5, 0.2)
    np.testing.assert_array_equal(got, want)
    assert np.abs(got - T).max() < 0.05 and not np.array_equal(got, guess)
    assert icp._grid_of(vhm) is g
    # remove_far_away_points, add_points and clear on such a map
    origin = T[:3, 3] + [6.0, 0.0, 0.0]
    vhm.remove_far_away_points(origin)
    ref.remove_far(origin)
    np.testing.assert_array_equal(vhm.point_cloud(), ref.points())
    more = crowded_cloud(2000, vs, seed=40)
    vhm.add_points(more)
    ref.update(more, None, None)
    g2 = icp._grid_of(vhm)
    rk, rs, rp = ref.grid()
    np.testing.assert_array_equal(g2.keys.cpu().numpy(), rk)
    np.testing.assert_array_equal(g2.pts.cpu().numpy().reshape(-1, 3), rp)
    assert sorted(map(tuple, vhm.point_cloud())) == sorted(map(tuple, rp))
    vhm.update(np.zeros((0, 3)), T)                                             # no points: the removal alone
    ref.update(np.zeros((0, 3)), T)
    np.testing.assert_array_equal(vhm.point_cloud(), ref.points())
    vhm.clear()
    assert vhm.empty() and vhm.point_cloud().shape == (0, 3)
    vhm.update(more[:10])
    assert len(vhm.point_cloud()) == 10


def test_a_map_that_was_never_updated_is_as_before():
    from oracle import oracle
    from vfmreg import icp
    from vfmreg.mapping import VoxelHashMap
    p = crowded_cloud(20000, 1.0, seed=50)
    vhm = VoxelHashMap(1.0, 100.0, 20)
    vhm.add_points(p[:12000])
    vhm.add_points(p[12000:])
    np.testing.assert_array_equal(vhm.point_cloud(), p[oracle.voxel_hash_map_points(p, 1.0, 20)])   # the container's order
    assert not hasattr(vhm, "last_update")
    keys, start, pts = oracle.voxel_grid_csr(vhm.point_cloud(), 1.0)
    g = icp._grid_of(vhm)
    np.testing.assert_array_equal(g.keys.cpu().numpy(), keys)
    np.testing.assert_array_equal(g.pts.cpu().numpy().reshape(-1, 3), pts)


# ------------------------------------------------------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def drive():
    scans, gt, stamps = oo.synthetic_drive()
    rng = np.random.default_rng(99)
    wide = [np.ascontiguousarray(np.c_[s, rng.normal(size=(len(s), 4))]) for s in scans]
    return dict(scans=scans, wide=wide, gt=gt, stamps=stamps)


def _run_oracle(frames, stamps, threshold, deskewed=None, deskew=False):
    k = oo.KissICP(oo.load_config(max_range=20, deskew=deskew), threshold)
    out = [k.register_frame(f, t, None if deskewed is None else deskewed[i]) for i, (f, t) in enumerate(zip(frames, stamps))]
    return k, out


@pytest.fixture(scope="module")
def oracle_run(drive):
    """the oracle loop on the 7-column frames (their first three columns are the 3-column drive), once"""
    return _run_oracle(drive["wide"], drive["stamps"], 0.0)


def _config(**kw):
    from vfmreg.config import load_config
    return load_config(max_range=20, **kw)


def _assert_same_run(k, got, ref_k, ref_out, columns=None):
    for f, ((pose, down, upd), (rpose, rdown, rupd)) in enumerate(zip(got, ref_out)):
        np.testing.assert_array_equal(pose, rpose, err_msg=f"pose of frame {f}")
        assert upd == rupd, f
        np.testing.assert_array_equal(down, rdown if columns is None else rdown[:, :columns], err_msg=f"rows of frame {f}")
    assert len(k.poses) == len(ref_k.poses)
    from vfmreg import icp
    g = icp._grid_of(k.local_map)
    rk, rs, rp = ref_k.local_map.grid()
    np.testing.assert_array_equal(g.keys.cpu().numpy(), rk)
    np.testing.assert_array_equal(g.start.cpu().numpy(), rs)
    np.testing.assert_array_equal(g.pts.cpu().numpy().reshape(-1, 3), rp)


def test_the_oracle_drive_is_not_vacuous(drive, oracle_run):
    ref_k, ref_out = oracle_run
    T0 = drive["gt"][0]
    err = [np.linalg.norm((T0 @ pose)[:3, 3] - gt[:3, 3]) for (pose, _, _), gt in zip(ref_out, drive["gt"])]
    print("trajectory error: worst %.4f m, at the end %.4f m" % (max(err), err[-1]))
    assert max(err) < 0.1                                                       # half a voxel (0.2 m) at every frame
    thresholds = sorted(set(ref_k.thresholds), reverse=True)
    print("thresholds:", [round(t, 3) for t in thresholds])
    assert len(thresholds) >= 3
    removed = sum(s["voxels_removed"] for s in ref_k.stats)
    refused = sum(s["offered"] - s["points_added"] for s in ref_k.stats)
    print("voxels removed:", removed, "points refused by the cap:", refused)
    assert removed > 1000 and refused > 0
    assert all(upd for _, _, upd in ref_out)


def test_kiss_icp_equals_the_oracle_loop(drive, oracle_run):
    from vfmreg.kiss_icp import KissICP
    ref_k, ref_out = oracle_run
    k = KissICP(_config())
    got = [k.register_frame(f, t) for f, t in zip(drive["scans"], drive["stamps"])]
    _assert_same_run(k, got, ref_k, ref_out, columns=3)
    assert k.local_map.last_update == ref_k.local_map.last


def test_kiss_icp_carries_descriptor_columns(drive, oracle_run):
    from vfmreg.kiss_icp import KissICP
    ref_k, ref_out = oracle_run
    k = KissICP(_config())
    got = [k.register_frame(f, t) for f, t in zip(drive["wide"], drive["stamps"])]
    assert got[-1][1].shape[1] == 7
    _assert_same_run(k, got, ref_k, ref_out)


def test_kiss_icp_skips_updates_below_the_motion_threshold(drive):
    from vfmreg.kiss_icp import KissICP
    ref_k, ref_out = _run_oracle(drive["scans"], drive["stamps"], 0.7)
    flags = [upd for _, _, upd in ref_out]
    assert not all(flags[:20]) and all(flags[21:]) and 2 < flags.count(False) < 20      # skipped in the slow half only
    k = KissICP(_config(), map_update_threshold=0.7)
    got = [k.register_frame(f, t) for f, t in zip(drive["scans"], drive["stamps"])]
    _assert_same_run(k, got, ref_k, ref_out)


def test_kiss_icp_with_deskew(drive):
    """de-skew is bounded, not bit-equal (its own test above): the oracle loop is fed the device's de-skewed points, and every pose has to
    be bit-equal from there"""
    from vfmreg.kiss_icp import KissICP
    k = KissICP(_config(deskew=True))
    ref_k = oo.KissICP(oo.load_config(max_range=20, deskew=True), 0.0)
    used = 0
    for f, (frame, t) in enumerate(zip(drive["scans"], drive["stamps"])):
        fed = None
        if len(k.poses) >= 2:
            fed = k.compensator.deskew_device(dev(frame), k.poses, dev(t)).cpu().numpy()
            own = oo.deskew(frame[:100], t[:100], oo.se3_log(np.linalg.inv(ref_k.poses[-2]) @ ref_k.poses[-1]))
            assert np.abs(fed[:100] - own).max() < 1e-12 and not np.array_equal(fed, frame)
            used += 1
        pose, down, upd = k.register_frame(frame, t)
        rpose, rdown, rupd = ref_k.register_frame(frame, t, fed)
        np.testing.assert_array_equal(pose, rpose, err_msg=f"pose of frame {f}")
        np.testing.assert_array_equal(down, rdown, err_msg=f"rows of frame {f}")
        assert upd == rupd
    assert used == len(drive["scans"]) - 2
    np.testing.assert_array_equal(k.local_map.point_cloud(), ref_k.local_map.points())


def test_kiss_icp_small_interfaces():
    from vfmreg.kiss_icp import KissICP
    k = KissICP(_config())
    assert not k.has_moved() and k.get_adaptive_threshold() == 2.0 and np.array_equal(k.get_prediction_model(), np.eye(4))
    pose, down, upd = k.register_frame(np.zeros((0, 3)), np.zeros(0))           # an empty scan
    assert np.array_equal(pose, np.eye(4)) and down.shape == (0, 3) and upd and k.local_map.empty()
    cloud = crowded_cloud(3000, 1.0, seed=60) * 2.0
    from oracle import oracle
    source, down = k.voxelize(cloud)
    want_down = oracle.voxel_down_sample(cloud, 0.2 * 0.5)
    np.testing.assert_array_equal(down, want_down)
    np.testing.assert_array_equal(source, oracle.voxel_down_sample(want_down, 0.2 * 1.5))
    pose, down, upd = k.register_frame(cloud * 0.01, np.zeros(len(cloud)))      # everything inside min_range: nothing survives the crop
    assert down.shape == (0, 3) and k.local_map.empty()

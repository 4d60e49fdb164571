"""The local map that carries descriptors, on the GPU against tests/odometry_desc_oracle.py: the grid update with provenance
(``vfm_icp_grid_update_src``), the payload's move (``vfm_rows_merge``), ``VoxelHashMap.update`` on 387-column rows and
``KissICP.register_frame(use_descriptors=True)``.  Everything is compared bit for bit; the C entries write into guarded buffers of
exactly the documented sizes."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import odometry_desc_oracle as do  # noqa: E402
from tests import odometry_oracle as oo  # noqa: E402
from tests import test_gpu_odometry as tgo  # noqa: E402  (the update test's clouds, pose and origin)
from tests.guarded import GuardedBuffer  # noqa: E402

VS, CAP = tgo.VS, tgo.CAP


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _intact(bufs):
    for name, b in bufs.items():
        assert b.intact(), f"{name}: {b.intact()!r}"


# ------------------------------------------------------------------------------------------------------------------ update with provenance
def _call_update(g, new_h, T, origin, max_distance, with_src):
    from vfmreg import _lib, ops
    lib = _lib.load()
    nv, nk, m = g.n_voxels, g.n_kept, len(new_h)
    new = GuardedBuffer((m, 3), torch.float64, seed=1)
    if m:
        new.set(new_h)
    new.poison_guards("nan")
    keys = GuardedBuffer(nv + m, torch.int64, seed=2).fill_bytes(0xFF)
    start = GuardedBuffer(nv + m + 1, torch.int32, seed=3).fill_bytes(0xFF)
    pts = GuardedBuffer((nk + m, 3), torch.float64, seed=4).fill_bytes(0xFF)
    info = GuardedBuffer(6, torch.int32, seed=5).fill_bytes(0xFF)
    src = GuardedBuffer(nk + m, torch.int32, seed=7).fill_bytes(0xFF)
    ws_bytes = lib.vfm_icp_grid_update_workspace_bytes(nv, nk, m)
    assert ws_bytes > 0
    ws = GuardedBuffer(ws_bytes, torch.uint8, seed=6).fill_bytes(0xFF)
    Th = np.ascontiguousarray(T, dtype=np.float64)
    oh = np.ascontiguousarray(origin, dtype=np.float64)
    head = (g.keys.data_ptr() if nv else None, g.start.data_ptr() if nv else None, g.pts.data_ptr() if nv else None, nv, nk,
            new.ptr() if m else None, m, Th.ctypes.data, VS, CAP, oh.ctypes.data, max_distance, keys.ptr(), start.ptr(), pts.ptr(), info.ptr())
    if with_src:
        _lib.check(lib.vfm_icp_grid_update_src(*head, src.ptr(), ws.ptr(), ws_bytes, ops._stream()), "icp_grid_update_src")
    else:
        _lib.check(lib.vfm_icp_grid_update(*head, ws.ptr(), ws_bytes, ops._stream()), "icp_grid_update")
    torch.cuda.synchronize()
    _intact(dict(new=new, keys=keys, start=start, pts=pts, info=info, src=src, ws=ws))
    return dict(keys=keys.numpy(), start=start.numpy(), pts=pts.numpy(), pts_bytes=pts.body_bytes(), info=info.numpy().tolist(),
                src=src.numpy())


@pytest.mark.parametrize("m", [0, 1, 257, 5000])
@pytest.mark.parametrize("n_old", [0, 1, 70000])
def test_update_with_provenance_equals_the_update_and_the_oracle(n_old, m):
    from oracle import oracle
    T = tgo._pose()
    origin, md = T[:3, 3], 15.0
    old_p, old_map = tgo._old_map(n_old)
    ref = copy.deepcopy(old_map)
    ref.max_distance = md
    g = tgo._device_grid(old_p)
    new_h = tgo._new_points(m, T)
    ref.update(new_h, T, origin)
    rk, rs, rp = ref.grid()
    plain = _call_update(g, new_h, T, origin, md, with_src=False)
    got = _call_update(g, new_h, T, origin, md, with_src=True)
    assert got["info"] == plain["info"] == ref.info()
    n_voxels, n_kept = got["info"][:2]
    for name in ("keys", "start", "pts"):                                       # bit for bit the plain entry's, written ranges and beyond
        np.testing.assert_array_equal(got[name].view(np.uint8), plain[name].view(np.uint8), err_msg=name)
    np.testing.assert_array_equal(got["keys"][:n_voxels], rk)
    np.testing.assert_array_equal(got["start"][:n_voxels + 1], rs)
    np.testing.assert_array_equal(got["pts"][:n_kept], rp)
    assert (got["pts_bytes"][24 * n_kept:] == 0xFF).all()
    assert (plain["src"] == -1).all()                                           # the plain entry has no such output
    src = got["src"]
    nk = g.n_kept
    assert (src[n_kept:] == -1).all()                                           # behind n_kept: untouched
    assert ((src[:n_kept] >= 0) & (src[:n_kept] < nk + m)).all() and len(np.unique(src[:n_kept])) == n_kept
    moved = oracle.transform_pcl(new_h, T) if m else np.zeros((0, 3))
    both = np.concatenate((g.pts.cpu().numpy().reshape(-1, 3), moved))
    np.testing.assert_array_equal(both[src[:n_kept]], got["pts"][:n_kept])
    if n_old == 70000 and m >= 257:
        assert (src[:n_kept] < nk).any() and (src[:n_kept] >= nk).any() and n_kept < nk + m
        assert ref.last["voxels_removed"] > 0 and 0 < ref.last["points_added"] < m


def test_the_provenance_entry_checks_its_arguments():
    from vfmreg import _lib
    lib = _lib.load()
    T = np.eye(4)
    args = lambda src: (None, None, None, 0, 0, 1, 7, T.ctypes.data, 1.0, 20, None, 10.0, 6, 7, 8, 9, src, 10, 1 << 30, None)  # noqa: E731
    assert lib.vfm_icp_grid_update_src(*args(None)) == -1 and b"src_out" in lib.vfm_last_error()
    assert lib.vfm_rows_merge(1, 5, 2, 5, 6, 3, 4, 10, 5, None) == -1 and b"row_bytes" in lib.vfm_last_error()
    assert lib.vfm_rows_merge(1, 5, 2, 5, 0, 3, 4, 10, 5, None) == -1 and b"row_bytes" in lib.vfm_last_error()
    assert lib.vfm_rows_merge(1, -1, 2, 5, 16, 3, 4, 10, 5, None) == -1 and b"sizes" in lib.vfm_last_error()
    assert lib.vfm_rows_merge(1, 5, 2, 5, 16, None, 4, 10, 5, None) == -1 and b"null" in lib.vfm_last_error()
    assert lib.vfm_rows_merge(None, 5, 2, 5, 16, 3, 4, 10, 5, None) == -1 and b"null" in lib.vfm_last_error()
    assert lib.vfm_rows_merge(1, 5, 2, 5, 16, 3, 4, 10, 1, None) == -1 and b"alias" in lib.vfm_last_error()
    assert lib.vfm_rows_merge(None, 0, None, 0, 16, None, None, 0, None, None) == 0            # n_max == 0: nothing to do


# ------------------------------------------------------------------------------------------------------------------ rows merge
def _merge(rows_old_h, rows_new_h, src_h, n_out, row_bytes, offset=0):
    """vfm_rows_merge on guarded buffers; ``offset``: bytes by which the old rows' base pointer is moved off its alignment"""
    from vfmreg import _lib, ops
    lib = _lib.load()
    nk, m, n_max = len(rows_old_h), len(rows_new_h), len(src_h)
    old = GuardedBuffer(nk * row_bytes + offset, torch.uint8, seed=1)
    if nk:
        old.t[offset:].copy_(torch.from_numpy(rows_old_h.reshape(-1)))
    new = GuardedBuffer(m * row_bytes, torch.uint8, seed=2)
    if m:
        new.set(rows_new_h.reshape(-1))
    src = GuardedBuffer(n_max, torch.int32, seed=3).set(src_h)
    src.poison_guards("zero")
    count = GuardedBuffer(1, torch.int32, seed=4).set(np.array([n_out], dtype=np.int32))
    out = GuardedBuffer(n_max * row_bytes, torch.uint8, seed=5).fill_bytes(0xFF)
    _lib.check(lib.vfm_rows_merge(old.ptr() + offset if nk else None, nk, new.ptr() if m else None, m, row_bytes, src.ptr(), count.ptr(), n_max,
                                  out.ptr(), ops._stream()), "rows_merge")
    torch.cuda.synchronize()
    _intact(dict(old=old, new=new, src=src, count=count, out=out))
    if nk:
        assert torch.equal(old.t[offset:].cpu(), torch.from_numpy(rows_old_h.reshape(-1)))     # the inputs are not written
    return out.numpy().reshape(n_max, row_bytes)


def _merge_case(nk, m, row_bytes, seed):
    rng = np.random.default_rng(seed)
    rows_old = rng.integers(0, 255, (nk, row_bytes), dtype=np.uint8)           # (no 0xFF byte: an unwritten output byte cannot pass for one)
    rows_new = rng.integers(0, 255, (m, row_bytes), dtype=np.uint8)
    src = rng.permutation(nk + m).astype(np.int32)                              # old and new rows interleaved, every row once
    return rows_old, rows_new, src


@pytest.mark.parametrize("nk,m", [(0, 5), (5, 0), (1, 1), (70000, 5000)])
@pytest.mark.parametrize("row_bytes", [4, 12, 16, 1536, 1548, 3072])
def test_rows_merge_equals_the_gather(row_bytes, nk, m):
    rows_old, rows_new, src = _merge_case(nk, m, row_bytes, seed=row_bytes + nk)
    both = np.concatenate((rows_old, rows_new))
    n_max = nk + m
    if n_max > 100:                                                             # two rows whose source is outside [0, nk + m): nothing is written
        src[[7, n_max // 2]] = [-1, nk + m]
    n_out = n_max - max(n_max // 3, 1)                                          # *n_out_dev below nk + m
    got = _merge(rows_old, rows_new, src, n_out, row_bytes)
    want = np.full((n_max, row_bytes), 0xFF, dtype=np.uint8)
    ok = (src[:n_out] >= 0) & (src[:n_out] < nk + m)
    want[:n_out][ok] = both[src[:n_out][ok]]
    np.testing.assert_array_equal(got, want)                                    # the gather; behind the count and for bad sources: untouched
    if (nk, m) == (1, 1) or (nk, row_bytes) == (70000, 1548):                   # *n_out_dev above n_max: n_max rows, no more
        short = src[:n_max - 1].copy()
        got = _merge(rows_old, rows_new, short, n_max + 1000, row_bytes)
        ok = (short >= 0) & (short < nk + m)
        want = np.full((n_max - 1, row_bytes), 0xFF, dtype=np.uint8)
        want[ok] = both[short[ok]]
        np.testing.assert_array_equal(got, want)


def test_rows_merge_from_a_base_pointer_off_16_bytes():
    rows_old, rows_new, src = _merge_case(3000, 500, 1536, seed=5)
    aligned = _merge(rows_old, rows_new, src, 3400, 1536)
    shifted = _merge(rows_old, rows_new, src, 3400, 1536, offset=4)            # the dword path: the same bytes out
    np.testing.assert_array_equal(shifted, aligned)
    np.testing.assert_array_equal(aligned[:3400], np.concatenate((rows_old, rows_new))[src[:3400]])
    assert (aligned[3400:] == 0xFF).all()


def test_the_wrappers_move_fp32_and_fp64_rows():
    from vfmreg import ops
    rng = np.random.default_rng(3)
    for dtype in (np.float32, np.float64):
        old, new = rng.normal(size=(40, 384)).astype(dtype), rng.normal(size=(9, 384)).astype(dtype)
        src = rng.permutation(49).astype(np.int32)
        out = ops.rows_merge(dev(old), dev(new), dev(src), dev(np.array([30], dtype=np.int32)))
        np.testing.assert_array_equal(out[:30].cpu().numpy(), np.concatenate((old, new))[src[:30]])
    xyz = tgo._new_points(257, np.eye(4))
    rows = rng.normal(size=(257, 384)).astype(np.float32)
    out = ops.icp_grid_update(None, None, None, dev(xyz), None, VS, CAP, None, 15.0, rows_new=dev(rows))
    plain = ops.icp_grid_update(None, None, None, dev(xyz), None, VS, CAP, None, 15.0)
    n_kept = int(out["info"][1])
    assert set(plain) == {"keys", "start", "pts", "info"} and torch.equal(plain["pts"][:n_kept], out["pts"][:n_kept])
    s = out["src"][:n_kept].cpu().numpy()
    np.testing.assert_array_equal(out["rows"][:n_kept].cpu().numpy(), rows[s])
    np.testing.assert_array_equal(out["pts"][:n_kept].cpu().numpy(), xyz[s])


# ------------------------------------------------------------------------------------------------------------------ the map
MAP_VS, MAP_CAP, MAP_MD = 1.0, 3, 6.0


def _map_blocks(dtype, seed=31):
    """five blocks of 600 rows in the sensor frame + their poses: ~3 points a voxel (the cap of 3 refuses some), the sensor advances 1.5 m
    a block (voxels fall behind max_distance 6); block 3 holds one descriptor twice, in two voxels"""
    from oracle import oracle
    rng = np.random.default_rng(seed)
    blocks, poses = [], []
    T = np.eye(4)
    for k in range(5):
        xyz = np.c_[rng.uniform(-5.0, 5.0, (600, 2)), rng.uniform(-1.0, 1.0, 600)]
        rows = np.c_[xyz, rng.normal(size=(600, do.DESCRIPTOR_SIZE))]
        if k == 3:      # (the first rows of their block, ahead of everything the blocks before covered: the cap takes them)
            rows[:2, :3] = [[4.5, 0.5, 0.5], [4.5, -2.5, 0.5]]
            rows[1, 3:] = rows[0, 3:]
        T = oracle.se3_exp(np.array([1.5, 0.1, 0.0, 0.0, 0.0, 0.04])) @ T
        blocks.append(np.ascontiguousarray(rows.astype(dtype)))
        poses.append(T)
    return blocks, poses


def _assert_same_map(vhm, ref, stats=True):
    np.testing.assert_array_equal(vhm.point_cloud_n(), ref.rows())
    if stats:
        assert vhm.last_update == ref.last
    assert vhm.empty_n() == ref.empty() and vhm.empty()
    np.testing.assert_array_equal(vhm.point_cloud(), ref.rows()[:, :3])        # map_ is empty: map_n_'s heads


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_voxel_hash_map_update_on_rows_that_carry_descriptors(dtype, on_device):
    from oracle import oracle
    from vfmreg import icp
    from vfmreg.mapping import VoxelHashMap
    blocks, poses = _map_blocks(dtype)
    vhm, ref = VoxelHashMap(MAP_VS, MAP_MD, MAP_CAP), do.RowVoxelMap(MAP_VS, MAP_MD, MAP_CAP)
    refused = removed = 0
    for rows, T in zip(blocks, poses):
        vhm.update(dev(rows) if on_device else rows, T)
        ref.update(rows, T)
        _assert_same_map(vhm, ref)
        refused += len(rows) - ref.last["points_added"]
        removed += ref.last["voxels_removed"]
    assert refused > 100 and removed > 20 and ref.full_voxels() > 20          # the cap and the removal acted
    assert vhm._device_map()[0].dtype == torch.float32
    if dtype == np.float32:
        assert vhm._device_map()[0].data_ptr() == vhm._chunks["n"][0][0].data_ptr()         # float32 rows: searched without a copy
    # the search: rows of the map under noise, and the descriptor that sits in two voxels
    map_rows = ref.rows()
    rng = np.random.default_rng(8)
    q = map_rows[rng.permutation(len(map_rows))[:60]].copy()
    q[:, 3:] += rng.normal(0.0, 0.05, (60, do.DESCRIPTOR_SIZE))
    twin = np.flatnonzero((map_rows[:, 3:] == blocks[3][0, 3:].astype(np.float64)).all(axis=1))
    assert len(twin) == 2 and oo.voxel_keys(map_rows[twin, :3], MAP_VS)[0][0] != oo.voxel_keys(map_rows[twin, :3], MAP_VS)[0][1]
    q = np.r_[q, map_rows[twin[1]:twin[1] + 1]]
    q[30:40, 3:] = rng.normal(size=(10, do.DESCRIPTOR_SIZE))                    # ... and some that match nothing
    qi, mi, _ = vhm.get_vfm_correspondence_indices(q, 0.8)
    _, want_tgt, want_qi, want_mi, _ = oracle.get_vfm_correspondences(q, map_rows, 0.8)
    np.testing.assert_array_equal(qi, want_qi)
    np.testing.assert_array_equal(mi, want_mi)
    assert 40 < len(qi) < 61 and mi[-1] == twin[0]                              # equal cosines: the lower grid row
    VoxelHashMap.quiet, was = True, VoxelHashMap.quiet
    try:
        s_xyz, t_xyz = vhm.get_vfm_correspondences(q, 0.8)
    finally:
        VoxelHashMap.quiet = was
    np.testing.assert_array_equal(t_xyz, want_tgt)
    np.testing.assert_array_equal(s_xyz, q[want_qi, :3])
    qk, mk, rank, _ = vhm.get_vfm_correspondence_indices_topk(q, 0.8, 2)
    np.testing.assert_array_equal(mk[rank == 0], want_mi)
    assert mk[(qk == 60) & (rank == 1)].tolist() == [twin[1]]
    # register_frame on 387-column points against the updated map: the ICP grid is the updated grid itself
    T = poses[-1]
    assert len(map_rows) > 200
    scan = map_rows[rng.permutation(len(map_rows))[:200]].copy()
    scan[:, :3] = (scan[:, :3] - T[:3, 3]) @ T[:3, :3] + rng.normal(0.0, 0.01, (200, 3))
    guess = oracle.se3_exp(np.array([0.05, -0.04, 0.02, 0.0, 0.0, 0.01])) @ T
    grid = vhm._wide_grid
    got = icp.register_frame(scan, vhm, guess, 1.5, 0.2)
    np.testing.assert_array_equal(got, oracle.register_frame_nd(scan, map_rows, MAP_VS, guess, 1.5, 0.2)[0])
    assert icp._grid_of(vhm.xyz_map()) is grid and not np.array_equal(got, guess)
    # remove_far_away_points alone
    origin = T[:3, 3] + [3.0, 0.0, 0.0]
    vhm.remove_far_away_points(origin)
    ref.remove_far(origin)
    assert ref.last["voxels_removed"] > 0 and vhm.last_update["voxels_removed"] == ref.last["voxels_removed"]
    assert vhm.last_update["points_removed"] == ref.last["points_removed"]
    _assert_same_map(vhm, ref, stats=False)
    # add_points on an updated map: plain AddPoints, the grid order kept
    vhm.add_points(blocks[0])
    ref.update(blocks[0], None, None)
    _assert_same_map(vhm, ref)
    # no rows: the removal alone; then clear() and reuse
    vhm.update(np.zeros((0, do.POINT_SIZE), dtype=dtype), poses[2])
    ref.update(np.zeros((0, do.POINT_SIZE)), poses[2])
    _assert_same_map(vhm, ref)
    vhm.clear()
    assert vhm.empty_n() and vhm.point_cloud_n().shape == (0, 3)
    ref = do.RowVoxelMap(MAP_VS, MAP_MD, MAP_CAP)
    vhm.update(blocks[3], poses[0])
    ref.update(blocks[3], poses[0])
    _assert_same_map(vhm, ref)


def test_a_map_filled_by_add_points_converts_at_its_first_update():
    from oracle import oracle
    from vfmreg.mapping import VoxelHashMap
    blocks, poses = _map_blocks(np.float32)
    vhm, ref = VoxelHashMap(MAP_VS, MAP_MD, MAP_CAP), do.RowVoxelMap(MAP_VS, MAP_MD, MAP_CAP)
    vhm.add_points(blocks[0])
    vhm.add_points(blocks[1])
    ref.update(blocks[0], None, None)
    ref.update(blocks[1], None, None)
    both = np.concatenate(blocks[:2]).astype(np.float64)
    np.testing.assert_array_equal(vhm.point_cloud_n(), both[oracle.voxel_hash_map_points(both, MAP_VS, MAP_CAP)])   # the container's order
    assert not hasattr(vhm, "last_update")
    vhm.update(blocks[2].astype(np.float64), poses[0])                          # mixed precisions: everything to double
    ref.update(blocks[2], poses[0])
    _assert_same_map(vhm, ref)
    assert vhm._chunks["n"][0][0].dtype == torch.float64
    with pytest.raises(ValueError, match="voxel coordinate outside"):
        bad = blocks[3].copy()
        bad[5, 1] = float(1 << 20)
        vhm.update(bad)
    _assert_same_map(vhm, ref)                                                  # the map is left as it was


# ------------------------------------------------------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def drive():
    frames, gt, stamps = do.descriptor_drive(14, 2500, 11)
    return dict(frames=frames, gt=gt, stamps=stamps)


def _oracle_run(frames, stamps, threshold):
    k = do.KissICPDesc(do.drive_config(oo.load_config), threshold)
    return k, [k.register_frame(f, t) for f, t in zip(frames, stamps)]


def _device_run(frames, stamps, threshold):
    from vfmreg.config import load_config
    from vfmreg.kiss_icp import KissICP
    k = KissICP(do.drive_config(load_config), map_update_threshold=threshold)
    return k, [k.register_frame(f, t, use_descriptors=True) for f, t in zip(frames, stamps)]


def _assert_same_run(k, got, ref_k, ref_out):
    for f, ((pose, down, upd), (rpose, rdown, rupd)) in enumerate(zip(got, ref_out)):
        np.testing.assert_array_equal(pose, rpose, err_msg=f"pose of frame {f}")
        assert upd == rupd, f
        np.testing.assert_array_equal(down, rdown, err_msg=f"rows of frame {f}")
    assert len(k.poses) == len(ref_k.poses) and k.local_map.empty()
    np.testing.assert_array_equal(k.local_map.point_cloud_n(), ref_k.local_map.rows())
    assert k.local_map.last_update == ref_k.local_map.last


def test_kiss_icp_with_descriptors_equals_the_oracle_loop(drive):
    ref_k, ref_out = _oracle_run(drive["frames"], drive["stamps"], 0.0)
    assert len(ref_k.history) == 13 and all(any(h[0] == "vfm" for h in hist) for hist in ref_k.history)
    k, got = _device_run(drive["frames"], drive["stamps"], 0.0)
    assert got[-1][1].shape[1] == do.POINT_SIZE and all(upd for _, _, upd in got)
    _assert_same_run(k, got, ref_k, ref_out)


def test_kiss_icp_with_descriptors_on_float32_frames(drive):
    frames = [f.astype(np.float32) for f in drive["frames"]]
    ref_k, ref_out = _oracle_run(frames, drive["stamps"], 0.0)
    k, got = _device_run(frames, drive["stamps"], 0.0)
    _assert_same_run(k, got, ref_k, ref_out)
    assert k.local_map._chunks["n"][0][0].dtype == torch.float32 and got[-1][1].dtype == np.float64


def test_kiss_icp_with_descriptors_skips_updates_below_the_motion_threshold(drive):
    ref_k, ref_out = _oracle_run(drive["frames"], drive["stamps"], 0.7)
    flags = [upd for _, _, upd in ref_out]
    assert 2 < flags.count(False) < len(flags) - 2                              # some frames update the map, some do not
    k, got = _device_run(drive["frames"], drive["stamps"], 0.7)
    _assert_same_run(k, got, ref_k, ref_out)

"""The k-best descriptor search at 640 / 768 columns (the 4-wave form of ``match_topk_coarse_kernel``, csrc/match_topk.hip) and on
operands prepared beforehand (``ops.match_ip_topk_prepared``, the image ``VoxelHashMap.search_device_topk`` keeps) against the oracle of
tests/topk_oracle.py: ``idx`` and ``sim`` EQUAL bit for bit, and ``info`` says that the matrix-core path answered."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import topk_oracle as to  # noqa: E402

FAST, EXACT = 0, 1
INFO = ("max_records", "fallback", "slices", "reserved")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def run(q, b, k, prec=FAST):
    from vfmreg import ops
    idx, sim, info = ops.match_ip_topk(dev(q), dev(b), k, prec, return_info=True)
    return idx.cpu().numpy(), sim.cpu().numpy(), dict(zip(INFO, info.cpu().tolist()))


def equal(idx, sim, want, msg=""):
    np.testing.assert_array_equal(idx, want[0], err_msg=msg)
    np.testing.assert_array_equal(sim.view(np.uint32), want[1].view(np.uint32), err_msg=msg)


def check(q, b, k, prec=FAST, msg="", want=None):
    idx, sim, info = run(q, b, k, prec)
    print(f"{msg} n={len(q)} m={len(b)} d={q.shape[1]} k={k} prec={prec}: {info}")
    equal(idx, sim, want if want is not None else to.topk(q, b, k), msg)
    assert info["reserved"] == 0
    return idx, sim, info


@functools.lru_cache(maxsize=None)
def rows(n, m, d, seed=0, common=False):
    return to.gaussian_rows(n, m, d, seed, common)


@functools.lru_cache(maxsize=None)
def oracle8(n, m, d, seed=0, common=False):
    """the oracle's eight best of rows(...): computed once, read-only; its first k columns are the oracle's answer for k (the oracle
    picks round by round among the rows not yet chosen)"""
    idx, sim = to.topk(*rows(n, m, d, seed, common), 8)
    idx.setflags(write=False)
    sim.setflags(write=False)
    return idx, sim


def oracle(n, m, d, k, seed=0, common=False):
    idx, sim = oracle8(n, m, d, seed, common)
    return idx[:, :k], sim[:, :k]


# ------------------------------------------------------------------------------------------------- 1. every tiling edge
# every N of {1, 33, 129, 257} (a wide workgroup holds 128 queries), M of {1, 5, 127, 129, 300, 4097} (4097: two launches, the second
# in two slices), d of {640, 768} and k of {1, 2, 5, 8}; M < k among them
WIDE_SHAPES = [(1, 1, 640, 1), (1, 5, 768, 8), (33, 127, 640, 2), (33, 129, 768, 5), (129, 300, 640, 8), (257, 4097, 768, 8),
               (33, 4097, 640, 5), (257, 1, 768, 2), (129, 300, 768, 5), (257, 5, 640, 8), (1, 127, 768, 1), (129, 129, 640, 1),
               (1, 4097, 640, 2), (129, 4097, 768, 2), (257, 300, 640, 2)]


@pytest.mark.parametrize("n,m,d,k", WIDE_SHAPES)
def test_fast_equals_the_oracle_across_the_tiling_edges(n, m, d, k):
    q, b = rows(n, m, d)
    _, _, info = check(q, b, k, FAST, want=oracle(n, m, d, k))
    assert info["slices"] >= 1, "FAST at d = 640 / 768 runs the matrix-core pass"


# ------------------------------------------------------------------------------------------------- 2. the fast path answered
@pytest.mark.parametrize("common", [False, True], ids=["gaussian", "common-component"])
@pytest.mark.parametrize("d", [640, 768])
def test_matrix_core_path_answers_ordinary_data(d, common):
    """tools/sim_topk_records.py gives at most ~215 records per query at this shape: a query that overflows a list of 1024 here is a
    kernel fault, not bad luck -- and a FAST mode that quietly ran the all-pairs kernel would report every query as a fallback."""
    from vfmreg import ops
    q, b = rows(257, 4097, d, 1, common)
    _, _, info = check(q, b, 8, FAST, msg="common" if common else "gaussian", want=oracle(257, 4097, d, 8, 1, common))
    assert info["fallback"] == 0
    assert 8 <= info["max_records"] <= ops.MATCH_TOPK_RECORD_CAP
    assert info["slices"] >= 1


# ------------------------------------------------------------------------------------------------- 3. k = 1 is the top-1 search
def test_k1_equals_the_top1_search_at_768():
    from vfmreg import ops
    q, b = rows(257, 4097, 768, 2)
    rng = np.random.default_rng(3)
    q2, b2 = q.copy(), b.copy()
    b2[rng.integers(0, 4097, 600)] = b2[rng.integers(0, 4097, 600)]   # duplicated map rows
    q2[:40] = b2[rng.integers(0, 4097, 40)]                           # queries that ARE map rows (several tie at the top)
    q2[[7, 100, 256]] = 0                                             # zero rows on both sides
    b2[[0, 5, 4096]] = 0
    for name, qq, bb in (("gaussian", q, b), ("duplicates and zero rows", q2, b2)):
        want = to.topk(qq, bb, 5)
        idx, sim, _ = check(qq, bb, 1, FAST, msg=name, want=(want[0][:, :1], want[1][:, :1]))
        i1, s1 = ops.match_ip_top1(dev(qq), dev(bb))
        np.testing.assert_array_equal(idx[:, 0], i1.cpu().numpy(), err_msg=name)
        np.testing.assert_array_equal(sim[:, 0].view(np.uint32), s1.cpu().numpy().view(np.uint32), err_msg=name)
        check(qq, bb, 5, FAST, msg=name, want=want)


# ------------------------------------------------------------------------------------------------- 4. ties, overflow, worst order
def test_three_copies_of_every_map_row_come_in_index_order_at_768():
    rng = np.random.default_rng(4)
    base = rng.standard_normal((500, 768)).astype(np.float32)
    b = np.repeat(base, 3, axis=0)[rng.permutation(1500)]             # each distinct row three times, at scattered indices
    q = (base[rng.integers(0, 500, 64)] + 0.05 * rng.standard_normal((64, 768))).astype(np.float32)
    idx, sim, info = check(q, b, 5, FAST)
    assert info["slices"] >= 1
    assert (sim[:, 0] == sim[:, 1]).all() and (sim[:, 1] == sim[:, 2]).all() and (sim[:, 3] == sim[:, 4]).all()
    assert (idx[:, 0] < idx[:, 1]).all() and (idx[:, 1] < idx[:, 2]).all() and (idx[:, 3] < idx[:, 4]).all()
    assert (b[idx[:, 0]] == b[idx[:, 2]]).all()


def test_more_copies_of_a_row_than_a_list_holds_fall_back_to_all_pairs_at_768():
    from vfmreg import ops
    rng = np.random.default_rng(5)
    b = rng.standard_normal((2048, 768)).astype(np.float32)
    assert ops.MATCH_TOPK_RECORD_CAP < 1500
    b[rng.permutation(2048)[:1500]] = b[0]                            # one row 1500 times: every copy is inside every window
    q = rng.standard_normal((33, 768)).astype(np.float32)
    q[0] = b[0]
    _, _, info = check(q, b, 8, FAST)
    assert info["fallback"] >= 1 and info["max_records"] > ops.MATCH_TOPK_RECORD_CAP and info["slices"] >= 1


def test_map_sorted_ascending_by_score_at_768():
    from oracle import oracle as orc
    q, b = rows(33, 4097, 768, 6)
    qn, _ = orc.l2norm_rows(q)
    bn, _ = orc.l2norm_rows(b)
    b = b[np.argsort(bn.astype(np.float64) @ qn[0].astype(np.float64), kind="stable")]   # every step raises query 0's bound
    want = to.topk(q, b, 8)
    check(q, b, 8, FAST, want=want)
    check(q, b, 2, FAST, want=(want[0][:, :2], want[1][:, :2]))


# ------------------------------------------------------------------------------------------------- 5. the two kernels agree
@pytest.mark.parametrize("d", [640, 768])
def test_fast_equals_exact(d):
    q, b = rows(33, 300, d)
    f_idx, f_sim, f_info = check(q, b, 5, FAST, want=oracle(33, 300, d, 5))
    e_idx, e_sim, e_info = check(q, b, 5, EXACT, want=oracle(33, 300, d, 5))
    assert f_info["slices"] >= 1 and (e_info["max_records"], e_info["fallback"], e_info["slices"]) == (0, 33, 0)
    equal(f_idx, f_sim, (e_idx, e_sim))


# ------------------------------------------------------------------------------------------------- 6. prepared operands
@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("m", [129, 4097])
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("d", [128, 256, 384, 640, 768])   # ops.MATCH_TOPK_FAST_WIDTHS
def test_prepared_entry_equals_the_unprepared_call(d, n, m, k):
    from vfmreg import ops
    q, b = rows(n, m, d)
    qd, bd = dev(q), dev(b)
    idx, sim, info = ops.match_ip_topk_prepared(ops.PreparedRows(qd), ops.PreparedRows(bd), k, return_info=True)
    u_idx, u_sim, u_info = ops.match_ip_topk(qd, bd, k, FAST, return_info=True)
    info, u_info = info.cpu().tolist(), u_info.cpu().tolist()
    print(f"n={n} m={m} d={d} k={k}: prepared {info}, unprepared {u_info}")
    equal(idx.cpu().numpy(), sim.cpu().numpy(), (u_idx.cpu().numpy(), u_sim.cpu().numpy()), "prepared vs unprepared")
    assert info[1] == u_info[1] and info[2] >= 1 and info[3] == 0
    equal(idx.cpu().numpy(), sim.cpu().numpy(), oracle(n, m, d, k), "prepared vs oracle")


@pytest.mark.parametrize("d", [128, 256, 384, 640, 768])   # ops.MATCH_TOPK_FAST_WIDTHS
def test_a_prepared_map_is_left_as_it_was(d):
    from vfmreg import ops
    _, b = rows(257, 4097, d)
    bp = ops.PreparedRows(dev(b))
    image = bp.buf.clone()
    queries = [rows(257, 4097, d)[0], rows(33, 4097, d, 11)[0], rows(129, 300, d, 12)[0]]
    wants = [oracle(257, 4097, d, 8)] + [to.topk(q, b, 8) for q in queries[1:]]
    first = []
    for q, want in zip(queries, wants):
        idx, sim = ops.match_ip_topk_prepared(ops.PreparedRows(dev(q)), bp, 8)
        equal(idx.cpu().numpy(), sim.cpu().numpy(), want)
        first.append((idx, sim))
    qp = ops.PreparedRows(dev(queries[1]))
    i1, s1 = ops.match_search(qp, bp)                                  # an unrelated top-1 search on the same prepared map
    np.testing.assert_array_equal(i1.cpu().numpy(), wants[1][0][:, 0])
    np.testing.assert_array_equal(s1.cpu().numpy().view(np.uint32), wants[1][1][:, 0].view(np.uint32))
    for q, (idx0, sim0) in zip(queries, first):
        idx, sim = ops.match_ip_topk_prepared(ops.PreparedRows(dev(q)), bp, 8)
        assert torch.equal(idx, idx0) and torch.equal(sim.view(torch.int32), sim0.view(torch.int32))
    assert torch.equal(bp.buf, image)


def test_prepared_entry_refuses_widths_without_a_kernel():
    from vfmreg import ops

    def unprepared(rows, d):   # vfm_match_prepare itself refuses 33 columns: an object with a prepared operand's fields, image unwritten
        p = ops.PreparedRows.__new__(ops.PreparedRows)
        p.x, p.rows, p.d, p.buf = dev(np.ones((rows, d))), rows, d, torch.zeros(256, dtype=torch.uint8, device="cuda")
        return p

    for dq, db in ((512, 512), (128, 384)):
        with pytest.raises(ValueError, match="Invalid shape"):
            ops.match_ip_topk_prepared(ops.PreparedRows(dev(np.ones((4, dq)))), ops.PreparedRows(dev(np.ones((8, db)))), 2)
    with pytest.raises(ValueError, match="Invalid shape"):
        ops.match_ip_topk_prepared(unprepared(4, 33), unprepared(8, 33), 2)
    with pytest.raises(ValueError, match="k must be"):
        ops.match_ip_topk_prepared(ops.PreparedRows(dev(np.ones((4, 128)))), ops.PreparedRows(dev(np.ones((8, 128)))), 9)


# ------------------------------------------------------------------------------------------------- 7. the map keeps its operand
def search_map(vm, qd, k, thr=0.8):
    _, _, _, sim = vm.search_device_topk(None, thr, k, q_desc=dev(qd))
    return sim.cpu().numpy()


def test_map_keeps_its_prepared_operand():
    from vfmreg.mapping import VoxelHashMap
    VoxelHashMap.quiet = True
    rng = np.random.default_rng(13)
    q, b = rows(257, 4097, 384)
    vm = VoxelHashMap(0.01, 1.0e9, 20)
    vm.add_points(np.c_[rng.uniform(-500, 500, (len(b), 3)).astype(np.float32), b])
    mp = vm.point_cloud_n()[:, 3:].astype(np.float32)                  # the map's rows in the container's order
    assert len(mp) == len(b) and vm._prep is None
    want = to.topk(q, mp, 8)
    np.testing.assert_array_equal(search_map(vm, q, 8).view(np.uint32), want[1].view(np.uint32))
    prep = vm._prep
    assert prep is not None
    np.testing.assert_array_equal(search_map(vm, q[:33], 4).view(np.uint32), want[1][:33, :4].view(np.uint32))
    assert vm._prep is prep, "the second k-best search prepared the map again"
    qi, mi, _ = vm.search_device(None, 0.0, q_desc=dev(q))             # the top-1 search shares the image
    assert vm._prep is prep, "the top-1 search prepared the map again"
    reach = want[1][:, 0] >= 0.0
    np.testing.assert_array_equal(qi.cpu().numpy(), np.nonzero(reach)[0])
    np.testing.assert_array_equal(mi.cpu().numpy(), want[0][reach, 0])
    # an update drops the operand; the next search prepares the new map
    extra = rows(5, 1, 384, 14)[0]
    vm.update(np.c_[rng.uniform(-500, 500, (5, 3)).astype(np.float32), extra])
    assert vm._prep is None
    mp = vm.point_cloud_n()[:, 3:].astype(np.float32)
    assert len(mp) == len(b) + 5
    want = to.topk(q[:129], mp, 8)
    _, mi, _, sim = vm.search_device_topk(None, -1.0, 8, q_desc=dev(q[:129]))
    np.testing.assert_array_equal(sim.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    np.testing.assert_array_equal(mi.cpu().numpy(), want[0].reshape(-1))
    assert vm._prep is not None and vm._prep is not prep


def test_wide_map_is_searched_on_the_matrix_cores():
    from vfmreg import ops
    from vfmreg.mapping import VoxelHashMap
    VoxelHashMap.quiet = True
    rng = np.random.default_rng(15)
    q, b = rows(257, 4097, 768)
    xyz = rng.uniform(-500, 500, (len(b), 3))
    vm = VoxelHashMap(0.01, 1.0e9, 20)
    vm.add_points_device(dev(np.c_[xyz, b]), torch.from_numpy(xyz).cuda())
    mp = vm.point_cloud_n()[:, 3:].astype(np.float32)
    assert len(mp) == len(b)
    want = to.topk(q, mp, 8)
    _, mi, _, sim = vm.search_device_topk(None, -1.0, 8, q_desc=dev(q))
    np.testing.assert_array_equal(sim.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    np.testing.assert_array_equal(mi.cpu().numpy(), want[0].reshape(-1))
    # the method returns no info: the same search on the operand the map kept
    assert vm._prep is not None and vm._prep.d == 768
    idx, sim, info = ops.match_ip_topk_prepared(ops.PreparedRows(dev(q)), vm._prep, 8, return_info=True)
    equal(idx.cpu().numpy(), sim.cpu().numpy(), want)
    info = dict(zip(INFO, info.cpu().tolist()))
    assert info["fallback"] == 0 and info["slices"] >= 1 and 8 <= info["max_records"] <= ops.MATCH_TOPK_RECORD_CAP


# ------------------------------------------------------------------------------------------------- 8. through the node
def test_node_with_a_kept_map_prepares_it_once():
    from vfmreg import synth
    from vfmreg.mapping import VoxelHashMap
    from vfmreg.registration import RegistrationNode
    VoxelHashMap.quiet = True
    p = synth.make_pair(4000, 20000, 128, seed=9, outlier=0.2, noise_m=0.01)
    voxel_map = np.c_[p["b_xyz"], p["b_desc"]]
    raw_scan = np.c_[p["q_xyz"], p["q_desc"]]
    kw = dict(ransac_iterations=20000, max_correspondence_distance=0.5, vfm_candidates=4)
    fresh, kept = RegistrationNode(cache_map=False, **kw), RegistrationNode(cache_map=True, **kw)
    pose0 = fresh.ransac_registration(voxel_map, raw_scan)[0]
    s0, t0 = fresh.compute_vfm_correspondences(voxel_map, raw_scan)
    pose1 = kept.ransac_registration(voxel_map, raw_scan)[0]
    vm = kept._map_cache[2]
    prep = vm._prep
    assert prep is not None
    np.testing.assert_array_equal(pose1, pose0)
    pose2 = kept.ransac_registration(voxel_map, raw_scan)[0]
    s1, t1 = kept.compute_vfm_correspondences(voxel_map, raw_scan)
    assert kept._map_cache[2] is vm and vm._prep is prep, "a later call on the kept map prepared it again"
    np.testing.assert_array_equal(pose2, pose0)
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(t1, t0)
    assert len(s0) >= 75 and np.linalg.norm(pose0 - p["T_gt"]) < 0.05

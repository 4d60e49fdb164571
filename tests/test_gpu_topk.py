"""The exact k-best descriptor search on the GPU (csrc/match_topk.hip, ``ops.match_ip_topk``) and what stands on it
(``VoxelHashMap.get_vfm_correspondence_indices_topk``, ``RegistrationNode(vfm_candidates=k)``) against the oracle of
tests/topk_oracle.py: ``idx`` and ``sim`` EQUAL bit for bit -- across every tiling edge, in both precision modes, with ties, with more
near-copies than a record list holds, with the map in the worst order, across map slices -- and ``info`` says that the matrix-core
path, not the all-pairs kernel, answered the ordinary cases."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import topk_oracle as to  # noqa: E402

FAST, EXACT = 0, 1


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def run(q, b, k, prec=FAST):
    from vfmreg import ops
    idx, sim, info = ops.match_ip_topk(dev(q), dev(b), k, prec, return_info=True)
    return idx.cpu().numpy(), sim.cpu().numpy(), dict(zip(("max_records", "fallback", "slices", "reserved"), info.cpu().tolist()))


def check(q, b, k, prec=FAST, msg=""):
    idx, sim, info = run(q, b, k, prec)
    want_idx, want_sim = to.topk(q, b, k)
    print(f"{msg} n={len(q)} m={len(b)} d={q.shape[1]} k={k} prec={prec}: {info}")
    np.testing.assert_array_equal(idx, want_idx, err_msg=msg)
    np.testing.assert_array_equal(sim.view(np.uint32), want_sim.view(np.uint32), err_msg=msg)
    assert info["reserved"] == 0
    return idx, sim, info


@functools.lru_cache(maxsize=None)
def rows(n, m, d, seed=0, common=False):
    return to.gaussian_rows(n, m, d, seed, common)


# ------------------------------------------------------------------------------------------------- 1. every tiling edge
# every N of {1, 33, 257}, M of {1, 5, 127, 129, 300, 4097}, d of {128, 384} and k of {1, 2, 5, 8}; M < k among them; then d = 256
# (match_topk_coarse_kernel<16, 8>) at every N and k, M of {1, 129, 300, 4097}
FAST_SHAPES = [(1, 1, 128, 1), (1, 5, 384, 8), (33, 127, 128, 2), (33, 129, 384, 5), (257, 300, 128, 8), (257, 4097, 384, 8),
               (33, 4097, 128, 5), (257, 1, 384, 2), (1, 300, 128, 5), (257, 5, 128, 8), (1, 127, 384, 1), (257, 129, 128, 1),
               (1, 4097, 128, 2), (33, 300, 384, 2),
               (1, 1, 256, 1), (33, 129, 256, 5), (257, 300, 256, 8), (257, 4097, 256, 8), (33, 4097, 256, 2), (1, 300, 256, 5),
               (257, 129, 256, 1), (1, 4097, 256, 8)]
# the same N, M and k at d of {33, 128, 512}; then the two sides of the row norm's paths: d = 1024 is the last width whose sum of
# squares takes the float4 chunks (all four of a lane in use), d = 1028 the first multiple of 4 that takes the element loop
EXACT_SHAPES = [(1, 1, 33, 1), (33, 5, 128, 8), (257, 300, 512, 5), (33, 129, 33, 2), (1, 127, 512, 8), (257, 4097, 33, 8),
                (33, 4097, 128, 1), (257, 1, 128, 2), (1, 300, 33, 5), (33, 127, 512, 2), (33, 129, 1024, 2), (33, 129, 1028, 2)]


@pytest.mark.parametrize("n,m,d,k", FAST_SHAPES)
def test_fast_equals_the_oracle_across_the_tiling_edges(n, m, d, k):
    q, b = rows(n, m, d)
    _, _, info = check(q, b, k, FAST)
    assert info["slices"] >= 1, "FAST at d = 128 / 256 / 384 runs the matrix-core pass"


@pytest.mark.parametrize("n,m,d,k", EXACT_SHAPES)
def test_exact_equals_the_oracle_across_the_same_shapes(n, m, d, k):
    q, b = rows(n, m, d)
    _, _, info = check(q, b, k, EXACT)
    assert (info["max_records"], info["fallback"], info["slices"]) == (0, n, 0)


@pytest.mark.parametrize("n,m,d,k", [(33, 300, 512, 5), (257, 129, 33, 8), (1, 4097, 512, 2)])
def test_fast_at_a_width_without_a_kernel_runs_exact(n, m, d, k):
    q, b = rows(n, m, d)
    idx, sim, info = check(q, b, k, FAST)
    assert (info["max_records"], info["fallback"], info["slices"]) == (0, n, 0)
    e_idx, e_sim, _ = run(q, b, k, EXACT)
    np.testing.assert_array_equal(idx, e_idx)
    np.testing.assert_array_equal(sim.view(np.uint32), e_sim.view(np.uint32))


def test_no_map_rows_is_all_padding():
    idx, sim, info = run(np.ones((5, 128), np.float32), np.zeros((0, 128), np.float32), 3)
    assert (idx == -1).all() and (sim == np.finfo(np.float32).min).all() and info["fallback"] == 0
    from vfmreg import ops
    i0, s0 = ops.match_ip_topk(dev(np.zeros((0, 128))), dev(np.ones((7, 128))), 2)
    assert tuple(i0.shape) == (0, 2) and tuple(s0.shape) == (0, 2)
    with pytest.raises(ValueError, match="k must be"):
        ops.match_ip_topk(dev(np.ones((2, 128))), dev(np.ones((7, 128))), 9)


# ------------------------------------------------------------------------------------------------- 2. the fast path answered
@pytest.mark.parametrize("common", [False, True], ids=["gaussian", "common-component"])
@pytest.mark.parametrize("d", [128, 256, 384])
def test_matrix_core_path_answers_ordinary_data(d, common):
    """tools/sim_topk_records.py gives at most ~250 records per query on these cases: a query that overflows a list of 1024 here is a
    kernel fault, not bad luck -- and a FAST mode that quietly ran the all-pairs kernel would report every query as a fallback."""
    from vfmreg import ops
    q, b = rows(257, 4097, d, 1, common)
    _, _, info = check(q, b, 8, FAST, msg="common" if common else "gaussian")
    assert info["fallback"] == 0
    assert 8 <= info["max_records"] <= ops.MATCH_TOPK_RECORD_CAP
    assert info["slices"] >= 1


# ------------------------------------------------------------------------------------------------- 3. k = 1 is today's search
def _k1_equals_the_top1_search(d):
    from vfmreg import ops
    q, b = rows(257, 4097, d, 2)
    cases = [("gaussian", q, b)]
    rng = np.random.default_rng(3)
    q2, b2 = q.copy(), b.copy()
    b2[rng.integers(0, 4097, 600)] = b2[rng.integers(0, 4097, 600)]   # duplicated map rows
    q2[:40] = b2[rng.integers(0, 4097, 40)]                           # queries that ARE map rows (several tie at the top)
    q2[[7, 100, 256]] = 0                                             # zero rows on both sides
    b2[[0, 5, 4096]] = 0
    cases.append(("duplicates and zero rows", q2, b2))
    for name, qq, bb in cases:
        idx, sim, _ = check(qq, bb, 1, FAST, msg=name)
        i1, s1 = ops.match_ip_top1(dev(qq), dev(bb))
        np.testing.assert_array_equal(idx[:, 0], i1.cpu().numpy(), err_msg=name)
        np.testing.assert_array_equal(sim[:, 0].view(np.uint32), s1.cpu().numpy().view(np.uint32), err_msg=name)
        check(qq, bb, 5, FAST, msg=name)


def test_k1_equals_the_top1_search():
    _k1_equals_the_top1_search(384)


def test_k1_equals_the_top1_search_at_256():
    _k1_equals_the_top1_search(256)   # (the top-1 search serves 256 columns too: column 0 is its answer)


# ------------------------------------------------------------------------------------------------- 4. ties and twins
@pytest.mark.parametrize("prec", [FAST, EXACT])
def test_three_copies_of_every_map_row_come_in_index_order(prec):
    rng = np.random.default_rng(4)
    base = rng.standard_normal((500, 128)).astype(np.float32)
    b = np.repeat(base, 3, axis=0)[rng.permutation(1500)]             # each distinct row three times, at scattered indices
    q = (base[rng.integers(0, 500, 64)] + 0.05 * rng.standard_normal((64, 128))).astype(np.float32)
    idx, sim, _ = check(q, b, 5, prec)
    assert (sim[:, 0] == sim[:, 1]).all() and (sim[:, 1] == sim[:, 2]).all() and (sim[:, 3] == sim[:, 4]).all()
    assert (idx[:, 0] < idx[:, 1]).all() and (idx[:, 1] < idx[:, 2]).all() and (idx[:, 3] < idx[:, 4]).all()
    assert (b[idx[:, 0]] == b[idx[:, 2]]).all()


# ------------------------------------------------------------------------------------------------- 5. inside the window
def test_more_near_copies_than_a_list_holds_fall_back_to_all_pairs():
    from vfmreg import ops
    rng = np.random.default_rng(5)
    d = 128
    unit = rng.standard_normal(d).astype(np.float32)
    unit /= np.linalg.norm(unit)
    near = ops.MATCH_TOPK_RECORD_CAP + 64
    b = np.concatenate([unit + 1e-4 * rng.standard_normal((near, d)), rng.standard_normal((1000, d))]).astype(np.float32)
    _, _, info = check(unit[None], b, 8, FAST)
    assert info["fallback"] >= 1 and info["max_records"] > ops.MATCH_TOPK_RECORD_CAP   # every near-copy is inside the window


# ------------------------------------------------------------------------------------------------- 6. worst order
def test_map_sorted_ascending_by_score():
    from oracle import oracle as orc
    q, b = rows(1, 4097, 128, 6)
    qn, _ = orc.l2norm_rows(q)
    bn, _ = orc.l2norm_rows(b)
    b = b[np.argsort(bn.astype(np.float64) @ qn[0].astype(np.float64), kind="stable")]   # every step raises the bound
    check(q, b, 8, FAST)
    check(q, b, 2, FAST)


# ------------------------------------------------------------------------------------------------- 7. several slices
def test_several_map_slices_share_one_bound():
    from vfmreg import ops
    q, b = rows(64, 20000, 128, 7)
    _, _, info = check(q, b, 8, FAST)
    assert info["slices"] >= 2      # (this size gives 11 slices in its last launch: no other M needed)
    assert info["fallback"] == 0 and info["max_records"] <= ops.MATCH_TOPK_RECORD_CAP
    qc, bc = rows(64, 20000, 128, 7, True)
    _, _, info = check(qc, bc, 8, FAST, msg="common")
    assert info["slices"] >= 2 and info["fallback"] == 0


# ------------------------------------------------------------------------------------------------- 8. gate and emission order
def test_gate_and_emission_order_of_the_map_method():
    from vfmreg.mapping import VoxelHashMap
    VoxelHashMap.quiet = True
    rng = np.random.default_rng(8)
    d, nq, k, thr = 128, 300, 3, 0.8
    qd = rng.standard_normal((nq, d)).astype(np.float32)
    qd /= np.linalg.norm(qd, axis=1, keepdims=True)
    sigma = np.sqrt((1 / 0.9 ** 2 - 1) / d)                            # twins at cosine ~0.9
    twins = [qd[i] + sigma * rng.standard_normal(d) for i in range(0, 100) for _ in range(3)]      # a third: three twins above 0.8
    twins += [qd[i] + sigma * rng.standard_normal(d) for i in range(100, 200)]                     # a third: one; the rest: none
    bd = np.concatenate([np.asarray(twins), rng.standard_normal((3000, d))]).astype(np.float32)
    bd = bd[rng.permutation(len(bd))]
    vm = VoxelHashMap(0.01, 1.0e9, 20)
    vm.add_points(np.c_[rng.uniform(-500, 500, (len(bd), 3)).astype(np.float32), bd])
    mp = vm.point_cloud_n()                                            # the map's rows in the container's order
    assert len(mp) == len(bd)
    points = np.c_[np.zeros((nq, 3), np.float32), qd]
    qi, mi, rank, sim = vm.get_vfm_correspondence_indices_topk(points, thr, k)
    want_idx, want_sim = to.topk(qd, mp[:, 3:].astype(np.float32), k)
    np.testing.assert_array_equal(sim.view(np.uint32), want_sim.view(np.uint32))
    valid = ~(want_sim.astype(np.float64) < thr)                       # VoxelHashMap.cpp:503
    wq, wr = np.nonzero(valid)                                         # query-major, rank-minor (VoxelHashMap.cpp:590-600)
    np.testing.assert_array_equal(qi, wq)
    np.testing.assert_array_equal(rank, wr)
    np.testing.assert_array_equal(mi, want_idx[valid])
    per_query = np.bincount(qi, minlength=nq)
    assert (per_query[:100] == 3).all() and (per_query[100:200] == 1).all() and (per_query[200:] == 0).all()
    assert (np.diff(qi) >= 0).all() and all((np.diff(rank[qi == i]) == 1).all() for i in range(100))
    # k = 1 emits what the existing method emits
    q1, m1, r1, _ = vm.get_vfm_correspondence_indices_topk(points, thr, 1)
    q0, m0, _ = vm.get_vfm_correspondence_indices(points, thr)
    np.testing.assert_array_equal(q1, q0)
    np.testing.assert_array_equal(m1, m0)
    assert (r1 == 0).all()


# ------------------------------------------------------------------------------------------------- 9. through the node
def test_node_with_candidates_registers_past_a_decoy_at_every_point():
    from vfmreg import synth
    from vfmreg.mapping import VoxelHashMap
    from vfmreg.registration import RegistrationNode
    VoxelHashMap.quiet = True
    p = synth.make_pair(4000, 20000, 128, seed=9, outlier=0.2, noise_m=0.01)
    rng = np.random.default_rng(9)
    # every scan descriptor once more in the map, at a wrong place: cosine 1.0 there, ~0.9 at the true row
    decoy_xyz = np.c_[rng.uniform(-60, 60, 4000), rng.uniform(-60, 60, 4000), rng.uniform(-3, 12, 4000)]
    voxel_map = np.r_[np.c_[p["b_xyz"], p["b_desc"]], np.c_[decoy_xyz, p["q_desc"]]]
    voxel_map = voxel_map[rng.permutation(len(voxel_map))]
    raw_scan = np.c_[p["q_xyz"], p["q_desc"]]
    # (an inlier distance that means something: under the node's default of 10 km every pair is an inlier of every hypothesis and RANSAC
    # returns the least-squares fit of ALL pairs, decoys included -- the reference's setting assumes pairs that are all correct)
    kw = dict(ransac_iterations=20000, max_correspondence_distance=0.5)
    plain, one, three = RegistrationNode(**kw), RegistrationNode(vfm_candidates=1, **kw), RegistrationNode(vfm_candidates=3, **kw)
    # vfm_candidates = 1 is the node without the keyword, bit for bit
    s0, t0 = plain.compute_vfm_correspondences(voxel_map, raw_scan)
    s1, t1 = one.compute_vfm_correspondences(voxel_map, raw_scan)
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(t1, t0)
    np.testing.assert_array_equal(one.ransac_registration(voxel_map, raw_scan)[0], plain.ransac_registration(voxel_map, raw_scan)[0])
    np.testing.assert_array_equal(one.teaser_registration(voxel_map, raw_scan, "vfm")[0], plain.teaser_registration(voxel_map, raw_scan, "vfm")[0])
    # the best match of every scan point is its decoy: one candidate per point gives no pair at the right place ...
    moved = (p["T_gt"][:3, :3] @ s0.T).T + p["T_gt"][:3, 3]
    print("k = 1:", len(s0), "pairs,", int((np.linalg.norm(moved - t0, axis=1) < 0.5).sum()), "at the planted place")
    # ... three candidates hold the true row second
    s3, t3 = three.compute_vfm_correspondences(voxel_map, raw_scan)
    moved = (p["T_gt"][:3, :3] @ s3.T).T + p["T_gt"][:3, 3]
    good = int((np.linalg.norm(moved - t3, axis=1) < 0.5).sum())
    print("k = 3:", len(s3), "pairs,", good, "at the planted place")
    assert len(s3) > len(s0) and good >= 50
    pose, _ = three.ransac_registration(voxel_map, raw_scan)
    print("ransac: |T - T_gt| =", np.linalg.norm(pose - p["T_gt"]))
    assert np.linalg.norm(pose - p["T_gt"]) < 0.05
    pose, _ = three.teaser_registration(voxel_map, raw_scan, "vfm")
    print("teaser: |T - T_gt| =", np.linalg.norm(pose - p["T_gt"]))
    assert np.linalg.norm(pose - p["T_gt"]) < 0.05

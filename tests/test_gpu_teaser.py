"""TEASER++ registration on the GPU (csrc/teaser.hip, csrc/teaser_host.cpp, ``vfmreg.teaser``, ``RegistrationNode.teaser_registration``)
against tests/teaser_oracle.py: the bit matrix and the degrees EQUAL, the reduction's kept set and the clique equal for every h the
heuristic may find, the GNC-TLS rotation, weights and iteration count bit for bit, the whole solve with difference 0.0 on planted
scenes, the registration methods on the correspondences they compute, and every output and workspace between guard bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import teaser_oracle as to  # noqa: E402
from tests.guarded import GuardedBuffer  # noqa: E402


def dev(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool((a.view(np.int64) == b.view(np.int64)).all())


# ------------------------------------------------------------------------------------------------- the graph
def check_graph(src, tgt, noise_bound=0.2, msg=""):
    from vfmreg import ops
    n = len(src)
    adj, deg = ops.teaser_graph(dev(src), dev(tgt), noise_bound)
    assert adj.dtype == torch.int64 and tuple(adj.shape) == (n, (n + 63) // 64) and deg.dtype == torch.int32
    want = to.graph(src, tgt, noise_bound)
    got = adj.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(got, to.pack(want), err_msg=msg)              # padding bits and the diagonal included
    np.testing.assert_array_equal(deg.cpu().numpy(), want.sum(1), err_msg=msg)
    return want


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 700])
def test_graph_equals_the_oracle(n):
    src, tgt, _, _ = to.planted_scene(n, max(1, n // 3), seed=n)
    adj = check_graph(src, tgt, msg="planted")
    if n >= 63:
        assert adj.sum() > 0
    # a lattice where abs(da - db) is 0, 0.5 or 1 exactly and beta = 0.5 exactly: 3-4-5 triangles, noise_bound = 0.25
    i = np.arange(n, dtype=np.float64)
    src = np.c_[3 * i, 4 * i, 0 * i]
    tgt = np.c_[5 * i + 0.5 * (i % 3), 0 * i, 0 * i]
    adj = check_graph(src, tgt, noise_bound=0.25, msg="lattice")
    if n >= 3:
        assert adj[0, 1] and adj[1, 2] and not adj[0, 2] and adj[0, 3]          # the difference 0.5 == beta is an edge, 1.0 is not
        assert adj.sum() == sum(abs(a % 3 - b % 3) <= 1 for a in range(n) for b in range(n) if a != b)
    # duplicate correspondences (edges among themselves: both distances are 0), and a NaN row (no edge at all)
    src, tgt, _, _ = to.planted_scene(n, max(1, n // 2), seed=100 + n)
    if n >= 2:
        src[n // 2:], tgt[n // 2:] = src[:n - n // 2], tgt[:n - n // 2]
    adj = check_graph(src, tgt, msg="duplicates")
    if n >= 2:
        assert adj[0, n // 2] and adj[n // 2, 0]
    src[n // 3, 1] = np.nan
    adj = check_graph(src, tgt, msg="a NaN row")
    assert not adj[n // 3].any() and not adj[:, n // 3].any()
    tgt[n - 1, 2] = np.nan
    check_graph(src, tgt, msg="two NaN rows")


# ------------------------------------------------------------------------------------------------- the reduction and the clique
def embedded_cliques(n, cliques, density, seed):
    rng = np.random.default_rng(seed)
    a = np.triu(rng.random((n, n)) < density, 1)
    adj = a | a.T
    for c in cliques:
        for i in c:
            for j in c:
                adj[i, j] = i != j
    return adj


REDUCTION_CASES = {
    "random 130 at 0.3": lambda: embedded_cliques(130, [], 0.3, 1),
    "random 65 at 0.9": lambda: embedded_cliques(65, [], 0.9, 2),
    "one planted clique": lambda: embedded_cliques(200, [list(range(5, 200, 9))], 0.05, 3),
    "two disjoint maximum cliques": lambda: embedded_cliques(150, [list(range(1, 150, 10)), list(range(4, 150, 10))], 0.03, 4),
    "two overlapping maximum cliques": lambda: embedded_cliques(150, [[3, 20, 41, 60, 77, 99, 120, 140], [3, 20, 41, 60, 80, 101, 119, 149]], 0.03, 5),
    "no edge": lambda: np.zeros((70, 70), bool),
    "complete": lambda: ~np.eye(129, dtype=bool),
    "planted scene": lambda: to.graph(*to.planted_scene(400, 160, 0)[:2]),
}


@pytest.mark.parametrize("name", list(REDUCTION_CASES))
def test_reduction_keeps_the_clique_for_every_h(name):
    from vfmreg import ops
    adj = REDUCTION_CASES[name]()
    n = len(adj)
    want = to.max_clique(adj)
    words = torch.from_numpy(to.pack(adj).view(np.int64)).cuda()
    deg = dev(adj.sum(1), np.int32)
    seen_h = set()
    for seeds in (1, 2, 16):
        kept, info = ops.teaser_reduce(words, deg, seeds=seeds)
        h, k = (int(x) for x in info.cpu().numpy())
        assert h == max(to.greedy_clique_size(adj, r) for r in range(seeds)), (name, seeds)       # the heuristic, restated
        assert 1 <= h <= len(want)
        kept = kept[:k].cpu().numpy()
        np.testing.assert_array_equal(kept, to.core(adj, h), err_msg=f"{name} seeds {seeds}")      # THE fixpoint, ascending
        assert set(want) <= set(kept.tolist())
        sub = ops.teaser_submatrix(words, dev(kept, np.int32))
        np.testing.assert_array_equal(sub.cpu().numpy().view(np.uint64), to.pack(adj[np.ix_(kept, kept)]))
        got = ops.teaser_max_clique_host(sub.cpu().numpy(), kept, known=h)
        assert got.tolist() == want, (name, seeds, h)                                              # whatever h was
        seen_h.add(h)
    # ... and for an h below what the heuristic finds (more is kept, the answer is the same)
    for h in sorted({1, min(2, len(want)), max(1, min(seen_h) - 1)}):
        kept = to.core(adj, h)
        sub = ops.teaser_submatrix(words, dev(kept, np.int32))
        assert ops.teaser_max_clique_host(sub.cpu().numpy(), kept, known=h).tolist() == want, (name, h)
    if name.startswith("two disjoint"):
        assert want == list(range(1, 150, 10))                                                     # the lower indices win


# ------------------------------------------------------------------------------------------------- GNC-TLS
def check_gnc(src, tgt, clique, msg="", **kw):
    from vfmreg import ops
    R, w, it, v = ops.teaser_gnc(dev(src), dev(tgt), dev(clique, np.int32), kw.get("noise_bound", 0.2), kw.get("factor", 1.4),
                                 kw.get("max_iterations", 10000), kw.get("cost_threshold", 1e-16))
    wR, ww, wit, wv = to.gnc_tls(src, tgt, clique, kw.get("noise_bound", 0.2), kw.get("factor", 1.4), kw.get("max_iterations", 10000),
                                 kw.get("cost_threshold", 1e-16))
    got_it = int(it.item())
    print(f"{msg}: chain {len(clique) - 1}, iterations {got_it} (oracle {wit})")
    assert got_it == wit, msg
    assert bits_equal(R.cpu().numpy(), wR), (msg, np.abs(R.cpu().numpy() - wR).max())
    assert bits_equal(w.cpu().numpy(), ww), (msg, np.abs(w.cpu().numpy() - ww).max())
    assert bits_equal(v.cpu().numpy(), wv), msg
    return wR, ww, wit


@pytest.mark.parametrize("chain", [1, 2, 255, 256, 257, 700])
def test_gnc_equals_the_oracle(chain):
    k = chain + 1
    # every correspondence is taken as a member (GNC does not ask whether they are a clique): 30 % outliers make the loop work
    src, tgt, _, inl = to.planted_scene(k, max(2, (7 * k) // 10), seed=chain)
    R, w, it = check_gnc(src, tgt, np.arange(k), msg="planted")
    if chain >= 255:
        assert it >= 3 and (w == 0).any() and (w == 1).any()
    # a clique that is a strict subset, in gaps
    if k >= 4:
        check_gnc(src, tgt, np.arange(0, k, 3), msg="every third")
    # few iterations allowed; another factor and bound
    check_gnc(src, tgt, np.arange(k), msg="2 iterations", max_iterations=2)
    check_gnc(src, tgt, np.arange(k), msg="factor 2, bound 0.05", factor=2.0, noise_bound=0.05)


def test_gnc_all_consistent_chain_stops_at_its_first_iteration():
    src, _, T, _ = to.planted_scene(300, 300, seed=7)
    tgt = src @ T[:3, :3].T + T[:3, 3]                                                             # no noise
    R, w, it = check_gnc(src, tgt, np.arange(300), msg="all consistent")
    assert it == 0 and (w == 1).all() and np.abs(R - T[:3, :3]).max() < 1e-12


def test_gnc_collinear_chain_gives_the_identity():
    i = np.arange(120, dtype=np.float64)
    src = np.c_[1.5 * i, 0 * i, 0 * i]
    tgt = np.c_[1.5 * i + 0.01 * (i % 5), 0 * i, 0 * i] + np.array([4.0, -2.0, 1.0])
    R, w, it = check_gnc(src, tgt, np.arange(120), msg="collinear")
    assert (R == np.eye(3)).all()
    tgt = np.c_[0 * i, 1.5 * i, 0 * i]                                                             # ... turned by 90 degrees: still rank 1
    R, w, it = check_gnc(src, tgt, np.arange(120), msg="collinear, turned")
    assert (R == np.eye(3)).all()


# ------------------------------------------------------------------------------------------------- the whole solve
def reference_params():
    from vfmreg import teaser
    S = teaser.RobustRegistrationSolver
    p = S.Params()                                                                                 # RN:112-124
    p.cbar2 = 1.0
    p.noise_bound = 0.2
    p.estimate_scaling = False
    p.inlier_selection_mode = S.INLIER_SELECTION_MODE.PMC_EXACT
    p.rotation_tim_graph = S.INLIER_GRAPH_FORMULATION.CHAIN
    p.rotation_estimation_algorithm = S.ROTATION_ESTIMATION_ALGORITHM.GNC_TLS
    p.rotation_gnc_factor = 1.4
    p.rotation_max_iterations = 10000
    p.rotation_cost_threshold = 1e-16
    return p


@pytest.mark.parametrize("n,inliers", to.PLANTED)
@pytest.mark.parametrize("seed", [0, 1])
def test_whole_solve_on_planted_scenes(n, inliers, seed):
    from vfmreg import teaser
    src, tgt, T, inl = to.planted_scene(n, inliers, seed)
    want = to.solve(src, tgt)
    assert want["valid"] and np.array_equal(want["clique"], inl)                                   # (the oracle: unique clique = the inliers)
    solver = teaser.RobustRegistrationSolver(reference_params())
    solver.solve(src.T, tgt.T)                                                                     # 3 x N, as RN:110, 127
    s = solver.getSolution()
    assert s.valid is True and s.scale == 1.0
    dR, dt = np.abs(s.rotation - want["rotation"]).max(), np.abs(s.translation - want["translation"]).max()
    rre, rte = to.errors(s.rotation, s.translation, T)
    print(f"N {n} inliers {inliers} seed {seed}: |dR| {dR} |dt| {dt} iterations {solver.getRotationIterations()} RRE {rre:.4f} deg RTE {rte:.4f} m "
          f"h {solver._h} kept {solver._kept}")
    assert dR == 0.0 and dt == 0.0
    assert bits_equal(s.rotation, want["rotation"]) and bits_equal(s.translation, want["translation"])
    assert solver.getInlierMaxClique() == inl.tolist()
    assert solver.getRotationIterations() == want["iterations"]
    np.testing.assert_array_equal(solver.getRotationInliersMask(), want["rotation_inliers"])
    np.testing.assert_array_equal(solver.getTranslationInliersMask(), want["translation_inliers"])
    assert rre <= 0.5 and rte <= 0.1
    assert solver._kept == inliers                                                                 # the fixpoint leaves exactly the clique
    # device tensors are taken as they are
    again = teaser.RobustRegistrationSolver(reference_params())
    again.solve(dev(src.T), dev(tgt.T))
    assert bits_equal(again.getSolution().rotation, s.rotation) and bits_equal(again.getSolution().translation, s.translation)


def test_degenerate_sizes_are_invalid_solutions():
    from vfmreg import teaser
    solver = teaser.RobustRegistrationSolver(reference_params())
    far = np.array([[0.0, 0, 0], [10.0, 0, 0], [0, 30.0, 0]])
    for src, tgt in ((np.zeros((0, 3)), np.zeros((0, 3))), (np.ones((1, 3)), np.zeros((1, 3))), (far, 2 * far)):
        s = solver.solve(src.T, tgt.T)
        assert s is solver.getSolution() and s.valid is False and s.scale == 1.0
        assert (s.rotation == np.eye(3)).all() and (s.translation == 0).all()
        assert not to.solve(src, tgt)["valid"]
    # two correspondences: a chain of one measurement, a rank-1 H, the identity; the translation is still estimated
    src, tgt = np.array([[0.0, 0, 0], [3.0, 4, 0]]), np.array([[1.0, 1, 1], [4.1, 5, 1]])
    s = solver.solve(src.T, tgt.T)
    want = to.solve(src, tgt)
    assert s.valid and want["valid"] and (s.rotation == np.eye(3)).all()
    assert bits_equal(s.translation, want["translation"]) and solver.getInlierMaxClique() == [0, 1]
    with pytest.raises(ValueError):
        solver.solve(np.zeros((4, 3)), np.zeros((4, 3)))                                           # N x 3 with N != 3: not 3 x N
    with pytest.raises(ValueError, match="32768"):
        solver.solve(np.zeros((3, 32769)), np.zeros((3, 32769)))


# ------------------------------------------------------------------------------------------------- the registration methods
def test_teaser_registration_vfm_equals_the_oracle_on_its_correspondences():
    from oracle import oracle as orc
    from vfmreg import synth
    from vfmreg.config import load_config
    from vfmreg.mapping import VoxelHashMap
    from vfmreg.registration import RegistrationNode
    VoxelHashMap.quiet = True
    cfg = load_config(None, None)
    vs, sigma = cfg.mapping.voxel_size, cfg.adaptive_threshold.initial_threshold
    p = synth.make_pair(3000, 20000, 128, seed=3)
    voxel_map, raw_scan = np.c_[p["b_xyz"], p["b_desc"]], np.c_[p["q_xyz"], p["q_desc"]]
    node = RegistrationNode(cfg)
    src, tgt = node.compute_vfm_correspondences(voxel_map, raw_scan)
    want = to.solve(src, tgt, reduce=True)
    print(f"vfm: {len(src)} correspondences, clique {len(want['clique'])}, iterations {want['iterations']}")
    assert want["valid"] and len(want["clique"]) >= 10
    pose, none = node.teaser_registration(voxel_map, raw_scan, "vfm")
    assert none is None
    np.testing.assert_array_equal(pose, to.pose_of(want))
    pose, refined = node.teaser_registration(voxel_map, raw_scan, "vfm", run_icp=True)
    guess = orc.orthogonalize_rotation(to.pose_of(want))                                           # RN:145-148
    np.testing.assert_array_equal(pose, guess)
    scan = orc.voxel_down_sample(orc.voxel_down_sample(raw_scan, vs * 0.5), vs * 1.0)              # RN:139-141
    mp = np.asarray(voxel_map, dtype=np.float64)[orc.voxel_hash_map_points(voxel_map, vs, cfg.mapping.max_points_per_voxel)]
    np.testing.assert_array_equal(refined, orc.register_frame(scan[:, :3], mp[:, :3], vs, guess, 3 * sigma, sigma / 3))   # RN:151-155
    # a handle in place of the array
    handle = node.set_map(voxel_map)
    np.testing.assert_array_equal(node.teaser_registration(handle, raw_scan, "vfm")[0], to.pose_of(want))
    rre, rte = to.errors(pose[:3, :3], pose[:3, 3], p["T_gt"])
    print(f"vfm: RRE {rre:.3f} deg RTE {rte:.3f} m of the scene's pose")
    assert rre <= 1.5 and rte <= 0.6                                                               # (the success threshold of the error table)


def test_teaser_registration_fpfh_equals_the_oracle_on_its_correspondences():
    from oracle import oracle as orc
    from vfmreg import synth
    from vfmreg.config import load_config
    from vfmreg.mapping import VoxelHashMap
    from vfmreg.registration import RegistrationNode
    VoxelHashMap.quiet = True
    cfg = load_config(None, None)
    vs, sigma = cfg.mapping.voxel_size, cfg.adaptive_threshold.initial_threshold
    sc = synth.make_structured_scene(6000, 30000, seed=0)
    scan = orc.voxel_down_sample(sc["scan"], .1)                                                   # RN:593
    map_xyz = sc["map"]
    node = RegistrationNode(cfg, baseline_methods=("fpfh",))
    src, tgt = node.compute_correspondences(map_xyz, scan, "fpfh", mutual_filter=True)             # RN:98-101
    want = to.solve(src, tgt, reduce=True)
    print(f"fpfh: {len(src)} correspondences, clique {len(want['clique'])}, valid {want['valid']}, iterations {want['iterations']}")
    assert len(src) >= 30 and want["valid"]
    pose, none = node.teaser_registration(map_xyz, scan, "fpfh")
    assert none is None
    np.testing.assert_array_equal(pose, to.pose_of(want))
    pose, refined = node.teaser_registration(map_xyz, scan, "fpfh", run_icp=True)
    guess = orc.orthogonalize_rotation(to.pose_of(want))
    np.testing.assert_array_equal(pose, guess)
    voxel_scan = orc.voxel_down_sample(orc.voxel_down_sample(scan, vs * 0.5), vs * 1.0)
    mp = np.asarray(map_xyz, dtype=np.float64)[orc.voxel_hash_map_points(map_xyz, vs, cfg.mapping.max_points_per_voxel)]
    np.testing.assert_array_equal(refined, orc.register_frame(voxel_scan, mp, vs, guess, 3 * sigma, sigma / 3))
    # 387-column rows: the baseline reads the coordinates only (RN:98-99)
    wide_map, wide_scan = np.c_[map_xyz, np.ones((len(map_xyz), 4))], np.c_[scan, np.ones((len(scan), 4))]
    np.testing.assert_array_equal(node.teaser_registration(wide_map, wide_scan, "fpfh")[0], to.pose_of(want))
    with pytest.raises(ValueError, match="Invalid method: fpfh"):
        RegistrationNode(cfg).teaser_registration(map_xyz, scan, "fpfh")                           # opt-in, as the RANSAC row


def test_evaluate_scene_with_teaser_rows():
    from tests.test_gpu_icp_registration import _errors, _synthetic_scene
    from vfmreg.evaluation import Evaluation, build_local_map, evaluate_scene
    from vfmreg.mapping import VoxelHashMap
    from vfmreg.registration import RegistrationNode
    from vfmreg.utils import transform_pcl
    from vfmreg.voxelization import voxel_down_sample
    VoxelHashMap.quiet = True
    scene = _synthetic_scene()
    ev = evaluate_scene(scene, RegistrationNode(ransac_iterations=4000, cache_map=True), Evaluation(), teaser=True)
    assert list(ev.rot_errors) == ["vfm_ransac", "vfm_ransac_icp", "vfm_teaser", "vfm_teaser_icp"]   # RN:895-904 behind RN:867-883
    local_map = build_local_map(scene["map_poses"], scene["map_point_clouds"], n_descriptors=128)
    direct = RegistrationNode()
    for i, (gt, cloud) in enumerate(zip(scene["scene_poses"], scene["scene_point_clouds"])):
        cloud = transform_pcl(voxel_down_sample(cloud, .1).astype(cloud.dtype), np.eye(4))
        p0, p1 = direct.teaser_registration(local_map, cloud, "vfm", True)
        for k, v in (("vfm_teaser", p0), ("vfm_teaser_icp", p1)):
            rte, rre = _errors(v @ np.eye(4), gt)
            assert ev.trans_errors[k][i] == rte and ev.rot_errors[k][i] == rre, (k, i)
    print("teaser rows:", {k: (ev.trans_errors[k], ev.rot_errors[k]) for k in ("vfm_teaser", "vfm_teaser_icp")})
    assert max(ev.trans_errors["vfm_teaser_icp"]) < 0.6 and max(ev.rot_errors["vfm_teaser_icp"]) < 1.5
    # with the FPFH baseline its TEASER rows come first, as RN:895-898 lists them; without run_icp only the TEASER poses join
    node = RegistrationNode(ransac_iterations=4000, cache_map=True, baseline_methods=("fpfh",))
    ev = evaluate_scene(scene, node, Evaluation(), run_icp=False, baselines=("fpfh",), teaser=True)
    assert list(ev.rot_errors) == ["fpfh_ransac", "vfm_ransac", "fpfh_teaser", "vfm_teaser"]


# ------------------------------------------------------------------------------------------------- buffers
def test_outputs_and_workspaces_stay_inside_their_buffers():
    from vfmreg import _lib
    lib = _lib.load()
    n, inliers = 333, 70
    src_h, tgt_h, _, inl = to.planted_scene(n, inliers, seed=5)
    W = (n + 63) // 64
    stream = torch.cuda.current_stream().cuda_stream
    src, tgt = GuardedBuffer((n, 3), torch.float64).set(src_h), GuardedBuffer((n, 3), torch.float64).set(tgt_h)
    src.poison_guards("nan"), tgt.poison_guards("nan")
    adj = GuardedBuffer((n, W), torch.int64).fill_bytes(0xFF)
    deg = GuardedBuffer(n, torch.int32).fill_bytes(0xFF)
    _lib.check(lib.vfm_teaser_graph(src.ptr(), tgt.ptr(), n, 0.2, 1.0, adj.ptr(), deg.ptr(), stream), "teaser_graph")
    torch.cuda.synchronize()
    want_adj = to.graph(src_h, tgt_h)
    np.testing.assert_array_equal(adj.numpy().view(np.uint64), to.pack(want_adj))
    np.testing.assert_array_equal(deg.numpy(), want_adj.sum(1))
    # the reduction: one byte short is refused before any launch, the exact size is enough
    kept = GuardedBuffer(n, torch.int32).fill_bytes(0xFF)
    info = GuardedBuffer(2, torch.int32).fill_bytes(0xFF)
    need = lib.vfm_teaser_reduce_workspace_bytes(n)
    ws = GuardedBuffer(need, torch.uint8).fill_bytes(0xFF)
    assert lib.vfm_teaser_reduce(adj.ptr(), deg.ptr(), n, 16, kept.ptr(), info.ptr(), ws.ptr(), need - 1, stream) in (-1, -2)
    assert b"workspace" in lib.vfm_last_error()
    torch.cuda.synchronize()
    assert (info.numpy() == -1).all() and (kept.numpy() == -1).all()
    _lib.check(lib.vfm_teaser_reduce(adj.ptr(), deg.ptr(), n, 16, kept.ptr(), info.ptr(), ws.ptr(), need, stream), "teaser_reduce")
    torch.cuda.synchronize()
    h, k = info.numpy().tolist()
    assert h == inliers and k == inliers
    np.testing.assert_array_equal(kept.numpy()[:k], inl)
    assert (kept.numpy()[k:] == -1).all()                                                          # entries behind the count are not written
    kept_k = GuardedBuffer(k, torch.int32).set(kept.numpy()[:k])
    sub = GuardedBuffer((k, (k + 63) // 64), torch.int64).fill_bytes(0xFF)
    _lib.check(lib.vfm_teaser_submatrix(adj.ptr(), n, kept_k.ptr(), k, sub.ptr(), stream), "teaser_submatrix")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(sub.numpy().view(np.uint64), to.pack(want_adj[np.ix_(inl, inl)]))
    # GNC-TLS
    R = GuardedBuffer(9, torch.float64).fill_nan()
    w = GuardedBuffer(k - 1, torch.float64).fill_nan()
    it = GuardedBuffer(1, torch.int32).fill_bytes(0xFF)
    v = GuardedBuffer((k, 3), torch.float64).fill_nan()
    need_g = lib.vfm_teaser_gnc_workspace_bytes(k)
    ws_g = GuardedBuffer(need_g, torch.uint8).fill_bytes(0xFF)
    assert lib.vfm_teaser_gnc(src.ptr(), tgt.ptr(), n, kept_k.ptr(), k, 0.2, 1.4, 10000, 1e-16, R.ptr(), w.ptr(), it.ptr(), v.ptr(), ws_g.ptr(),
                              need_g - 1, stream) in (-1, -2)
    assert b"workspace" in lib.vfm_last_error()
    _lib.check(lib.vfm_teaser_gnc(src.ptr(), tgt.ptr(), n, kept_k.ptr(), k, 0.2, 1.4, 10000, 1e-16, R.ptr(), w.ptr(), it.ptr(), v.ptr(),
                                  ws_g.ptr(), need_g, stream), "teaser_gnc")
    torch.cuda.synchronize()
    for name, buf in (("src", src), ("tgt", tgt), ("adj", adj), ("degree", deg), ("kept", kept), ("info", info), ("reduce workspace", ws),
                      ("kept[:k]", kept_k), ("sub", sub), ("R", R), ("weights", w), ("iterations", it), ("v", v), ("gnc workspace", ws_g)):
        assert buf.intact(), f"{name}: {buf.intact()}"
    wR, ww, wit, wv = to.gnc_tls(src_h, tgt_h, inl)
    assert bits_equal(R.numpy().reshape(3, 3), wR) and bits_equal(w.numpy(), ww) and it.numpy()[0] == wit and bits_equal(v.numpy(), wv)
    # an index outside the correspondences is reported, and nothing is read through it
    bad = GuardedBuffer(k, torch.int32).set(np.r_[inl[:-1], n])
    it.fill_bytes(0x00)
    _lib.check(lib.vfm_teaser_gnc(src.ptr(), tgt.ptr(), n, bad.ptr(), k, 0.2, 1.4, 10000, 1e-16, R.ptr(), w.ptr(), it.ptr(), v.ptr(), ws_g.ptr(),
                                  need_g, stream), "teaser_gnc")
    torch.cuda.synchronize()
    assert it.numpy()[0] == -1 and all(b.intact() for b in (R, w, it, v, ws_g))

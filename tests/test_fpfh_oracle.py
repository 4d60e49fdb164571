"""CPU checks of the FPFH path: the numpy oracle (tests/fpfh_oracle.py) on hand cases and invariants, its two neighbour searches
against each other, the host-side refusals of the new API, and the vfm_fpfh_* entry points in the cross-compiled library."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import fpfh_oracle as fo

ROOT = Path(__file__).resolve().parent.parent


def test_planar_patch_normal_is_z():
    g = np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0), indexing="ij"), -1).reshape(-1, 2) * 0.05
    pts = np.c_[g, np.zeros(len(g))]
    idx, _, cnt = fo.hybrid_search_brute(pts, 0.12, 30)
    nv = fo.estimate_normals(pts, idx, cnt)
    # +-z everywhere, the sign as the solver gives it: a symmetric neighbourhood has a diagonal covariance with a zero z entry (the
    # diagonal branch: +z); an asymmetric one at the border takes the trigonometric branch
    np.testing.assert_allclose(np.abs(nv), np.tile([0.0, 0.0, 1.0], (len(pts), 1)), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(nv[12], [0.0, 0.0, 1.0])
    assert (nv[:, 2] < 0).any()


def test_tilted_patch_normal_is_the_smallest_eigenvector():
    rng = np.random.default_rng(3)
    uv = rng.uniform(-0.1, 0.1, (200, 2))
    a = np.array([1.0, 0.0, 0.4]) / np.linalg.norm([1.0, 0.0, 0.4])
    b = np.array([0.2, 1.0, 0.1])
    b = b - (b @ a) * a
    b /= np.linalg.norm(b)
    pts = uv[:, :1] * a + uv[:, 1:] * b + np.array([3.0, -2.0, 1.0])
    idx, _, cnt = fo.hybrid_search_brute(pts, 0.5, 30)
    C = fo.covariances(pts, idx, cnt)
    nv = fo.fast_eigen3x3(C)
    truth = np.cross(a, b)
    for k in range(len(pts)):
        w, V = np.linalg.eigh(C[k])
        assert abs(abs(V[:, 0] @ nv[k]) - 1.0) < 1e-9
        assert abs(abs(truth @ nv[k]) - 1.0) < 1e-6
    # no orientation step follows: the sign is whatever the solver's branch gives, and on one patch both occur
    s = np.sign(nv @ truth)
    assert (s > 0).any() and (s < 0).any()


def test_identity_covariance_gives_z():
    np.testing.assert_array_equal(fo.fast_eigen3x3(np.eye(3)[None]), [[0.0, 0.0, 1.0]])
    np.testing.assert_array_equal(fo.fast_eigen3x3(np.zeros((1, 3, 3))), [[0.0, 0.0, 0.0]])
    pts = np.array([[0.0, 0.0, 0.0], [0.01, 0.0, 0.0], [5.0, 5.0, 5.0]])
    idx, _, cnt = fo.hybrid_search_brute(pts, 0.1, 30)   # 2, 2 and 1 neighbours: identity covariance
    np.testing.assert_array_equal(fo.estimate_normals(pts, idx, cnt), np.tile([0.0, 0.0, 1.0], (3, 1)))


def test_pair_features_hand_cases():
    z, x, y = np.array([[0.0, 0, 1]]), np.array([[1.0, 0, 0]]), np.array([[0.0, 1, 0]])
    o = np.zeros((1, 3))
    f, _ = fo.pair_features(o, z, x, z)          # d = x, both normals up: (0, 0, 0)
    np.testing.assert_array_equal(f, [[0.0, 0.0, 0.0]])
    f, _ = fo.pair_features(o, z, x, y)          # v = d x n1 = -y, w = n1 x v = x: (atan2(0, 0), v.n2, 0) = (0, -1, 0)
    np.testing.assert_array_equal(f, [[0.0, -1.0, 0.0]])
    f, _ = fo.pair_features(o, z, o, y)          # zero distance: all zero
    np.testing.assert_array_equal(f, [[0.0, 0.0, 0.0]])
    # swap: n2 is more aligned with d than n1 -> the roles change, d flips, f2 = -angle2
    n2 = np.array([[0.6, 0.0, 0.8]])
    f, _ = fo.pair_features(o, y, x, n2)
    assert f[0, 2] == -0.6
    # the margin reports a value on a bin edge: f1 = -1 gives 11 (f1 + 1) / 2 = 0 exactly
    _, m = fo.pair_features(o, z, x, y)
    assert m[0] == 0.0


def _cloud(seed=0):
    import vfmreg.synth as synth
    sc = synth.make_structured_scene(4000, 4000, seed=seed, extent=4.0, scan_range=4.0, boxes=3, cylinders=2)
    return sc["map"]


def test_spfh_and_fpfh_group_sums():
    pts = _cloud(1)
    idx, _, cnt = fo.hybrid_search(pts, 0.2, 30)
    nv = fo.estimate_normals(pts, idx, cnt)
    down, dn = fo.voxel_down_sample(pts, 0.1, nv)
    i, d, c = fo.hybrid_search(down, 0.5, 100)
    sp, _ = fo.spfh(down, dn, i, c)
    live = c >= 2
    assert live.mean() > 0.9
    for g in range(3):
        np.testing.assert_allclose(sp[live, 11 * g:11 * g + 11].sum(1), 100.0, rtol=0, atol=1e-9)
    assert (sp[~live] == 0).all()
    f, _ = fo.fpfh(sp, i, d, c)
    weighted = f - sp
    for g in range(3):
        part = weighted[:, 11 * g:11 * g + 11].sum(1)
        rows = live & (np.abs(part) > 0)
        assert rows.mean() > 0.9
        np.testing.assert_allclose(f[rows, 11 * g:11 * g + 11].sum(1), 200.0, rtol=0, atol=1e-9)


def test_down_sample_means_in_input_order():
    pts = np.array([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [1.0, 1.0, 1.0], [0.02, 0.01, 0.0], [0.99, 1.0, 1.04]])
    nrm = np.array([[0.0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, 1], [0, 0, 1]])
    p, nv = fo.voxel_down_sample(pts, 0.2, nrm)
    np.testing.assert_array_equal(p[0], ((0.0 + pts[0] + pts[1]) + pts[3]) / 3.0)
    np.testing.assert_array_equal(nv[0], [0.0, 1 / 3, 2 / 3])    # not renormalised
    np.testing.assert_array_equal(p[1], ((0.0 + pts[2]) + pts[4]) / 2.0)


@pytest.mark.parametrize("case", ["lattice", "lattice_edge", "dense_dups", "random"])
def test_brute_force_equals_ckdtree(case):
    rng = np.random.default_rng(7)
    if case.startswith("lattice"):
        g = np.stack(np.meshgrid(*(np.arange(7.0),) * 3, indexing="ij"), -1).reshape(-1, 3)
        pts, r, k = g, (2.0 if case == "lattice_edge" else 2.01), 30
    elif case == "dense_dups":
        pts = rng.uniform(-0.05, 0.05, (700, 3))
        pts = np.r_[pts, pts[:200], pts[:50]]
        pts, r, k = pts, 0.2, 100
    else:
        pts, r, k = rng.uniform(-1, 1, (1500, 3)), 0.3, 30
    a = fo.hybrid_search_brute(pts, r, k)
    b = fo.hybrid_search(pts, r, k, chunk=333)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    idx, d2, cnt = a
    assert (idx[np.arange(len(pts)), 0] >= 0).all()
    # rows are ascending by (d2, index)
    for q in range(0, len(pts), 37):
        c = cnt[q]
        key = list(zip(d2[q, :c], idx[q, :c]))
        assert key == sorted(key)
    if case == "lattice_edge":
        assert cnt.max() == 27    # d2 == r^2 is outside: 1 + 6 + 12 + 8 neighbours of an inner point


def test_new_api_refuses_on_the_host():
    import vfmreg.o3d as o3d
    from vfmreg.registration import RegistrationNode

    node = RegistrationNode()
    for m in ("dip", "gedi", "fcgf", "gcl", "spinnet"):
        with pytest.raises(NotImplementedError):
            node.compute_correspondences(np.zeros((4, 3)), np.zeros((4, 3)), m)
    with pytest.raises(ValueError, match="Invalid method: vfm2"):
        node.compute_correspondences(np.zeros((4, 3)), np.zeros((4, 3)), "vfm2")
    assert node.map_descriptor_cache == {}
    pcd = o3d.geometry.PointCloud()
    pcd.points = o3d.utility.Vector3dVector(np.zeros((4, 3)))
    assert not pcd.has_normals()
    with pytest.raises(NotImplementedError):
        pcd.estimate_normals(o3d.geometry.KDTreeSearchParamHybrid(radius=0.2, max_nn=30), fast_normal_computation=False)
    with pytest.raises(RuntimeError, match="no normal"):
        o3d.pipelines.registration.compute_fpfh_feature(pcd, o3d.geometry.KDTreeSearchParamHybrid(radius=0.5, max_nn=100))


def test_fpfh_entry_points_are_declared_and_exported():
    subprocess.run([sys.executable, str(ROOT / "vfm-registration_amd" / "build.py")], check=True, stdout=subprocess.DEVNULL)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "vfmreg.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(vfm_fpfh_[a-z0-9_]+)\s*\(", text))
    want = {"vfm_fpfh_workspace_bytes", "vfm_fpfh_grid_build", "vfm_fpfh_search_hybrid", "vfm_fpfh_normals",
            "vfm_fpfh_voxel_down_sample", "vfm_fpfh_spfh", "vfm_fpfh_fpfh"}
    assert declared == want
    from vfmreg import _lib
    assert want <= set(_lib.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split()}
    assert want <= exported
    lib = _lib.load()
    assert lib.vfm_fpfh_workspace_bytes(200000) > 200000 * 16
    # argument checks run on the host, before any launch
    assert lib.vfm_fpfh_search_hybrid(1, 10, 1, 1, 0.5, 0, 1, 1, 1, None, None) != 0
    assert b"max_nn" in lib.vfm_last_error()
    assert lib.vfm_fpfh_search_hybrid(1, 10, 1, 1, 0.5, 1025, 1, 1, 1, None, None) != 0
    assert lib.vfm_fpfh_grid_build(1, 10, -1.0, 1, 1, 1, 1 << 30, None) != 0
    assert lib.vfm_fpfh_voxel_down_sample(1, None, 10, 0.1, 1, None, 1, 1, 16, None) != 0
    assert b"workspace" in lib.vfm_last_error()


# ------------------------------------------------------------------------------------ the crafted rows of tests/fpfh_branch_cases.py
# Exits no finite input reaches, so the census cannot ask rows of them:
#   EIG_POS_EVEC   eval2 = q + p beta2 with beta2 = 2 cos(angle) >= sqrt(3) and beta0 <= -1: p >= 0 and rounding is monotone, so
#                  eval2 < eval0 never holds;
#   EIG_POS_EVEC1, EIG_NEG_EVEC1   want eval1 < eval0, that is beta1 < beta0 after monotone rounding; beta0 <= beta1 over the whole
#                  range of half_det (test_eigenvalue_order_leaves_three_exits_dead sweeps it, the ends and their neighbours included);
#   EV1_M11_ZERO   |m00| >= |m11| is false with |m11| not above 0 only if m00 or m11 is a NaN; a NaN covariance has norm > 0 false and
#                  takes the diagonal branch, and eigenvector0 divides by a length that is 0 only if norm is.
DEAD_EIG_EXITS = (fo.EIG_POS_EVEC, fo.EIG_POS_EVEC1, fo.EIG_NEG_EVEC1)
DEAD_EV1_ARMS = (fo.EV1_M11_ZERO,)


def test_eigenvalue_order_leaves_three_exits_dead():
    hd = np.concatenate([np.linspace(-1.0, 1.0, 2000001), np.nextafter(1.0, 0) - np.arange(64) * 2.0 ** -53,
                         -1.0 + np.arange(64) * 2.0 ** -53, np.arange(-64, 65) * 2.0 ** -1074, np.arange(-64, 65) * 2.0 ** -60])
    angle = np.arccos(hd) / 3.0
    beta2 = np.cos(angle) * 2.0
    beta0 = np.cos(angle + 2.09439510239319549) * 2.0
    beta1 = -(beta0 + beta2)
    assert (beta0 <= beta1).all() and (beta0 < beta2).all()


@pytest.fixture(scope="module")
def normal_rows():
    from tests import fpfh_branch_cases as bc
    c = bc.normal_cases()
    C = fo.covariances(c["pts"], c["idx"], c["count"])
    nv, ex, u, arm = fo.fast_eigen3x3(C, branches=True)
    return c, C, nv, ex, u, arm


def test_branch_census_of_the_crafted_normals(normal_rows):
    c, C, nv, ex, u, arm = normal_rows
    assert len(c["pts"]) <= 5000
    for e in fo.EIG_EXITS:
        rows = int((ex == e).sum())
        assert rows == 0 if e in DEAD_EIG_EXITS else rows >= 3, (e, rows)
    for a in fo.EV1_ARMS:
        rows = int((arm == a).sum())
        assert rows == 0 if a in DEAD_EV1_ARMS else rows >= 3, (a, rows)
    for uc in (fo.EV1_U_XZ, fo.EV1_U_YZ):
        assert (u == uc).sum() >= 3
    for k in (0, 1, 2):
        assert (c["count"] == k).sum() >= 3
    assert ((c["count"] < 3) == (np.char.startswith(c["kind"], "cnt"))).all()
    assert (ex[c["count"] < 3] == fo.EIG_DIAG_TIE).all()                       # the identity: a three-way tie
    # every family of the case list took the exits it was made for
    want = {"zero": {fo.EIG_ZERO}, "diag_x": {fo.EIG_DIAG_X}, "diag_y": {fo.EIG_DIAG_Y}, "diag_z": {fo.EIG_DIAG_Z},
            "diag_tie": {fo.EIG_DIAG_TIE}, "isotropic": {fo.EIG_POS_CROSS, fo.EIG_NEG_CROSS}}
    for kind, exits in want.items():
        assert set(ex[c["kind"] == kind].tolist()) == exits, kind
    shifted = np.char.endswith(c["kind"], "_shifted")
    assert {fo.EIG_POS_CROSS, fo.EIG_NEG_EVEC} <= set(ex[shifted].tolist())
    assert np.isfinite(nv).all()
    est = fo.estimate_normals(c["pts"], c["idx"], c["count"])
    np.testing.assert_array_equal(est[ex == fo.EIG_ZERO], np.tile([0.0, 0.0, 1.0], (int((ex == fo.EIG_ZERO).sum()), 1)))


def gapped_rows(C):
    """rows with a unique smallest eigenvalue: (lambda1 - lambda0) / lambda2 >= 1e-3; and the eigh vectors"""
    w, V = np.linalg.eigh(C)
    with np.errstate(all="ignore"):
        gap = (w[:, 1] - w[:, 0]) / w[:, 2]
    return gap >= 1e-3, V[:, :, 0]


def test_crafted_gapped_normals_are_the_smallest_eigenvector(normal_rows):
    c, C, nv, ex, u, arm = normal_rows
    gapped, v0 = gapped_rows(C)
    rows = np.flatnonzero(gapped & (c["count"] >= 3))
    assert len(rows) >= 60 and {fo.EIG_DIAG_X, fo.EIG_DIAG_Y, fo.EIG_DIAG_Z, fo.EIG_POS_CROSS, fo.EIG_NEG_EVEC} <= set(ex[rows].tolist())
    worst = np.abs(np.abs(np.einsum("ij,ij->i", v0[rows], nv[rows])) - 1.0)
    assert worst.max() < 1e-9, (rows[worst.argmax()], worst.max())


def test_crafted_feature_rows_census_and_no_flagged_row():
    from tests import fpfh_branch_cases as bc
    f = bc.feature_cases()
    assert len(f["pts"]) <= 5000
    sp, near, exits, ends = fo.spfh(f["pts"], f["normals"], f["idx"], f["count"], exact_ok=True, branches=True)
    _, fnear = fo.fpfh(sp, f["idx"], f["d2"], f["count"], near)
    assert not near.any() and not fnear.any()
    # the rows that sit on an edge on purpose are the ones the plain margin flags: every one of them is exact
    _, plain = fo.spfh(f["pts"], f["normals"], f["idx"], f["count"])
    assert plain.any()
    for e in fo.PAIR_EXITS:
        assert (exits[:, e] > 0).sum() >= 3, e
    assert (ends.sum(0) >= 3).all(), ends.sum(0)             # clamp_bin's bin 0 and bin 10, for each of the three features
    kinds = f["kind"]
    assert exits[kinds == "symmetric"][:, fo.PAIR_KEPT_TIE].sum() >= 9
    assert (exits[kinds == "coincident"][:, fo.PAIR_DN_ZERO] == 2).all()
    for k in (0, 1, 2, 64, 65, 1024):
        assert (f["count"] == k).sum() >= (1 if k == 1024 else 3), k
    assert (sp[f["count"] <= 1] == 0).all()
    # s == 0: every weighted neighbour's SPFH row is zero
    rows = np.flatnonzero(kinds == "zero_spfh_nbrs")
    assert len(rows) >= 3
    for r in rows:
        assert (sp[f["idx"][r, 1:f["count"][r]]] == 0).all() and (f["d2"][r, 1:f["count"][r]] > 0).all()
    # the dist == 0 skip
    assert ((f["d2"][:, 1:] == 0) & (np.arange(1, f["idx"].shape[1]) < f["count"][:, None])).sum() >= 3

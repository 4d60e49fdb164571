"""CPU anchors of the lifting restatement in tests/lift_reference.py (no GPU): it reproduces the fixtures the reference's
own code produced, its separable upsample is torch's, its undecided set holds the planted boundary points and almost no
random ones, and the comparison helper the GPU tests use (lift_reference.check_lift) rejects each mutation a lifting bug
would make -- a swapped winning camera, a rot90 column off by one, a zeroed row, a value off by 2^-18, an inadmissible
answer on an undecided point."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from tests import lift_reference as LR  # noqa: E402


def _proj_fixture(g, name):
    """(camera, projection image) of a proj_*.npz fixture"""
    s = int(g["subsample"])
    if name == "kitti":
        return LR.kitti_camera(g["P2"], g["Tr"], s), np.zeros((int(g["H"]), int(g["W"]), 3), np.uint8)
    if name == "oxf":
        return (LR.robotcar_camera(g["lidar_in_ego"], g["cam_in_ego"], g["G"], g["fc"], s),
                np.zeros((int(g["H"]), int(g["W"]), 3), np.uint8))
    return LR.nclt_camera(g["T_c_body"], g["K"], g["coords"], s), g["image"]


def _lift_fixture_cams(g, name):
    s = int(g["subsample"])
    if name == "oxf":
        return [LR.robotcar_camera(g["lidar_in_ego"], g["cam_in_ego"][i], g["G"], g["fc"], s, raw=g["images"][i])
                for i in range(len(g["images"]))]
    return [LR.nclt_camera(g["T_c_body"][i], g["K"][i], g["coords"], s, raw=g["images"][i]) for i in range(len(g["images"]))]


@pytest.mark.parametrize("name", ["kitti", "nclt", "oxf"])
def test_projection_reproduces_the_reference_fixtures(golden, name):
    g = golden(f"proj_{name}.npz")
    cam, image = _proj_fixture(g, name)
    P = LR.project(cam, g["pcl"], image)
    assert P.decided.all(), f"{(~P.decided).sum()} undecided points in a reference fixture"
    idx, u, v = P.indices()
    assert len(idx) > 500
    np.testing.assert_array_equal(idx, g["idx"])
    np.testing.assert_array_equal(u, g["u"])
    np.testing.assert_array_equal(v, g["v"])
    LR.check_projection(P, g["idx"], g["u"], g["v"], name)


def test_nclt_extrinsic_is_the_one_the_reference_formed(golden):
    g = golden("proj_nclt.npz")
    np.testing.assert_allclose(LR.nclt_extrinsic(g["x_lb3_c"]), g["T_c_body"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ["oxf", "nclt"])
def test_lifting_reproduces_the_reference_fixtures(golden, name):
    g = golden(f"lift_{name}.npz")
    cams = _lift_fixture_cams(g, name)
    L = LR.lift(cams, g["xyz"])
    assert L.decided.all()
    desc, filled = LR.render(L, cams, list(g["grids"]))
    ref = g["desc"]
    np.testing.assert_array_equal(np.abs(desc).sum(1) > 0, np.abs(ref).sum(1) > 0)
    np.testing.assert_allclose(desc, ref, rtol=0, atol=1e-6)
    assert len(np.unique(L.seen[L.seen >= 0])) == len(cams)           # every camera wins some points


# ------------------------------------------------------------------------------------------------- separable upsample
SIZES = [(4, 5, 12, 17), (6, 8, 90, 120), (7, 9, 96, 128), (16, 21, 50, 73), (16, 20, 308, 404)]


def _upsample(G, H, W):
    t = torch.from_numpy(np.ascontiguousarray(G)).permute(2, 0, 1)[None]
    return F.interpolate(t, size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize("gh,gw,H,W", SIZES[:3])
def test_separable_weights_are_torchs_float32_weights(gh, gw, H, W):
    """F.interpolate of every unit impulse of a gh x gw grid equals, bit for bit in float32, the outer product of the
    identity-derived weight columns Ah[:, i] (x) Aw[:, j]: the 2-D upsample is separable with exactly these weights.
    Exception: in the last rows / columns torch adds l0 * x + l1 * x of ONE source row (index clamped to the edge), which
    the identity sees as a single weight l0 + l1 = 1; there the two may differ by an ulp."""
    Ah, Aw = LR.interp_matrix(gh, H), LR.interp_matrix(gw, W)
    h0, h1, _, _ = LR.taps(gh, H)
    w0, w1, _, _ = LR.taps(gw, W)
    inner = ~((h0 == h1) & (h0 == gh - 1))[:, None] & ~((w0 == w1) & (w0 == gw - 1))[None, :]
    assert inner.mean() > 0.5
    for i in range(gh):
        for j in range(gw):
            G = np.zeros((gh, gw, 1), np.float32)
            G[i, j] = 1.0
            up = _upsample(G, H, W)[..., 0]
            sep = np.outer(Ah[:, i], Aw[:, j]).astype(np.float32)
            np.testing.assert_array_equal(sep[inner].view(np.uint32), up[inner].view(np.uint32), err_msg=f"impulse {i}, {j}")
            np.testing.assert_allclose(sep[~inner], up[~inner], rtol=2.0 ** -22, atol=0)


@pytest.mark.parametrize("gh,gw,H,W", SIZES)
def test_separable_construction_equals_interpolate_in_float64(gh, gw, H, W):
    rng = np.random.default_rng(gh * 1000 + H)
    G = rng.standard_normal((gh, gw, 3))
    up = _upsample(G, H, W)
    sep = np.einsum("ri,ijc,sj->rsc", LR.interp_matrix(gh, H, "float64"), G, LR.interp_matrix(gw, W, "float64"))
    assert np.abs(sep - up).max() <= 1e-12


@pytest.mark.parametrize("gh,gw,H,W", SIZES)
def test_sampling_at_pixels_equals_interpolate_then_index(gh, gw, H, W):
    """lift_reference.sample (fp64 at the needed pixels) against the float32 upsample indexed at those pixels"""
    rng = np.random.default_rng(H * W)
    G = rng.standard_normal((gh, gw, 6)).astype(np.float32)
    raw = rng.integers(1, 256, (H, W, 3), dtype=np.uint8)
    up = _upsample(G, H, W)
    u, v = rng.integers(0, W, 500), rng.integers(0, H, 500)
    got, scale, zero = LR.sample(LR.kitti_camera(np.eye(3, 4), np.eye(4), 1, raw=raw), G, u, v)
    assert not zero.any()
    assert (np.abs(got - up[v, u]) <= 2.0 ** -22 * scale[:, None]).all()


@pytest.mark.parametrize("gh,gw,H,W", [(16, 20, 1232, 1616), (16, 21, 960, 1280), (16, 52, 376, 1241), (16, 20, 308, 404)])
def test_oracle_gather_uses_torchs_lambdas(gh, gw, H, W):
    """the C oracle's "interpolate at the pixel" (the kernels' operation order) against the restatement, at every row and
    every column of production-sized maps.  torch rounds the source index scale * (dst + 0.5) - 0.5 once; rounding the
    product first moves ~8 % of the lambdas by an ulp of the source index, up to 2^-19.5 of the corner rows."""
    from oracle import oracle as orc
    rng = np.random.default_rng(gh + gw + H)
    G = rng.standard_normal((gh, gw, 4)).astype(np.float32)
    raw = np.full((H, W, 3), 7, np.uint8)
    u = np.r_[np.arange(W), rng.integers(0, W, H)]
    v = np.r_[rng.integers(0, H, W), np.arange(H)]
    exp, scale, _ = LR.sample(LR.kitti_camera(np.eye(3, 4), np.eye(4), 1, raw=raw), G, u, v)
    got = orc.gather_bilinear(G, H, W, 0, u, v)
    err = np.abs(got - exp).max(axis=1) / scale
    assert err.max() <= 2.0 ** -22, (np.log2(err.max()), int((err > 2.0 ** -22).sum()))


# ------------------------------------------------------------------------------------------------- undecided points
def _edges(cam, image):
    if cam["mode"] == LR.NCLT:
        r0, c0, h, w = (int(t) for t in cam["win"])
        return r0, c0, h, w
    return 0, 0, image.shape[0], image.shape[1]


@pytest.mark.parametrize("name", ["kitti", "nclt", "oxf"])
def test_planted_boundary_points_are_undecided(golden, name):
    cam, image = _proj_fixture(golden(f"proj_{name}.npz"), name)
    r0, c0, h, w = _edges(cam, image)
    rng = np.random.default_rng(3)
    xm, ym = c0 + w // 2 + 1, r0 + h // 2 + 2
    xs = np.r_[c0, c0 + w, xm, xm, c0 + w, rng.integers(c0 + 1, c0 + w - 1, 8)]
    ys = np.r_[ym, ym, r0, r0 + h, r0 + h, rng.integers(r0 + 1, r0 + h - 1, 8)]
    pix = LR.backproject(cam, xs, ys, rng.uniform(4.0, 25.0, len(xs)))        # exact integers, bounds, window edges
    depth0 = LR.from_projective(cam, [[300.0, 200.0, d] for d in (0.0, 5e-324, -5e-324)])   # depth 0 and +-1 ulp
    P = LR.project(cam, np.insert(np.r_[pix, depth0], 3, 1, axis=1).T, image)
    assert not P.decided.any(), np.flatnonzero(P.decided)
    assert all(len(P.alts[i]) >= 2 for i in range(len(pix)) if P.alts[i] != {(False, 0, 0)})
    if cam["mode"] != LR.NCLT:   # the inclusive bound: u == W / v == H is one of the admissible answers
        assert (True, int(image.shape[1]), int(ym)) in P.alts[1]


def test_random_points_are_almost_never_undecided(golden):
    rng = np.random.default_rng(5)
    n = 300_000
    xyz = np.c_[rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(-3, 8, n)].astype(np.float32)
    pcl = np.insert(xyz, 3, 1, axis=1).T
    undecided = kept = 0
    for name in ("kitti", "nclt", "oxf"):
        cam, image = _proj_fixture(golden(f"proj_{name}.npz"), name)
        P = LR.project(cam, pcl, image)
        undecided += int((~P.decided).sum())
        kept += int(P.keep.sum())
    print(f"random points: {undecided} undecided of {3 * n} projections ({kept} kept)")
    assert kept > n // 4
    assert undecided < 3 * n * 1e-5


# ------------------------------------------------------------------------------------------------- negative controls
@pytest.fixture(scope="module")
def control_case(golden):
    """the lift_nclt fixture's two cameras, its cloud, plus points planted on integer pixels of camera 0"""
    g = golden("lift_nclt.npz")
    cams = _lift_fixture_cams(g, "nclt")
    r0, c0, h, w = (int(t) for t in cams[0]["win"])
    img = LR.projection_image(cams[0])
    ok = np.argwhere(np.any(img[1:h - 1, 1:w - 1] != 0, axis=-1) & np.any(img[:h - 2, :w - 2] != 0, axis=-1)) + 1
    pick = ok[np.random.default_rng(9).choice(len(ok), 6, replace=False)]
    planted = LR.backproject(cams[0], pick[:, 1] + c0, pick[:, 0] + r0, 6.0)
    L = LR.lift(cams, np.r_[planted, g["xyz"].astype(np.float64)])
    grids = list(g["grids"])
    desc, filled = LR.render(L, cams, grids)
    assert all(i in L.alts for i in range(len(planted)))
    return cams, grids, L, desc, filled


def test_helper_accepts_the_reference_output(control_case):
    cams, grids, L, desc, filled = control_case
    LR.check_lift(L, cams, grids, desc, filled)


def _mutate(case, what):
    cams, grids, L, desc, filled = case
    desc = desc.copy()
    if what == "winning_camera_swapped":
        i = int(np.flatnonzero(L.decided & (L.seen == 0) & L.projs[1].keep & L.projs[1].decided)[0])
        desc[i] = LR.rows(cams, grids, [1], [L.projs[1].u[i]], [L.projs[1].v[i]])[0][0]
    elif what == "rot90_column_off_by_one":
        desc = LR.render(L, cams, grids, _col_shift=1)[0]
    elif what == "non_black_row_zeroed":
        desc[int(np.flatnonzero(L.decided & np.any(desc != 0, axis=1))[0])] = 0.0
    elif what == "value_off_by_2^-18_relative":
        sel = np.flatnonzero(L.decided & np.any(desc != 0, axis=1))
        _, scale = LR.rows(cams, grids, L.seen[sel], L.u[sel], L.v[sel])
        ratio = np.abs(desc[sel]) / scale[:, None]
        j, c = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio[j, c] > 0.5
        desc[sel[j], c] *= np.float32(1 + 2.0 ** -18)
    elif what == "undecided_point_inadmissible":
        i = min(i for i in L.alts if L.seen[i] >= 0)
        s, u, v = int(L.seen[i]), int(L.u[i]) + 3, int(L.v[i])
        assert all((s, u, v) != a for a in L.alts[i])
        desc[i] = LR.rows(cams, grids, [s], [u], [v])[0][0]
    return desc, filled


@pytest.mark.parametrize("mutation", ["winning_camera_swapped", "rot90_column_off_by_one", "non_black_row_zeroed",
                                      "value_off_by_2^-18_relative", "undecided_point_inadmissible"])
def test_helper_rejects_a_mutated_output(control_case, mutation):
    cams, grids, L, _, _ = control_case
    desc, filled = _mutate(control_case, mutation)
    with pytest.raises(AssertionError):
        LR.check_lift(L, cams, grids, desc, filled)

"""create_descriptors on the GPU -- the fused vfm_lift_multicam kernel and the per-camera path -- against the independent
long-double / fp64 restatement of the reference in tests/lift_reference.py, for every camera model at the shapes the
product runs:

* NCLT: 5 cameras, raw images of 1232 x 1616 turned for the projection, a crop window per camera with black borders
  outside it, black pixels filtered in the projection image; image_subsample 1 and 4 (window // subsample);
* Oxford RobotCar: 4 cameras, one facing backwards, three chained 4 x 4 matrices, the inclusive u <= W bound;
  image_subsample 1 and 2;
* KITTI: 1 camera of 376 x 1241, and a 7-camera KITTI-mode rig (more than ops.LIFT_MAX_CAMS: the per-camera path);

at C = 384 and 768 (30 -- the scalar branch -- and 4 on the RobotCar rig), patch grids of 16 x gw (gw as image_features
computes it) and n = 1, 3, 4, 5, 4097, 60 000.  Every cloud starts with planted points: exact integer pixels, pixels on
the bounds and window edges, depth 0 and +-1 ulp, points behind the camera, non-finite rows, black pixels.  Each case
runs both device paths, which must agree bit for bit.  Decided points must match the reference exactly (filled, winning
camera) and to 2^-20 of the corner rows; undecided points must take an admissible answer and equal the fp64 oracle bit
for bit.  The undecided count of every rig is printed (`pytest -s`)."""
import types
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import lift_reference as LR  # noqa: E402

GH = 16                                   # patch rows (image_features.py: patch_h)
N_CLOUD = 60_000
NS = (1, 3, 4, 5, 4097, N_CLOUD)
RIGS = ("nclt_s1", "nclt_s4", "robotcar_s1", "robotcar_s2", "kitti", "kitti_7cam")
ROBOTCAR_CAMS = ("stereo/centre", "mono_left", "mono_right", "mono_rear")
KITTI_P2 = np.array([[718.856, 0.0, 607.1928, 45.38225], [0.0, 718.856, 185.2157, -0.1130887], [0.0, 0.0, 1.0, 0.003779761]])
KITTI_TR = np.array([[4.276802385584e-04, -9.999672484946e-01, -8.084491683471e-03, -1.198459927713e-02],
                     [-7.210626507497e-03, 8.081198471645e-03, -9.999413164504e-01, -5.403984729748e-02],
                     [9.999738645903e-01, 4.859485810390e-04, -7.206933692422e-03, -2.921968648686e-01],
                     [0.0, 0.0, 0.0, 1.0]])


def _gw(H, W):
    return int((14 * GH / H) * W / 14)    # image_features.py:67-69 (patch size 14)


def _pose(roll, pitch, yaw, t):
    from scipy.spatial.transform import Rotation
    T = np.eye(4)
    T[:3, :3] = Rotation.from_euler("xyz", [roll, pitch, yaw], degrees=True).as_matrix()
    T[:3, 3] = t
    return T


def _noise(rng, H, W):
    return rng.integers(1, 256, size=(H, W, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------- rigs
def _nclt(s):
    """5 Ladybug cameras 72 degrees apart; raw images as the dataset class returns them (cropped, turned clockwise)"""
    from vfmreg.dataloader import NCLT
    rng = np.random.default_rng(10 + s)
    names = [f"Cam{k + 1}" for k in range(5)]
    params, masks, images = {}, {}, {}
    for k, c in enumerate(names):
        coords = [40 + 8 * k, 24 + 4 * k, 1520 - 16 * k, 1160 - 8 * k]       # [row0, col0, h, w] in the turned frame
        params[c] = {"K": np.array([[450.0, 0.0, 604.0], [0.0, 450.0, 800.0], [0.0, 0.0, 1.0]]),
                     "x_lb3": _pose(-90.0, 0.0, 72.0 * k, [0.02, -0.01, 0.03])}
        masks[c] = {"coords": coords}
        r0, c0, h, w = np.array(coords) // s
        proj = _noise(rng, 1616 // s, 1232 // s)                          # what the projection sees
        proj[h:] = 0                                                      # black outside the window ...
        proj[:, w:] = 0
        proj[:, :max(1, 12 // s)] = 0                                     # ... a black band inside it ...
        proj[h // 3:h // 3 + 60 // s, w // 4:w // 4 + 90 // s] = 0        # ... and a black block
        images[c] = np.ascontiguousarray(np.rot90(proj, -1))             # raw image: (1232 x 1616) / s
    seq = NCLT(params, masks, image_subsample=s, cameras=names)
    cams = [LR.nclt_camera(LR.nclt_extrinsic(params[c]["x_lb3"]), params[c]["K"], masks[c]["coords"], s, raw=images[c])
            for c in names]
    return seq, cams, images


def _robotcar(s, order=ROBOTCAR_CAMS):
    """4 cameras, one facing backwards; ``order``: the camera dict order (= priority)"""
    from vfmreg.dataloader import OxfordRobotcar
    rng = np.random.default_rng(20 + s)
    H, W = 960 // s, 1280 // s
    G = np.array([[0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    fc = (400.0, 400.0, 640.0, 480.0)
    calib = {"lidar_in_ego": _pose(0.4, -0.3, 1.0, [0.5, 0.0, -0.2])}
    cm, images = {}, {}
    for k, (c, yaw) in enumerate(zip(ROBOTCAR_CAMS, (0.0, 75.0, -75.0, 180.0))):
        t = [0.2 * np.cos(np.deg2rad(yaw)), 0.2 * np.sin(np.deg2rad(yaw)), -0.1]
        calib[f"{c}_in_ego"] = np.linalg.inv(_pose(0.3 * k, -0.2, yaw, t))
        cm[c] = types.SimpleNamespace(G_camera_image=G, focal_length=fc[:2], principal_point=fc[2:])
        img = _noise(rng, H, W)
        img[H - 80 // s:] = 0
        img[H // 4:H // 4 + 50 // s, W // 3:W // 3 + 120 // s] = 0
        images[c] = img
    seq = OxfordRobotcar(calib, cm, image_subsample=s, cameras=list(order))
    images = {c: images[c] for c in order}
    cams = [LR.robotcar_camera(calib["lidar_in_ego"], calib[f"{c}_in_ego"], G, fc, s, raw=images[c]) for c in order]
    return seq, cams, images


def _kitti():
    from vfmreg.dataloader import KittiOdometry
    rng = np.random.default_rng(30)
    img = _noise(rng, 376, 1241)
    img[:, :24] = 0
    img[150:200, 500:640] = 0
    seq = KittiOdometry({"P2": KITTI_P2, "Tr_velo_to_cam": KITTI_TR}, image_subsample=1)
    return seq, [LR.kitti_camera(KITTI_P2, KITTI_TR, 1, raw=img)], {"camera": img}


class _KittiModeRig:
    """several KITTI-mode cameras (the dataset class has one): what create_descriptors asks of a sequence"""
    image_subsample = 1

    def __init__(self, Ps):
        from vfmreg.dataloader import KittiOdometry
        self._k = {c: KittiOdometry({"P2": P, "Tr_velo_to_cam": np.eye(4)}) for c, P in Ps.items()}
        self.cameras = list(Ps)

    def projection_params(self, camera, image_shape):
        return self._k[camera].projection_params("camera", image_shape)

    def project_pcl_to_image(self, pcl, image, camera, _device_inputs=None):
        return self._k[camera].project_pcl_to_image(pcl, image, "camera", _device_inputs=_device_inputs)


def _kitti_7cam():
    rng = np.random.default_rng(40)
    K = np.array([[400.0, 0.0, 620.0], [0.0, 400.0, 188.0], [0.0, 0.0, 1.0]])
    Ps, images = {}, {}
    for i in range(7):
        yaw = 2 * np.pi * i / 7
        R = np.stack([[np.sin(yaw), -np.cos(yaw), 0.0], [0.0, 0.0, -1.0], [np.cos(yaw), np.sin(yaw), 0.0]])
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = -R @ np.array([0.1 * np.cos(yaw), 0.1 * np.sin(yaw), 0.3])
        Ps[f"cam{i}"] = K @ T[:3]
        img = _noise(rng, 376, 1241)
        img[:, :30] = 0
        img[150:200, 500:640] = 0
        images[f"cam{i}"] = img
    cams = [LR.kitti_camera(Ps[c], np.eye(4), 1, raw=images[c]) for c in Ps]
    return _KittiModeRig(Ps), cams, images


BUILD = {"nclt_s1": lambda: _nclt(1), "nclt_s4": lambda: _nclt(4), "robotcar_s1": lambda: _robotcar(1),
         "robotcar_s2": lambda: _robotcar(2), "kitti": _kitti, "kitti_7cam": _kitti_7cam}


def _unseen(rng, n):
    """points straight above and below the rig: outside every camera's field of view"""
    return np.c_[rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.choice([-1.0, 1.0], n) * rng.uniform(60, 100, n)]


def _plant(cams, rng):
    """the planted rows, and the (camera, row) pairs that must come out undecided for that camera"""
    pts, boundary = [], []

    def add(p, cam=None):
        p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
        start = sum(len(a) for a in pts)
        if cam is not None:
            boundary.extend((cam, start + j) for j in range(len(p)))
        pts.append(p)

    add([[np.nan, 1.0, 1.0], [1.0, np.inf, 1.0]])
    for k, cam in enumerate(cams[:3]):
        img = LR.projection_image(cam)
        if cam["mode"] == LR.NCLT:
            r0, c0, h, w = (int(t) for t in cam["win"])
        else:
            r0, c0, h, w = 0, 0, img.shape[0], img.shape[1]
        xm, ym = c0 + w // 2 + 3, r0 + h // 2 + 5
        xs = np.r_[c0, c0 + w, xm, xm, c0 + w, rng.integers(c0 + 1, c0 + w - 1, 6)]
        ys = np.r_[ym, ym, r0, r0 + h, r0 + h, rng.integers(r0 + 1, r0 + h - 1, 6)]
        add(LR.backproject(cam, xs, ys, rng.uniform(4.0, 25.0, len(xs))), k)    # exact integers, bounds / window edges
        add(LR.from_projective(cam, [[300.0, 200.0, d] for d in (0.0, 5e-324, -5e-324)]), k)   # depth 0, +-1 ulp
        add(LR.backproject(cam, xm + 0.25, ym + 0.25, -6.0))                    # behind the camera, in line with the image
        black = np.argwhere(~np.any(img[:h, :w] != 0, axis=-1))
        pick = black[rng.choice(len(black), 3, replace=False)]
        add(LR.backproject(cam, pick[:, 1] + c0 + 0.5, pick[:, 0] + r0 + 0.5, rng.uniform(5.0, 20.0, 3)))  # black pixels
    add([[np.inf, 0.0, 0.0], [-np.inf, 5.0, 1.0], [1.0, 1.0, np.nan], [np.inf, -np.inf, np.nan]])
    add(_unseen(rng, 4))
    return np.concatenate(pts), boundary


_RIGS = {}


def _rig(name):
    if name not in _RIGS:
        seq, cams, images = BUILD[name]()
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        planted, boundary = _plant(cams, rng)
        m = N_CLOUD - len(planted)
        rand = np.c_[rng.uniform(-40, 40, m), rng.uniform(-40, 40, m), rng.uniform(-3, 8, m)].astype(np.float32)
        cloud = np.r_[planted, rand.astype(np.float64)]
        L = LR.lift(cams, cloud)
        _RIGS[name] = types.SimpleNamespace(name=name, seq=seq, cams=cams, images=images, cloud=cloud, lift=L,
                                            boundary=boundary, n_planted=len(planted))
        print(f"\n[lift] {name}: {len(L.alts)} of {N_CLOUD} points undecided (per camera {[len(p.alts) for p in L.projs]}; "
              f"{len(boundary)} planted boundary points)")
    return _RIGS[name]


def _grids(rig, C):
    H, W = next(iter(rig.images.values())).shape[:2]
    rng = np.random.default_rng(zlib.crc32(f"{rig.name}/{C}".encode()))
    return list(rng.standard_normal((len(rig.cams), GH, _gw(H, W), C)).astype(np.float32))


class _Grids:
    """patch_features_device stand-in (ImageFeatureGenerator without a ViT): seeded patch grids in batch order"""

    def __init__(self, grids):
        self.grids = grids

    def patch_features_device(self, images):
        assert images.shape[0] == len(self.grids)
        return torch.from_numpy(np.ascontiguousarray(np.stack(self.grids))).cuda()


@pytest.fixture
def run(monkeypatch):
    """create_descriptors on one path ('fused' / 'per_camera' forced); returns (desc, filled, path taken)"""
    from vfmreg import ops
    from vfmreg import prepare_scenes as PS
    last = {}
    real_lift, real_gather = ops.lift_multicam, ops.gather_bilinear

    def lift_spy(pcl4xn, cams, desc, filled):
        last.update(path="fused", filled=filled)
        return real_lift(pcl4xn, cams, desc, filled)

    def gather_spy(*args):
        last.update(path="per_camera", filled=args[-1])
        return real_gather(*args)
    monkeypatch.setattr(ops, "lift_multicam", lift_spy)
    monkeypatch.setattr(ops, "gather_bilinear", gather_spy)

    def go(seq, images, grids, pcl, per_camera):
        monkeypatch.setattr(PS, "_FORCE_PER_CAMERA", per_camera)
        last.clear()
        desc = PS.create_descriptors(None, seq, _Grids(grids), pcl, images=images)
        torch.cuda.synchronize()
        return desc, last["filled"].cpu().numpy(), last["path"]
    return go


def _oracle_check(seq, images, cams, grids, pcl4, L, gproj, desc, name):
    """undecided points: the product equals the fp64 oracle (orc.project, orc.create_descriptors) bit for bit"""
    from oracle import oracle as orc
    pts = np.array(sorted(set(L.alts) | {i for P in L.projs for i in P.alts}), dtype=np.int64)
    if len(pts) == 0:
        return
    sub = np.ascontiguousarray(pcl4[:, pts])
    ocams = []
    for k, (c, cam) in enumerate(zip(images, cams)):
        img = np.ascontiguousarray(LR.projection_image(cam))
        q = seq.projection_params(c, img.shape)
        ou, ov, oi = orc.project(q["mode"], sub, q["mats"], q["fc"], q["subsample"], q["win"],
                                 img if q.get("needs_image") else None, q["H"], q["W"])
        u, v, idx = gproj[k]
        m = np.isin(idx, pts)
        np.testing.assert_array_equal(np.searchsorted(pts, idx[m]), oi, err_msg=f"{name}: camera {c}, oracle indices")
        np.testing.assert_array_equal(u[m], ou, err_msg=f"{name}: camera {c}, oracle u")
        np.testing.assert_array_equal(v[m], ov, err_msg=f"{name}: camera {c}, oracle v")
        raw = cam["raw"]    # the product's zero row at u == W / v == H: a black pixel past the image's edge
        black = np.pad(~np.any(raw != 0, axis=-1), ((0, 1), (0, 1)), constant_values=True)
        ocams.append(dict(grid=grids[k], Hup=raw.shape[0], Wup=raw.shape[1], rot_mode=int(cam["mode"] == LR.NCLT),
                          black=black, u=ou, v=ov, idx=oi))
    np.testing.assert_array_equal(desc[pts], orc.create_descriptors(len(pts), ocams), err_msg=f"{name}: oracle rows")


def _check_case(run, seq, images, cams, grids, pcl, L, name):
    from vfmreg import ops
    n = len(pcl)
    d_f, f_f, path_f = run(seq, images, grids, pcl, False)
    d_p, f_p, path_p = run(seq, images, grids, pcl, True)
    assert path_f == ("fused" if len(cams) <= ops.LIFT_MAX_CAMS else "per_camera") and path_p == "per_camera"
    assert d_f.shape == (n, np.asarray(grids[0]).shape[2]) and d_f.dtype == np.float32
    np.testing.assert_array_equal(d_f.view(np.uint32), d_p.view(np.uint32), err_msg=f"{name}: fused vs per-camera")
    np.testing.assert_array_equal(f_f, f_p, err_msg=f"{name}: filled, fused vs per-camera")
    LR.check_lift(L, cams, grids, d_f, f_f)
    # the product's projection per camera (ops.project_pinhole through the dataset class) and its winning camera
    pcl4 = np.ascontiguousarray(np.insert(np.asarray(pcl)[:, :3], 3, values=1, axis=1).T, dtype=np.float64)
    won = np.full(n, -1, dtype=np.int64)
    gproj = []
    for k, (c, cam) in enumerate(zip(images, cams)):
        u, v, idx = seq.project_pcl_to_image(pcl4, np.ascontiguousarray(LR.projection_image(cam)), c)
        LR.check_projection(L.projs[k], idx, u, v, f"{name}: camera {c}")
        won[idx[won[idx] < 0]] = k
        gproj.append((u, v, idx))
    np.testing.assert_array_equal(won[L.decided], L.seen[L.decided], err_msg=f"{name}: winning camera")
    _oracle_check(seq, images, cams, grids, pcl4, L, gproj, d_f, name)
    print(f"[lift] {name}: {len(L.alts)} undecided of {n}; filled {int(f_f.sum())}")


CASES = [pytest.param(r, C, n, id=f"{r}-C{C}-n{n}") for r in RIGS for C in (384, 768) for n in NS]
CASES += [pytest.param("robotcar_s1", C, n, id=f"robotcar_s1-C{C}-n{n}") for C in (30, 4) for n in (5, 4097, N_CLOUD)]


@pytest.mark.parametrize("rig_name,C,n", CASES)
def test_lift_matches_the_fp64_reference(run, rig_name, C, n):
    rig = _rig(rig_name)
    _check_case(run, rig.seq, rig.images, rig.cams, _grids(rig, C), rig.cloud[:n], rig.lift.head(n), f"{rig_name} C={C} n={n}")


@pytest.mark.parametrize("rig_name", RIGS)
def test_rig_is_what_the_cases_claim(rig_name):
    """planted boundary points are undecided for their camera, fields of view overlap, every camera wins points"""
    rig = _rig(rig_name)
    L = rig.lift
    missed = [(k, i) for k, i in rig.boundary if L.projs[k].decided[i]]
    assert not missed, f"planted boundary points that came out decided: {missed[:8]}"
    rand = slice(rig.n_planted, None)
    seen_by = np.sum([p.keep[rand] for p in L.projs], axis=0)
    assert (seen_by >= 1).mean() > 0.1
    if len(rig.cams) > 1:
        assert (seen_by >= 2).mean() >= 0.2, (seen_by >= 2).mean()
    assert set(np.unique(L.seen[L.seen >= 0]).tolist()) == set(range(len(rig.cams)))
    assert not L.filled[:2].any() and not L.filled[rig.n_planted - 8:rig.n_planted].any()   # non-finite rows, unseen points


@pytest.mark.parametrize("rig_name", RIGS)
def test_an_all_black_camera(run, rig_name):
    """NCLT: the projection filters every point of an all-black camera; the others: its points keep zero rows"""
    rig = _rig(rig_name)
    k = 1 if len(rig.cams) > 1 else 0
    images = dict(rig.images)
    c = list(images)[k]
    images[c] = np.zeros_like(images[c])
    cams = [dict(cam, raw=images[nm]) for cam, nm in zip(rig.cams, images)]
    pcl = rig.cloud[:4097]
    L = LR.lift(cams, pcl)
    if cams[k]["mode"] == LR.NCLT:
        assert not (L.seen == k).any() and L.projs[k].keep.sum() == 0
    else:
        assert (L.seen == k).sum() > 100
    grids = _grids(rig, 384)
    _check_case(run, rig.seq, images, cams, grids, pcl, L, f"{rig_name} camera {c} black")


@pytest.mark.parametrize("rig_name", RIGS)
def test_a_cloud_no_camera_sees(run, rig_name):
    """all-zero descriptors, nothing filled (documented deviation: the reference fails on `pcl_indices is None`)"""
    rig = _rig(rig_name)
    pcl = _unseen(np.random.default_rng(1), 300)
    L = LR.lift(rig.cams, pcl)
    assert (L.seen < 0).all() and L.decided.all()
    _check_case(run, rig.seq, rig.images, rig.cams, _grids(rig, 384), pcl, L, f"{rig_name} unseen cloud")


def test_permuted_camera_dict_changes_the_winners_like_the_reference(run):
    base = _rig("robotcar_s1")
    order = ("mono_rear", "mono_right", "stereo/centre", "mono_left")
    seq, cams, images = _robotcar(1, order)
    n = 20_000
    pcl = base.cloud[:n]
    L = LR.lift(cams, pcl)
    names = np.array(list(order) + [""])
    base_names = np.array(list(ROBOTCAR_CAMS) + [""])
    both = L.decided & base.lift.decided[:n]
    changed = names[L.seen[both]] != base_names[base.lift.seen[:n][both]]
    assert changed.mean() > 0.05, changed.mean()
    grids_base = _grids(base, 384)
    grids = [grids_base[ROBOTCAR_CAMS.index(c)] for c in order]     # each camera keeps its own features
    _check_case(run, seq, images, cams, grids, pcl, L, "robotcar_s1 permuted")


@pytest.mark.parametrize("rig_name", ["nclt_s4", "robotcar_s2"])
def test_scene_batch_equals_the_per_cloud_calls(rig_name):
    """create_descriptors_batch (one ViT call for all clouds x cameras) gives every cloud the bits of its own call"""
    from vfmreg.prepare_scenes import create_descriptors, create_descriptors_batch
    rig = _rig(rig_name)
    rng = np.random.default_rng(7)
    names = list(rig.images)
    clouds = [rig.cloud[np.sort(rng.permutation(N_CLOUD)[:5000 + 1000 * i])] for i in range(3)]
    images_list = [{c: np.roll(rig.images[c], 37 * (i + 1), axis=1) for c in names} for i in range(3)]
    shape = (len(names),) + _grids(rig, 384)[0].shape
    grids = [list(rng.standard_normal(shape).astype(np.float32)) for _ in range(3)]
    single = [create_descriptors(None, rig.seq, _Grids(grids[i]), clouds[i], images=images_list[i]) for i in range(3)]
    batched = create_descriptors_batch(None, rig.seq, _Grids([g for gs in grids for g in gs]), clouds, images_list=images_list)
    for i, (a, b) in enumerate(zip(single, batched)):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"cloud {i}")
        assert (np.abs(a).sum(1) > 0).sum() > 1000

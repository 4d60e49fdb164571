"""The camera front end on the GPU (csrc/camera.hip) against the numpy restatement in tests/rectify_reference.py, bit for bit,
with every output in a guarded buffer (tests/guarded.py) so that a write outside it shows.

Inputs are the mosaics and tables of tests/golden/rectify_robotcar.npz: 24 x 32, 50 x 38 and 6 x 8 frames with a saturated
255 patch in the corner and a zero patch; tables with a smooth warp plus noise and planted entries -- exact integers, x = W-1 and
y = H-1 exactly, -1e-12, W-1+1e-12, -0.5, NaN, infinity, samples on the outermost ring whose demosaic overshoots 255, one whole row
pointing outside.  24 * 32 = 768 and 50 * 38 = 1900 pixels are 3 and 8 workgroups of 256, the second with a partial one; the
cropped outputs end inside a workgroup, so the dword and the byte tails of the staged stores both run."""
import types
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import rectify_reference as RR  # noqa: E402
from tests.guarded import GuardedBuffer  # noqa: E402

SHAPES = (0, 1, 2)
GUARD = 1 << 16


@pytest.fixture(scope="module")
def fx(golden):
    return golden("rectify_robotcar.npz")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("pattern", RR.PATTERNS)
@pytest.mark.parametrize("i", SHAPES)
def test_demosaic(fx, i, pattern):
    from vfmreg import _lib, ops
    cfa = fx[f"cfa{i}"]
    want = RR.demosaic_bilinear(cfa, pattern)
    assert want.max() > 255.0                                    # the outermost ring's overshoot is in the case
    out = GuardedBuffer(cfa.shape + (3,), torch.float32, guard=GUARD).fill_nan()
    cfa_d = _dev(cfa)
    _lib.check(_lib.load().vfm_demosaic_bilinear(cfa_d.data_ptr(), cfa.shape[0], cfa.shape[1], ops.BAYER_PATTERNS[pattern], out.ptr(),
                                                 torch.cuda.current_stream().cuda_stream), "demosaic")
    torch.cuda.synchronize()
    assert out.intact(), out.intact()
    assert np.array_equal(out.numpy().astype(np.float64), want)
    assert np.array_equal(ops.demosaic_bilinear(cfa_d, pattern).cpu().numpy(), want.astype(np.float32))


@pytest.mark.parametrize("dtype", ("uint8", "float32", "float64"))
@pytest.mark.parametrize("i", SHAPES)
def test_undistort(fx, i, dtype):
    from vfmreg import _lib, ops
    lut = fx[f"lut{i}"]
    assert np.isnan(lut).any() and np.isinf(lut).any()
    img = fx[f"img{i}"]
    image = {"uint8": img, "float32": (img / 3).astype(np.float32), "float64": RR.demosaic_bilinear(fx[f"cfa{i}"], "GBRG")}[dtype]
    want = RR.undistort_lut(image, lut)
    tdt = getattr(torch, dtype)
    out = GuardedBuffer(image.shape, tdt, guard=GUARD).fill_bytes(0xFF)
    image_d, lut_d = _dev(image), _dev(lut)
    H, W, C = image.shape
    _lib.check(_lib.load().vfm_undistort_lut(image_d.data_ptr(), {"uint8": 0, "float32": 1, "float64": 2}[dtype], H, W, C, lut_d.data_ptr(),
                                             out.ptr(), torch.cuda.current_stream().cuda_stream), "undistort")
    torch.cuda.synchronize()
    assert out.intact(), out.intact()
    got = out.numpy()
    assert got.dtype == want.dtype and np.array_equal(got, want)
    outside = ~((lut[:, 0] >= 0) & (lut[:, 0] <= W - 1) & (lut[:, 1] >= 0) & (lut[:, 1] <= H - 1))
    assert outside.sum() >= W and not got.reshape(H * W, C)[outside].any()      # NaN, infinity, -1e-12, the row outside: exactly 0
    assert np.array_equal(ops.undistort_lut(image_d, lut_d).cpu().numpy(), want)


def test_undistort_matches_the_reference_output(fx):
    """... and the reference's own CameraModel.undistort, recorded in the fixture, through vfmreg.camera_model.CameraModel"""
    from vfmreg.camera_model import CameraModel
    for i in SHAPES:
        cm = CameraModel((1.0, 1.0), (0.0, 0.0), np.eye(4), fx[f"lut{i}"])
        assert np.array_equal(cm.undistort(fx[f"img{i}"]), fx[f"undist_u8_{i}"])
        got = cm.undistort((fx[f"img{i}"] / 3).astype(np.float32))
        assert got.dtype == np.float32 and np.array_equal(got, fx[f"undist_f32_{i}"])
        assert np.array_equal(cm.undistort(fx[f"demosaic{i}_RGGB"]), fx[f"undist{i}_RGGB"])
        dev = cm.undistort(torch.from_numpy(fx[f"img{i}"]).cuda())
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), fx[f"undist_u8_{i}"])
        with pytest.raises(ValueError, match="Incorrect image size for camera model"):
            cm.undistort(np.zeros((3, 5, 3), np.uint8))


def _rectify_guarded(cams):
    """ops.rectify_bayer with guarded outputs and a guarded workspace; returns the outputs as numpy"""
    from vfmreg import ops
    outs = []
    for c in cams:
        H, W = c["mosaic"].shape
        s = c["subsample"]
        outs.append(GuardedBuffer(((H - c["crop_bottom"]) // s, W // s, 3), torch.uint8, guard=GUARD).fill_bytes(0xA5))
    ws_bytes = sum((3 * (c["mosaic"].shape[0] - c["crop_bottom"]) * c["mosaic"].shape[1] + 255) // 256 * 256 for c in cams if c["subsample"] == 2)
    ws = GuardedBuffer(max(ws_bytes, 256), torch.uint8, guard=GUARD)
    ops.rectify_bayer([dict(c, mosaic=_dev(c["mosaic"]), table=_dev(c["table"]), out=o.t) for c, o in zip(cams, outs)], ws=ws.t)
    torch.cuda.synchronize()
    for o in outs + [ws]:
        assert o.intact(), o.intact()
    return [o.numpy() for o in outs]


@pytest.mark.parametrize("subsample", (1, 2))
@pytest.mark.parametrize("pattern", RR.PATTERNS)
@pytest.mark.parametrize("i", SHAPES)
def test_rectify_one_camera(fx, i, pattern, subsample):
    cfa, lut, crop = fx[f"cfa{i}"], fx[f"lut{i}"], int(fx[f"crop{i}"])
    want = RR.rectify_bayer(cfa, pattern, lut, crop, subsample)
    got, = _rectify_guarded([dict(mosaic=cfa, pattern=pattern, table=lut, crop_bottom=crop, subsample=subsample)])
    assert np.array_equal(got, want)
    assert np.array_equal(got, fx[f"rect{subsample}{i}_{pattern}"])          # what PIL and the reference's undistort recorded
    if subsample == 1:
        full = RR.undistort_lut(RR.demosaic_bilinear(cfa, pattern), lut)[:cfa.shape[0] - crop]
        assert (full > 256).any()                                           # the low-8-bits cast is in the case
        H, W = cfa.shape
        outside = ~((lut[:, 0] >= 0) & (lut[:, 0] <= W - 1) & (lut[:, 1] >= 0) & (lut[:, 1] <= H - 1))[:(H - crop) * W]
        assert not got.reshape(-1, 3)[outside].any()                        # exactly (0, 0, 0)


def test_rectify_four_cameras(fx):
    """two sizes, both crops (150 and 200 rows scaled down to 8 and 6), factors 1 and 2 in one call"""
    cams = [dict(mosaic=fx["cfa1"], pattern="GBRG", table=fx["lut1"], crop_bottom=8, subsample=2),
            dict(mosaic=fx["cfa0"], pattern="RGGB", table=fx["lut0"], crop_bottom=6, subsample=1),
            dict(mosaic=fx["cfa0"][::-1].copy(), pattern="RGGB", table=fx["lut0"], crop_bottom=6, subsample=2),
            dict(mosaic=fx["cfa1"][:, ::-1].copy(), pattern="RGGB", table=fx["lut1"], crop_bottom=8, subsample=1)]
    for c, got in zip(cams, _rectify_guarded(cams)):
        assert np.array_equal(got, RR.rectify_bayer(c["mosaic"], c["pattern"], c["table"], c["crop_bottom"], c["subsample"]))


def test_rectify_refuses_on_the_device(fx):
    from vfmreg import ops
    cam = dict(mosaic=_dev(fx["cfa0"]), pattern="RGGB", table=_dev(fx["lut0"]), crop_bottom=6, subsample=2)
    with pytest.raises(RuntimeError, match="workspace"):
        ops.rectify_bayer([cam], ws=torch.empty(256, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="not divisible"):
        ops.rectify_bayer([dict(cam, crop_bottom=5)])
    with pytest.raises(NotImplementedError, match="resize"):
        ops.rectify_bayer([dict(cam, subsample=3)])
    with pytest.raises(ValueError, match="Incorrect image size"):
        ops.rectify_bayer([dict(cam, table=_dev(fx["lut1"]))])


# ------------------------------------------------------------------------------------------------- the dataset class
CAMS = ("stereo/centre", "mono_left", "mono_right")
G_CAMERA_IMAGE = np.array([[0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])


def _sequence(fx, subsample):
    """stereo/centre on the 50 x 38 frame (GBRG, crop 8), the mono cameras on the 24 x 32 frame (RGGB, crop 6)"""
    from scipy.spatial.transform import Rotation
    from vfmreg.camera_model import CameraModel
    from vfmreg.dataloader import OxfordRobotcar
    shape = {"stereo/centre": 1, "mono_left": 0, "mono_right": 0}
    calib = {"lidar_in_ego": np.eye(4)}
    cm, raw = {}, {}
    for k, (c, yaw) in enumerate(zip(CAMS, (0.0, 50.0, -50.0))):
        T = np.eye(4)
        T[:3, :3] = Rotation.from_euler("z", yaw, degrees=True).as_matrix()
        calib[f"{c}_in_ego"] = np.linalg.inv(T)
        cfa = fx[f"cfa{shape[c]}"]
        H, W = cfa.shape
        cm[c] = CameraModel((12.0, 12.0), (W / 2, H / 3), G_CAMERA_IMAGE, fx[f"lut{shape[c]}"])
        raw[c] = np.roll(cfa, 3 * k, axis=1) if k else cfa
    seq = OxfordRobotcar(calib, cm, image_subsample=subsample, cameras=list(CAMS))
    seq.FRONT_END = {"stereo/centre": ("GBRG", 8)}
    seq.FRONT_END_DEFAULT = ("RGGB", 6)
    return seq, raw, shape


@pytest.mark.parametrize("subsample", (1, 2))
def test_rectify_images(fx, subsample, monkeypatch):
    from vfmreg import ops
    seq, raw, shape = _sequence(fx, subsample)
    calls = []
    real = ops.rectify_bayer
    monkeypatch.setattr(ops, "rectify_bayer", lambda cams, ws=None: calls.append(len(cams)) or real(cams, ws))
    got = seq.rectify_images(raw)
    assert calls == [3] and list(got.keys()) == list(CAMS)                  # one call for the rig
    for c in CAMS:
        pattern, crop = ("GBRG", 8) if c == "stereo/centre" else ("RGGB", 6)
        want = RR.rectify_bayer(raw[c], pattern, fx[f"lut{shape[c]}"], crop, subsample)
        assert isinstance(got[c], np.ndarray) and got[c].dtype == np.uint8 and np.array_equal(got[c], want)
    dev = seq.rectify_images({c: torch.from_numpy(raw[c]).cuda() for c in CAMS}, device=True)
    for c in CAMS:
        assert dev[c].is_cuda and dev[c].dtype == torch.uint8 and np.array_equal(dev[c].cpu().numpy(), got[c])
    with pytest.raises(NotImplementedError):
        seq.read_images(["a.png"])


def test_the_dataset_front_end_constants():
    from vfmreg.dataloader import OxfordRobotcar
    assert OxfordRobotcar.FRONT_END == RR.ROBOTCAR_FRONT_END and OxfordRobotcar.FRONT_END_DEFAULT == RR.ROBOTCAR_DEFAULT


class _Grids:
    """patch_features_device stand-in: a patch grid seeded by each image's bytes, so it does not depend on the batching"""

    def patch_features_device(self, images):
        out = []
        for im in images.cpu().numpy():
            rng = np.random.default_rng(zlib.crc32(im.tobytes()))
            out.append(rng.standard_normal((4, 5, 8)).astype(np.float32))
        return torch.from_numpy(np.stack(out)).cuda()


def test_create_descriptors_takes_device_images(fx, monkeypatch):
    from vfmreg import prepare_scenes as PS
    seq, raw, _ = _sequence(fx, 1)
    dev = seq.rectify_images(raw, device=True)
    host = {c: dev[c].cpu().numpy() for c in CAMS}
    rng = np.random.default_rng(5)
    pcl = np.c_[rng.uniform(-20, 20, 3000), rng.uniform(-20, 20, 3000), rng.uniform(-3, 8, 3000)].astype(np.float32)
    want = PS.create_descriptors(None, seq, _Grids(), pcl, images=host)
    assert (np.abs(want).sum(1) > 0).sum() > 100                           # points are lifted, and black pixels zero some
    downloads = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: downloads.append(t.dtype) or real_cpu(t, *a, **k))
    fg = types.SimpleNamespace(patch_features_device=lambda images: _grids_no_spy(images, real_cpu))
    got = PS.create_descriptors(None, seq, fg, pcl, images=dev)
    assert np.array_equal(got, want)
    assert torch.uint8 not in downloads                                     # no image came back to the host
    monkeypatch.undo()
    both = PS.create_descriptors_batch([None, None], seq, _Grids(), [pcl, pcl[:1000]], images_list=[dev, dev])
    assert np.array_equal(both[0], want) and np.array_equal(both[1], want[:1000])
    # two cameras of one size: the batched forward stacks the device images
    mono_dev, mono_host = {c: dev[c] for c in CAMS[1:]}, {c: host[c] for c in CAMS[1:]}
    both = PS.create_descriptors_batch([None, None], seq, _Grids(), [pcl, pcl[:1000]], images_list=[mono_dev, mono_dev])
    assert np.array_equal(both[0], PS.create_descriptors(None, seq, _Grids(), pcl, images=mono_host))
    assert np.array_equal(both[1], both[0][:1000])


def _grids_no_spy(images, real_cpu):
    out = []
    for im in real_cpu(images).numpy():
        rng = np.random.default_rng(zlib.crc32(im.tobytes()))
        out.append(rng.standard_normal((4, 5, 8)).astype(np.float32))
    return torch.from_numpy(np.stack(out)).cuda()

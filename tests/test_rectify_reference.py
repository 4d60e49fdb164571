"""tests/rectify_reference.py against the libraries it restates: bit for bit at every stage on what they recorded in
tests/golden/rectify_robotcar.npz (scipy's convolve demosaic, the reference's CameraModel.undistort, numpy's cast, PIL's crop and
resize), and on fresh random inputs where scipy / PIL are importable.  Also what the wrappers refuse without a device."""
import numpy as np
import pytest

from tests import rectify_reference as RR

SHAPES = (0, 1, 2)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("rectify_robotcar.npz")


@pytest.mark.parametrize("pattern", RR.PATTERNS)
@pytest.mark.parametrize("i", SHAPES)
def test_every_stage_equals_the_fixture(fx, i, pattern):
    cfa, lut, crop = fx[f"cfa{i}"], fx[f"lut{i}"], int(fx[f"crop{i}"])
    dem = RR.demosaic_bilinear(cfa, pattern)
    assert np.array_equal(dem, fx[f"demosaic{i}_{pattern}"])
    assert dem.max() in (382.5, 573.75)                      # the outermost ring's overshoot at the saturated corner
    und = RR.undistort_lut(dem, lut)
    assert und.dtype == np.float64 and np.array_equal(und, fx[f"undist{i}_{pattern}"])
    u8 = RR.cast_u8(und)
    assert np.array_equal(u8, fx[f"u8{i}_{pattern}"])
    assert (und >= 256).any() and not np.array_equal(u8, np.clip(und, 0, 255).astype(np.uint8))   # low 8 bits, not a clamp
    assert np.array_equal(RR.rectify_bayer(cfa, pattern, lut, crop, 1), fx[f"rect1{i}_{pattern}"])
    assert np.array_equal(RR.rectify_bayer(cfa, pattern, lut, crop, 2), fx[f"rect2{i}_{pattern}"])


@pytest.mark.parametrize("i", SHAPES)
def test_undistort_of_uint8_and_float32_images(fx, i):
    img, lut = fx[f"img{i}"], fx[f"lut{i}"]
    got = RR.undistort_lut(img, lut)
    assert got.dtype == np.uint8 and np.array_equal(got, fx[f"undist_u8_{i}"])
    got = RR.undistort_lut((img / 3).astype(np.float32), lut)
    assert got.dtype == np.float32 and np.array_equal(got, fx[f"undist_f32_{i}"])


@pytest.mark.parametrize("i", SHAPES)
def test_the_planted_entries_are_in_the_tables(fx, i):
    lut = fx[f"lut{i}"]
    H, W = fx[f"cfa{i}"].shape
    x, y = lut[:, 0].reshape(H, W), lut[:, 1].reshape(H, W)
    assert np.isnan(x).any() and np.isnan(y).any() and np.isinf(x).any()
    assert (x[0, 0], y[0, 0]) == (0.0, 0.0) and (x == W - 1).any() and (y == H - 1).any()
    for v in (-1e-12, -0.5, W - 1 + 1e-12):
        assert (x == v).any()
    assert (x[3] > W - 1).all()                              # one whole row outside
    out = RR.undistort_lut(RR.demosaic_bilinear(fx[f"cfa{i}"], "RGGB"), lut)
    assert not out[3].any() and not out[1, 1:8].any()        # outside, NaN and infinity: exactly 0
    assert out[0, 0, 0] == 573.75


def test_interp_against_scipy_on_fresh_coordinates():
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1)
    H, W = 37, 29
    ch = rng.uniform(0, 600, (H, W))
    n = 200_000
    y, x = rng.uniform(-1, H, n), rng.uniform(-1, W, n)
    y[:4000], x[4000:8000] = np.floor(y[:4000]), np.floor(x[4000:8000])          # exact integers
    y[8000:8100], x[8100:8200] = H - 1, W - 1                                    # the last row / column
    y[8200:8300] = np.nextafter(H - 1.0, np.inf)
    x[8300:8400] = np.nextafter(0.0, -np.inf)
    assert np.array_equal(RR.interp_lut(ch, x, y), nd.map_coordinates(ch, np.stack([y, x]), order=1))
    u8 = rng.integers(0, 256, (H, W)).astype(np.uint8)
    lut = np.stack([x[:H * W], y[:H * W]], 1)
    assert np.array_equal(RR.undistort_lut(u8[:, :, None], lut)[:, :, 0], nd.map_coordinates(u8, np.stack([y[:H * W], x[:H * W]]).reshape(2, H, W), order=1))


@pytest.mark.parametrize("pattern", RR.PATTERNS)
def test_demosaic_against_scipy_on_a_fresh_mosaic(pattern):
    nd = pytest.importorskip("scipy.ndimage")
    cfa = np.random.default_rng(2).integers(0, 256, (21, 34)).astype(np.uint8)
    f = cfa.astype(np.float64)
    mask = {c: np.zeros(cfa.shape) for c in "RGB"}
    for c, (y, x) in zip(pattern, [(0, 0), (0, 1), (1, 0), (1, 1)]):
        mask[c][y::2, x::2] = 1
    k_g = np.array([[0, 1, 0], [1, 4, 1], [0, 1, 0]]) / 4
    k_rb = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]]) / 4
    want = np.stack([nd.convolve(f * mask["R"], k_rb), nd.convolve(f * mask["G"], k_g), nd.convolve(f * mask["B"], k_rb)], -1)
    assert np.array_equal(RR.demosaic_bilinear(cfa, pattern), want)


@pytest.mark.parametrize("shape", ((2, 2), (4, 6), (18, 32), (42, 38), (810 // 5, 1280 // 5)))
def test_resize_against_pil_on_fresh_images(shape):
    Image = pytest.importorskip("PIL.Image")
    img = np.random.default_rng(3).integers(0, 256, shape + (3,)).astype(np.uint8)
    img[: shape[0] // 2, : shape[1] // 2] = 255
    want = np.asarray(Image.fromarray(img).resize((shape[1] // 2, shape[0] // 2), Image.BILINEAR))
    assert np.array_equal(RR.resize2_bilinear(img), want)


def test_pil_weights_by_integers():
    """csrc/camera.hip forms the same weights without floating point: (w * 2^23 + S) // (2 S) for taps 1, 3, 3, 1 of sum S"""
    for n_in in (2, 4, 6, 38, 810, 1024):
        for i, (lo, ks) in enumerate(RR.pil_bilinear_coeffs(n_in, n_in // 2)):
            taps = [j for j in range(2 * i - 1, 2 * i + 3) if 0 <= j < n_in]
            w = [1 if j in (2 * i - 1, 2 * i + 2) else 3 for j in taps]
            assert lo == taps[0] and ks == [(v * (1 << 23) + sum(w)) // (2 * sum(w)) for v in w] and sum(ks) == 1 << 22


# ------------------------------------------------------------------------------------------------- refusals (no device needed)
def _cpu_cam(H=24, W=32, **over):
    torch = pytest.importorskip("torch")
    cam = dict(mosaic=torch.zeros((H, W), dtype=torch.uint8), pattern="RGGB", table=torch.zeros((H * W, 2), dtype=torch.float64),
               crop_bottom=6, subsample=1)
    cam.update(over)
    return cam


def test_wrappers_refuse_cpu_tensors():
    torch = pytest.importorskip("torch")
    from vfmreg import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.demosaic_bilinear(torch.zeros((4, 6), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.undistort_lut(torch.zeros((4, 6, 3), dtype=torch.uint8), torch.zeros((24, 2), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rectify_bayer([_cpu_cam()])


def test_wrappers_refuse_bad_shapes():
    torch = pytest.importorskip("torch")
    from vfmreg import ops
    with pytest.raises(ValueError, match="Incorrect image size for camera model"):
        ops.undistort_lut(torch.zeros((4, 6, 3), dtype=torch.uint8), torch.zeros((23, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="multi-channel"):
        ops.undistort_lut(torch.zeros((4, 6), dtype=torch.uint8), torch.zeros((24, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="Incorrect image size for camera model"):
        ops.rectify_bayer([_cpu_cam(table=torch.zeros((24 * 32 - 1, 2), dtype=torch.float64))])
    with pytest.raises(ValueError, match="not divisible by the subsample factor 2"):
        ops.rectify_bayer([_cpu_cam(crop_bottom=5, subsample=2)])           # 19 rows
    with pytest.raises(ValueError, match="not divisible by the subsample factor 2"):
        ops.rectify_bayer([_cpu_cam(W=31, subsample=2)])
    with pytest.raises(NotImplementedError, match="resize"):
        ops.rectify_bayer([_cpu_cam(subsample=3)])
    with pytest.raises(ValueError, match="pattern"):
        ops.demosaic_bilinear(torch.zeros((4, 6), dtype=torch.uint8), "RGBG")
    with pytest.raises(ValueError):
        ops.rectify_bayer([])


def test_camera_model_and_dataset_refusals(tmp_path):
    pytest.importorskip("torch")
    from vfmreg.camera_model import CameraModel, model_name
    from vfmreg.dataloader import OxfordRobotcar
    H, W = 24, 32
    rng = np.random.default_rng(4)
    lut = rng.uniform(0, 20, (H * W, 2))
    G = np.arange(16.0).reshape(4, 4)
    (tmp_path / "mono_left.txt").write_text("400.5 399.25 508.0 498.5\n" + "\n".join(" ".join(repr(float(v)) for v in row) for row in G) + "\n")
    np.ascontiguousarray(lut.T).tofile(tmp_path / "mono_left_distortion_lut.bin")
    cm = CameraModel.from_files(tmp_path, "/data/2019-01-10-11-46-21/mono_left")
    assert cm.focal_length == (400.5, 399.25) and cm.principal_point == (508.0, 498.5)
    assert np.array_equal(cm.G_camera_image, G) and np.array_equal(cm.bilinear_lut, lut)
    assert [model_name(d) for d in ("a/stereo/centre", "a/stereo/left", "a/stereo/right", "a/mono_rear")] == \
        ["stereo_narrow_left", "stereo_wide_left", "stereo_wide_right", "mono_rear"]
    with pytest.raises(ValueError, match="Incorrect image size for camera model"):
        cm.undistort(np.zeros((H, W + 1, 3), np.uint8))
    with pytest.raises(ValueError, match="Undistortion function only works with multi-channel images"):
        cm.undistort(np.zeros((H, W), np.uint8))
    for s, exc, text in ((3, NotImplementedError, "resize"), (4, NotImplementedError, "resize")):
        with pytest.raises(exc, match=text):
            OxfordRobotcar({}, {"mono_left": cm}, image_subsample=s).rectify_images({"mono_left": np.zeros((H, W), np.uint8)})
    seq = OxfordRobotcar({}, {"mono_left": cm}, image_subsample=2)
    seq.FRONT_END_DEFAULT = ("RGGB", 5)
    with pytest.raises(ValueError, match="not divisible"):
        seq.rectify_images({"mono_left": np.zeros((H, W), np.uint8)})
    with pytest.raises(ValueError, match="Incorrect image size for camera model"):
        OxfordRobotcar({}, {"mono_left": cm}).rectify_images({"mono_left": np.zeros((300, W), np.uint8)})
    with pytest.raises(NotImplementedError):
        seq.read_images(["frame.png"])

"""Generate tests/golden/rectify_robotcar.npz: seeded Bayer mosaics and look-up tables, and what the LIBRARIES make of them.

    python tests/golden/make_rectify_fixture.py <reference>/src/vfm-reg/src

Runs only where scipy, PIL and the reference tree are present.  Nothing of the reference travels: the fixture holds arrays only.
Per shape i (0: 24 x 32, 1: 50 x 38, 2: 6 x 8):
  cfa{i}            uint8 [H, W]: random, a saturated 255 patch in the top-left corner, a zero patch
  lut{i}            fp64 [H*W, 2] in the SDK's layout (x, y): a smooth warp plus noise, with planted entries (below)
  crop{i}           rows dropped at the bottom (the dataset's 150 / 200 scaled down to 6 / 8 / 2)
  img{i}            uint8 [H, W, 3]: a random RGB image for the uint8 / float32 undistortion
and per Bayer pattern p:
  demosaic{i}_{p}   fp64: scipy.ndimage.convolve of the masked mosaic with colour_demosaicing's two kernels (that library is absent
                    everywhere; its formula is restated on scipy's convolve, so the ``reflect`` border is scipy's own)
  undist{i}_{p}     fp64: the reference's CameraModel.undistort of that image (object.__new__ + a planted bilinear_lut)
  u8{i}_{p}         numpy's .astype(np.uint8) of it
  rect1{i}_{p}      PIL's crop, as oxford_robotcar.py:119-124
  rect2{i}_{p}      ... and Image.resize((W // 2, H // 2), BILINEAR), oxford_robotcar.py:132-135
  undist_u8_{i}, undist_f32_{i}: CameraModel.undistort of img{i} and of img{i} / 3 as float32
scipy leaves the result at a NaN coordinate undefined; this project defines it as 0.  The tables hold NaN
entries, and the libraries are run on a copy in which they are replaced by -5 (outside, hence 0).
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np
from PIL import Image as PIL_Image
from scipy.ndimage import convolve

OUT = Path(__file__).resolve().parent
SHAPES = [(24, 32, 6), (50, 38, 8), (6, 8, 2)]
PATTERNS = ("RGGB", "GBRG", "GRBG", "BGGR")


def make_cfa(rng, H, W):
    cfa = rng.integers(0, 256, (H, W)).astype(np.uint8)
    cfa[:max(H // 4, 2), :max(W // 4, 2)] = 255
    cfa[H // 2:H // 2 + max(H // 6, 1), W // 2:W // 2 + max(W // 5, 1)] = 0
    return cfa


def make_lut(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    lx = xx + 1.7 * np.sin(yy / 5) + rng.uniform(-0.5, 0.5, (H, W))
    ly = yy + 1.3 * np.cos(xx / 7) + rng.uniform(-0.5, 0.5, (H, W))
    # row 0: the outermost ring (its demosaic overshoots 255 in the saturated corner), exact integers
    plant0 = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.25, 0.0), (0.0, 0.5), (2.0, 1.0), (W - 1.0, H - 1.0), (W - 1.0, 2.0)]
    # row 1: the last row / column exactly, just outside, half a pixel outside, NaN, infinity
    plant1 = [(3.0, H - 1.0), (-1e-12, 2.0), (2.0, -1e-12), (W - 1 + 1e-12, 3.0), (3.0, H - 1 + 1e-12), (-0.5, 1.0), (np.nan, 1.0),
              (1.0, np.nan)]
    for row, plant in ((0, plant0), (1, plant1)):
        for k, (x, y) in enumerate(plant[:W]):
            lx[row, k], ly[row, k] = x, y
    lx[1, min(8, W - 1)] = np.inf
    lx[3, :] = W + 2.0 + xx[3]      # one whole row pointing outside
    return np.stack([lx.ravel(), ly.ravel()], 1)


def demosaic_scipy(cfa, pattern):
    """colour_demosaicing.demosaicing_CFA_Bayer_bilinear on scipy.ndimage.convolve (default mode: reflect)."""
    cfa = cfa.astype(np.float64)
    ch = {c: np.zeros(cfa.shape) for c in "RGB"}
    for c, (y, x) in zip(pattern, [(0, 0), (0, 1), (1, 0), (1, 1)]):
        ch[c][y::2, x::2] = 1
    H_G = np.array([[0, 1, 0], [1, 4, 1], [0, 1, 0]], np.float64) / 4
    H_RB = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.float64) / 4
    return np.stack([convolve(cfa * ch["R"], H_RB), convolve(cfa * ch["G"], H_G), convolve(cfa * ch["B"], H_RB)], -1)


def load_camera_model(ref_src: Path):
    spec = importlib.util.spec_from_file_location("ref_camera_model", ref_src / "dataloader" / "robotcar_sdk" / "python" / "camera_model.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CameraModel


def library_outputs(CameraModel, cfa, lut, crop, img):
    """{name: array} for one shape: every stage through the reference / scipy / numpy / PIL."""
    cm = object.__new__(CameraModel)
    cm.bilinear_lut = np.where(np.isnan(lut), -5.0, lut)
    out = {}
    for p in PATTERNS:
        dem = demosaic_scipy(cfa, p)
        und = cm.undistort(dem)
        u8 = und.astype(np.uint8)
        pil = PIL_Image.fromarray(u8)
        pil = pil.crop((0, 0, pil.size[0], pil.size[1] - crop))
        half = pil.resize((pil.size[0] // 2, pil.size[1] // 2), PIL_Image.BILINEAR)
        out.update({f"demosaic_{p}": dem, f"undist_{p}": und, f"u8_{p}": u8, f"rect1_{p}": np.asarray(pil), f"rect2_{p}": np.asarray(half)})
    out["undist_u8"] = cm.undistort(img)
    out["undist_f32"] = cm.undistort((img / 3).astype(np.float32))
    return out


def main():
    CameraModel = load_camera_model(Path(sys.argv[1]))
    rng = np.random.default_rng(20261020)
    arrays = {}
    for i, (H, W, crop) in enumerate(SHAPES):
        cfa, lut = make_cfa(rng, H, W), make_lut(rng, H, W)
        img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        arrays.update({f"cfa{i}": cfa, f"lut{i}": lut, f"crop{i}": np.int64(crop), f"img{i}": img})
        for name, a in library_outputs(CameraModel, cfa, lut, crop, img).items():
            head, _, tail = name.partition("_")
            arrays[f"{head}{i}_{tail}" if tail in PATTERNS else f"{name}_{i}"] = a
    np.savez_compressed(OUT / "rectify_robotcar.npz", **arrays)
    print("rectify_robotcar.npz", (OUT / "rectify_robotcar.npz").stat().st_size, "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()

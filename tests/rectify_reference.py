"""numpy-only restatement of the RobotCar camera front end: bilinear Bayer demosaic, look-up-table
undistortion, the uint8 casts, the bottom crop and the factor-2 bilinear resize.  It imports neither scipy nor PIL, so the GPU tests can
use it where those libraries are absent; tests/test_rectify_reference.py pins every stage bit for bit against the libraries' own
outputs recorded in tests/golden/rectify_robotcar.npz (and against the libraries themselves where they are importable).

    demosaic_bilinear(cfa uint8 [H, W], pattern)          -> float64 [H, W, 3]   colour_demosaicing.demosaicing_CFA_Bayer_bilinear
    undistort_lut(image [H, W, C], bilinear_lut [H*W, 2]) -> image.dtype         CameraModel.undistort (map_coordinates, order=1)
    cast_u8(float64)                                      -> uint8               numpy's astype(np.uint8): truncate, keep the low 8 bits
    resize2_bilinear(uint8 [H, W, 3])                     -> uint8 [H/2, W/2, 3] PIL's Image.resize((W/2, H/2), BILINEAR)
    rectify_bayer(cfa, pattern, lut, crop_bottom, s)      -> uint8               oxford_robotcar.py:109-124,132-135
"""
from __future__ import annotations

import numpy as np

PATTERNS = ("RGGB", "GBRG", "GRBG", "BGGR")
# oxford_robotcar.py:111-124: (Bayer pattern, rows cropped at the bottom) of stereo/centre and of every other camera
ROBOTCAR_FRONT_END = {"stereo/centre": ("GBRG", 150)}
ROBOTCAR_DEFAULT = ("RGGB", 200)


def _reflect(i: np.ndarray, n: int) -> np.ndarray:
    """scipy.ndimage's ``reflect`` border (d c b a | a b c d) for indices in [-n, 2n)."""
    i = np.where(i < 0, -i - 1, i)
    return np.where(i >= n, 2 * n - 1 - i, i)


def demosaic_bilinear(cfa: np.ndarray, pattern: str) -> np.ndarray:
    """R, B = conv(CFA * mask, [[1,2,1],[2,4,2],[1,2,1]] / 4), G = conv(CFA * mask, [[0,1,0],[1,4,1],[0,1,0]] / 4) with the ``reflect``
    border; values stay on 0..255 (up to 573.75 on the outermost ring, where the border doubles a pixel of the same colour).  Sums of
    uint8 values are taken in integers and divided by 4 once: exact, so equal to any order of floating-point summation."""
    assert pattern in PATTERNS and cfa.dtype == np.uint8 and cfa.ndim == 2
    H, W = cfa.shape
    colour = np.empty((2, 2), np.int64)
    for ch, (y, x) in zip(pattern, [(0, 0), (0, 1), (1, 0), (1, 1)]):
        colour[y, x] = "RGB".index(ch)
    yy, xx = np.mgrid[0:H, 0:W]
    masked = np.zeros((3, H, W), np.int64)
    for ch in range(3):
        masked[ch] = np.where(colour[yy & 1, xx & 1] == ch, cfa.astype(np.int64), 0)
    k_rb = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]])
    k_g = np.array([[0, 1, 0], [1, 4, 1], [0, 1, 0]])
    out = np.zeros((H, W, 3), np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ry, rx = _reflect(yy + dy, H), _reflect(xx + dx, W)
            for ch, k in ((0, k_rb), (1, k_g), (2, k_rb)):
                out[:, :, ch] += k[dy + 1, dx + 1] * masked[ch][ry, rx]
    return out.astype(np.float64) / 4.0


def interp_lut(channel: np.ndarray, x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """map_coordinates(channel, (y, x), order=1) in fp64, before any cast of the output: 0 outside [0, H-1] x [0, W-1] (NaN and
    infinite coordinates included), else t = sum (v[a][b] * wr[a]) * wc[b] over (0,0), (0,1), (1,0), (1,1) with w0 = 1 - f,
    w1 = 1 - w0; a tap past the last row / column has weight 0 and reads the clamped pixel."""
    H, W = channel.shape
    ch = channel.astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
    ys, xs = np.where(inside, y, 0.0), np.where(inside, x, 0.0)
    r0, c0 = np.floor(ys), np.floor(xs)
    wr0 = 1.0 - (ys - r0)
    wc0 = 1.0 - (xs - c0)
    wr, wc = (wr0, 1.0 - wr0), (wc0, 1.0 - wc0)
    r0, c0 = r0.astype(np.int64), c0.astype(np.int64)
    t = np.zeros(ys.shape)
    for a in (0, 1):
        for b in (0, 1):
            v = ch[np.minimum(r0 + a, H - 1), np.minimum(c0 + b, W - 1)]
            t = t + (v * wr[a]) * wc[b]
    return np.where(inside, t, 0.0)


def undistort_lut(image: np.ndarray, bilinear_lut: np.ndarray) -> np.ndarray:
    """CameraModel.undistort: ``bilinear_lut`` [H*W, 2] fp64, column 0 = x, column 1 = y, row v*W + u for output pixel (v, u).
    Float images come back in their own dtype; uint8 images as scipy's integer output (t + 0.5 truncated, clamped to 0..255)."""
    H, W = image.shape[:2]
    if H * W != bilinear_lut.shape[0]:
        raise ValueError("Incorrect image size for camera model")
    x, y = bilinear_lut[:, 0].reshape(H, W), bilinear_lut[:, 1].reshape(H, W)
    t = np.stack([interp_lut(image[:, :, c], x, y) for c in range(image.shape[2])], -1)
    if image.dtype == np.uint8:
        return np.clip(np.trunc(t + 0.5), 0, 255).astype(np.uint8)
    return t.astype(image.dtype)


def cast_u8(t: np.ndarray) -> np.ndarray:
    """numpy's float64 -> uint8 ``astype`` for the non-negative finite values of this pipeline: truncate, keep the low 8 bits."""
    return (np.trunc(t).astype(np.int64) & 255).astype(np.uint8)


PIL_PRECISION_BITS = 32 - 8 - 2


def pil_bilinear_coeffs(n_in: int, n_out: int):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the triangle filter: per output index (first tap, integer weights)."""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    out = []
    for i in range(n_out):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        w = [max(0.0, 1.0 - abs((j - center + 0.5) / filterscale)) for j in range(lo, hi)]
        total = sum(w)
        out.append((lo, [int(0.5 + (v / total) * (1 << PIL_PRECISION_BITS)) for v in w]))
    return out


def _pil_pass(img: np.ndarray, n_out: int) -> np.ndarray:
    """One resampling pass along axis 1 of a uint8 [A, n_in, C] image: 32-bit accumulation from 1 << (bits - 1), shift, clip."""
    acc = np.full((img.shape[0], n_out, img.shape[2]), 1 << (PIL_PRECISION_BITS - 1), np.int64)
    for i, (lo, ks) in enumerate(pil_bilinear_coeffs(img.shape[1], n_out)):
        for j, k in enumerate(ks):
            acc[:, i] += img[:, lo + j].astype(np.int64) * k
    return np.clip(acc >> PIL_PRECISION_BITS, 0, 255).astype(np.uint8)


def resize2_bilinear(img: np.ndarray, factor: int = 2) -> np.ndarray:
    """PIL's Image.resize((W // factor, H // factor), BILINEAR) of a uint8 RGB image: the horizontal pass, a uint8 rounding, the
    vertical pass.  H and W divisible by the factor."""
    H, W = img.shape[:2]
    if H % factor or W % factor:
        raise ValueError("cropped image size must be divisible by the subsample factor")
    h = _pil_pass(img, W // factor)
    return np.ascontiguousarray(_pil_pass(np.ascontiguousarray(h.transpose(1, 0, 2)), H // factor).transpose(1, 0, 2))


def rectify_bayer(cfa: np.ndarray, pattern: str, bilinear_lut: np.ndarray, crop_bottom: int, subsample: int = 1) -> np.ndarray:
    """oxford_robotcar.py:109-124,132-135 for one camera: demosaic -> undistort (float) -> astype(uint8) -> crop -> resize."""
    img = cast_u8(undistort_lut(demosaic_bilinear(cfa, pattern), bilinear_lut))
    img = np.ascontiguousarray(img[:img.shape[0] - crop_bottom])
    return img if subsample == 1 else resize2_bilinear(img, subsample)

"""The RobotCar SDK's camera model (src/vfm-reg/src/dataloader/robotcar_sdk/python/camera_model.py) with the undistortion on the GPU.

    cm = CameraModel(focal_length, principal_point, G_camera_image, bilinear_lut)     # or CameraModel.from_files(models_dir, images_dir)
    rgb = cm.undistort(image)          # image [H, W, C] uint8 / float32 / float64, numpy in -> numpy out, device tensor in -> device tensor out

``bilinear_lut`` is the SDK's table [H*W, 2] fp64 (x, y): it goes to the device on first use and stays there.  An instance carries
``focal_length``, ``principal_point`` and ``G_camera_image``, which is all ``OxfordRobotcar(camera_model={...})`` reads of it.
The arithmetic of ``undistort`` is scipy's map_coordinates(order=1), bit for bit (csrc/camera.hip).
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import torch

from . import ops


def model_name(images_dir) -> str:
    """The SDK's file stem for an image directory: mono_left / mono_right / mono_rear, or for the stereo camera the sensor's model
    (left -> stereo_wide_left, right -> stereo_wide_right, centre -> stereo_narrow_left)."""
    camera = re.search(r"stereo|mono_left|mono_right|mono_rear", str(images_dir))
    if camera is None:
        raise RuntimeError(f"Unknown camera model for given directory: {images_dir}")
    if camera.group(0) != "stereo":
        return camera.group(0)
    sensor = re.search(r"left|centre|right", str(images_dir))
    if sensor is None:
        raise RuntimeError(f"Unknown camera model for given directory: {images_dir}")
    return {"left": "stereo_wide_left", "right": "stereo_wide_right", "centre": "stereo_narrow_left"}[sensor.group(0)]


class CameraModel:
    def __init__(self, focal_length, principal_point, G_camera_image, bilinear_lut):
        self.focal_length = (float(focal_length[0]), float(focal_length[1]))
        self.principal_point = (float(principal_point[0]), float(principal_point[1]))
        self.G_camera_image = np.asarray(G_camera_image, dtype=np.float64)
        if isinstance(bilinear_lut, torch.Tensor):
            self.bilinear_lut = bilinear_lut
            self._lut_d = bilinear_lut if bilinear_lut.is_cuda else None
        else:
            self.bilinear_lut = np.ascontiguousarray(bilinear_lut, dtype=np.float64)
            self._lut_d = None
        if self.bilinear_lut.ndim != 2 or self.bilinear_lut.shape[1] != 2:
            raise ValueError("bilinear_lut: expected [H*W, 2] (x, y)")

    @classmethod
    def from_files(cls, models_dir, images_dir) -> "CameraModel":
        """``<model>.txt``: a line fx fy cx cy, then the rows of G_camera_image; ``<model>_distortion_lut.bin``: fp64, all x then all y."""
        name = model_name(images_dir)
        lines = (Path(models_dir) / f"{name}.txt").read_text().splitlines()
        fx, fy, cx, cy = (float(v) for v in lines[0].split()[:4])
        G = np.array([[float(v) for v in line.split()] for line in lines[1:] if line.split()])
        lut = np.fromfile(Path(models_dir) / f"{name}_distortion_lut.bin", np.float64)
        return cls((fx, fy), (cx, cy), G, np.ascontiguousarray(lut.reshape(2, lut.size // 2).T))

    def lut_device(self) -> torch.Tensor:
        """The table on the device (uploaded once)."""
        if self._lut_d is None:
            lut = self.bilinear_lut if isinstance(self.bilinear_lut, torch.Tensor) else torch.from_numpy(self.bilinear_lut)
            self._lut_d = lut.to("cuda", torch.float64).contiguous()
        return self._lut_d

    def undistort(self, image):
        shape = tuple(image.shape)
        if len(shape) >= 2 and shape[0] * shape[1] != self.bilinear_lut.shape[0]:
            raise ValueError("Incorrect image size for camera model")
        if len(shape) != 3:
            raise ValueError("Undistortion function only works with multi-channel images")
        if isinstance(image, torch.Tensor):
            return ops.undistort_lut(image.contiguous(), self.lut_device())
        img = np.ascontiguousarray(image)
        if img.dtype not in (np.uint8, np.float32, np.float64):
            raise TypeError(f"image: expected uint8, float32 or float64, got {img.dtype}")
        return ops.undistort_lut(torch.from_numpy(img).cuda(), self.lut_device()).cpu().numpy()

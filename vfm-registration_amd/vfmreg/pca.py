"""Descriptor PCA: ``ImageFeatureGenerator.run_pca`` / ``get_image_features_pca`` (image_features.py:119-192) and FeatUp's ``pca``
behind them, on the kernels of csrc/pca.hip.

    fit = pca.fit(x, 3)                  # exact: mean and scatter on the GPU (fp64 matrix cores), one d x d eigh on the host
    y = pca.transform(x, fit)            # (x - mean) . components^T, fp64, in a fixed order of addition
    rgb = pca.colours(x, fit)            # (y - min) / (max - min) * 255 truncated, black for all-zero rows

Rows are float32 or float16 (anything else is cast to float32 first); numpy in gives numpy out, device tensors in give device tensors out.

Deviations from the reference: its fit is ``torch.pca_lowrank(niter=4)``, a randomised range finder whose results and signs change from
run to run; here the fit is exact and in every component the entry of largest magnitude (lowest index on a tie) is positive.  The
arithmetic is fp64 where the reference's is fp32: a value within fp32 rounding of an integer after ``* 255`` may truncate to the
neighbouring colour.  Eigenvalues that coincide leave their eigenvectors undefined, as they are in the reference.  A fit from elsewhere --
anything with ``mean_`` and ``components_``, e.g. the objects of the reference's own ``pca_fit.pkl`` -- can be handed in, and the
reference's colour constants (``utils.TREE_COLOURS``) keep their meaning under it.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Optional

import numpy as np
import torch

from . import ops


class PCAFit:
    """``mean_`` [d], ``components_`` [k, d], ``singular_values_`` [k] (fp64 numpy) and ``n_samples_``."""

    def __init__(self, mean_, components_, singular_values_=None, n_samples_=None):
        self.mean_ = np.ascontiguousarray(_to_numpy(mean_), dtype=np.float64).reshape(-1)
        self.components_ = np.ascontiguousarray(_to_numpy(components_), dtype=np.float64)
        if self.components_.ndim != 2 or self.components_.shape[1] != self.mean_.shape[0]:
            raise ValueError(f"components_ {self.components_.shape} do not match mean_ {self.mean_.shape}")
        self.singular_values_ = None if singular_values_ is None else np.ascontiguousarray(_to_numpy(singular_values_), dtype=np.float64)
        self.n_samples_ = None if n_samples_ is None else int(n_samples_)


def _to_numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def as_fit(obj) -> PCAFit:
    """A PCAFit from anything with ``mean_`` and ``components_`` (numpy arrays or torch tensors)."""
    if isinstance(obj, PCAFit):
        return obj
    if not (hasattr(obj, "mean_") and hasattr(obj, "components_")):
        raise TypeError("a fit needs the attributes mean_ and components_")
    return PCAFit(obj.mean_, obj.components_, getattr(obj, "singular_values_", None), getattr(obj, "n_samples_", None))


def _rows(x, device="cuda"):
    """(rows [N, C] on the device in float32 or float16, leading shape, came from the device)"""
    device_in = isinstance(x, torch.Tensor)
    if device_in:
        if not x.is_cuda:
            raise RuntimeError("x: a tensor must be on the ROCm device (no CPU path exists); numpy arrays are copied there")
        t = x
    else:
        a = np.asarray(x)
        if a.dtype not in (np.float32, np.float16):
            a = a.astype(np.float32)
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a if a.flags.writeable else a.copy()).to(device)      # (torch refuses to wrap read-only memory quietly)
    if t.dtype not in (torch.float32, torch.float16):
        t = t.to(torch.float32)
    if t.dim() < 2:
        raise ValueError(f"shape {tuple(t.shape)}: expected rows of features [..., C]")
    lead = tuple(t.shape[:-1])
    t = t.reshape(-1, t.shape[-1]).contiguous()
    if t.shape[0] < 1 or not 1 <= t.shape[1] <= ops.PCA_MAX_D:
        raise ValueError(f"{t.shape[0]} rows of {t.shape[1]} features: at least one row of 1..{ops.PCA_MAX_D} features is implemented")
    return t, lead, device_in


def sign_rule(components: np.ndarray) -> np.ndarray:
    """In every component the entry of largest magnitude, lowest index on a tie, is positive."""
    out = np.array(components, dtype=np.float64)
    for row in out:
        if row[int(np.argmax(np.abs(row)))] < 0:
            row *= -1.0
    return out


def fit_from_moments(mean: np.ndarray, scatter: np.ndarray, n_components: int, n_samples: int) -> PCAFit:
    """The host part of ``fit``: ``np.linalg.eigh`` of the d x d scatter in fp64, the top eigenvectors by descending eigenvalue, the sign
    rule, ``singular_values_ = sqrt(eigenvalue)``."""
    w, V = np.linalg.eigh(np.asarray(scatter, dtype=np.float64))
    order = np.argsort(-w, kind="stable")[:n_components]
    return PCAFit(mean, sign_rule(V[:, order].T), np.sqrt(np.maximum(w[order], 0.0)), n_samples)


def fit(x, n_components: int = 3) -> PCAFit:
    rows, _, _ = _rows(x)
    k = int(n_components)
    if not 1 <= k <= min(ops.PCA_MAX_K, rows.shape[1]):
        raise ValueError(f"n_components = {n_components}: 1..{min(ops.PCA_MAX_K, rows.shape[1])} are implemented")
    mean, scatter = ops.pca_moments(rows)
    return fit_from_moments(mean.cpu().numpy(), scatter.cpu().numpy(), k, rows.shape[0])


def _project(rows: torch.Tensor, f: PCAFit):
    if f.mean_.shape[0] != rows.shape[1]:
        raise ValueError(f"the fit is of {f.mean_.shape[0]} features, the rows have {rows.shape[1]}")
    mean = torch.from_numpy(f.mean_).to(rows.device)
    comps = torch.from_numpy(f.components_).to(rows.device)
    return ops.pca_project(rows, mean, comps)


def _out(t: torch.Tensor, lead, device_in: bool):
    t = t.reshape(lead + (t.shape[-1],))
    return t if device_in else t.cpu().numpy()


def transform(x, fit_) -> "np.ndarray | torch.Tensor":
    """``(x - mean_) @ components_.T`` in fp64 [..., k]."""
    rows, lead, device_in = _rows(x)
    y, _, _, _ = _project(rows, as_fit(fit_))
    return _out(y, lead, device_in)


def normalised(x, fit_) -> "np.ndarray | torch.Tensor":
    """FeatUp's ``pca``: the transform, then per component over all rows ``Y -= Y.min(0); Y /= Y.max(0)``; float32 [..., k]."""
    rows, lead, device_in = _rows(x)
    y, _, lo, hi = _project(rows, as_fit(fit_))
    return _out(ops.pca_colours(y, None, lo, hi, rgb=False), lead, device_in)


def colours(x, fit_) -> "np.ndarray | torch.Tensor":
    """image_features.py:184-190 for a fit of three components: ``(normalised * 255.0).astype(uint8)``, black where every feature is 0."""
    rows, lead, device_in = _rows(x)
    f = as_fit(fit_)
    if f.components_.shape[0] != 3:
        raise ValueError(f"colours need a fit of 3 components, this one has {f.components_.shape[0]}")
    y, zero, lo, hi = _project(rows, f)
    return _out(ops.pca_colours(y, zero, lo, hi, rgb=True), lead, device_in)


class DescriptorPCA:
    """The ``fit_pca`` dict of image_features.py and ``run_pca`` on it.  ``fit_pca[n_components]`` may hold anything with ``mean_`` and
    ``components_``.  ``fit_pca_file`` (default None: nothing is read or written): an ``.npz`` the fits are loaded from when it exists
    and stored to whenever one is added."""

    def __init__(self, fit_pca_file=None):
        self.fit_pca: Dict[int, object] = {}
        self.fit_pca_file: Optional[Path] = None if fit_pca_file is None else Path(fit_pca_file)
        self.fits_computed = 0          # how many times run_pca / fit_once had to fit
        if self.fit_pca_file is not None and self.fit_pca_file.exists():
            self.load(self.fit_pca_file)

    def load(self, path) -> None:
        with np.load(path) as z:
            for k in sorted({int(name.split("_", 1)[0]) for name in z.files}):
                sv, ns = z[f"{k}_singular_values"], int(z[f"{k}_n_samples"])
                self.fit_pca[k] = PCAFit(z[f"{k}_mean"], z[f"{k}_components"], sv if sv.size else None, ns if ns >= 0 else None)

    def save(self, path) -> None:
        data = {}
        for k, f in self.fit_pca.items():
            if f is None:
                continue
            f = as_fit(f)
            data[f"{k}_mean"], data[f"{k}_components"] = f.mean_, f.components_
            data[f"{k}_singular_values"] = np.zeros(0) if f.singular_values_ is None else f.singular_values_
            data[f"{k}_n_samples"] = np.int64(-1 if f.n_samples_ is None else f.n_samples_)
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        with open(path, "wb") as fh:
            np.savez(fh, **data)

    def fit_once(self, x, n_components: int):
        """The fit ``pca([x], dim, fit_pca=self.fit_pca.get(dim))`` uses (a new one when that is None), stored as image_features.py
        stores it: only when the dict has no entry for ``n_components`` -- after ``refit_pca`` the entry is None and stays None, so
        every later call fits again (IF:170-178)."""
        f = self.fit_pca.get(n_components, None)
        if f is None:
            f = fit(x, n_components)
            self.fits_computed += 1
        if n_components not in self.fit_pca:
            self.fit_pca[n_components] = f
            if self.fit_pca_file is not None:
                self.save(self.fit_pca_file)
        return as_fit(f)

    def run_pca(self, features, refit_pca: bool = False, n_components: int = 3):
        """image_features.py:162-192: uint8 RGB [..., 3] for three components, float32 [..., n_components] otherwise."""
        if refit_pca:
            self.fit_pca[n_components] = None
        f = self.fit_once(features, n_components)
        return colours(features, f) if n_components == 3 else normalised(features, f)

"""Tensor-level wrappers over the C ABI (include/vfmreg.h).

Inputs and outputs are torch tensors resident on a ROCm device; PyTorch is used only for device
memory and the current HIP stream.  Nothing here synchronises the device.  There is no CPU
implementation: every function raises if the tensors are not on a GPU.
"""
from __future__ import annotations

import math
import threading
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

FAST = 0
EXACT = 1
NARROW = 2          # match_mutual_l2 only: rows of at most NARROW_MAX_D columns on the f32 MFMA (VFM_MATCH_NARROW)
NARROW_MAX_D = 64

PROJ_NCLT, PROJ_ROBOTCAR, PROJ_KITTI = 0, 1, 2


_tls = threading.local()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _chk(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the ROCm device (no CPU path exists)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------- matching
def l2norm_rows_(x: torch.Tensor, inv_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In-place faiss::fvec_renorm_L2 per row (VoxelHashMap.cpp:474,480)."""
    _chk(x, torch.float32, "x")
    lib = _lib.load()
    _lib.check(lib.vfm_l2norm_rows_f32(x.data_ptr(), x.shape[0], x.shape[1], _ptr(inv_out), _stream()), "l2norm")
    return x


def match_ip_top1(q: torch.Tensor, b: torch.Tensor, prec: int = FAST,
                  ws: Optional[torch.Tensor] = None, gate: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Normalise + IndexFlatIP top-1 (VoxelHashMap.cpp:469-495). Returns (idx int64[N], sim fp32[N]).
    ``gate`` (the gated family of include/vfmreg.h): for a caller that keeps only matches with similarity >= gate
    (VoxelHashMap.cpp:501-511) -- queries that provably cannot reach it come back as (-1, -2.0); ``-inf`` resolves all."""
    _chk(q, torch.float32, "q")
    _chk(b, torch.float32, "b")
    if q.dim() != 2 or b.dim() != 2 or q.shape[1] != b.shape[1]:
        raise ValueError("Invalid shape")
    lib = _lib.load()
    n, d = q.shape
    m = b.shape[0]
    need = lib.vfm_match_ip_top1_workspace_bytes(n, m, d, prec)
    if ws is None or ws.numel() < need:
        ws = _ws(need, q.device)
    idx = torch.empty(n, dtype=torch.int64, device=q.device)
    sim = torch.empty(n, dtype=torch.float32, device=q.device)
    if gate is None:
        _lib.check(lib.vfm_match_ip_top1(q.data_ptr(), n, b.data_ptr(), m, d, prec, idx.data_ptr(), sim.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _stream()), "match_ip_top1")
    else:
        _lib.check(lib.vfm_match_ip_top1_gated(q.data_ptr(), n, b.data_ptr(), m, d, prec, float(gate), idx.data_ptr(),
                                               sim.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "match_ip_top1")
    return idx, sim


MATCH_TOPK_MAX_K = 8            # VFM_MATCH_TOPK_MAX
MATCH_TOPK_RECORD_CAP = 1024    # records a query can hold in FAST mode before the all-pairs kernel decides it (csrc/match_topk.hip)


def match_ip_topk(q: torch.Tensor, b: torch.Tensor, k: int, prec: int = FAST, ws: Optional[torch.Tensor] = None,
                  return_info: bool = False):
    """Normalise + IndexFlatIP.search(n, x, k, D, I) (the k-candidate loop of VoxelHashMap.cpp:491-511).  Returns
    (idx int64[N, k], sim fp32[N, k]): per query the k best map rows by fp64 score, descending, equal scores to the lower index;
    with fewer than k map rows the last columns are (-1, lowest finite float32).  Column 0 is ``match_ip_top1``'s answer.  No gate:
    apply ``~(sim < thr)`` to the result.  ``return_info``: also int32[4] on the device -- largest record count of a query, queries
    decided by the all-pairs kernel, map slices of the coarse pass, 0 (a call that ran EXACT: 0, N, 0, 0)."""
    _chk(q, torch.float32, "q")
    _chk(b, torch.float32, "b")
    if q.dim() != 2 or b.dim() != 2 or q.shape[1] != b.shape[1]:
        raise ValueError("Invalid shape")
    k = int(k)
    if not 1 <= k <= MATCH_TOPK_MAX_K:
        raise ValueError(f"k must be in 1 .. {MATCH_TOPK_MAX_K}, got {k}")
    lib = _lib.load()
    n, d = q.shape
    m = b.shape[0]
    need = lib.vfm_match_ip_topk_workspace_bytes(n, m, d, k, prec)
    if ws is None or ws.numel() < need:
        ws = _ws(need, q.device)
    idx = torch.empty((n, k), dtype=torch.int64, device=q.device)
    sim = torch.empty((n, k), dtype=torch.float32, device=q.device)
    info = torch.zeros(4, dtype=torch.int32, device=q.device) if return_info else None
    if n > 0:   # (no queries: nothing to write, and an empty tensor has no address to pass)
        _lib.check(lib.vfm_match_ip_topk(q.data_ptr(), n, b.data_ptr(), m, d, k, prec, idx.data_ptr(), sim.data_ptr(), _ptr(info),
                                         ws.data_ptr(), ws.numel(), _stream()), "match_ip_topk")
    return (idx, sim, info) if return_info else (idx, sim)


class PreparedRows:
    """IndexFlatIP.add (VoxelHashMap.cpp:486-487): 1/|row| + fp16 fragment tiles of the rows."""

    def __init__(self, x: torch.Tensor):
        _chk(x, torch.float32, "x")
        lib = _lib.load()
        self.x = x
        self.rows, self.d = x.shape
        self.buf = _ws(lib.vfm_match_prepared_bytes(self.rows, self.d), x.device)
        self.refresh()

    def refresh(self) -> None:
        lib = _lib.load()
        _lib.check(lib.vfm_match_prepare(self.x.data_ptr(), self.rows, self.d, self.buf.data_ptr(), _stream()),
                   "match_prepare")


MATCH_TOPK_FAST_WIDTHS = (128, 256, 384, 640, 768)   # row widths the k-best search has a matrix-core kernel for


def match_ip_topk_prepared(q: PreparedRows, b: PreparedRows, k: int, ws: Optional[torch.Tensor] = None, return_info: bool = False):
    """``match_ip_topk(q.x, b.x, k, FAST)`` on operands prepared beforehand (vfm_match_ip_topk_prepared) -- for a map that is
    prepared once and searched by many scans.  The same (idx, sim[, info]), bit for bit; both operands are left as they were.  A width
    outside ``MATCH_TOPK_FAST_WIDTHS`` is refused: a prepared image means nothing to the all-pairs kernel."""
    if q.d != b.d or q.d not in MATCH_TOPK_FAST_WIDTHS:
        raise ValueError("Invalid shape")
    k = int(k)
    if not 1 <= k <= MATCH_TOPK_MAX_K:
        raise ValueError(f"k must be in 1 .. {MATCH_TOPK_MAX_K}, got {k}")
    lib = _lib.load()
    dev = q.x.device
    n = q.rows
    need = lib.vfm_match_ip_topk_prepared_workspace_bytes(n, q.d, k)
    if ws is None or ws.numel() < need:
        ws = _ws(need, dev)
    idx = torch.empty((n, k), dtype=torch.int64, device=dev)
    sim = torch.empty((n, k), dtype=torch.float32, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev) if return_info else None
    if n > 0:
        _lib.check(lib.vfm_match_ip_topk_prepared(q.x.data_ptr(), q.buf.data_ptr(), n, b.x.data_ptr(), b.buf.data_ptr(), b.rows, q.d, k,
                                                  idx.data_ptr(), sim.data_ptr(), _ptr(info), ws.data_ptr(), ws.numel(), _stream()),
                   "match_ip_topk_prepared")
    return (idx, sim, info) if return_info else (idx, sim)


def match_search(q: PreparedRows, b: PreparedRows, idx: Optional[torch.Tensor] = None,
                 sim: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None):
    lib = _lib.load()
    if q.d != b.d:
        raise ValueError("Invalid shape")
    need = lib.vfm_match_search_workspace_bytes(q.rows, b.rows, q.d)
    if ws is None or ws.numel() < need:
        ws = _ws(need, q.x.device)
    if idx is None:
        idx = torch.empty(q.rows, dtype=torch.int64, device=q.x.device)
    if sim is None:
        sim = torch.empty(q.rows, dtype=torch.float32, device=q.x.device)
    _lib.check(lib.vfm_match_search_prepared(q.x.data_ptr(), q.buf.data_ptr(), q.rows, b.x.data_ptr(),
                                             b.buf.data_ptr(), b.rows, q.d, idx.data_ptr(), sim.data_ptr(),
                                             ws.data_ptr(), ws.numel(), _stream()), "match_search")
    return idx, sim


def gated_split_ok(d: int) -> bool:
    """Widths for which the gated family's split calls exist (the int8 coarse pass: d = 256 ... 768 in steps of 128)."""
    return d % 128 == 0 and 256 <= d <= 768


def match_search_gated(q: PreparedRows, b: PreparedRows, gate: float, idx: Optional[torch.Tensor] = None,
                       sim: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None, records: Optional[int] = None,
                       rescans_out: Optional[torch.Tensor] = None):
    """vfm_match_search_coarse_gated + vfm_match_search_finish_gated on prepared operands: what vfm_match_ip_top1_gated does after
    preparing both -- for a map that is prepared once and searched by many scans.  Same answers (idx -1 / sim -2.0 for queries that
    provably cannot reach ``gate``).  ``records``: the record kind of the coarse pass (include/vfmreg.h VFM_RECORDS_*; None = the
    default, best-score records); ``rescans_out``: a pinned 1-element int32 tensor that receives the search's load figure
    (vfm_match_search_rescans_async: candidate chunks rescanned) once the stream has passed this call."""
    lib = _lib.load()
    if q.d != b.d or not gated_split_ok(q.d):
        raise ValueError("Invalid shape")
    dev = q.x.device
    need = lib.vfm_match_search_workspace_bytes(q.rows, b.rows, q.d)
    if ws is None or ws.numel() < need:
        ws = _ws(need, dev)
    if idx is None:
        idx = torch.empty(q.rows, dtype=torch.int64, device=dev)
    if sim is None:
        sim = torch.empty(q.rows, dtype=torch.float32, device=dev)
    st = _stream()
    if records is None:
        _lib.check(lib.vfm_match_search_coarse_gated(q.buf.data_ptr(), q.rows, b.buf.data_ptr(), b.rows, q.d, ws.data_ptr(), ws.numel(), st),
                   "search(coarse)")
        _lib.check(lib.vfm_match_search_finish_gated(q.x.data_ptr(), q.buf.data_ptr(), q.rows, b.x.data_ptr(), b.buf.data_ptr(), b.rows, q.d,
                                                     idx.data_ptr(), sim.data_ptr(), ws.data_ptr(), ws.numel(), float(gate), st), "search(finish)")
    else:
        _lib.check(lib.vfm_match_search_coarse_gated_g(q.buf.data_ptr(), q.rows, b.buf.data_ptr(), b.rows, q.d, ws.data_ptr(), ws.numel(),
                                                       int(records), float(gate), st), "search(coarse)")
        _lib.check(lib.vfm_match_search_finish_gated_r(q.x.data_ptr(), q.buf.data_ptr(), q.rows, b.x.data_ptr(), b.buf.data_ptr(), b.rows, q.d,
                                                       idx.data_ptr(), sim.data_ptr(), ws.data_ptr(), ws.numel(), float(gate), int(records), st),
                   "search(finish)")
    if rescans_out is not None:
        _lib.check(lib.vfm_match_search_rescans_async(ws.data_ptr(), q.rows, b.rows, rescans_out.data_ptr(), st), "rescans")
    return idx, sim


def match_probe_half(q: PreparedRows, b: PreparedRows, gate: float, out: torch.Tensor, ws: Optional[torch.Tensor] = None) -> None:
    """vfm_match_search_probe_half: the (query, chunk) pairs the half-width coarse pass would leave for this pair, to the pinned
    1-element int32 tensor ``out`` (asynchronously on the current stream)."""
    lib = _lib.load()
    need = lib.vfm_match_search_workspace_bytes(q.rows, b.rows, q.d)
    if ws is None or ws.numel() < need:
        ws = _ws(need, q.x.device)
    _lib.check(lib.vfm_match_search_probe_half(q.buf.data_ptr(), q.rows, b.buf.data_ptr(), b.rows, q.d, ws.data_ptr(), ws.numel(),
                                               float(gate), out.data_ptr(), _stream()), "probe_half")


def threshold_compact(sim: torch.Tensor, idx: Optional[torch.Tensor], thr: float,
                      q_xyz: Optional[torch.Tensor] = None, b_xyz: Optional[torch.Tensor] = None,
                      want_corres: bool = True):
    """VoxelHashMap.cpp:501-511 + 587-600. Returns dict(keep, count, corres, src, tgt); `count` is a
    1-element int64 device tensor (no host sync); the arrays are sized N, valid up to count."""
    _chk(sim, torch.float32, "sim")
    n = sim.shape[0]
    dev = sim.device
    lib = _lib.load()
    keep = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    corres = torch.empty((n, 2), dtype=torch.int32, device=dev) if (want_corres and idx is not None) else None
    src = torch.empty((n, 3), dtype=torch.float64, device=dev) if q_xyz is not None else None
    tgt = torch.empty((n, 3), dtype=torch.float64, device=dev) if (b_xyz is not None and idx is not None) else None
    if idx is not None:
        _chk(idx, torch.int64, "idx")
    if q_xyz is not None:
        _chk(q_xyz, torch.float64, "q_xyz")
    if b_xyz is not None:
        _chk(b_xyz, torch.float64, "b_xyz")
    _lib.check(lib.vfm_threshold_compact(sim.data_ptr(), _ptr(idx), n, float(thr), keep.data_ptr(), count.data_ptr(),
                                         _ptr(corres), _ptr(q_xyz), _ptr(b_xyz), _ptr(src), _ptr(tgt), _stream()),
               "threshold_compact")
    return dict(keep=keep, count=count, corres=corres, src=src, tgt=tgt)


def match_mutual_l2(a: torch.Tensor, b: torch.Tensor, mutual: bool = True, prec: int = FAST):
    """Exact Euclidean 1-NN a->b (and b->a) (registration_node.py:485-496).  FAST, EXACT and NARROW return the same
    indices and distances; FAST runs the all-pairs part on the fp16 matrix cores, NARROW (rows of at most 64 columns)
    on the f32 ones with the exact decision inline."""
    _chk(a, torch.float32, "a")
    _chk(b, torch.float32, "b")
    if a.shape[1] != b.shape[1]:
        raise ValueError("Invalid shape")
    if prec == NARROW and a.shape[1] > NARROW_MAX_D:
        raise ValueError(f"match_mutual_l2: NARROW serves rows of at most {NARROW_MAX_D} columns, got {a.shape[1]}")
    lib = _lib.load()
    n, m, d = a.shape[0], b.shape[0], a.shape[1]
    nn_ab = torch.empty(n, dtype=torch.int64, device=a.device)
    d2 = torch.empty(n, dtype=torch.float64, device=a.device)
    nn_ba = torch.empty(m, dtype=torch.int64, device=a.device) if mutual else None
    ws = torch.empty(lib.vfm_match_mutual_l2_workspace_bytes(n, m, d, prec, int(mutual)), dtype=torch.uint8, device=a.device)
    _lib.check(lib.vfm_match_mutual_l2(a.data_ptr(), n, b.data_ptr(), m, d, prec, nn_ab.data_ptr(), d2.data_ptr(),
                                       _ptr(nn_ba), ws.data_ptr(), ws.numel(), _stream()), "match_mutual_l2")
    return nn_ab, d2, nn_ba


def match_mutual_pairs(a: torch.Tensor, b: torch.Tensor, want_nn: bool = False):
    """find_correspondences(mutual_filter=True) in one call (registration_node.py:482-538): (idx0, idx1, count[, nn_ab, d2_ab]);
    idx0 / idx1 hold ``count`` valid pairs in ascending idx0 (device tensors, count is a 1-element int64 tensor: no host sync)."""
    _chk(a, torch.float32, "a")
    _chk(b, torch.float32, "b")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("Invalid shape")
    lib = _lib.load()
    n, m, d = a.shape[0], b.shape[0], a.shape[1]
    dev = a.device
    idx0 = torch.empty(n, dtype=torch.int64, device=dev)
    idx1 = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    nn_ab = torch.empty(n, dtype=torch.int64, device=dev) if want_nn else None
    d2 = torch.empty(n, dtype=torch.float64, device=dev) if want_nn else None
    ws = _ws(lib.vfm_match_mutual_pairs_workspace_bytes(n, m, d), dev)
    _lib.check(lib.vfm_match_mutual_pairs(a.data_ptr(), n, b.data_ptr(), m, d, idx0.data_ptr(), idx1.data_ptr(), count.data_ptr(),
                                          _ptr(nn_ab), _ptr(d2), ws.data_ptr(), ws.numel(), _stream()), "match_mutual_pairs")
    return (idx0, idx1, count, nn_ab, d2) if want_nn else (idx0, idx1, count)


# --------------------------------------------------------------------------------------- RANSAC
def ransac_corr(src: torch.Tensor, tgt: torch.Tensor, corres: torch.Tensor, max_dist: float, n_iter: int,
                seed: int = 42, count: Optional[torch.Tensor] = None, want_mask: bool = True,
                ws: Optional[torch.Tensor] = None, out: Optional[dict] = None, check_bounds: bool = False):
    """registration_ransac_based_on_correspondence (registration_node.py:319-327).  `count`
    (1-element int64 device tensor) gives the number of valid rows of `corres` without a host sync.  ``check_bounds``: the kernel that
    gathers the point pairs tests every index against the clouds' lengths (vfm_ransac_corr_bounded); ``out["bad"]`` (int32[1]) is 1
    if one was out of range -- such an entry is read as row 0 and the caller discards the result."""
    _chk(src, torch.float64, "src")
    _chk(tgt, torch.float64, "tgt")
    _chk(corres, torch.int32, "corres")
    lib = _lib.load()
    dev = src.device
    c_max = corres.shape[0]
    need = lib.vfm_ransac_workspace_bytes(c_max, n_iter)
    if ws is None or ws.numel() < need:
        ws = _ws(need, dev)
    if out is None:
        out = dict(T=torch.empty((4, 4), dtype=torch.float64, device=dev),
                   fitness=torch.empty(1, dtype=torch.float64, device=dev),
                   rmse=torch.empty(1, dtype=torch.float64, device=dev),
                   best_hyp=torch.empty(1, dtype=torch.int32, device=dev),
                   mask=torch.empty(max(c_max, 1), dtype=torch.uint8, device=dev) if want_mask else None)
    if count is not None:
        _chk(count, torch.int64, "count")
    if check_bounds:
        out["bad"] = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.vfm_ransac_corr_bounded(src.data_ptr(), src.shape[0], tgt.data_ptr(), tgt.shape[0], corres.data_ptr(), _ptr(count), c_max,
                                               float(max_dist), int(n_iter), int(seed) & 0xFFFFFFFFFFFFFFFF, out["T"].data_ptr(),
                                               out["fitness"].data_ptr(), out["rmse"].data_ptr(), _ptr(out.get("mask")),
                                               out["best_hyp"].data_ptr(), out["bad"].data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
                   "ransac_corr")
        return out
    _lib.check(lib.vfm_ransac_corr(src.data_ptr(), tgt.data_ptr(), corres.data_ptr(), _ptr(count), c_max,
                                   float(max_dist), int(n_iter), int(seed) & 0xFFFFFFFFFFFFFFFF, out["T"].data_ptr(),
                                   out["fitness"].data_ptr(), out["rmse"].data_ptr(), _ptr(out.get("mask")),
                                   out["best_hyp"].data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "ransac_corr")
    return out


def kabsch_batched(A: torch.Tensor, B: torch.Tensor, w: Optional[torch.Tensor] = None, denom_eps: float = 0.0):
    """Eigen::umeyama (no scaling) / pointdsc rigid_transform_3d, batched: A, B [b, n, 3] fp64."""
    _chk(A, torch.float64, "A")
    _chk(B, torch.float64, "B")
    if w is not None:
        _chk(w, torch.float64, "w")
    lib = _lib.load()
    b, n, _ = A.shape
    T = torch.empty((b, 4, 4), dtype=torch.float64, device=A.device)
    valid = torch.empty(b, dtype=torch.int32, device=A.device)
    _lib.check(lib.vfm_kabsch_batched(A.data_ptr(), B.data_ptr(), _ptr(w), b, n, float(denom_eps), T.data_ptr(),
                                      valid.data_ptr(), _stream()), "kabsch_batched")
    return T, valid


# ----------------------------------------------------------------------------------- projection
def project_pinhole(mode: int, pcl4xn: torch.Tensor, mats, fc=None, subsample: float = 1.0, win=None,
                    image: Optional[torch.Tensor] = None, H: int = 0, W: int = 0):
    """Dataset.project_pcl_to_image. pcl4xn: [4, N] fp64 device tensor. mats: up to three host
    matrices (see include/vfmreg.h). Returns (u int32[N], v int32[N], idx int64[N], count int64[1])."""
    import ctypes as C
    _chk(pcl4xn, torch.float64, "pcl")
    if pcl4xn.dim() != 2 or pcl4xn.shape[0] != 4:
        raise ValueError("Invalid shape")
    lib = _lib.load()
    n = pcl4xn.shape[1]
    dev = pcl4xn.device
    flat = [0.0] * 48
    for k, m in enumerate(list(mats)[:3]):
        vals = [float(x) for x in (m.reshape(-1).tolist() if hasattr(m, "reshape") else m)]
        flat[16 * k:16 * k + len(vals)] = vals
    mats_c = (C.c_double * 48)(*flat)
    fc_c = (C.c_double * 4)(*([float(x) for x in fc] if fc is not None else [0.0] * 4))
    win_c = (C.c_int64 * 4)(*([int(x) for x in win] if win is not None else [0] * 4))
    if image is not None:
        _chk(image, torch.uint8, "image")
        H, W = image.shape[0], image.shape[1]
    u = torch.empty(n, dtype=torch.int32, device=dev)
    v = torch.empty(n, dtype=torch.int32, device=dev)
    idx = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = _ws(lib.vfm_project_workspace_bytes(n), dev)
    _lib.check(lib.vfm_project_pinhole_f64(mode, pcl4xn.data_ptr(), n, C.cast(mats_c, C.c_void_p),
                                           C.cast(fc_c, C.c_void_p), float(subsample), C.cast(win_c, C.c_void_p),
                                           _ptr(image), int(H), int(W), u.data_ptr(), v.data_ptr(), idx.data_ptr(),
                                           count.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "project")
    return u, v, idx, count


LIFT_MAX_CAMS = 6


class LiftPlan:
    """The camera records of ``lift_multicam`` marshalled once (mode, matrices, image / grid pointers): a caller that lifts
    scan after scan with the same rig -- prepare_scenes.py:50-107 walks a sequence -- pays the Python-side packing once, and a
    call is one kernel launch.  The tensors named in ``cams`` are kept alive by the plan; their CONTENTS may change between
    calls (new images, new patch grids in the same buffers)."""

    def __init__(self, cams: list, C: int):
        if not 1 <= len(cams) <= LIFT_MAX_CAMS:
            raise ValueError("Invalid shape")
        self.C = int(C)
        self.arr = (_lib.LiftCamera * len(cams))()
        self.keep = []
        for k, c in enumerate(cams):
            g = c["grid"]
            _chk(g, torch.float32, "grid")
            if g.shape[-1] != self.C:
                raise ValueError("Invalid shape")
            a = self.arr[k]
            a.mode = int(c["mode"])
            flat = [0.0] * 48
            for j, m in enumerate(list(c["mats"])[:3]):
                vals = [float(x) for x in (m.reshape(-1).tolist() if hasattr(m, "reshape") else m)]
                flat[16 * j:16 * j + len(vals)] = vals
            a.mats[:] = flat
            a.fc[:] = [float(x) for x in c["fc"]] if c.get("fc") is not None else [0.0] * 4
            a.subsample = float(c.get("subsample", 1.0))
            a.win[:] = [int(x) for x in c["win"]] if c.get("win") is not None else [0] * 4
            a.H, a.W = int(c["H"]), int(c["W"])
            for name in ("proj_image", "raw_image"):
                t = c.get(name)
                if t is not None:
                    _chk(t, torch.uint8, name)
                    self.keep.append(t)
                setattr(a, name, _ptr(t))
            self.keep.append(g)
            a.grid = g.data_ptr()
            a.gh, a.gw = int(g.shape[0]), int(g.shape[1])
            a.Hup, a.Wup, a.rot_mode = int(c["Hup"]), int(c["Wup"]), int(c.get("rot_mode", 0))
        import ctypes as C_
        self._ptr = C_.cast(self.arr, C_.c_void_p)
        self._lib = _lib.load()

    def __call__(self, pcl4xn: torch.Tensor, desc: torch.Tensor, filled: torch.Tensor) -> None:
        _chk(pcl4xn, torch.float64, "pcl")
        _chk(desc, torch.float32, "desc")
        _chk(filled, torch.uint8, "filled")
        if pcl4xn.dim() != 2 or pcl4xn.shape[0] != 4 or desc.shape[1] != self.C:
            raise ValueError("Invalid shape")
        _lib.check(self._lib.vfm_lift_multicam(pcl4xn.data_ptr(), pcl4xn.shape[1], len(self.arr), self._ptr, self.C,
                                               desc.data_ptr(), filled.data_ptr(), _stream()), "lift_multicam")


def lift_multicam(pcl4xn: torch.Tensor, cams: list, desc: torch.Tensor, filled: torch.Tensor) -> None:
    """create_descriptors (prepare_scenes.py:50-107) for all cameras in one launch.  ``cams``: list (priority
    order) of dicts with the projection parameters of ``project_pinhole`` (mode, mats, fc, subsample, win, H, W,
    proj_image) and of ``gather_bilinear`` (grid [gh, gw, C], Hup, Wup, rot_mode, raw_image).  Every row of ``desc`` is
    written (zeros for points no camera sees / black pixels); ``filled`` receives 1 for every point some camera saw."""
    LiftPlan(cams, desc.shape[1])(pcl4xn, desc, filled)


def gather_bilinear(grid: torch.Tensor, Hup: int, Wup: int, rot_mode: int, image: Optional[torch.Tensor],
                    u: torch.Tensor, v: torch.Tensor, idx: torch.Tensor, count: Optional[torch.Tensor],
                    desc: torch.Tensor, filled: torch.Tensor) -> None:
    """One camera of create_descriptors (prepare_scenes.py:57-104) fused with the bilinear upsample
    of image_features.py:104-108; call per camera in priority order."""
    _chk(grid, torch.float32, "grid")
    _chk(u, torch.int32, "u")
    _chk(v, torch.int32, "v")
    _chk(idx, torch.int64, "idx")
    _chk(desc, torch.float32, "desc")
    _chk(filled, torch.uint8, "filled")
    if image is not None:
        _chk(image, torch.uint8, "image")
    gh, gw, Cc = grid.shape
    lib = _lib.load()
    _lib.check(lib.vfm_gather_bilinear_patchgrid(grid.data_ptr(), gh, gw, Cc, int(Hup), int(Wup), int(rot_mode),
                                                 _ptr(image), u.data_ptr(), v.data_ptr(), idx.data_ptr(), _ptr(count),
                                                 u.shape[0], desc.data_ptr(), filled.data_ptr(), _stream()), "gather")


# ----------------------------------------------------------------------------- camera front end
BAYER_PATTERNS = {"RGGB": 0, "GBRG": 1, "GRBG": 2, "BGGR": 3}   # VFM_BAYER_*
RECTIFY_MAX_CAMS = 8                                            # VFM_RECTIFY_MAX_CAMS
_IMAGE_DTYPES = {torch.uint8: 0, torch.float32: 1, torch.float64: 2}   # VFM_IMAGE_*


def _bayer(pattern: str) -> int:
    if pattern not in BAYER_PATTERNS:
        raise ValueError(f"pattern: expected one of {sorted(BAYER_PATTERNS)}, got {pattern!r}")
    return BAYER_PATTERNS[pattern]


def _lut_rows(lut: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Shapes are judged before residence: a table of the wrong length is the reference's ValueError wherever the tensors live."""
    if getattr(lut, "ndim", 0) != 2 or lut.shape[1] != 2 or lut.shape[0] != H * W:
        raise ValueError("Incorrect image size for camera model")   # camera_model.py:103-104
    return lut


def demosaic_bilinear(cfa: torch.Tensor, pattern: str = "RGGB") -> torch.Tensor:
    """colour_demosaicing.demosaicing_CFA_Bayer_bilinear: uint8 mosaic [H, W] -> float32 [H, W, 3] on 0..255 (border ``reflect``)."""
    code = _bayer(pattern)
    if getattr(cfa, "ndim", 0) != 2:
        raise ValueError("cfa: expected a 2-D mosaic")
    _chk(cfa, torch.uint8, "cfa")
    out = torch.empty(cfa.shape + (3,), dtype=torch.float32, device=cfa.device)
    _lib.check(_lib.load().vfm_demosaic_bilinear(cfa.data_ptr(), cfa.shape[0], cfa.shape[1], code, out.data_ptr(), _stream()),
               "demosaic_bilinear")
    return out


def undistort_lut(image: torch.Tensor, bilinear_lut: torch.Tensor) -> torch.Tensor:
    """CameraModel.undistort (robotcar_sdk camera_model.py:89-117): image [H, W, C] uint8 / float32 / float64, ``bilinear_lut``
    [H*W, 2] fp64 in the SDK's layout (x, y); the result has the image's dtype, as scipy's map_coordinates(order=1) gives it."""
    if not isinstance(image, torch.Tensor) or image.dtype not in _IMAGE_DTYPES:
        raise TypeError(f"image: expected a uint8, float32 or float64 tensor, got {getattr(image, 'dtype', type(image))}")
    if image.dim() != 3:
        raise ValueError("Undistortion function only works with multi-channel images")   # camera_model.py:108-109
    H, W, Cc = image.shape
    _lut_rows(bilinear_lut, H, W)
    _chk(image, image.dtype, "image")
    _chk(bilinear_lut, torch.float64, "bilinear_lut")
    out = torch.empty_like(image)
    _lib.check(_lib.load().vfm_undistort_lut(image.data_ptr(), _IMAGE_DTYPES[image.dtype], H, W, Cc, bilinear_lut.data_ptr(),
                                             out.data_ptr(), _stream()), "undistort_lut")
    return out


def rectify_bayer(cams: list, ws: Optional[torch.Tensor] = None) -> list:
    """oxford_robotcar.py:109-124,132-135 for a whole rig in one call.  ``cams``: dicts with ``mosaic`` (uint8 [H, W]), ``pattern``
    (a BAYER_PATTERNS name), ``table`` (bilinear_lut [H*W, 2] fp64), ``crop_bottom`` (rows), ``subsample`` (1 or 2) and optionally
    ``out`` (uint8 [(H - crop_bottom) / s, W / s, 3]).  Returns the output tensors in camera order."""
    if not 1 <= len(cams) <= RECTIFY_MAX_CAMS:
        raise ValueError(f"rectify_bayer: 1..{RECTIFY_MAX_CAMS} cameras per call")
    plans = []
    for c in cams:   # shapes first: they are refused the same way wherever the tensors live
        m = c["mosaic"]
        if getattr(m, "ndim", 0) != 2:
            raise ValueError("mosaic: expected a 2-D Bayer frame")
        H, W = m.shape
        s, crop = int(c.get("subsample", 1)), int(c.get("crop_bottom", 0))
        if s not in (1, 2):
            raise NotImplementedError(f"subsample {s}: only PIL's resize(BILINEAR) by 1 or 2 is restated")
        if not 0 <= crop < H:
            raise ValueError("crop_bottom: expected 0 <= crop_bottom < H")
        if (H - crop) % s or W % s:
            raise ValueError(f"cropped size {H - crop} x {W} is not divisible by the subsample factor {s}")
        _lut_rows(c["table"], H, W)
        plans.append((H, W, s, crop, ((H - crop) // s, W // s, 3)))
    arr = (_lib.RectifyCamera * len(cams))()
    outs = []
    for k, (c, (H, W, s, crop, shape)) in enumerate(zip(cams, plans)):
        m = _chk(c["mosaic"], torch.uint8, "mosaic")
        table = _chk(c["table"], torch.float64, "table")
        out = c.get("out")
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=m.device)
        elif tuple(_chk(out, torch.uint8, "out").shape) != shape:
            raise ValueError("Invalid shape")
        a = arr[k]
        a.mosaic, a.H, a.W, a.pattern = m.data_ptr(), H, W, _bayer(c["pattern"])
        a.table, a.crop_bottom, a.subsample, a.out = table.data_ptr(), crop, s, out.data_ptr()
        outs.append(out)
    import ctypes as C_
    lib = _lib.load()
    p = C_.cast(arr, C_.c_void_p)
    need = lib.vfm_rectify_bayer_workspace_bytes(len(cams), p)
    if ws is None and need:
        ws = _ws(need, outs[0].device)
    _lib.check(lib.vfm_rectify_bayer(len(cams), p, _ptr(ws), ws.numel() if ws is not None else 0, _stream()), "rectify_bayer")
    return outs


def transform_xyz(xyz: torch.Tensor, T: torch.Tensor) -> torch.Tensor:
    """transform_pcl's coordinate part (vfm_reg/utils.py:47-54): fp64 [N,3] x [4,4]."""
    _chk(xyz, torch.float64, "xyz")
    _chk(T, torch.float64, "T")
    out = torch.empty_like(xyz)
    lib = _lib.load()
    _lib.check(lib.vfm_transform_xyz_f64(xyz.data_ptr(), xyz.shape[0], T.data_ptr(), out.data_ptr(), _stream()),
               "transform_xyz")
    return out


# ------------------------------------------------------------------------------------ voxel maps
def voxel_robin_level(pts: torch.Tensor, voxel_size: float, idx: Optional[torch.Tensor] = None, n_dev: Optional[torch.Tensor] = None,
                      n_max: Optional[int] = None, T: Optional[torch.Tensor] = None, hash_mul: int = 19349663, want_local: bool = False):
    """One level of a chain of VoxelDownsample()s, enqueued without a read-back (vfm_voxel_robin_level): the points ``pts[idx[:n_dev]]``
    (``idx`` None: ``pts`` itself), moved by the pose ``T`` first when given.  Returns ``dict(keep, local, count, info)`` of device tensors:
    ``keep`` the survivors in the container's order as rows of ``pts`` (the next level's ``idx``), ``local`` their positions in this
    level's input (``want_local``), ``count`` int64[1], ``info`` int64[8] = {buckets, voxels or -1, probe distance, wrapped, -, done}."""
    _chk(pts, torch.float64, "pts")
    lib = _lib.load()
    stride = pts.shape[1]
    n_max = int(n_max if n_max is not None else (idx.shape[0] if idx is not None else pts.shape[0]))
    dev = pts.device
    keep = torch.empty(n_max, dtype=torch.int64, device=dev)
    local = torch.empty(n_max, dtype=torch.int64, device=dev) if want_local else None
    count = torch.empty(1, dtype=torch.int64, device=dev)
    info = torch.empty(8, dtype=torch.int64, device=dev)
    ws = _ws(lib.vfm_voxel_robin_workspace_bytes(n_max), dev)
    if idx is not None:
        _chk(idx, torch.int64, "idx")
    if T is not None:
        _chk(T, torch.float64, "T")
    _lib.check(lib.vfm_voxel_robin_level(pts.data_ptr(), stride, _ptr(idx), n_max, _ptr(n_dev), _ptr(T), float(voxel_size), int(hash_mul),
                                         keep.data_ptr(), _ptr(local), count.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
               "voxel_robin_level")
    return dict(keep=keep, local=local, count=count, info=info, ws=ws)



def voxel_first(xyz: torch.Tensor, voxel_size: float, max_per_voxel: int = 1) -> torch.Tensor:
    """Indices (ascending) of the points that are among the first `max_per_voxel` of their voxel:
    VoxelDownsample (Preprocessing.cpp:50-137) for 1, VoxelHashMap::AddPoints' cap otherwise."""
    _chk(xyz, torch.float64, "xyz")
    lib = _lib.load()
    n, stride = xyz.shape
    keep = torch.empty(max(n, 1), dtype=torch.int64, device=xyz.device)
    count = torch.empty(1, dtype=torch.int64, device=xyz.device)
    ws = _ws(lib.vfm_voxel_first_workspace_bytes(n), xyz.device)
    _lib.check(lib.vfm_voxel_first(xyz.data_ptr(), n, stride, float(voxel_size), int(max_per_voxel), keep.data_ptr(),
                                   count.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "voxel_first")
    return keep[:int(count.item())]


HASH_DOWNSAMPLE = 19349663  # VoxelHash of Preprocessing.cpp:44
HASH_MAP = 19349669         # VoxelHash of VoxelHashMap.hpp:75


def voxel_robin(xyz: torch.Tensor, voxel_size: float, max_per_voxel: int = 1, reserve: bool = True,
                hash_mul: int = HASH_DOWNSAMPLE, return_info: bool = False):
    """The survivors of ``voxel_first`` in the order the reference emits them (tsl::robin_map iteration
    order): ``reserve=True, HASH_DOWNSAMPLE`` = VoxelDownsample (Preprocessing.cpp:50-69);
    ``reserve=False, HASH_MAP`` = a fresh VoxelHashMap after AddPoints, as Pointcloud*() walk it."""
    _chk(xyz, torch.float64, "xyz")
    lib = _lib.load()
    n, stride = xyz.shape
    keep = torch.empty(max(n, 1), dtype=torch.int64, device=xyz.device)
    count = torch.empty(1, dtype=torch.int64, device=xyz.device)
    info = getattr(_tls, "voxel_info", None)     # page-locked: the entry point's one read-back lands in it by DMA
    if info is None:
        info = _tls.voxel_info = torch.zeros(4, dtype=torch.int64).pin_memory()
    ws = _ws(lib.vfm_voxel_robin_workspace_bytes(n), xyz.device)
    _lib.check(lib.vfm_voxel_robin(xyz.data_ptr(), n, stride, float(voxel_size), int(max_per_voxel), int(hash_mul),
                                   n if reserve else -1, keep.data_ptr(), count.data_ptr(), info.data_ptr(),
                                   ws.data_ptr(), ws.numel(), _stream()), "voxel_robin")
    # (the entry point synchronises and reports the number of voxels: with one point per voxel that IS the count -- no second read-back)
    vals = info.tolist()
    out = keep[:vals[1] if max_per_voxel == 1 else int(count.item())]
    return (out, vals) if return_info else out


# ------------------------------------------------------------------------------------- FPFH (csrc/fpfh.hip)
FPFH_MAX_NN = 1024


def fpfh_grid(pts: torch.Tensor, radius: float, ws: Optional[torch.Tensor] = None):
    """The search structure of KDTreeFlann(cloud): (sorted cell keys int64[n], point indices in that order int32[n])."""
    _chk(pts, torch.float64, "pts")
    lib = _lib.load()
    n = pts.shape[0]
    keys = torch.empty(n, dtype=torch.int64, device=pts.device)
    order = torch.empty(n, dtype=torch.int32, device=pts.device)
    need = lib.vfm_fpfh_workspace_bytes(n)
    if ws is None or ws.numel() < need:
        ws = _ws(need, pts.device)
    _lib.check(lib.vfm_fpfh_grid_build(pts.data_ptr(), n, float(radius), keys.data_ptr(), order.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _stream()), "fpfh_grid_build")
    return keys, order


def fpfh_search(pts: torch.Tensor, radius: float, max_nn: int, grid=None, want_scanned: bool = False):
    """KDTreeFlann::SearchHybrid(radius, max_nn) for every point of the cloud: dict(idx int32[n, max_nn] (-1 padded), d2 fp64[n, max_nn],
    count int32[n]; scanned int32[n], the grid points each query read, if asked)."""
    _chk(pts, torch.float64, "pts")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("Invalid shape")
    if not 1 <= int(max_nn) <= FPFH_MAX_NN:
        raise ValueError(f"max_nn must be in 1..{FPFH_MAX_NN}")
    lib = _lib.load()
    n = pts.shape[0]
    keys, order = grid if grid is not None else fpfh_grid(pts, radius)
    idx = torch.empty((n, max_nn), dtype=torch.int32, device=pts.device)
    d2 = torch.empty((n, max_nn), dtype=torch.float64, device=pts.device)
    cnt = torch.empty(n, dtype=torch.int32, device=pts.device)
    scanned = torch.empty(n, dtype=torch.int32, device=pts.device) if want_scanned else None
    _lib.check(lib.vfm_fpfh_search_hybrid(pts.data_ptr(), n, keys.data_ptr(), order.data_ptr(), float(radius), int(max_nn), idx.data_ptr(),
                                          d2.data_ptr(), cnt.data_ptr(), _ptr(scanned), _stream()), "fpfh_search_hybrid")
    out = dict(idx=idx, d2=d2, count=cnt)
    if want_scanned:
        out["scanned"] = scanned
    return out


def fpfh_normals(pts: torch.Tensor, nbrs: dict) -> torch.Tensor:
    """EstimateNormals(fast_normal_computation=True) from SearchHybrid rows (``fpfh_search``): n x 3 fp64."""
    _chk(pts, torch.float64, "pts")
    lib = _lib.load()
    n = pts.shape[0]
    out = torch.empty((n, 3), dtype=torch.float64, device=pts.device)
    _lib.check(lib.vfm_fpfh_normals(pts.data_ptr(), n, nbrs["idx"].data_ptr(), nbrs["count"].data_ptr(), nbrs["idx"].shape[1],
                                    out.data_ptr(), _stream()), "fpfh_normals")
    return out


def fpfh_voxel_down_sample(pts: torch.Tensor, voxel_size: float, normals: Optional[torch.Tensor] = None):
    """PointCloud::VoxelDownSample: (points m x 3, normals m x 3 or None), voxels in ascending (ix, iy, iz) order.  Reads the voxel
    count back (synchronises the stream)."""
    _chk(pts, torch.float64, "pts")
    if normals is not None:
        _chk(normals, torch.float64, "normals")
        if normals.shape != pts.shape:
            raise ValueError("normals must match points")
    if not voxel_size > 0:
        raise ValueError("voxel_size must be positive")
    lib = _lib.load()
    n = pts.shape[0]
    out = torch.empty((n, 3), dtype=torch.float64, device=pts.device)
    nout = torch.empty((n, 3), dtype=torch.float64, device=pts.device) if normals is not None else None
    count = torch.empty(1, dtype=torch.int32, device=pts.device)
    ws = _ws(lib.vfm_fpfh_workspace_bytes(n), pts.device)
    _lib.check(lib.vfm_fpfh_voxel_down_sample(pts.data_ptr(), _ptr(normals), n, float(voxel_size), out.data_ptr(), _ptr(nout),
                                              count.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "fpfh_voxel_down_sample")
    m = int(count.item())
    if m < 0:
        raise ValueError("voxel_size is too small for the extent of the point cloud (2^21 voxels per axis)")
    return out[:m], (nout[:m] if nout is not None else None)


def fpfh_spfh(pts: torch.Tensor, normals: torch.Tensor, nbrs: dict) -> torch.Tensor:
    """ComputeSPFHFeature from SearchHybrid rows: n x 33 fp64."""
    _chk(pts, torch.float64, "pts")
    _chk(normals, torch.float64, "normals")
    lib = _lib.load()
    n = pts.shape[0]
    out = torch.empty((n, 33), dtype=torch.float64, device=pts.device)
    _lib.check(lib.vfm_fpfh_spfh(pts.data_ptr(), normals.data_ptr(), n, nbrs["idx"].data_ptr(), nbrs["count"].data_ptr(),
                                 nbrs["idx"].shape[1], out.data_ptr(), _stream()), "fpfh_spfh")
    return out


def fpfh_fpfh(spfh: torch.Tensor, nbrs: dict) -> torch.Tensor:
    """ComputeFPFHFeature from the SPFH rows and the same SearchHybrid rows: n x 33 fp64 (Open3D's Feature.data is its transpose)."""
    _chk(spfh, torch.float64, "spfh")
    lib = _lib.load()
    n = spfh.shape[0]
    out = torch.empty((n, 33), dtype=torch.float64, device=spfh.device)
    _lib.check(lib.vfm_fpfh_fpfh(spfh.data_ptr(), n, nbrs["idx"].data_ptr(), nbrs["d2"].data_ptr(), nbrs["count"].data_ptr(),
                                 nbrs["idx"].shape[1], out.data_ptr(), _stream()), "fpfh_fpfh")
    return out


# ------------------------------------------------------------------------------------- exact 1-NN in 3-D (csrc/nn3.hip)
class Nn3Grid:
    """The search structure of ``nn3_build``: sorted cell keys int64[n], point indices in that order int32[n], the points in that
    order fp64[n, 3], and the cell size they were built with."""

    __slots__ = ("keys", "order", "sorted", "cell", "n")

    def __init__(self, keys, order, sorted_pts, cell, n):
        self.keys, self.order, self.sorted, self.cell, self.n = keys, order, sorted_pts, float(cell), int(n)


def nn3_build(pts: torch.Tensor, cell: float, ws: Optional[torch.Tensor] = None) -> Nn3Grid:
    """vfm_nn3_build: the grid of cubic cells of edge ``cell`` over an n x 3 fp64 cloud (n >= 1).  The cell size changes the time of
    a query, never its answer; ``vfmreg.neighbors.choose_cell`` picks one from the cloud."""
    _chk(pts, torch.float64, "pts")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("Invalid shape")
    n = pts.shape[0]
    if n == 0:
        raise ValueError("Found array with 0 sample(s) while a minimum of 1 is required")
    lib = _lib.load()
    keys = torch.empty(n, dtype=torch.int64, device=pts.device)
    order = torch.empty(n, dtype=torch.int32, device=pts.device)
    sorted_pts = torch.empty((n, 3), dtype=torch.float64, device=pts.device)
    need = lib.vfm_nn3_workspace_bytes(n)
    if ws is None or ws.numel() < need:
        ws = _ws(need, pts.device)
    _lib.check(lib.vfm_nn3_build(pts.data_ptr(), n, float(cell), keys.data_ptr(), order.data_ptr(), sorted_pts.data_ptr(), ws.data_ptr(),
                                 ws.numel(), _stream()), "nn3_build")
    return Nn3Grid(keys, order, sorted_pts, cell, n)


def _nn3_head(grid: Nn3Grid, q: torch.Tensor) -> tuple:
    """the arguments vfm_nn3_query and vfm_nn3_knn open with: the structure, then the checked nq x 3 fp64 rows of ``q``"""
    _chk(q, torch.float64, "q")
    if q.dim() != 2 or q.shape[1] != 3:
        raise ValueError("Invalid shape")
    return grid.keys.data_ptr(), grid.order.data_ptr(), grid.sorted.data_ptr(), grid.n, grid.cell, q.data_ptr(), q.shape[0]


def nn3_query(grid: Nn3Grid, q: torch.Tensor, want_fallbacks: bool = False):
    """vfm_nn3_query: (idx int64[nq], dist fp64[nq]) of the nearest point of the cloud for every row of ``q`` (nq x 3 fp64) --
    ``KDTree.query(k=1)`` of registration_node.py:297-298; with ``want_fallbacks`` also int32[1], the number of queries that read every
    point instead of cells.  No read-back."""
    head = _nn3_head(grid, q)
    idx = torch.empty(q.shape[0], dtype=torch.int64, device=q.device)
    dist = torch.empty(q.shape[0], dtype=torch.float64, device=q.device)
    fb = torch.empty(1, dtype=torch.int32, device=q.device) if want_fallbacks else None
    _lib.check(_lib.load().vfm_nn3_query(*head, idx.data_ptr(), dist.data_ptr(), _ptr(fb), _stream()), "nn3_query")
    return (idx, dist, fb) if want_fallbacks else (idx, dist)


NN3_KNN_MAX_K = 64


def nn3_knn(grid: Nn3Grid, q: torch.Tensor, k: int, max_d2: float = math.inf, want_fallbacks: bool = False):
    """vfm_nn3_knn: (idx int64[nq, k], d2 fp64[nq, k], count int32[nq]) -- the k nearest points (1 <= k <= 64) of the cloud for every
    row of ``q`` (nq x 3 fp64), rows ascending in (d2, index), SQUARED distances, only points with ``d2 <= max_d2``; entries past
    ``count`` are (-1, +inf).  ``faiss.IndexFlatL2.search`` of vfm_reg/utils.py:31,40.  With ``want_fallbacks`` also int32[1], the
    number of queries that read every point.  No read-back."""
    head = _nn3_head(grid, q)
    nq, k = q.shape[0], int(k)
    idx = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=q.device)
    d2 = torch.empty((nq, max(k, 0)), dtype=torch.float64, device=q.device)
    count = torch.empty(nq, dtype=torch.int32, device=q.device)
    fb = torch.empty(1, dtype=torch.int32, device=q.device) if want_fallbacks else None
    _lib.check(_lib.load().vfm_nn3_knn(*head, k, float(max_d2), idx.data_ptr(), d2.data_ptr(), count.data_ptr(), _ptr(fb), _stream()),
               "nn3_knn")
    return (idx, d2, count, fb) if want_fallbacks else (idx, d2, count)


# ------------------------------------------------------------------------------------- exact HDBSCAN* in 3-D (csrc/hdbscan.hip)
def mreach_mst(grid: Nn3Grid, core2: torch.Tensor, want_counts: bool = False, ws: Optional[torch.Tensor] = None):
    """vfm_mreach_mst: (lo int32[n-1], hi int32[n-1], w2 fp64[n-1]) -- the edges of THE minimum spanning tree of the grid's points under
    ``w2(i, j) = max(core2[i], core2[j], d2(i, j))`` and the total order ``(w2, lo, hi)``, in no particular order; ``core2`` fp64[n] by
    point index, finite and >= 0.  With ``want_counts`` also (rounds int32[1], fallbacks int32[1]): the Boruvka rounds that did work
    and the searches that read every point.  No read-back."""
    _chk(core2, torch.float64, "core2")
    n = grid.n
    if core2.dim() != 1 or core2.shape[0] != n:
        raise ValueError(f"core2: expected {n} values, one per point of the grid")
    lib = _lib.load()
    dev = core2.device
    lo = torch.empty(max(n - 1, 0), dtype=torch.int32, device=dev)
    hi = torch.empty(max(n - 1, 0), dtype=torch.int32, device=dev)
    w2 = torch.empty(max(n - 1, 0), dtype=torch.float64, device=dev)
    rounds = torch.empty(1, dtype=torch.int32, device=dev) if want_counts else None
    fb = torch.empty(1, dtype=torch.int32, device=dev) if want_counts else None
    need = lib.vfm_mreach_mst_workspace_bytes(n)
    if ws is None or ws.numel() < need:
        ws = _ws(need, dev)
    _lib.check(lib.vfm_mreach_mst(grid.keys.data_ptr(), grid.order.data_ptr(), grid.sorted.data_ptr(), n, grid.cell, core2.data_ptr(),
                                  lo.data_ptr(), hi.data_ptr(), w2.data_ptr(), _ptr(rounds), _ptr(fb), ws.data_ptr(), ws.numel(), _stream()),
               "mreach_mst")
    return (lo, hi, w2, rounds, fb) if want_counts else (lo, hi, w2)


def hdbscan_labels_host(lo, hi, w2, min_cluster_size: int):
    """vfm_hdbscan_labels_host: labels int32[n] (numpy, on the host) from the n - 1 edges of the spanning tree ascending in
    ``(w2, lo, hi)`` (numpy int32, int32, fp64).  No device is touched."""
    import numpy as np
    lo = np.ascontiguousarray(lo, dtype=np.int32)
    hi = np.ascontiguousarray(hi, dtype=np.int32)
    w2 = np.ascontiguousarray(w2, dtype=np.float64)
    if not (lo.ndim == hi.ndim == w2.ndim == 1 and len(lo) == len(hi) == len(w2)):
        raise ValueError("lo, hi and w2 must be three vectors of one length")
    labels = np.empty(len(lo) + 1, dtype=np.int32)
    _lib.check(_lib.load().vfm_hdbscan_labels_host(lo.ctypes.data, hi.ctypes.data, w2.ctypes.data, len(lo) + 1, int(min_cluster_size),
                                                   labels.ctypes.data), "hdbscan_labels_host")
    return labels


# ------------------------------------------------------------------------------------- TEASER++ registration (csrc/teaser.hip, teaser_host.cpp)
TEASER_MAX_N = 32768
TEASER_MAX_SEEDS = 16
TEASER_NODE_LIMIT = 50_000_000     # nodes of the host's exact clique search before it gives up (VFM_ELIMIT), the default of the wrappers


def _teaser_rows(t: torch.Tensor, name: str) -> torch.Tensor:
    _chk(t, torch.float64, name)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name}: expected n x 3 rows")
    return t


def teaser_graph(src: torch.Tensor, tgt: torch.Tensor, noise_bound: float, cbar2: float = 1.0):
    """vfm_teaser_graph: (adj uint64-as-int64 [n, ceil(n / 64)], degree int32[n]) of the consistency graph of n correspondences
    (``src`` / ``tgt``: n x 3 fp64, 1 <= n <= 32768).  No read-back."""
    _teaser_rows(src, "src"), _teaser_rows(tgt, "tgt")
    n = src.shape[0]
    if tgt.shape[0] != n:
        raise ValueError("src and tgt must have one row per correspondence each")
    adj = torch.empty((n, (n + 63) // 64), dtype=torch.int64, device=src.device)
    deg = torch.empty(n, dtype=torch.int32, device=src.device)
    _lib.check(_lib.load().vfm_teaser_graph(src.data_ptr(), tgt.data_ptr(), n, float(noise_bound), float(cbar2), adj.data_ptr(), deg.data_ptr(),
                                            _stream()), "teaser_graph")
    return adj, deg


def teaser_reduce(adj: torch.Tensor, deg: torch.Tensor, seeds: int = TEASER_MAX_SEEDS, ws: Optional[torch.Tensor] = None):
    """vfm_teaser_reduce: (kept int32[n], info int32[2] = {h, number kept}) on the device -- the first info[1] entries of kept are the
    vertices that can belong to a clique of h members or more, ascending.  No read-back."""
    _chk(adj, torch.int64, "adj"), _chk(deg, torch.int32, "degree")
    n = deg.shape[0]
    if tuple(adj.shape) != (n, (n + 63) // 64):
        raise ValueError("adj: expected n x ceil(n / 64) words")
    lib = _lib.load()
    kept = torch.empty(n, dtype=torch.int32, device=adj.device)
    info = torch.empty(2, dtype=torch.int32, device=adj.device)
    need = lib.vfm_teaser_reduce_workspace_bytes(n)
    if ws is None or ws.numel() < need:
        ws = _ws(need, adj.device)
    _lib.check(lib.vfm_teaser_reduce(adj.data_ptr(), deg.data_ptr(), n, int(seeds), kept.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _stream()), "teaser_reduce")
    return kept, info


def teaser_submatrix(adj: torch.Tensor, kept: torch.Tensor) -> torch.Tensor:
    """vfm_teaser_submatrix: the rows and columns ``kept`` (int32[k], ascending) of adj as [k, ceil(k / 64)] words.  No read-back."""
    _chk(adj, torch.int64, "adj"), _chk(kept, torch.int32, "kept")
    n, k = adj.shape[0], kept.shape[0]
    sub = torch.empty((k, (k + 63) // 64), dtype=torch.int64, device=adj.device)
    _lib.check(_lib.load().vfm_teaser_submatrix(adj.data_ptr(), n, kept.data_ptr(), k, sub.data_ptr(), _stream()), "teaser_submatrix")
    return sub


def teaser_max_clique_host(sub, kept, known: int = 0, node_limit: int = TEASER_NODE_LIMIT) -> np.ndarray:
    """vfm_teaser_max_clique_host: THE maximum clique (int32, the entries of ``kept`` of its members, ascending) of the graph ``sub``
    (numpy, [k, ceil(k / 64)] uint64 or int64 words).  Raises RuntimeError when ``node_limit`` runs out.  No device is touched."""
    import ctypes as C
    kept = np.ascontiguousarray(kept, dtype=np.int32)
    k = len(kept)
    sub = np.ascontiguousarray(sub).view(np.uint64).reshape(k, (k + 63) // 64)
    clique = np.full(max(k, 1), -1, dtype=np.int32)
    size = C.c_int64(-1)
    _lib.check(_lib.load().vfm_teaser_max_clique_host(sub.ctypes.data, kept.ctypes.data, k, int(known), int(node_limit), clique.ctypes.data,
                                                      C.byref(size)), "teaser_max_clique_host")
    return clique[:size.value].copy()


def teaser_gnc(src: torch.Tensor, tgt: torch.Tensor, clique: torch.Tensor, noise_bound: float, gnc_factor: float = 1.4,
               max_iterations: int = 10000, cost_threshold: float = 1e-16, ws: Optional[torch.Tensor] = None):
    """vfm_teaser_gnc: (R fp64[3, 3], weights fp64[k - 1], iterations int32[1], v fp64[k, 3]) on the device for the clique (int32[k],
    k >= 2, ascending rows of src / tgt).  No read-back."""
    _teaser_rows(src, "src"), _teaser_rows(tgt, "tgt"), _chk(clique, torch.int32, "clique")
    n, k = src.shape[0], clique.shape[0]
    lib = _lib.load()
    dev = src.device
    R = torch.empty((3, 3), dtype=torch.float64, device=dev)
    w = torch.empty(max(k - 1, 0), dtype=torch.float64, device=dev)
    it = torch.empty(1, dtype=torch.int32, device=dev)
    v = torch.empty((k, 3), dtype=torch.float64, device=dev)
    need = lib.vfm_teaser_gnc_workspace_bytes(k)
    if ws is None or ws.numel() < need:
        ws = _ws(need, dev)
    _lib.check(lib.vfm_teaser_gnc(src.data_ptr(), tgt.data_ptr(), n, clique.data_ptr(), k, float(noise_bound), float(gnc_factor),
                                  int(max_iterations), float(cost_threshold), R.data_ptr(), w.data_ptr(), it.data_ptr(), v.data_ptr(),
                                  ws.data_ptr(), ws.numel(), _stream()), "teaser_gnc")
    return R, w, it, v


def teaser_tls_translation_host(v, rng: float):
    """vfm_teaser_tls_translation_host: (t fp64[3], inliers bool[k]) from the rows ``v`` (numpy, k x 3).  No device is touched."""
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3)
    t = np.empty(3, dtype=np.float64)
    inl = np.empty(len(v), dtype=np.uint8)
    _lib.check(_lib.load().vfm_teaser_tls_translation_host(v.ctypes.data, len(v), float(rng), t.ctypes.data, inl.ctypes.data),
               "teaser_tls_translation_host")
    return t, inl.astype(bool)


# ------------------------------------------------------------------------------------- descriptor PCA and the colour gate (csrc/pca.hip)
PCA_MAX_D = 768
PCA_MAX_K = 8
ROWS_F32, ROWS_F16 = 0, 1      # VFM_ROWS_F32 / VFM_ROWS_F16


def _pca_rows(x: torch.Tensor) -> int:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("x: expected a tensor on the ROCm device (no CPU path exists)")
    if x.dtype not in (torch.float32, torch.float16):
        raise TypeError(f"x: expected float32 or float16 rows, got {x.dtype}")
    if x.dim() != 2 or not x.is_contiguous():
        raise ValueError("x: must be a contiguous n x d matrix")
    return ROWS_F16 if x.dtype == torch.float16 else ROWS_F32


def pca_moments(x: torch.Tensor, ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """vfm_pca_moments: (mean fp64[d], scatter fp64[d, d]) of the rows x (n x d, float32 or float16): the column means and
    ``sum_n (x_n - mean)(x_n - mean)^T`` on the fp64 matrix cores, exactly symmetric, the same bits on every run.  No read-back."""
    dtype = _pca_rows(x)
    n, d = x.shape
    lib = _lib.load()
    mean = torch.empty(d, dtype=torch.float64, device=x.device)
    scatter = torch.empty((d, d), dtype=torch.float64, device=x.device)
    need = lib.vfm_pca_moments_workspace_bytes(d)
    if ws is None or ws.numel() < need:
        ws = _ws(need, x.device)
    _lib.check(lib.vfm_pca_moments(x.data_ptr(), dtype, n, d, mean.data_ptr(), scatter.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
               "pca_moments")
    return mean, scatter


def pca_project(x: torch.Tensor, mean: torch.Tensor, components: torch.Tensor, ws: Optional[torch.Tensor] = None):
    """vfm_pca_project: (y fp64[n, k], zero_rows uint8[n], min fp64[k], max fp64[k]) for mean fp64[d] and components fp64[k, d]:
    ``y = (x - mean) . components^T`` in the order of addition DESIGN §7.6 fixes, the rows whose features are all zero, and the
    extremes of every component over all rows.  No read-back."""
    dtype = _pca_rows(x)
    n, d = x.shape
    _chk(mean, torch.float64, "mean")
    _chk(components, torch.float64, "components")
    if mean.shape != (d,) or components.dim() != 2 or components.shape[1] != d:
        raise ValueError(f"expected mean [{d}] and components [k, {d}], got {tuple(mean.shape)} and {tuple(components.shape)}")
    k = components.shape[0]
    lib = _lib.load()
    dev = x.device
    y = torch.empty((n, k), dtype=torch.float64, device=dev)
    zero = torch.empty(n, dtype=torch.uint8, device=dev)
    lo = torch.empty(k, dtype=torch.float64, device=dev)
    hi = torch.empty(k, dtype=torch.float64, device=dev)
    need = lib.vfm_pca_project_workspace_bytes()
    if ws is None or ws.numel() < need:
        ws = _ws(need, dev)
    _lib.check(lib.vfm_pca_project(x.data_ptr(), dtype, n, d, mean.data_ptr(), components.data_ptr(), k, y.data_ptr(), zero.data_ptr(),
                                   lo.data_ptr(), hi.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "pca_project")
    return y, zero, lo, hi


def pca_colours(y: torch.Tensor, zero_rows: Optional[torch.Tensor], lo: torch.Tensor, hi: torch.Tensor, rgb: bool) -> torch.Tensor:
    """vfm_pca_colours: ``(y - min) / (max - min)`` as float32 [n, k], or with ``rgb`` (k == 3) as the uint8 colours of
    image_features.py:184-190: times 255.0, truncated, black where ``zero_rows`` is set."""
    _chk(y, torch.float64, "y")
    _chk(lo, torch.float64, "min")
    _chk(hi, torch.float64, "max")
    n, k = y.shape
    if rgb:
        _chk(zero_rows, torch.uint8, "zero_rows")
    out = torch.empty((n, k), dtype=torch.uint8 if rgb else torch.float32, device=y.device)
    _lib.check(_lib.load().vfm_pca_colours(y.data_ptr(), _ptr(zero_rows), n, k, lo.data_ptr(), hi.data_ptr(), None if rgb else out.data_ptr(),
                                           out.data_ptr() if rgb else None, _stream()), "pca_colours")
    return out


def colour_gate(colours: torch.Tensor, gate_colours: torch.Tensor, radius: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """vfm_colour_gate: (idx int64[m, n], counts int64[m]) -- per colour of ``gate_colours`` (fp64 [m, 3]) the rows of ``colours``
    (uint8 [n, 3]) nearer than ``radius``, ascending, in the first ``counts[c]`` entries of ``idx[c]``.  No read-back."""
    _chk(colours, torch.uint8, "colours")
    _chk(gate_colours, torch.float64, "gate_colours")
    if colours.dim() != 2 or colours.shape[1] != 3 or gate_colours.dim() != 2 or gate_colours.shape[1] != 3:
        raise ValueError("expected colours [n, 3] and gate_colours [m, 3]")
    n, m = colours.shape[0], gate_colours.shape[0]
    idx = torch.empty((m, n), dtype=torch.int64, device=colours.device)
    counts = torch.empty(m, dtype=torch.int64, device=colours.device)
    _lib.check(_lib.load().vfm_colour_gate(colours.data_ptr(), n, gate_colours.data_ptr(), m, float(radius), idx.data_ptr(), counts.data_ptr(),
                                           _stream()), "colour_gate")
    return idx, counts


# ------------------------------------------------------------------------------------- odometry (csrc/odometry.hip)
def _rows_f64(rows: torch.Tensor, name: str) -> torch.Tensor:
    _chk(rows, torch.float64, name)
    if rows.dim() != 2 or rows.shape[1] < 3:
        raise ValueError("Invalid shape")
    return rows


def range_crop(rows: torch.Tensor, min_range: float, max_range: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """vfm_range_crop (Preprocess, Preprocessing.cpp:139-197): (idx int64[n], count int64[1]) -- the rows of ``rows`` (fp64 [n, w >= 3],
    xyz first) with min_range < |xyz| < max_range, ascending, in the first ``count`` entries of ``idx``.  No read-back."""
    _rows_f64(rows, "rows")
    n, stride = rows.shape
    idx = torch.empty(max(n, 1), dtype=torch.int64, device=rows.device)
    count = torch.empty(1, dtype=torch.int64, device=rows.device)
    _lib.check(_lib.load().vfm_range_crop(rows.data_ptr() if n else None, n, stride, float(min_range), float(max_range), idx.data_ptr(),
                                          count.data_ptr(), _stream()), "range_crop")
    return idx, count


def deskew_scan(rows: torch.Tensor, timestamps: torch.Tensor, delta) -> torch.Tensor:
    """vfm_deskew_scan (DeSkewScan, Deskew.cpp:40-68): exp((t_i - 0.5) delta) applied to the coordinates of ``rows`` (fp64 [n, w >= 3]);
    ``delta``: the twist [upsilon, omega] on the host.  Returns fp64 [n, 3]."""
    _rows_f64(rows, "rows")
    _chk(timestamps, torch.float64, "timestamps")
    n, stride = rows.shape
    if timestamps.dim() != 1 or timestamps.shape[0] != n:
        raise ValueError("expected one timestamp per row")
    d = np.ascontiguousarray(delta, dtype=np.float64)
    if d.shape != (6,):
        raise ValueError("expected a twist of 6 values")
    out = torch.empty((n, 3), dtype=torch.float64, device=rows.device)
    _lib.check(_lib.load().vfm_deskew_scan(rows.data_ptr() if n else None, n, stride, timestamps.data_ptr() if n else None, d.ctypes.data,
                                           out.data_ptr() if n else None, _stream()), "deskew_scan")
    return out


def rows_merge(rows_old: Optional[torch.Tensor], rows_new: Optional[torch.Tensor], src: torch.Tensor, n_out_dev: torch.Tensor,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vfm_rows_merge: ``out[q] = cat(rows_old, rows_new)[src[q]]`` for q < min(n_out_dev[0], len(src)) -- the payload rows of a grid update
    in the new grid's order.  ``rows_old`` [nk, w] / ``rows_new`` [m, w]: device tensors of one dtype (4 or 8 bytes per element) and width, either
    may be None; ``src``: int32 (the update's provenance); ``n_out_dev``: int32[>= 1] on the device (``info[1:]`` of the update).  Returns
    ``out`` [len(src), w]; the rows behind the count are not written.  No read-back."""
    given = [r for r in (rows_old, rows_new) if r is not None]
    if not given:
        raise ValueError("rows_merge: no rows")
    for r, name in ((rows_old, "rows_old"), (rows_new, "rows_new")):
        if r is not None:
            _chk(r, given[0].dtype, name)
            if r.dim() != 2 or r.shape[1] != given[0].shape[1]:
                raise ValueError("Invalid shape")
    _chk(src, torch.int32, "src")
    _chk(n_out_dev, torch.int32, "n_out_dev")
    w = int(given[0].shape[1])
    row_bytes = w * given[0].element_size()
    if row_bytes <= 0 or row_bytes % 4:
        raise ValueError("rows_merge: a row must be a positive multiple of 4 bytes")
    nk = 0 if rows_old is None else int(rows_old.shape[0])
    m = 0 if rows_new is None else int(rows_new.shape[0])
    n_max = int(src.shape[0])
    if out is None:
        out = torch.empty((max(n_max, 1), w), dtype=given[0].dtype, device=given[0].device)
    else:
        _chk(out, given[0].dtype, "out")
        if out.dim() != 2 or out.shape[1] != w or out.shape[0] < n_max:
            raise ValueError("Invalid shape")
    _lib.check(_lib.load().vfm_rows_merge(rows_old.data_ptr() if nk else None, nk, rows_new.data_ptr() if m else None, m, row_bytes,
                                          src.data_ptr() if n_max else None, n_out_dev.data_ptr(), n_max, out.data_ptr(), _stream()), "rows_merge")
    return out


def icp_grid_update(keys: Optional[torch.Tensor], start: Optional[torch.Tensor], pts: Optional[torch.Tensor], xyz_new: Optional[torch.Tensor],
                    T, voxel_size: float, max_points_per_voxel: int, origin, max_distance: float, ws: Optional[torch.Tensor] = None,
                    rows_old: Optional[torch.Tensor] = None, rows_new: Optional[torch.Tensor] = None):
    """vfm_icp_grid_update: VoxelHashMap::Update on the sorted-key grid (keys int64[nv], start int32[nv + 1], pts fp64[nk, 3]; all None:
    an empty grid).  ``xyz_new``: fp64 [m, 3] on the device or None; ``T``: a 4 x 4 on the host or None (points as they are); ``origin``:
    3 values on the host or None (nothing is removed).  Returns ``dict(keys, start, pts, info)`` of device tensors sized nv + m, nv + m + 1,
    nk + m and 6 -- info = {n_voxels, n_kept, status, points_added, voxels_removed, points_removed}.  No read-back.
    ``rows_old`` [nk, w] / ``rows_new`` [m, w] (a payload per point, see ``rows_merge``; None where there are no such points): the update runs
    as vfm_icp_grid_update_src and the dict also holds ``src`` (int32[nk + m]) and ``rows`` ([nk + m, w]: the payload in the new grid's order,
    its first n_kept rows written) -- two enqueues, still no read-back."""
    lib = _lib.load()
    payload = rows_old is not None or rows_new is not None
    nv = 0 if keys is None else int(keys.shape[0])
    nk = 0 if pts is None else int(pts.shape[0])
    m = 0 if xyz_new is None else int(xyz_new.shape[0])
    if nv:
        _chk(keys, torch.int64, "keys")
        _chk(start, torch.int32, "start")
        _chk(pts, torch.float64, "pts")
        if start.shape[0] != nv + 1 or pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError("expected start [nv + 1] and pts [nk, 3]")
    if m:
        _chk(xyz_new, torch.float64, "xyz_new")
        if xyz_new.dim() != 2 or xyz_new.shape[1] != 3:
            raise ValueError("Invalid shape")
    dev = xyz_new.device if m else (keys.device if nv else torch.device("cuda"))
    Th = None if T is None else np.ascontiguousarray(T, dtype=np.float64)
    if Th is not None and Th.shape != (4, 4):
        raise ValueError("expected a 4 x 4 pose")
    oh = None if origin is None else np.ascontiguousarray(origin, dtype=np.float64)
    if oh is not None and oh.shape != (3,):
        raise ValueError("expected an origin of 3 values")
    keys_out = torch.empty(max(nv + m, 1), dtype=torch.int64, device=dev)
    start_out = torch.empty(nv + m + 1, dtype=torch.int32, device=dev)
    pts_out = torch.empty((max(nk + m, 1), 3), dtype=torch.float64, device=dev)
    info = torch.empty(6, dtype=torch.int32, device=dev)
    need = lib.vfm_icp_grid_update_workspace_bytes(nv, nk, m)
    if ws is None or ws.numel() < need:
        ws = _ws(need, dev)
    head = (keys.data_ptr() if nv else None, start.data_ptr() if nv else None, pts.data_ptr() if nv else None, nv, nk,
            xyz_new.data_ptr() if m else None, m, None if Th is None else Th.ctypes.data, float(voxel_size), int(max_points_per_voxel),
            None if oh is None else oh.ctypes.data, float(max_distance), keys_out.data_ptr(), start_out.data_ptr(), pts_out.data_ptr(),
            info.data_ptr())
    if not payload:
        _lib.check(lib.vfm_icp_grid_update(*head, ws.data_ptr(), ws.numel(), _stream()), "icp_grid_update")
        return dict(keys=keys_out, start=start_out, pts=pts_out, info=info)
    if (0 if rows_old is None else int(rows_old.shape[0])) != nk or (0 if rows_new is None else int(rows_new.shape[0])) != m:
        raise ValueError("expected one payload row per point")
    src = torch.empty(nk + m, dtype=torch.int32, device=dev)
    _lib.check(lib.vfm_icp_grid_update_src(*head, src.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "icp_grid_update_src")
    if nk + m == 0:     # (an empty payload for an empty grid)
        given = rows_old if rows_old is not None else rows_new
        rows = torch.empty((1, given.shape[1]), dtype=given.dtype, device=dev)
    else:
        rows = rows_merge(rows_old if nk else None, rows_new if m else None, src, info[1:])
    return dict(keys=keys_out, start=start_out, pts=pts_out, info=info, src=src, rows=rows)


# ------------------------------------------------------------------------------------- descriptor-weighted ICP search (csrc/icp_rows.hip)
def _desc_rows(rows: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(rows, torch.Tensor) or not rows.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the ROCm device (no CPU path exists)")
    if rows.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{name}: expected float32 or float64 rows, got {rows.dtype}")
    if rows.dim() != 2 or rows.shape[1] < 1:
        raise ValueError("Invalid shape")
    if not rows.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return rows


def icp_rows_stats(desc: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """vfm_icp_rows_stats: (norm fp64[n], has uint8[n]) of the descriptor rows ``desc`` [n, f >= 1] (float32 or float64, contiguous, on the
    device) -- |row| and "element sum != 0" on the rows' fp64 image, sums in column order.  No read-back."""
    _desc_rows(desc, "desc")
    n, f = desc.shape
    norm = torch.empty(n, dtype=torch.float64, device=desc.device)
    has = torch.empty(n, dtype=torch.uint8, device=desc.device)
    _lib.check(_lib.load().vfm_icp_rows_stats(desc.data_ptr() if n else None, desc.element_size(), n, f, norm.data_ptr() if n else None,
                                              has.data_ptr() if n else None, _stream()), "icp_rows_stats")
    return norm, has


def icp_step_nearest_rows(src: torch.Tensor, T, src_desc: torch.Tensor, src_norm: torch.Tensor, src_has: torch.Tensor, keys: torch.Tensor,
                          start: torch.Tensor, pts: torch.Tensor, map_desc: torch.Tensor, map_norm: torch.Tensor, map_has: torch.Tensor,
                          voxel_size: float, max_dist: float, src_out: Optional[torch.Tensor] = None, tgt: Optional[torch.Tensor] = None,
                          valid: Optional[torch.Tensor] = None):
    """vfm_icp_step_nearest_rows: one iteration's search of the descriptor-weighted ICP.  ``src`` fp64 [n, 3]; ``T``: a 4 x 4 on the host
    applied to ``src`` first (None: the points as they are); ``src_desc`` [n, f] / ``map_desc`` [nk, f]: descriptor rows of ONE dtype
    (float32 or float64) with their statistics (``icp_rows_stats``); ``keys`` int64[nv], ``start`` int32[nv + 1], ``pts`` fp64 [nk, 3]: the
    grid, its rows in the order of ``map_desc``.  Returns (moved fp64 [n, 3] -- ``src`` itself without ``T`` --, tgt fp64 [n, 3], valid
    uint8[n]); ``src_out`` (may be ``src``), ``tgt`` and ``valid`` are written where given.  No read-back."""
    _chk(src, torch.float64, "src")
    if src.dim() != 2 or src.shape[1] != 3:
        raise ValueError("Invalid shape")
    n = int(src.shape[0])
    _desc_rows(src_desc, "src_desc")
    _desc_rows(map_desc, "map_desc")
    if map_desc.dtype != src_desc.dtype:
        raise TypeError(f"map_desc: expected the source rows' {src_desc.dtype}, got {map_desc.dtype}")
    f = int(src_desc.shape[1])
    if map_desc.shape[1] != f or src_desc.shape[0] != n:
        raise ValueError("Invalid shape")
    _chk(keys, torch.int64, "keys")
    _chk(start, torch.int32, "start")
    _chk(pts, torch.float64, "pts")
    nv, nk = int(keys.shape[0]), int(map_desc.shape[0])
    if start.shape[0] != nv + 1 or pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] != nk:
        raise ValueError("expected start [nv + 1] and one descriptor row per grid point")
    for t, dtype, name, rows in ((src_norm, torch.float64, "src_norm", n), (src_has, torch.uint8, "src_has", n),
                                 (map_norm, torch.float64, "map_norm", nk), (map_has, torch.uint8, "map_has", nk)):
        _chk(t, dtype, name)
        if t.dim() != 1 or t.shape[0] != rows:
            raise ValueError(f"{name}: expected one entry per row")
    Th = None if T is None else np.ascontiguousarray(T, dtype=np.float64)
    if Th is not None and Th.shape != (4, 4):
        raise ValueError("expected a 4 x 4 pose")
    if Th is None:
        src_out = src
    elif src_out is None:
        src_out = torch.empty_like(src)
    else:
        _chk(src_out, torch.float64, "src_out")
        if src_out.shape != src.shape:
            raise ValueError("Invalid shape")
    if tgt is None:
        tgt = torch.empty((n, 3), dtype=torch.float64, device=src.device)
    if valid is None:
        valid = torch.empty(n, dtype=torch.uint8, device=src.device)
    _chk(tgt, torch.float64, "tgt")
    _chk(valid, torch.uint8, "valid")
    if tgt.shape != src.shape or valid.shape != (n,):
        raise ValueError("Invalid shape")
    if n:
        _lib.check(_lib.load().vfm_icp_step_nearest_rows(
            src.data_ptr(), n, None if Th is None else Th.ctypes.data, None if Th is None else src_out.data_ptr(), src_desc.data_ptr(),
            src_norm.data_ptr(), src_has.data_ptr(), src_desc.element_size(), f, keys.data_ptr() if nv else None, start.data_ptr(),
            pts.data_ptr() if nv else None, map_desc.data_ptr() if nv else None, map_norm.data_ptr() if nv else None,
            map_has.data_ptr() if nv else None, nv, float(voxel_size), float(max_dist), tgt.data_ptr(), valid.data_ptr(), _stream()),
            "icp_step_nearest_rows")
    return src_out, tgt, valid

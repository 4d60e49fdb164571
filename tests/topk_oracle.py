"""The k-best inner-product oracle of vfm_match_ip_topk: k rounds of ``orc_match_ip_candidates`` (oracle/vfm_oracle.c) over all map
rows minus the rows already chosen, on rows normalised by ``oracle.l2norm_rows``.  The committed C code fixes the summation order
(``orc_dot_f64``: fp64, ascending column) and the tie rule (equal scores to the lower map row); the padding -- (-1, lowest finite
float32) behind the last map row, as faiss pads an inner-product heap -- is added here."""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import oracle as orc

PAD_IDX = -1
PAD_SIM = np.finfo(np.float32).min


def topk(q: np.ndarray, b: np.ndarray, k: int):
    """(idx int64[n, k], sim float32[n, k]) of raw rows q (n x d) among raw rows b (m x d)."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    n, d = q.shape
    m = b.shape[0]
    idx = np.full((n, k), PAD_IDX, np.int64)
    sim = np.full((n, k), PAD_SIM, np.float32)
    if n == 0 or m == 0:
        return idx, sim
    qn, _ = orc.l2norm_rows(q)
    bn, _ = orc.l2norm_rows(b)
    alive = np.ones((n, m), bool)
    rows = np.arange(n)
    for r in range(min(k, m)):
        cand = np.ascontiguousarray(np.nonzero(alive)[1], dtype=np.int64)        # row-major: ascending map rows per query
        ptr = np.arange(n + 1, dtype=np.int64) * (m - r)
        i_r = np.empty(n, np.int64)
        s_r = np.empty(n, np.float32)
        orc.lib().orc_match_ip_candidates(orc._p(qn, orc._f32p), C.c_int64(n), orc._p(bn, orc._f32p), C.c_int(d),
                                          orc._p(ptr, orc._i64p), orc._p(cand, orc._i64p), orc._p(i_r, orc._i64p),
                                          orc._p(s_r, orc._f32p))
        idx[:, r], sim[:, r] = i_r, s_r
        alive[rows, i_r] = False
    return idx, sim


def gaussian_rows(n: int, m: int, d: int, seed: int, common: bool = False):
    """Seeded Gaussian rows (not normalised: the search normalises); ``common`` adds a shared 2 x Gaussian vector to both sides."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n, d)).astype(np.float32)
    b = rng.standard_normal((m, d)).astype(np.float32)
    if common:
        c = (2 * rng.standard_normal(d)).astype(np.float32)
        q, b = q + c, b + c
    return q, b

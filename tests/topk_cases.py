"""Seeded inputs and launch arithmetic for the k-best descriptor search (csrc/match_topk.hip).  Shared by tests/test_topk_cases.py
(CPU: the plans and scenes have the properties claimed here, checked with the oracle of tests/topk_oracle.py alone), the k-best section of
tests/test_gpu_bounds.py and tests/test_gpu_topk_edges.py (GPU: the library returns the oracle's answer on them, bit for bit).  Every
generator returns float32 arrays; nothing here touches a device.

The kernel's geometry the cases aim at: the map is padded to 256 rows and walked in 128-row chunks -- 16 chunks in one slice first, then
launches of three times the chunks already done, each cut into slices of whole chunks; a workgroup holds 256 queries (128 at d = 640 /
768) and buffers ``LREC_CAP`` records in LDS before it writes them straight to the per-query lists of ``RECORD_CAP`` entries; a row is
recorded when its coarse score is within ``WINDOW`` of the query's bound, and the coarse score is within ``COARSE_ERROR`` of the exact
one.
"""
from __future__ import annotations

import numpy as np

FAST_WIDTHS = (128, 256, 384, 640, 768)   # ops.MATCH_TOPK_FAST_WIDTHS
SEED_CHUNKS = 16                          # TOPK_SEED_CHUNKS
CHUNK_ROWS = 128
RECORD_CAP = 1024                         # TOPK_RECORD_CAP, ops.MATCH_TOPK_RECORD_CAP
LREC_CAP = 1536                           # TOPK_LREC_CAP
WINDOW = 2.5e-3                           # DEFAULT_WINDOW
COARSE_ERROR = 1.15e-3                    # the proven |coarse - exact| bound E; WINDOW >= 2 E
FIRST_STEPS_ROWS = 64                     # rows a lane's half-waves record unconditionally before its list holds k scores of its own


# ------------------------------------------------------------------------------------------------------------------ 1. the launches
def choose_slices(nqb: int, nchunks: int, forced: int = 0) -> int:
    """csrc/match_internal.h, choose_slices: ``coarse_slices`` of vfm_config when set, else whole rounds of 256 workgroups with at
    least 8 chunks per slice (the unforced rule as tools/sim_topk_records.py has it)."""
    if forced > 0:
        return min(forced, nchunks)
    best_s, best_eff = 1, -1.0

    def eff_of(s):
        total = nqb * s
        rounds = (total + 255) // 256
        return total / (rounds * 256), rounds

    for s in range(1, min(nchunks, 64) + 1):
        if nchunks // s < 8 and s > 1:
            break
        eff, _ = eff_of(s)
        if eff > best_eff + 1e-9:
            best_eff, best_s = eff, s
    for s in range(1, best_s):
        eff, rounds = eff_of(s)
        if rounds >= 8 and eff >= best_eff - 0.01:
            return s
    return best_s


def wide(d: int) -> bool:
    """the 4-wave form of the coarse kernel: 128 queries per workgroup, one 32-row tile per step"""
    return d > 384


def launch_plan(n: int, m: int, d: int, forced: int = 0):
    """[(first chunk, chunks, slices)] of the coarse pass of run_topk_fast."""
    rows_padded = (n + 255) // 256 * 256
    nqb = rows_padded // (128 if wide(d) else 256)
    total = (m + 255) // 256 * 256 // CHUNK_ROWS
    out, done = [], 0
    while done < total:
        take = min(total - done, 3 * done if done else SEED_CHUNKS)
        out.append((done, take, choose_slices(nqb, take, forced) if done else 1))
        done += take
    return out


def max_slices(n: int, m: int, d: int, forced: int = 0) -> int:
    """what ``info`` reports as the slices of a call"""
    return max(s for _, _, s in launch_plan(n, m, d, forced))


# ------------------------------------------------------------------------------------------------------------------ 2. crowded workgroup
CROWD_N, CROWD_M, CROWD_K = 4, 2048, 8
CROWD_NEAR = 480            # near-copies per query, at rows 4 i + j
CROWD_FIRST_WINNER = 2000   # the eight exact copies of query j: rows 2000 + 8 j .. 2007 + 8 j


def crowded_workgroup(d: int, seed: int = 0):
    """(q [4, d], b [2048, d]): one launch, one slice, one workgroup with live queries in both kernel forms.  Per query 480 near-copies
    at cosine ~0.9999 -- spread far below the window, so every one is recorded under any bound the kernel can hold -- fill the
    workgroup's LDS record buffer (4 x 480 > 1536) while every query stays under its own cap; the eight exact copies of each query come
    after them, so their records take the buffer-full branch, and they differ from the near-copies by less than the coarse error: only
    the fp64 finish can rank them, and only if none of them was lost."""
    rng = np.random.default_rng(1000 * d + seed)
    q = rng.standard_normal((CROWD_N, d)).astype(np.float32)
    b = rng.standard_normal((CROWD_M, d)).astype(np.float32)
    eps = np.sqrt(2.0e-4 / d)
    for j in range(CROWD_N):
        norm = float(np.linalg.norm(q[j].astype(np.float64)))
        g = rng.standard_normal((CROWD_NEAR, d))
        b[4 * np.arange(CROWD_NEAR) + j] = (q[j].astype(np.float64) + eps * norm * g).astype(np.float32)
        b[CROWD_FIRST_WINNER + 8 * j:CROWD_FIRST_WINNER + 8 * j + 8] = q[j]
    return q, b


def crowded_near_rows(j: int) -> np.ndarray:
    return 4 * np.arange(CROWD_NEAR) + j


def crowded_winners(j: int) -> np.ndarray:
    return CROWD_FIRST_WINNER + 8 * j + np.arange(8)


# ------------------------------------------------------------------------------------------------------------------ 3. stale workspace
STALE_N, STALE_M, STALE_K = 2 * 257 + 3, 2560, 8
STALE_COPIES = 1100
STALE_QUERIES = (5, 300)   # the queries equal to the repeated row: they overflow their lists and are decided by the all-pairs kernel
#                            (so does every other query that has the repeated row among its best: a handful of the Gaussian ones)


def stale_maker(d: int, seed: int = 0):
    """(q [517, d], b [2560, d]) for k = 8: a LARGER call than every case that reuses its workspace.  One map row 1100 times (more than
    a list holds) and two queries equal to it, which overflow their lists whatever their bound: after the call the fallback count and
    list, every record count, every bound and the record lists hold plausible non-zero values -- the fallback list names query 300,
    beyond the queries of the calls that follow."""
    rng = np.random.default_rng(2000 * d + seed)
    q = rng.standard_normal((STALE_N, d)).astype(np.float32)
    b = rng.standard_normal((STALE_M, d)).astype(np.float32)
    at = np.sort(rng.permutation(STALE_M)[:STALE_COPIES])
    b[at] = b[at[0]]
    for i in STALE_QUERIES:
        q[i] = b[at[0]]
    return q, b

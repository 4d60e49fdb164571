"""Records per query of the k-best coarse pass (csrc/match_topk.hip), simulated on the CPU -- the table of DESIGN.md 7.9.

    python tools/sim_topk_records.py

Rows are L2-normalised Gaussian (seed 0); the "common" cases add a shared 2 x Gaussian vector to both sides first.  Scores are fp32
Q @ B.T.  A lane sees the rows of its half-wave, ((row % 32) >> 2) & 1, and updates its bound once per step -- 64 map rows up to
d = 384, 32 map rows in the 4-wave form of d = 640 / 768, whose workgroups hold 128 queries instead of 256 --; a row is a record
iff its score >= bound before the step - 2.5e-3.  Two schedules:
  one slice   the whole map in one workgroup per query block (the figures the feature request quotes);
  launches    what vfm_match_ip_topk launches: 16 chunks in one slice, then launches of three times the chunks already done, each
              sliced by choose_slices, every query's bound set to the k-th best score of the prefix between two launches
              (match_topk_bound_kernel) -- with the PESSIMISTIC assumption that the slices of a launch learn nothing from each other
              (on the device they also read each other's bound).
No GPU is involved: this is arithmetic on the schedule, not a measurement.
"""
from __future__ import annotations

import numpy as np

WINDOW = np.float32(2.5e-3)
SEED_CHUNKS = 16


def choose_slices(nqb: int, nchunks: int) -> int:
    """csrc/match_api.hip, choose_slices (factory settings)."""
    best_s, best_eff = 1, -1.0
    smax = min(nchunks, 64)

    def eff_of(s):
        total = nqb * s
        rounds = (total + 255) // 256
        return total / (rounds * 256), rounds

    for s in range(1, smax + 1):
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


def launches(n: int, m: int, d: int = 128):
    """[(first chunk, chunks, slices)] of the coarse pass."""
    nqb = (n + 255) // 256 * (2 if wide(d) else 1)
    total = (m + 255) // 256 * 2
    out, done = [], 0
    while done < total:
        take = min(total - done, 3 * done if done else SEED_CHUNKS)
        out.append((done, take, choose_slices(nqb, take) if done else 1))
        done += take
    return out


def walk(scores: np.ndarray, rows: np.ndarray, k: int, start: np.ndarray, step: int = 32):
    """One lane per query over `rows` in steps of `step` of its rows: (records per query, final bound)."""
    n = scores.shape[0]
    L = np.full((n, k), -np.inf, np.float32)
    tau = start.copy()
    count = np.zeros(n, np.int64)
    for s0 in range(0, len(rows), step):
        x = scores[:, rows[s0:s0 + step]]
        rec = x >= (tau - WINDOW)[:, None]
        count += rec.sum(1)
        L = -np.sort(-np.concatenate([L, np.where(rec, x, -np.inf)], 1), axis=1)[:, :k]
        tau = np.maximum(tau, L[:, -1])
    return count, tau


def simulate(scores: np.ndarray, k: int, schedule, step: int = 32):
    n, m = scores.shape
    half = ((np.arange(m) % 32) >> 2) & 1
    pub = np.full(n, -np.inf, np.float32)
    count = np.zeros(n, np.int64)
    for c0, nch, ns in schedule:
        nxt = pub.copy()
        for s in range(ns):
            lo, hi = (c0 + s * nch // ns) * 128, min((c0 + (s + 1) * nch // ns) * 128, m)
            for h in (0, 1):
                rows = np.arange(lo, hi)[half[lo:hi] == h]
                c, t = walk(scores, rows, k, pub, step)
                count += c
                nxt = np.maximum(nxt, t)
        pub = nxt
        end = min((c0 + nch) * 128, m)
        if len(schedule) > 1 and end >= k:   # match_topk_bound_kernel: the k-th best score of the prefix, from the records
            pub = np.maximum(pub, -np.partition(-scores[:, :end], k - 1, axis=1)[:, k - 1])
    return count


def rows_of(n, m, d, common, rng):
    q = rng.standard_normal((n, d)).astype(np.float32)
    b = rng.standard_normal((m, d)).astype(np.float32)
    if common:
        c = (2 * rng.standard_normal(d)).astype(np.float32)
        q, b = q + c, b + c
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    return q, b


def main():
    cases = [("Gaussian", 257, 4097, 128, 8, False), ("Gaussian", 257, 4097, 384, 8, False), ("Gaussian", 64, 20000, 128, 8, False),
             ("Gaussian", 64, 20000, 128, 2, False), ("common", 257, 4097, 384, 8, True), ("common", 64, 20000, 128, 8, True),
             ("Gaussian", 64, 200000, 128, 8, False), ("common", 64, 200000, 128, 8, True),
             ("Gaussian", 257, 4097, 640, 8, False), ("common", 257, 4097, 640, 8, True), ("Gaussian", 257, 4097, 768, 8, False),
             ("common", 257, 4097, 768, 8, True), ("Gaussian", 129, 300, 768, 8, False), ("common", 129, 300, 768, 8, True),
             ("Gaussian", 64, 200000, 768, 8, False), ("common", 64, 200000, 768, 8, True)]
    print("| Data | N x M x d | k | one slice: mean | max | launches: mean | max | launches (chunks x slices) |")
    print("|---|---|---|---|---|---|---|---|")
    for name, n, m, d, k, common in cases:
        q, b = rows_of(n, m, d, common, np.random.default_rng(0))
        scores = q @ b.T
        step = 16 if wide(d) else 32   # a lane's rows of a step
        one = simulate(scores, k, [(0, (m + 255) // 256 * 2, 1)], step)
        sched = launches(n, m, d)
        many = simulate(scores, k, sched, step)
        print(f"| {name} | {n} x {m} x {d} | {k} | {one.mean():.0f} | {one.max()} | {many.mean():.0f} | {many.max()} | "
              + " ".join(f"{c}x{s}" for _, c, s in sched) + " |")


if __name__ == "__main__":
    main()

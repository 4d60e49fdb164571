#!/usr/bin/env python
"""TEASER++ registration (csrc/teaser.hip, csrc/teaser_host.cpp, ``vfmreg.teaser``) timed stage by stage on one device.

    python tools/time_teaser.py [--out profiles/teaser_timing.md] [--cases 2000:200,8192:2048]

One child process per case ``N:inliers`` under ``timeout``.  The correspondences are the planted scenes of tests/teaser_oracle.py
(N = 2000 with 10 % inliers: the real data's correspondence counts are a few hundred to about 2000; N = 8192 with 25 %).  Stages, each
alone: the consistency graph, the reduction, the read-back of {h, kept}, the sub-matrix and its read-back, the host's exact clique
search, GNC-TLS, the read-back of its results, the host's translation; and the whole ``solve_rows``.  Comparisons on the same
correspondences: the Python oracle on the same host (its graph, its clique search on the reduced graph, its GNC-TLS and translation),
and the RANSAC solve ``ransac_registration`` makes (``ops.ransac_corr``, 50 000 iterations, the reference's 10 000 m).

Times are host clocks around calls that end in a device synchronise: medians of ten calls after three untimed ones (the oracle: once).
"""
import argparse
import sys
import time
from pathlib import Path

from _timing import med_of, run_steps, timed, write_report, write_step

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
sys.path.insert(0, str(ROOT))

LIMIT_S = 400
RANSAC_ITERATIONS = 50000


def host_ms(fn, reps=5):
    ts, r = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return sorted(ts)[len(ts) // 2], r


def step(case):
    import numpy as np
    import torch
    from tests import teaser_oracle as to
    from vfmreg import ops, teaser
    n, inliers = (int(x) for x in case.split(":"))
    src_h, tgt_h, T, inl = to.planted_scene(n, inliers, seed=0)
    src, tgt = (torch.from_numpy(a).cuda() for a in (src_h, tgt_h))
    res = dict(n=n, inliers=inliers)
    res["graph_ms"], _, (adj, deg) = med_of(lambda: ops.teaser_graph(src, tgt, 0.2))
    res["edges"] = int(deg.sum().item()) // 2
    res["reduce_ms"], _, (kept, info) = med_of(lambda: ops.teaser_reduce(adj, deg))
    res["readback1_ms"], _, hk = med_of(lambda: info.cpu().numpy())
    h, k = int(hk[0]), int(hk[1])
    res["h"], res["kept"] = h, k
    kept = kept[:k].contiguous()
    res["submatrix_ms"], _, sub = med_of(lambda: ops.teaser_submatrix(adj, kept))
    res["readback2_ms"], _, packed = med_of(lambda: torch.cat((kept.to(torch.int64), sub.reshape(-1))).cpu().numpy())
    res["clique_host_ms"], clique = host_ms(lambda: ops.teaser_max_clique_host(packed[k:], packed[:k].astype(np.int32), known=h))
    res["clique"] = len(clique)
    cl = torch.from_numpy(clique).cuda()
    res["gnc_ms"], _, (R, w, it, v) = med_of(lambda: ops.teaser_gnc(src, tgt, cl, 0.2))
    res["gnc_iterations"] = int(it.item())
    res["readback3_ms"], _, out = med_of(lambda: torch.cat((R.reshape(-1), w, v.reshape(-1), it.to(torch.float64))).cpu().numpy())
    vh = v.cpu().numpy()
    res["translation_host_ms"], (t, _) = host_ms(lambda: ops.teaser_tls_translation_host(vh, 0.2))
    p = teaser.RobustRegistrationSolver.Params()
    p.noise_bound, p.estimate_scaling, p.rotation_max_iterations, p.rotation_cost_threshold = 0.2, False, 10000, 1e-16
    solver = teaser.RobustRegistrationSolver(p)
    res["solve_ms"], res["solve_min_ms"], sol = med_of(lambda: solver.solve_rows(src, tgt))
    res["rre_deg"], res["rte_m"] = to.errors(sol.rotation, sol.translation, T)
    # the RANSAC solve of ransac_registration on the same correspondences
    corres = torch.arange(n, dtype=torch.int32, device=src.device).repeat_interleave(2).reshape(n, 2).contiguous()
    res["ransac_ms"], _, r = med_of(lambda: ops.ransac_corr(src, tgt, corres, 10000.0, RANSAC_ITERATIONS), reps=5, warm=2)
    Tr = r["T"].cpu().numpy()
    res["ransac_rre_deg"], res["ransac_rte_m"] = to.errors(Tr[:3, :3], Tr[:3, 3], T)
    # the oracle on the same host
    sys.setrecursionlimit(20000)
    t0 = time.perf_counter()
    want_adj = to.graph(src_h, tgt_h)
    res["oracle_graph_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    want_clique = to.max_clique_reduced(want_adj)
    res["oracle_clique_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    wR, ww, wit, wv = to.gnc_tls(src_h, tgt_h, want_clique)
    res["oracle_gnc_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    wt, _ = to.tls_translation(wv)
    res["oracle_translation_ms"] = 1e3 * (time.perf_counter() - t0)
    res["oracle_ms"] = res["oracle_graph_ms"] + res["oracle_clique_ms"] + res["oracle_gnc_ms"] + res["oracle_translation_ms"]
    res["equal_to_oracle"] = bool(np.array_equal(clique, want_clique) and np.array_equal(sol.rotation, wR) and np.array_equal(sol.translation, wt)
                                  and np.array_equal(adj.cpu().numpy().view(np.uint64), to.pack(want_adj)))
    return res


def render(res, box):
    L = ["# TEASER++ registration, stage by stage: `tools/time_teaser.py`", "", box, "",
         "| N | inliers | edges | h | kept | clique | graph ms | reduction ms | read-back 1 ms | sub-matrix ms | read-back 2 ms | host search ms | "
         "GNC-TLS ms (iterations) | read-back 3 ms | host translation ms | whole solve ms (min) | RRE deg | RTE m | RANSAC ms | RANSAC RRE deg | "
         "RANSAC RTE m | oracle ms (graph / clique / GNC / translation) | equal to the oracle |", "|" + "---|" * 23]
    for name in sorted(res, key=lambda c: int(c.split(":")[0])):
        r = res[name]
        L.append("| " + " | ".join(str(x) for x in [
            r["n"], r["inliers"], r["edges"], r["h"], r["kept"], r["clique"], f"{r['graph_ms']:.3f}", f"{r['reduce_ms']:.3f}", f"{r['readback1_ms']:.3f}",
            f"{r['submatrix_ms']:.3f}", f"{r['readback2_ms']:.3f}", f"{r['clique_host_ms']:.3f}", f"{r['gnc_ms']:.3f} ({r['gnc_iterations']})",
            f"{r['readback3_ms']:.3f}", f"{r['translation_host_ms']:.3f}", f"{r['solve_ms']:.3f} ({r['solve_min_ms']:.3f})", f"{r['rre_deg']:.4f}",
            f"{r['rte_m']:.4f}", f"{r['ransac_ms']:.3f}", f"{r['ransac_rre_deg']:.4f}", f"{r['ransac_rte_m']:.4f}",
            f"{r['oracle_ms']:.0f} ({r['oracle_graph_ms']:.0f} / {r['oracle_clique_ms']:.0f} / {r['oracle_gnc_ms']:.0f} / {r['oracle_translation_ms']:.0f})",
            "yes" if r["equal_to_oracle"] else "NO"]) + " |")
    L += ["", "Planted scenes of tests/teaser_oracle.py (seed 0).  Medians of host clocks around calls that end in a device synchronise, ten calls",
          f"after three untimed ones; the host stages five calls; the oracle once.  RANSAC: `ops.ransac_corr`, {RANSAC_ITERATIONS} iterations, 10 000 m,",
          "five calls after two.  The stages are timed each alone, so their sum is not the whole solve (which also allocates its outputs)."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--json")
    ap.add_argument("--cases", default="2000:200,8192:2048")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "teaser_timing.md"))
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "needs a ROCm device"
        write_step(Path(a.json), step(a.step), show=600)
        return 0
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    rc, res, box = run_steps(Path(__file__).resolve(), out, tuple((c, LIMIT_S) for c in a.cases.split(",")))
    if res:
        write_report(out, render(res, box), dict(box=box, **res))
    return rc


if __name__ == "__main__":
    sys.exit(main())

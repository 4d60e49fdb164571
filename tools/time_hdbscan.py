#!/usr/bin/env python
"""Exact HDBSCAN* (csrc/hdbscan.hip, csrc/hdbscan_host.cpp, ``vfmreg.clustering.HDBSCAN``) at (min_cluster_size, min_samples) =
(100, 25), the map filter's setting (registration_node.py:735), timed stage by stage on one device.

    python tools/time_hdbscan.py [--out profiles/hdbscan_timing.md] [--sizes 20000,50000,200000]

One child process per size under ``timeout``.  The points are the map of a structured scene of that size.  Stages: choosing the cell and
building the grid, the core distances (k = 25 nearest, no cap), the spanning tree (``vfm_mreach_mst``: all rounds in one call, with the
rounds that did work and the searches that read every point), the read-back and sort of the edges, the host tree.  Where sklearn has
``cluster.HDBSCAN`` it runs on the host on the same points and its labels are compared with the product's up to renumbering (the
condition of tests/test_hdbscan_oracle.py: the same number of clusters, at most 0.2 % of the points different).

The rounds are enqueued without a host synchronisation between them, so they are not timed one by one, and the cap of the walk is
not a switch, so there is no uncapped A/B.  Times are host clocks around calls that end in a device synchronise.
"""
import argparse
import sys
import time
from pathlib import Path

from _timing import med_of, run_steps, timed, write_report, write_step

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))

LIMIT_S = 500
MIN_CLUSTER_SIZE, MIN_SAMPLES = 100, 25
SKLEARN_MAX_N = 50000          # above this the host run is left out (it would take most of the step's limit)


def differing_points(a, b):
    import numpy as np
    wrong = int(np.sum((a == -1) != (b == -1)))
    both = (a != -1) & (b != -1)
    for label in np.unique(a[both]):
        theirs = b[both & (a == label)]
        wrong += len(theirs) - int(np.bincount(theirs).max())
    return wrong


def step(n):
    import numpy as np
    import torch
    from vfmreg import neighbors, ops, synth
    from vfmreg.clustering import HDBSCAN

    P = synth.make_structured_scene(max(n // 10, 100), n, seed=2)["map"][:, :3].astype(np.float32)
    pts = torch.from_numpy(np.ascontiguousarray(P, dtype=np.float64)).cuda()
    n = len(P)
    res = dict(n=n)
    res["grid_ms"], _, grid = med_of(lambda: neighbors.choose_cell(pts), reps=5, warm=2)
    res["cell"] = grid.cell
    res["core_ms"], _, knn = med_of(lambda: ops.nn3_knn(grid, pts, MIN_SAMPLES), reps=5, warm=2)
    core2 = knn[1][:, MIN_SAMPLES - 1].contiguous()
    ws = torch.empty(ops._lib.load().vfm_mreach_mst_workspace_bytes(n), dtype=torch.uint8, device=pts.device)
    res["mst_first_ms"], out = timed(lambda: ops.mreach_mst(grid, core2, want_counts=True, ws=ws))
    res["mst_ms"], res["mst_min_ms"], out = med_of(lambda: ops.mreach_mst(grid, core2, want_counts=True, ws=ws), reps=3, warm=0)
    lo, hi, w2, rounds, fb = out
    res["rounds"], res["fallbacks"] = int(rounds.item()), int(fb.item())
    t0 = time.perf_counter()
    lo, hi, w2 = lo.cpu().numpy(), hi.cpu().numpy(), w2.cpu().numpy()
    order = np.lexsort((hi, lo, w2))
    edges = (lo[order], hi[order], w2[order])
    res["sort_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    labels = ops.hdbscan_labels_host(*edges, MIN_CLUSTER_SIZE)
    res["host_tree_ms"] = 1e3 * (time.perf_counter() - t0)
    res["clusters"], res["noise"] = int(labels.max()) + 1, int(np.sum(labels == -1))
    res["fit_ms"], whole = timed(lambda: HDBSCAN(MIN_CLUSTER_SIZE, MIN_SAMPLES).fit(pts))
    assert np.array_equal(whole.labels_, labels)
    try:
        from sklearn.cluster import HDBSCAN as SkHDBSCAN
    except ImportError:
        SkHDBSCAN = None
    if SkHDBSCAN is not None and n <= SKLEARN_MAX_N:
        t0 = time.perf_counter()
        theirs = SkHDBSCAN(min_cluster_size=MIN_CLUSTER_SIZE, min_samples=MIN_SAMPLES).fit(P.astype(np.float64)).labels_
        res["sklearn_ms"] = 1e3 * (time.perf_counter() - t0)
        res["sklearn_clusters"] = int(theirs.max()) + 1
        res["sklearn_differing_points"] = differing_points(labels, theirs)
        res["sklearn_agrees"] = bool(res["sklearn_clusters"] == res["clusters"] and res["sklearn_differing_points"] <= 0.002 * n)
    return res


def render(res, box):
    L = ["# Exact HDBSCAN* at (100, 25): `tools/time_hdbscan.py`", "", box, "",
         "| n | cell | grid ms | core distances ms | tree ms (first call) | rounds | fallbacks | read-back + sort ms | host tree ms | whole `fit` ms | "
         "clusters | noise | sklearn ms | sklearn clusters | differing points | within 0.2 % |", "|" + "---|" * 16]
    for name in sorted(res, key=int):
        r = res[name]
        sk = [f"{r['sklearn_ms']:.0f}", r["sklearn_clusters"], r["sklearn_differing_points"], "yes" if r["sklearn_agrees"] else "NO"] \
            if "sklearn_ms" in r else ["not run"] * 4
        L.append("| " + " | ".join(str(v) for v in [
            r["n"], f"{r['cell']:.4g}", f"{r['grid_ms']:.2f}", f"{r['core_ms']:.2f}", f"{r['mst_ms']:.2f} ({r['mst_first_ms']:.2f})", r["rounds"],
            r["fallbacks"], f"{r['sort_ms']:.2f}", f"{r['host_tree_ms']:.2f}", f"{r['fit_ms']:.2f}", r["clusters"], r["noise"]] + sk) + " |")
    L += ["", "Medians of host clocks around calls that end in a device synchronise; the tree is the median of three calls after the first.",
          "The rounds are enqueued without a synchronise between them and are not timed one by one; the walk's cap is not a switch."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--json")
    ap.add_argument("--sizes", default="20000,50000,200000")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hdbscan_timing.md"))
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "needs a ROCm device"
        write_step(Path(a.json), step(int(a.step)), show=400)
        return 0
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    rc, res, box = run_steps(Path(__file__).resolve(), out, tuple((s, LIMIT_S) for s in a.sizes.split(",")))
    if res:
        write_report(out, render(res, box), dict(box=box, **res))
    return rc


if __name__ == "__main__":
    sys.exit(main())

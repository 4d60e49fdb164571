#!/usr/bin/env python
"""The exact 3-D k-NN query (csrc/nn3.hip, ``nn3_knn_kernel``) and the map filter on it (``vfmreg.utils.grow_deletion_set``), timed on
one device.

    python tools/time_knn3.py [--out profiles/knn3_timing.md]

One child process under ``timeout``.  The map is the 200 000-point map of a structured scene, the queries are 100 000 rows of it:

  k = 10 and k = 50 with the cap 0.5 (the two searches of registration_node.py:704-717), k = 25 without a cap (HDBSCAN's core distances),
  each at the host's choice of cell and over a sweep of points per occupied cell, against a torch brute force on the same device
  (``cdist`` in chunks of queries + ``topk``; the rows it returns are compared with the grid's) and, where they import, sklearn's
  KDTree and faiss's IndexFlatL2 on the host;
  the whole ``grow_deletion_set`` with the points above the ground as candidates, against the same steps on the brute force.

Times are host clocks around calls that end in a device synchronise (medians after untimed warm-up calls).
"""
import argparse
import json
import math
import sys
import time
from pathlib import Path

from _timing import med_of, run_steps, write_report, write_step

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))

LIMIT_S = 540
TARGETS = (1, 2, 4, 8, 16, 32, 64)
FORMS = ((10, 0.5), (50, 0.5), (25, math.inf))     # (k, max_d2)


def brute_knn(P, Q, k, chunk=2048):
    """torch on the device: (idx [nq, k], d2 [nq, k]) from cdist (no matrix-product form) in chunks of queries and topk"""
    import torch
    idx, d2 = [], []
    for s in range(0, Q.shape[0], chunk):
        d = torch.cdist(Q[s:s + chunk], P, compute_mode="donot_use_mm_for_euclid_dist")
        v, j = torch.topk(d, min(k, P.shape[0]), dim=1, largest=False)
        idx.append(j)
        d2.append(v * v)
    return torch.cat(idx), torch.cat(d2)


def rows_agree(idx, count, bidx):
    """share of the queries whose valid entries are the brute force's first entries, in order"""
    import torch
    valid = torch.arange(idx.shape[1], device=idx.device)[None, :] < count[:, None]
    return float((((idx == bidx) | ~valid).all(dim=1)).double().mean().item())


def brute_grow(xyz, cand):
    """the steps of registration_node.py:704-717 on brute_knn (float32 coordinates widened to fp64, as the stand-in searches them)"""
    import numpy as np
    import torch
    X = torch.from_numpy(np.ascontiguousarray(xyz.astype(np.float32), dtype=np.float64)).cuda()
    c = torch.from_numpy(cand).cuda()
    _, d2 = brute_knn(X[c], X[c], 10)
    c = c[((d2 > 0) & (d2 <= .5)).sum(1) >= 3]
    mask = torch.ones(len(xyz), dtype=torch.bool, device="cuda")
    mask[c] = False
    others = torch.nonzero(mask)[:, 0]
    idx, d2 = brute_knn(X[others], X[c], 50)
    joined = torch.unique(others[idx[(d2 > 0) & (d2 < .5)]])
    return torch.cat([c, joined]).cpu().numpy()


def step():
    import numpy as np
    import torch
    from vfmreg import neighbors, ops, synth, utils
    P = synth.make_structured_scene(20000, 200000, seed=2)["map"]
    rng = np.random.default_rng(0)
    rows = rng.choice(len(P), 100000, replace=False)
    Q = np.ascontiguousarray(P[rows])
    P_d, Q_d = torch.from_numpy(np.ascontiguousarray(P)).cuda(), torch.from_numpy(Q).cuda()
    out = dict(points=len(P), queries=len(Q), forms={})
    grids = {}
    for t in TARGETS:
        g = neighbors.choose_cell(P_d, float(t))
        grids[f"{t} per cell"] = g
    b_ms, _, host = med_of(lambda: neighbors.choose_cell(P_d), reps=5, warm=2)
    grids["host's choice"] = host
    out["choose_and_build_ms"] = b_ms
    for k, cap in FORMS:
        name = f"k={k}, " + ("no cap" if math.isinf(cap) else f"cap {cap}")
        bf_ms, bf_min, (bidx, bd2) = med_of(lambda: brute_knn(P_d, Q_d, k), reps=3, warm=1)
        r = dict(k=k, max_d2=None if math.isinf(cap) else cap, torch_brute_force_ms=bf_ms, torch_brute_force_min_ms=bf_min, grid={})
        for label, g in grids.items():
            q_ms, q_min, (idx, d2, count, fb) = med_of(lambda: ops.nn3_knn(g, Q_d, k, cap, want_fallbacks=True), reps=7, warm=2)
            occupied = int((g.keys[1:] != g.keys[:-1]).sum().item()) + 1
            agree = rows_agree(idx, count, bidx)
            assert agree > 0.99, f"{name} {label}: only {agree} of the rows equal the brute force's"
            r["grid"][label] = dict(cell_m=g.cell, points_per_occupied_cell=len(P) / occupied, query_ms=q_ms, query_min_ms=q_min,
                                    scanned_all_points=int(fb.item()), rows_equal_to_brute_force=agree,
                                    mean_count=float(count.double().mean().item()))
        del bidx, bd2
        sk = fa = None
        try:
            from sklearn.neighbors import KDTree
            t0 = time.perf_counter()
            tree = KDTree(P, metric="euclidean")
            t1 = time.perf_counter()
            sd, si = tree.query(Q, k=k, return_distance=True)
            sk = (1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1))
            free = ops.nn3_knn(host, Q_d, k)[0].cpu().numpy()
            r["rows_equal_to_sklearn"] = float((free == si).all(axis=1).mean())
        except ImportError:
            pass
        try:
            import faiss
            t0 = time.perf_counter()
            index = faiss.IndexFlatL2(3)
            index.add(P.astype(np.float32))
            t1 = time.perf_counter()
            index.search(Q.astype(np.float32), k)
            fa = (1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1))
        except ImportError:
            pass
        r["sklearn_host_build_query_ms"], r["faiss_host_build_query_ms"] = sk, fa
        out["forms"][name] = r
        print(name, json.dumps(r)[:1500], flush=True)
    # the whole map filter: the points above the ground (walls, roofs, cylinders) are the candidates
    cand = np.flatnonzero(P[:, 2] > 0.1)
    g_ms, g_min, (del_idx, keep_idx) = med_of(lambda: utils.grow_deletion_set(P, cand), reps=5, warm=1)
    bg_ms, bg_min, want = med_of(lambda: brute_grow(P, cand), reps=2, warm=0)
    same = bool(np.array_equal(del_idx, want))
    out["grow_deletion_set"] = dict(candidates=len(cand), deleted=len(del_idx), kept=len(keep_idx), ms=g_ms, min_ms=g_min,
                                    torch_brute_force_ms=bg_ms, torch_brute_force_min_ms=bg_min, same_rows_as_brute_force=same)
    assert len(np.setxor1d(del_idx, want)) <= 1e-3 * len(want), "grow_deletion_set and the brute force disagree"
    return out


def render(res, box):
    L = ["# The exact 3-D k-NN query and the map filter on one MI355X (`tools/time_knn3.py`)\n",
         f"Device: {box}.  Host clocks around calls that end in a device synchronise; medians (minimum in brackets) after untimed warm-up "
         f"calls.  {res['queries']} queries, rows of the {res['points']}-point map of a structured scene.  Latency- and gather-bound fp64 "
         f"work: no share of any peak is claimed.  Choosing the cell and building the grid (host's choice): {res['choose_and_build_ms']:.3f} ms.\n"]
    for name, r in res["forms"].items():
        L.append(f"## {name}\n")
        L.append("| grid | cell (m) | points per occupied cell | query (ms) | mean count | queries that scanned all points | rows equal to the brute force's |")
        L.append("|---|---|---|---|---|---|---|")
        for label, g in r["grid"].items():
            L.append(f"| {label} | {g['cell_m']:.4f} | {g['points_per_occupied_cell']:.2f} | {g['query_ms']:.3f} ({g['query_min_ms']:.3f}) | "
                     f"{g['mean_count']:.2f} | {g['scanned_all_points']} | {g['rows_equal_to_brute_force']:.6f} |")

        def host(v, what):
            return f"`{what}` on the host: " + ("not measured (does not import)" if v is None else f"build {v[0]:.1f} ms + query {v[1]:.1f} ms")
        L.append(f"\ntorch brute force on the same device (`cdist` in chunks of 2048 queries + `topk`, no cap): {r['torch_brute_force_ms']:.1f} ms "
                 f"({r['torch_brute_force_min_ms']:.1f}).  {host(r['sklearn_host_build_query_ms'], 'sklearn.neighbors.KDTree')}"
                 + (f" (rows equal to the grid's without a cap: {r['rows_equal_to_sklearn']:.6f})" if "rows_equal_to_sklearn" in r else "")
                 + f".  {host(r['faiss_host_build_query_ms'], 'faiss.IndexFlatL2')}.\n")
    g = res["grow_deletion_set"]
    L.append("## The whole `grow_deletion_set`\n")
    L.append(f"{g['candidates']} candidates of {res['points']} points (numpy in, numpy out: two uploads, two grids, k = 10 and k = 50 with the cap, "
             f"the cuts, `unique`, the downloads): {g['ms']:.2f} ms ({g['min_ms']:.2f}); {g['deleted']} rows deleted, {g['kept']} kept.  The same "
             f"steps on the torch brute force: {g['torch_brute_force_ms']:.1f} ms ({g['torch_brute_force_min_ms']:.1f}); same rows: "
             f"{g['same_rows_as_brute_force']}.\n")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "knn3_timing.md"))
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "needs a ROCm device"
        write_step(Path(a.json), step())
        return 0
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    rc, res, box = run_steps(Path(__file__).resolve(), out, (("", LIMIT_S),))
    if rc == 0:
        write_report(out, render(res[""], box), dict(box=box, **res[""]))
    return rc


if __name__ == "__main__":
    sys.exit(main())

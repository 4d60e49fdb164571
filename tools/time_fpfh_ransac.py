#!/usr/bin/env python
"""The exact 3-D 1-NN query (csrc/nn3.hip) and the whole ``ransac_registration('fpfh', run_icp=True)`` call, timed on one device.

    python tools/time_fpfh_ransac.py [--out profiles/fpfh_ransac_timing.md]

The driver runs two steps, each a child process of its own under ``timeout``; a step that fails ends the run:

  query   5000 queries (half rows of the cloud, half rows moved by a few centimetres, as voxel means are) against the 200 000-point
          map of a structured scene and against the scan's voxelised cloud (about 1200 points): the grid at 1 .. 64 points per occupied
          cell and at the host's own choice (build and query apart), sklearn.neighbors.KDTree build + query on the host where sklearn
          imports, and a torch brute force on the same device (the oracle's formula in chunks, no cdist).  Same indices everywhere.
  call    ``RegistrationNode(baseline_methods=("fpfh",)).ransac_registration(map, scan, "fpfh", True)`` on the 20 000 / 200 000
          scene (scan pre-voxelised at 0.1 m), whole and split into FPFH / matching / row recovery / RANSAC / ICP.

Times are host clocks around calls that end in a device synchronise (medians after untimed warm-up calls).
"""
import argparse
import sys
import time
from pathlib import Path

from _timing import med_of, median, run_steps, timed, write_report, write_step

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))

STEPS = (("query", 400), ("call", 400))
TARGETS = (1, 2, 4, 8, 16, 32, 64)


def brute_force(P, Q, chunk=512):
    """the oracle's formula on the device, in chunks of queries: (idx, dist)"""
    import torch
    px, py, pz = P[:, 0][None, :], P[:, 1][None, :], P[:, 2][None, :]
    idx, d2 = [], []
    for s in range(0, Q.shape[0], chunk):
        c = Q[s:s + chunk]
        dx, dy, dz = px - c[:, 0:1], py - c[:, 1:2], pz - c[:, 2:3]
        d = (dx * dx + dy * dy) + dz * dz
        m, j = d.min(dim=1)
        idx.append(j)
        d2.append(m)
    return torch.cat(idx), torch.sqrt(torch.cat(d2))


def step_query():
    import numpy as np
    import torch
    from vfmreg import neighbors, ops, synth
    from vfmreg.config import load_config
    from vfmreg.registration import RegistrationNode
    sc = synth.make_structured_scene(20000, 200000, seed=2)
    node = RegistrationNode(load_config(None, None))
    voxel_scan = node._voxel_scan(torch.from_numpy(sc["scan"]).cuda(), node.config.mapping.voxel_size).cpu().numpy()
    rng = np.random.default_rng(0)
    out = {}
    for name, cloud in (("map", sc["map"]), ("voxel_scan", voxel_scan)):
        n = len(cloud)
        rows = cloud[rng.integers(0, n, 5000)]
        Q = np.ascontiguousarray(np.r_[rows[:2500], rows[2500:] + rng.normal(0, 0.03, (2500, 3))])
        P_d, Q_d = torch.from_numpy(np.ascontiguousarray(cloud)).cuda(), torch.from_numpy(Q).cuda()
        bf_ms, bf_min, (bf_idx, bf_dist) = med_of(lambda: brute_force(P_d, Q_d), reps=7, warm=2)
        r = dict(points=n, queries=len(Q), torch_brute_force_ms=bf_ms, torch_brute_force_min_ms=bf_min, grid={})
        forms = [(f"{t} per cell", lambda t=t: neighbors.choose_cell(P_d, float(t))) for t in TARGETS]
        forms.append(("host's choice", lambda: neighbors.choose_cell(P_d)))
        for label, build in forms:
            b_ms, b_min, grid = med_of(build, reps=7, warm=2)
            q_ms, q_min, (idx, dist, fb) = med_of(lambda: ops.nn3_query(grid, Q_d, want_fallbacks=True), reps=30, warm=5)
            assert (cloud[idx.cpu().numpy()] == cloud[bf_idx.cpu().numpy()]).all(), f"{name} {label}: the grid query and the brute force disagree"
            r["same_distance_bits_as_brute_force"] = r.get("same_distance_bits_as_brute_force", True) and bool(torch.equal(dist, bf_dist))
            occupied = int((grid.keys[1:] != grid.keys[:-1]).sum().item()) + 1
            r["grid"][label] = dict(cell_m=grid.cell, points_per_occupied_cell=n / occupied, choose_and_build_ms=b_ms, query_ms=q_ms,
                                    query_min_ms=q_min, scanned_all_points=int(fb.item()))
        try:
            from sklearn.neighbors import KDTree
            sk = []
            for _ in range(5):
                t0 = time.perf_counter()
                tree = KDTree(cloud, metric="euclidean")
                t1 = time.perf_counter()
                sd, si = tree.query(Q, k=1, return_distance=True)
                sk.append((1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)))
            assert np.array_equal(sd[:, 0], dist.cpu().numpy()), "sklearn and the grid query disagree"
            r["sklearn_host_build_ms"], r["sklearn_host_query_ms"] = median([a for a, _ in sk]), median([b for _, b in sk])
        except ImportError:
            r["sklearn_host_build_ms"] = r["sklearn_host_query_ms"] = None
        out[name] = r
    return out


def step_call():
    import numpy as np
    import torch
    from vfmreg import o3d, synth
    from vfmreg.config import load_config
    from vfmreg.descriptors import extract_fpfh_features_device
    from vfmreg.icp import _grid_of, register_frame_on_grid
    from vfmreg.mapping import VoxelHashMap, get_voxel_hash_map
    from vfmreg.neighbors import KDTree
    from vfmreg.registration import (RegistrationNode, filter_recovered_rows, find_correspondences_device, orthogonalize_rotation)
    from vfmreg.voxelization import voxel_down_sample
    VoxelHashMap.quiet = True
    cfg = load_config(None, None)
    vs, sigma = cfg.mapping.voxel_size, cfg.adaptive_threshold.initial_threshold
    sc = synth.make_structured_scene(20000, 200000, seed=2)
    scan, m = voxel_down_sample(sc["scan"], .1), sc["map"]
    node = RegistrationNode(cfg, baseline_methods=("fpfh",))

    def cold():
        node.clear_map_descriptors()
        return node.ransac_registration(m, scan, "fpfh", True)
    cold_ms, cold_min, _ = med_of(cold, reps=5, warm=2)
    warm_ms, warm_min, (pose, pose_icp) = med_of(lambda: node.ransac_registration(m, scan, "fpfh", True), reps=7, warm=1)
    parts = {}

    def part(name, fn):
        ms, r = timed(fn)
        parts.setdefault(name, []).append(ms)
        return r
    for rep in range(7):
        raw = part("upload", lambda: (torch.from_numpy(np.ascontiguousarray(scan, dtype=np.float64)).cuda(), torch.from_numpy(m).cuda()))
        ds, fs = part("fpfh_scan", lambda: extract_fpfh_features_device(raw[0], .1))
        dm, fm = part("fpfh_map", lambda: extract_fpfh_features_device(raw[1], .1))
        i0, i1 = part("matching", lambda: find_correspondences_device(fs.float(), fm.float(), 5000, False))

        def recover():
            voxel_scan = node._voxel_scan(raw[0], vs)
            vhm = get_voxel_hash_map(cfg)
            vhm.add_points(m)
            mp = vhm.point_cloud_device()
            si, sd = KDTree(voxel_scan).query_device(ds[i0])
            ti, td = KDTree(mp).query_device(dm[i1])
            return voxel_scan, vhm, mp, filter_recovered_rows(si, sd, ti, td)
        voxel_scan, vhm, mp, pairs = part("row_recovery", recover)

        def ransac():
            a, b = o3d.geometry.PointCloud(), o3d.geometry.PointCloud()
            a.points = o3d.utility.Vector3dVector(o3d.utility.DeviceArray(voxel_scan))
            b.points = o3d.utility.Vector3dVector(o3d.utility.DeviceArray(mp))
            return np.array(o3d.pipelines.registration.registration_ransac_based_on_correspondence(
                a, b, o3d.utility.Vector2iVector(o3d.utility.DeviceArray(pairs.to(torch.int32))), node.max_correspondence_distance,
                criteria=o3d.pipelines.registration.RANSACConvergenceCriteria(node.ransac_iterations, 1)).transformation)
        rp = orthogonalize_rotation(part("ransac", ransac))
        refined = part("icp", lambda: register_frame_on_grid(voxel_scan, _grid_of(vhm), rp, 3 * sigma, sigma / 3))
    assert np.array_equal(rp, pose) and np.array_equal(refined, pose_icp), "the split steps and the call disagree"
    from vfmreg.registration import compute_errors
    return dict(sizes=dict(map=len(m), scan=len(scan), voxel_scan=int(voxel_scan.shape[0]), voxel_map_3d=int(mp.shape[0]),
                           surviving_pairs=int(pairs.shape[0])),
                call_ms=dict(map_features_computed=cold_ms, map_features_cached=warm_ms, map_features_computed_min=cold_min,
                             map_features_cached_min=warm_min),
                parts_ms={k: median(v[2:]) for k, v in parts.items()}, errors=dict(ransac=compute_errors(pose, sc["T_gt"]),
                                                                                  icp=compute_errors(pose_icp, sc["T_gt"])))


def render(res, box):
    L = ["# FPFH + RANSAC registration and the exact 3-D 1-NN query on one MI355X (`tools/time_fpfh_ransac.py`)\n",
         f"Device: {box}.  Host clocks around calls that end in a device synchronise; medians (minimum in brackets) after untimed "
         "warm-up calls.  5000 queries: half rows of the cloud, half rows moved by N(0, 3 cm).  Latency- and gather-bound fp64 work: no "
         "share of any peak is claimed.\n", "## The query alone\n"]
    for name in ("map", "voxel_scan"):
        r = res["query"][name]
        L.append(f"### {r['queries']} x {r['points']} ({name})\n")
        L.append("| grid | cell (m) | points per occupied cell | choose + build (ms) | query (ms) | queries that scanned all points |")
        L.append("|---|---|---|---|---|---|")
        for label, g in r["grid"].items():
            L.append(f"| {label} | {g['cell_m']:.4f} | {g['points_per_occupied_cell']:.2f} | {g['choose_and_build_ms']:.3f} | "
                     f"{g['query_ms']:.3f} ({g['query_min_ms']:.3f}) | {g['scanned_all_points']} |")
        sk = "not measured (sklearn does not import)" if r["sklearn_host_build_ms"] is None else \
            f"build {r['sklearn_host_build_ms']:.2f} ms + query {r['sklearn_host_query_ms']:.2f} ms on the host"
        L.append(f"\ntorch brute force on the same device (the oracle's formula in chunks of 512 queries): {r['torch_brute_force_ms']:.3f} ms "
                 f"({r['torch_brute_force_min_ms']:.3f}).  `sklearn.neighbors.KDTree`: {sk}.  All forms return the same points; the grid's "
                 f"distances equal sklearn's bit for bit, and torch's: {r['same_distance_bits_as_brute_force']}.\n")
    c = res["call"]
    L.append("## The whole call\n")
    L.append(f"`ransac_registration(map, scan, 'fpfh', run_icp=True)`, map {c['sizes']['map']} points, scan {c['sizes']['scan']} (pre-voxelised at "
             f"0.1 m); voxelised scan {c['sizes']['voxel_scan']}, 3-D map {c['sizes']['voxel_map_3d']}, surviving pairs {c['sizes']['surviving_pairs']}; "
             f"50 000 RANSAC iterations.  With the map's features computed: {c['call_ms']['map_features_computed']:.1f} ms "
             f"({c['call_ms']['map_features_computed_min']:.1f}); with them cached (every scan of a scene after the first): "
             f"{c['call_ms']['map_features_cached']:.1f} ms ({c['call_ms']['map_features_cached_min']:.1f}).\n")
    p = c["parts_ms"]
    L.append("| upload | FPFH, scan | FPFH, map | matching | row recovery (two voxel levels, hash map, two grids, two queries, filter) | RANSAC | ICP |")
    L.append("|---|---|---|---|---|---|---|")
    L.append(f"| {p['upload']:.2f} | {p['fpfh_scan']:.2f} | {p['fpfh_map']:.2f} | {p['matching']:.2f} | {p['row_recovery']:.2f} | {p['ransac']:.2f} | "
             f"{p['icp']:.2f} |")
    L.append(f"\n(ms, the steps run one by one with a synchronise after each; same poses as the call, bit for bit.)  Errors against the planted "
             f"pose (RTE m, RRE deg): RANSAC {c['errors']['ransac'][0]:.3f}, {c['errors']['ransac'][1]:.3f}; after ICP "
             f"{c['errors']['icp'][0]:.3f}, {c['errors']['icp'][1]:.3f}.\n")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--json")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fpfh_ransac_timing.md"))
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "needs a ROCm device"
        write_step(Path(a.json), step_query() if a.step == "query" else step_call(), show=3000)
        return 0
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    rc, res, box = run_steps(Path(__file__).resolve(), out, STEPS)
    if rc == 0:
        write_report(out, render(res, box), dict(box=box, **res))
    return rc


if __name__ == "__main__":
    sys.exit(main())

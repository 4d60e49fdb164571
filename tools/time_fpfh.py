"""Time the FPFH path (csrc/fpfh.hip) stage by stage on a structured scene: grid, search, normals, down-sample, SPFH, FPFH, and
extract_fpfh_features_device end to end, for a 20 000-point scan and a 200 000-point map; the numpy oracle (tests/fpfh_oracle.py)
on the same host for comparison.  Reports what bounds the search: the grid points each query reads and the candidates it keeps.

    python tools/time_fpfh.py [--reps 10] [--json out.json] [--no-oracle]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "vfm-registration_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def stages(pts_np, vs, reps):
    from vfmreg import descriptors, ops
    P = torch.from_numpy(pts_np).cuda()
    out = {"points": len(pts_np)}
    g = ops.fpfh_grid(P, vs * 2)
    nb = ops.fpfh_search(P, vs * 2, 30, grid=g, want_scanned=True)
    nv = ops.fpfh_normals(P, nb)
    D, DN = ops.fpfh_voxel_down_sample(P, vs, nv)
    g5 = ops.fpfh_grid(D, vs * 5)
    nb5 = ops.fpfh_search(D, vs * 5, 100, grid=g5, want_scanned=True)
    sp = ops.fpfh_spfh(D, DN, nb5)
    out["down_points"] = int(D.shape[0])
    for name, fn in [("grid_normals", lambda: ops.fpfh_grid(P, vs * 2)),
                     ("search_normals", lambda: ops.fpfh_search(P, vs * 2, 30, grid=g)),
                     ("normals", lambda: ops.fpfh_normals(P, nb)),
                     ("down_sample", lambda: ops.fpfh_voxel_down_sample(P, vs, nv)),
                     ("grid_features", lambda: ops.fpfh_grid(D, vs * 5)),
                     ("search_features", lambda: ops.fpfh_search(D, vs * 5, 100, grid=g5)),
                     ("spfh", lambda: ops.fpfh_spfh(D, DN, nb5)),
                     ("fpfh", lambda: ops.fpfh_fpfh(sp, nb5)),
                     ("end_to_end", lambda: descriptors.extract_fpfh_features_device(P, vs))]:
        med, mn = timed(fn, reps)
        out[name + "_ms"] = round(med, 4)
        out[name + "_min_ms"] = round(mn, 4)
    for tag, n in (("normals", nb), ("features", nb5)):
        sc, cnt = n["scanned"].double(), n["count"].double()
        out[f"search_{tag}_read_mean"] = round(float(sc.mean()), 1)
        out[f"search_{tag}_read_max"] = int(sc.max())
        out[f"search_{tag}_kept_mean"] = round(float(cnt.mean()), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_fpfh.py measures the GPU: no ROCm device here"
    from vfmreg import synth
    sc = synth.make_structured_scene(20000, 200000, seed=5)
    res = {"device": torch.cuda.get_device_name(0), "voxel_size": 0.1}
    for which in ("scan", "map"):
        res[which] = stages(sc[which], 0.1, a.reps)
        if not a.no_oracle:
            from tests import fpfh_oracle as fo
            t = time.perf_counter()
            fo.extract_fpfh_features(sc[which], 0.1)
            res[which]["numpy_oracle_s"] = round(time.perf_counter() - t, 3)
        print(json.dumps({which: res[which]}), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""``RegistrationNode.icp_registration`` (registration_node.py:359-394) against the composition it replaces, and the ICP grid built on the
device against the host build.

    python tools/time_icp_registration.py [--out profiles/icp_registration_timing.md]

The driver runs three steps, each a child process of its own under ``timeout``; a step that fails ends the run:

  grid    VoxelGridDevice(vhm.point_cloud(), vs) -- download, numpy argsort / unique, upload: what ``_grid_of`` ran before -- against
          VoxelGridDevice.from_device on the map's kept rows and on the raw cloud with the per-voxel cap, 200 000 and 30 000 points
  large   a 200 000-point map and a 20 000-point scan: (a) the composition of the commit before ``icp_registration`` existed --
          voxel_down_sample twice, get_voxel_hash_map + add_points, register_frame with the host-built grid (two ``point_cloud()`` calls,
          the container's replay included) -- and (b) ``icp_registration``, alternately in one process, dist 3 and 7
  small   the same at 30 000 / 3 000

Times are host clocks around calls that end in a device synchronise (medians); the poses of (a) and (b) must be equal bit for bit.
"""
import argparse
import sys
import time
from pathlib import Path

from _timing import median, run_steps, timed, write_report, write_step

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))

STEPS = (("grid", 240), ("large", 420), ("small", 240))
SIZES = {"large": (200000, 20000, 50.0), "small": (30000, 3000, 20.0)}


def scene(n_map, n_scan, half, seed):
    """seven tenths of the map a ground slab, the rest clutter above it (voxels of 1 m hold from one to over 20 points); the scan: map points seen
    from a planted pose with 0.02 m of noise; a guess 0.3 m off"""
    import numpy as np
    from vfmreg import synth
    rng = np.random.default_rng(seed)
    g = (7 * n_map) // 10
    m = np.r_[np.c_[rng.uniform(-half, half, (g, 2)), rng.uniform(0.0, 0.3, g)],
              np.c_[rng.uniform(-half, half, (n_map - g, 2)), rng.uniform(0.0, 10.0, n_map - g)]]
    m = np.ascontiguousarray(m[rng.permutation(n_map)])
    T = synth.random_pose(rng)
    T[:3, 3] *= 0.1
    pick = rng.choice(n_map, n_scan, replace=False)
    scan = np.ascontiguousarray((m[pick] - T[:3, 3]) @ T[:3, :3] + rng.normal(0, 0.02, (n_scan, 3)))
    guess = T.copy()
    guess[:3, 3] += rng.normal(0, 0.3, 3)
    return m, scan, guess


def step_grid():
    import numpy as np
    import torch
    from vfmreg.config import load_config
    from vfmreg.icp import VoxelGridDevice
    from vfmreg.mapping import VoxelHashMap, get_voxel_hash_map
    VoxelHashMap.quiet = True
    cfg = load_config(None, None)
    vs, cap = cfg.mapping.voxel_size, cfg.mapping.max_points_per_voxel
    out = {}
    for name, (n_map, n_scan, half) in SIZES.items():
        m, _, _ = scene(n_map, n_scan, half, seed=1)
        vhm = get_voxel_hash_map(cfg)
        vhm.add_points(m)
        vhm.point_cloud()                                    # (the container's order is cached from here on: not in the timings below)
        kept = vhm.point_cloud_device()
        raw = torch.from_numpy(m).cuda()
        forms = {"host": lambda: VoxelGridDevice(vhm.point_cloud(), vs),
                 "host_from_array": None,
                 "device_kept_rows": lambda: VoxelGridDevice.from_device(kept, vs),
                 "device_raw_capped": lambda: VoxelGridDevice.from_device(raw, vs, cap)}
        cloud = vhm.point_cloud()
        forms["host_from_array"] = lambda: VoxelGridDevice(cloud, vs)
        ts = {k: [] for k in forms}
        grids = {}
        for rep in range(12):
            for k, fn in forms.items():
                ms, grids[k] = timed(fn)
                if rep >= 2:
                    ts[k].append(ms)
        for k in forms:                                      # all four are the same grid
            assert torch.equal(grids[k].keys, grids["host"].keys) and torch.equal(grids[k].start, grids["host"].start)
            assert torch.equal(grids[k].pts, grids["host"].pts), k
        out[name] = dict(points=n_map, kept=int(grids["host"].pts.shape[0]), voxels=int(grids["host"].n_voxels),
                         ms={k: median(v) for k, v in ts.items()}, ms_min={k: min(v) for k, v in ts.items()})
    return out


def step_chain(name):
    import numpy as np
    import torch
    from vfmreg import icp
    from vfmreg.config import load_config
    from vfmreg.mapping import VoxelHashMap, get_voxel_hash_map
    from vfmreg.registration import RegistrationNode
    from vfmreg.voxelization import voxel_down_sample
    VoxelHashMap.quiet = True
    cfg = load_config(None, None)
    vs, sigma = cfg.mapping.voxel_size, cfg.adaptive_threshold.initial_threshold
    n_map, n_scan, half = SIZES[name]
    m, scan, guess = scene(n_map, n_scan, half, seed=2)
    node = RegistrationNode(cfg)
    iters = []
    loop = icp._icp_loop

    def counting_loop(*a, **k):
        r = loop(*a, **k)
        iters.append(r[2])
        return r
    icp._icp_loop = counting_loop

    def composition(dist, parts=None):
        """what a caller of the commit before wrote for RN:359-394, with that commit's ``_grid_of``: the grid from
        ``point_cloud()`` -- called twice, the first call replaying the container -- on the host"""
        t = time.perf_counter()
        voxel_scan = voxel_down_sample(voxel_down_sample(scan, vs * 0.5), vs * 1.0)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        vhm = get_voxel_hash_map(cfg)
        vhm.add_points(m)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        grid = (len(vhm.point_cloud()), icp.VoxelGridDevice(vhm.point_cloud(), vhm.voxel_size))[1]
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        src = torch.from_numpy(np.ascontiguousarray(voxel_scan, dtype=np.float64)).cuda()
        T_icp, _, _ = icp._icp_loop(src, grid, guess, dist * sigma, sigma / dist, icp.MAX_NUM_ITERATIONS)
        pose = T_icp @ guess
        t4 = time.perf_counter()
        if parts is not None:
            for k, v in (("scan", t1 - t), ("map", t2 - t1), ("grid", t3 - t2), ("loop", t4 - t3)):
                parts.setdefault(k, []).append(1e3 * v)
        return pose

    out = {}
    for dist in (3, 7):
        ta, tb, parts = [], [], {}
        ia = ib = None
        for rep in range(9):
            del iters[:]
            ms_a, pose_a = timed(lambda: composition(dist, parts if rep >= 2 else None))
            ia = list(iters)
            del iters[:]
            ms_b, pose_b = timed(lambda: node.icp_registration(m, scan, guess, dist=dist))
            ib = list(iters)
            assert np.array_equal(pose_a, pose_b), "icp_registration and the composition disagree"
            if rep >= 2:
                ta.append(ms_a)
                tb.append(ms_b)
        out[f"dist{dist}"] = dict(composition_ms=median(ta), icp_registration_ms=median(tb), composition_min_ms=min(ta),
                                  icp_registration_min_ms=min(tb), parts_ms={k: median(v) for k, v in parts.items()},
                                  iterations=dict(composition=ia, icp_registration=ib), all_composition_ms=ta, all_icp_registration_ms=tb)
    # the loop alone, on the kept grid (what both spend in common)
    h = node.set_map(m)
    node.icp_registration(h, scan, guess)
    th = [timed(lambda: node.icp_registration(h, scan, guess))[0] for _ in range(7)]
    out["handle_dist3_ms"] = median(th)
    out["sizes"] = dict(map=n_map, scan=n_scan)
    return out


def render(res, box):
    g, L = res["grid"], []
    L.append("# `icp_registration` and the device-built ICP grid on one MI355X (`tools/time_icp_registration.py`)\n")
    L.append(f"Device: {box}.  Host clocks around calls that end in a device synchronise; medians (grid: 10 timed builds per form, "
             "the forms alternating; chains: 7 timed calls per form after 2 untimed, (a) and (b) alternating in one process).  "
             "Maps: a ground slab (70 % of the points) under clutter; what the per-voxel cap of 20 drops is points minus kept.\n")
    L.append("## The grid build alone\n")
    L.append("| map points (kept / voxels) | host: `point_cloud()` download + numpy sort + upload | host, array already on the host | "
             "device, kept rows | device, raw cloud + cap |")
    L.append("|---|---|---|---|---|")
    for name in ("large", "small"):
        r = g[name]
        L.append(f"| {r['points']} ({r['kept']} / {r['voxels']}) | {r['ms']['host']:.3f} ms | {r['ms']['host_from_array']:.3f} ms | "
                 f"{r['ms']['device_kept_rows']:.3f} ms | {r['ms']['device_raw_capped']:.3f} ms |")
    L.append("\nAll four forms give the same `keys`, `start` and `pts` (checked in the run).\n")
    L.append("## The whole call\n")
    L.append("(a) = `voxel_down_sample` x 2, `get_voxel_hash_map` + `add_points`, `register_frame` with the host-built grid (two "
             "`point_cloud()` calls, the container's replay included) -- the composition of the commit before; (b) = "
             "`RegistrationNode.icp_registration` on the same arrays.  Equal poses, bit for bit, in every repetition.\n")
    L.append("| map / scan | dist | (a) ms (min) | (b) ms (min) | (a) parts: scan / map / grid / loop | iterations (a) / (b) |")
    L.append("|---|---|---|---|---|---|")
    for name in ("large", "small"):
        r = res[name]
        for d in ("dist3", "dist7"):
            x = r[d]
            p = x["parts_ms"]
            L.append(f"| {r['sizes']['map']} / {r['sizes']['scan']} | {d[4:]} | {x['composition_ms']:.2f} ({x['composition_min_ms']:.2f}) | "
                     f"{x['icp_registration_ms']:.2f} ({x['icp_registration_min_ms']:.2f}) | "
                     f"{p['scan']:.2f} / {p['map']:.2f} / {p['grid']:.2f} / {p['loop']:.2f} | "
                     f"{x['iterations']['composition']} / {x['iterations']['icp_registration']} |")
    L.append("")
    for name in ("large", "small"):
        L.append(f"Through a `set_map()` handle (grid kept), {res[name]['sizes']['map']} / {res[name]['sizes']['scan']}, dist 3: "
                 f"{res[name]['handle_dist3_ms']:.2f} ms.")
    L.append("")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--json")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "icp_registration_timing.md"))
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "needs a ROCm device"
        write_step(Path(a.json), step_grid() if a.step == "grid" else step_chain(a.step), show=2000)
        return 0
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    rc, res, box = run_steps(Path(__file__).resolve(), out, STEPS)
    if rc == 0:
        write_report(out, render(res, box), dict(box=box, **res))
    return rc


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python
"""The odometry front end (csrc/odometry.hip, ``vfmreg.kiss_icp``) on one device, in one session:

    python tools/time_odometry.py [--out profiles/odometry_timing.md]

``frame``: ``KissICP.register_frame`` on a stream of 120 000-point scans at the default 100 m range (voxel size 1 m) -- the whole call,
and split into upload (+ de-skew when on), crop, the two voxel levels, the ICP loop and the map update (the split run synchronises the
device between the stages).  ``update``: ``vfm_icp_grid_update`` against the rebuild made of the entry points the project had before
(move the new points, ``vfm_icp_grid_build`` of old + new with the cap, a torch mask on every voxel's first point), at maps of 100 000
and 400 000 points with 10 000 new points; the two forms alternate, 10 timed runs each after 2 untimed.  Both forms end in the read-back
of their counters.  Times are host clocks around calls that end in a device synchronise; each figure comes with its spread."""
import argparse
import sys
import time
from pathlib import Path

from _timing import median, run_steps, timed, write_report, write_step

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
sys.path.insert(0, str(ROOT))

LIMIT_S = 300
SCAN_POINTS = 120000
FRAMES = 14
WARM = 2


def world(rng, n=1500000):
    """a 500 x 260 m ground with walls along it and 400 boxes: enough structure in every direction for ICP to hold"""
    import numpy as np
    kind = rng.integers(0, 10, n)
    x = rng.uniform(-150.0, 350.0, n)
    p = np.empty((n, 3))
    g, w, b = kind < 5, (kind >= 5) & (kind < 7), kind >= 7
    p[g] = np.c_[x[g], rng.uniform(-130, 130, g.sum()), 0.05 * np.sin(0.1 * x[g])]
    side = np.where(rng.random(w.sum()) < 0.5, -1.0, 1.0)
    p[w] = np.c_[x[w], side * (60.0 + 5.0 * np.sin(0.05 * x[w] + side)), rng.uniform(0, 12, w.sum())]
    cx, cy = rng.uniform(-150, 350, 400), rng.uniform(-55, 55, 400)
    which, face, u = rng.integers(0, 400, b.sum()), rng.integers(0, 4, b.sum()), rng.uniform(-3, 3, b.sum())
    px = np.where(face < 2, np.where(face == 0, -3.0, 3.0), u)
    py = np.where(face < 2, u, np.where(face == 2, -3.0, 3.0))
    p[b] = np.c_[cx[which] + px, cy[which] + py, rng.uniform(0, 8, b.sum())]
    return p


def scans(rng, frames):
    import numpy as np
    w = world(rng)
    out = []
    for f in range(frames):
        pos = np.array([1.0 * f, 0.0, 1.8])
        near = np.flatnonzero(np.linalg.norm(w - pos, axis=1) < 105.0)
        pick = rng.choice(near, size=min(SCAN_POINTS, len(near)), replace=False)
        out.append(np.ascontiguousarray(w[pick] - pos + rng.normal(0, 0.01, (len(pick), 3))))
    return out


def frame_step():
    import numpy as np
    import torch
    from vfmreg.config import load_config
    from vfmreg.kiss_icp import KissICP
    rng = np.random.default_rng(1)
    S = scans(rng, FRAMES)
    stamps = [rng.uniform(0, 1, len(s)) for s in S]
    res = dict(points=[len(s) for s in S][:3], frames=FRAMES, warm=WARM)
    for name, deskew in (("plain", False), ("deskew", True)):
        whole, split = [], []
        for profile in (False, True):
            k = KissICP(load_config(deskew=deskew))
            k.profile = profile
            for f, (s, t) in enumerate(zip(S, stamps)):
                k.timings = {}
                ms, _ = timed(lambda: k.register_frame(s, t))
                if f >= WARM:
                    (split if profile else whole).append(dict(k.timings, total=ms * 1e-3) if profile else ms)
            torch.cuda.synchronize()
        r = dict(whole_ms=dict(median=median(whole), min=min(whole), max=max(whole)),
                 map_points=int(k.local_map.point_cloud_device().shape[0]), end_x=float(k.poses[-1][0, 3]))
        for key in ("upload_deskew", "crop", "voxel_chain", "icp", "update", "total"):
            v = [1e3 * d.get(key, 0.0) for d in split]
            r[key] = dict(median=median(v), min=min(v), max=max(v))
        res[name] = r
    return res


def update_step():
    import numpy as np
    import torch
    from vfmreg import ops
    from vfmreg.icp import VoxelGridDevice
    vs, cap, md, m = 1.0, 20, 100.0, 10000
    rng = np.random.default_rng(2)
    T = np.eye(4)
    T[:3, 3] = [3.0, 0.5, 0.0]
    T_d = torch.from_numpy(T).cuda()
    origin = T[:3, 3].copy()
    origin_d = torch.from_numpy(origin).cuda()
    res = {}
    for size in (100000, 400000):
        side = np.sqrt(size / 4.0 / 4.0)                        # a slab 4 m high with ~4 points per voxel
        half = np.array([side / 2, side / 2, 2.0])
        old = rng.uniform(-half, half, (size, 3))
        g = VoxelGridDevice.from_device(torch.from_numpy(old).cuda(), vs, cap)
        new = torch.from_numpy(rng.uniform(-half, half, (m, 3))).cuda()

        def update():
            out = ops.icp_grid_update(g.keys, g.start, g.pts, new, T, vs, cap, origin, md)
            return out, out["info"].cpu()

        def rebuild():
            moved = ops.transform_xyz(new, T_d)
            r = VoxelGridDevice.from_device(torch.cat((g.pts.reshape(-1, 3), moved)).contiguous(), vs, cap)
            start = r.start.long()
            d = r.pts.reshape(-1, 3)[start[:-1]] - origin_d
            far = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) > md * md
            sz = start[1:] - start[:-1]
            pts = r.pts.reshape(-1, 3)[torch.repeat_interleave(~far, sz)]
            return r.keys[~far], torch.cumsum(sz[~far], 0), pts, int((~far).sum().item())
        tu, tr = [], []
        for i in range(12):
            a, (out, info) = timed(update)
            b, reb = timed(rebuild)
            if i >= 2:
                tu.append(a)
                tr.append(b)
        same = bool(torch.equal(out["keys"][:int(info[0])], reb[0]) and torch.equal(out["pts"][:int(info[1])], reb[2]))
        res[str(size)] = dict(voxels=g.n_voxels, kept=g.n_kept, new=m, info=[int(v) for v in info], same_grid=same,
                              update_ms=dict(median=median(tu), min=min(tu), max=max(tu)),
                              rebuild_ms=dict(median=median(tr), min=min(tr), max=max(tr)))
    return res


def fmt(d, digits=3):
    return f"{d['median']:.{digits}f} ({d['min']:.{digits}f} - {d['max']:.{digits}f})"


def render(res, box):
    L = ["# LiDAR odometry: `tools/time_odometry.py`", "", box, "", "Median (minimum - maximum) in ms."]
    f = res.get("frame")
    if f:
        L += ["", f"`KissICP.register_frame`, scans of {f['points'][0]} points, 100 m range, 1 m voxels, {f['frames'] - f['warm']} frames timed after "
              f"{f['warm']} untimed; the split run synchronises the device between the stages.", "",
              "| run | whole call | upload (+ de-skew) | crop | voxel levels | ICP loop | map update | sum of the split run |", "|---|---|---|---|---|---|---|---|"]
        for name in ("plain", "deskew"):
            r = f[name]
            L.append(f"| {name} | {fmt(r['whole_ms'], 2)} | {fmt(r['upload_deskew'], 2)} | {fmt(r['crop'])} | {fmt(r['voxel_chain'], 2)} | "
                     f"{fmt(r['icp'], 2)} | {fmt(r['update'])} | {fmt(r['total'], 2)} |")
        L += ["", f"Local map at the end: {f['plain']['map_points']} points; the sensor moved 1 m per frame and the last pose's x is "
              f"{f['plain']['end_x']:.3f} m (plain), {f['deskew']['end_x']:.3f} m (de-skew).  The synthetic scans carry no motion distortion "
              "and their timestamps are random, so the de-skew run DISPLACES points by up to half a frame's motion: its ICP loop needs more "
              "iterations, which is what its ICP column shows; the de-skew kernel itself is inside the upload column."]
    u = res.get("update")
    if u:
        L += ["", "`vfm_icp_grid_update` (with the read-back of its counters) against the rebuild form (`vfm_transform_xyz_f64`, "
              "`vfm_icp_grid_build` of old + new with its read-back, a torch mask on the first points), 10 000 new points, the forms "
              "alternating, 10 timed runs each after 2 untimed.", "",
              "| map points | voxels | update | rebuild form | same grid |", "|---|---|---|---|---|"]
        for size, r in u.items():
            L.append(f"| {r['kept']} | {r['voxels']} | {fmt(r['update_ms'])} | {fmt(r['rebuild_ms'])} | {r['same_grid']} |")
    L += ["", "Host clocks around calls that end in a device synchronise."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--json")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "odometry_timing.md"))
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "needs a ROCm device"
        write_step(Path(a.json), frame_step() if a.step == "frame" else update_step(), show=600)
        return 0
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    rc, res, box = run_steps(Path(__file__).resolve(), out, (("frame", LIMIT_S), ("update", LIMIT_S)))
    if res:
        write_report(out, render(res, box), dict(box=box, **res))
    return rc


if __name__ == "__main__":
    sys.exit(main())

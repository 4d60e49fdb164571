#!/usr/bin/env python
"""The odometry with a local map that carries descriptors (``KissICP.register_frame(use_descriptors=True)``, ``VoxelHashMap.update`` on
387-column rows, ``vfm_rows_merge``) on one device, in one session:

    python tools/time_odometry_desc.py [--out profiles/odometry_desc_timing.md]

``frame``: ``register_frame(use_descriptors=True)`` on a stream of scans of 20 000 points x 387 float32 columns at the default 100 m range
(voxel size 1 m) -- the whole call, and split into the stages ``KissICP.profile`` gives (the split run synchronises the device between
the stages).  ``update``: ``VoxelHashMap.update`` of 5 000 new rows into wide maps of 50 000 and 200 000 rows -- alone, and followed by
the first ``search_device`` (the search operand is prepared again for the WHOLE map after every update) -- against the form it replaces:
``clear()``, ``add_points_device`` of the kept rows plus the new ones (moved by ``vfm_transform_xyz_f64``), then the first
``search_device``; that form removes no far voxel and leaves the rows in the container's order.  The forms alternate, 10 timed runs each
after 2 untimed, each from the same map.  ``merge``: ``vfm_rows_merge`` alone at those sizes with fp32 (1 536-byte) and fp64 (3 072-byte)
rows, device events around 20 launches after 3 untimed, as GB/s of rows read plus rows written against the HBM peak; ``src`` as an update
leaves it (old rows nearly in order) and as a random permutation.  Host clocks end in a device synchronise."""
import argparse
import sys
from pathlib import Path

from _timing import median, run_steps, timed, write_report, write_step

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
sys.path.insert(0, str(ROOT))

LIMIT_S = 300
SCAN_POINTS = 20000
FRAMES = 14
WARM = 2
D = 384
HBM_PEAK_GBS = 8000.0       # the specification's figure; a float4 copy reaches about 6 300 GB/s of it
MAP_ROWS = (50000, 200000)
NEW_ROWS = 5000


def descriptors(rng, world, P, phase, noise=0.02):
    import numpy as np
    return (np.cos(world @ P + phase) + rng.normal(0.0, noise, (len(world), D))).astype(np.float32)


def frame_step():
    import numpy as np
    import torch
    from time_odometry import world as make_world
    from vfmreg.config import load_config
    from vfmreg.kiss_icp import KissICP
    from vfmreg.mapping import VoxelHashMap
    VoxelHashMap.quiet = True
    rng = np.random.default_rng(1)
    w = make_world(rng)
    P, phase = rng.normal(0.0, 0.6, (3, D)), rng.uniform(0.0, 2.0 * np.pi, D)
    S = []
    for f in range(FRAMES):
        pos = np.array([1.0 * f, 0.0, 1.8])
        near = np.flatnonzero(np.linalg.norm(w - pos, axis=1) < 105.0)
        pick = rng.choice(near, size=min(SCAN_POINTS, len(near)), replace=False)
        local = (w[pick] - pos + rng.normal(0, 0.01, (len(pick), 3))).astype(np.float32)
        S.append(np.ascontiguousarray(np.c_[local, descriptors(rng, w[pick], P, phase)]))
    stamps = [rng.uniform(0, 1, len(s)) for s in S]
    res = dict(points=len(S[0]), columns=int(S[0].shape[1]), dtype=str(S[0].dtype), frames=FRAMES, warm=WARM)
    whole, split = [], []
    for profile in (False, True):
        k = KissICP(load_config())
        k.profile = profile
        for f, (s, t) in enumerate(zip(S, stamps)):
            k.timings = {}
            ms, _ = timed(lambda: k.register_frame(s, t, use_descriptors=True))
            if f >= WARM:
                (split if profile else whole).append(dict(k.timings, total=ms * 1e-3) if profile else ms)
        torch.cuda.synchronize()
    res["whole_ms"] = dict(median=median(whole), min=min(whole), max=max(whole))
    res["map_rows"] = int(k.local_map.point_cloud_device().shape[0])
    res["end_x"] = float(k.poses[-1][0, 3])
    for key in ("upload_deskew", "crop", "voxel_chain", "icp", "download", "update", "total"):
        v = [1e3 * d.get(key, 0.0) for d in split]
        res[key] = dict(median=median(v), min=min(v), max=max(v))
    return res


def snapshot_of(d):
    """a copy of a map's state (the tensors are shared: an update replaces them, it does not write into them)"""
    c = dict(d)
    c["_chunks"] = {k: list(v) for k, v in d["_chunks"].items()}
    c["_ordered"] = dict(d["_ordered"])
    return c


def restore(m, d):
    m.__dict__.clear()
    m.__dict__.update(snapshot_of(d))


def update_step():
    import numpy as np
    import torch
    from vfmreg import ops
    from vfmreg.mapping import VoxelHashMap
    VoxelHashMap.quiet = True
    vs, cap, md = 1.0, 20, 100.0
    rng = np.random.default_rng(2)
    T = np.eye(4)
    T[:3, 3] = [3.0, 0.5, 0.0]
    T_d = torch.from_numpy(T).cuda()
    res = {}
    for size in MAP_ROWS:
        side = np.sqrt(size / 4.0 / 4.0)                        # a slab 4 m high with ~4 points per voxel
        half = np.array([side / 2, side / 2, 2.0])
        old = np.c_[rng.uniform(-half, half, (size, 3)), rng.normal(size=(size, D))].astype(np.float32)
        new = torch.from_numpy(np.c_[rng.uniform(-half, half, (NEW_ROWS, 3)), rng.normal(size=(NEW_ROWS, D))].astype(np.float32)).cuda()
        vhm = VoxelHashMap(vs, md, cap)
        vhm.update(torch.from_numpy(old).cuda())
        base = snapshot_of(vhm.__dict__)
        kept = torch.cat((vhm._chunks["n"][0][1].float(), vhm._chunks["n"][0][0]), dim=1).contiguous()     # [n, 387] fp32, the grid's order
        q = (kept[torch.randperm(len(kept), device="cuda")[:500], 3:] + 0.05 * torch.randn(500, D, device="cuda")).contiguous()

        def update():
            restore(vhm, base)
            vhm.update(new, T)

        def update_search():
            update()
            return vhm.search_device(None, 0.8, q_desc=q)[0].shape[0]

        def rebuild_search():
            m = VoxelHashMap(vs, md, cap)
            m.clear()
            moved = torch.cat((ops.transform_xyz(new[:, :3].double().contiguous(), T_d).float(), new[:, 3:]), dim=1)
            rows = torch.cat((kept, moved))
            m.add_points_device(rows, rows[:, :3].double().contiguous())
            return m.search_device(None, 0.8, q_desc=q)[0].shape[0]
        ts = {"update": [], "update_search": [], "rebuild_search": []}
        pairs = {}
        for i in range(12):
            for name, fn in (("update", update), ("update_search", update_search), ("rebuild_search", rebuild_search)):
                ms, r = timed(fn)
                pairs[name] = r
                if i >= 2:
                    ts[name].append(ms)
        res[str(size)] = dict(kept=int(len(kept)), voxels=int(base["_wide_grid"].n_voxels), new=NEW_ROWS, rows_after=int(vhm._wide_grid.n_kept),
                              last_update=vhm.last_update, pairs_update=pairs["update_search"], pairs_rebuild=pairs["rebuild_search"],
                              **{k + "_ms": dict(median=median(v), min=min(v), max=max(v)) for k, v in ts.items()})
    return res


def merge_step():
    import torch
    from vfmreg import ops
    res = {}
    for size in MAP_ROWS:
        for dtype, name in ((torch.float32, "fp32"), (torch.float64, "fp64")):
            old = torch.randn(size, D, device="cuda", dtype=dtype)
            new = torch.randn(NEW_ROWS, D, device="cuda", dtype=dtype)
            n = size + NEW_ROWS
            out = torch.empty(n, D, device="cuda", dtype=dtype)
            count = torch.tensor([n], dtype=torch.int32, device="cuda")
            # as an update leaves it: the old rows in order, a new row after every (size / NEW_ROWS) of them; and a random permutation
            pos = torch.arange(n, device="cuda")
            is_new = (pos % (n // NEW_ROWS)) == (n // NEW_ROWS - 1)
            ordered = torch.where(is_new, size + torch.cumsum(is_new.int(), 0) - 1, torch.cumsum((~is_new).int(), 0) - 1).int().contiguous()
            assert int(ordered.max()) == n - 1 and len(torch.unique(ordered)) == n
            for src_name, src in (("ordered", ordered), ("permuted", torch.randperm(n, device="cuda").int().contiguous())):
                for _ in range(3):
                    ops.rows_merge(old, new, src, count, out=out)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(20):
                    ops.rows_merge(old, new, src, count, out=out)
                b.record()
                torch.cuda.synchronize()
                ms = a.elapsed_time(b) / 20
                same = bool(torch.equal(out, torch.cat((old, new))[src.long()]))
                moved = 2 * n * D * old.element_size()
                res[f"{size}_{name}_{src_name}"] = dict(rows=n, row_bytes=D * old.element_size(), ms=ms, gbs=moved / ms * 1e-6,
                                                        share_of_peak=moved / ms * 1e-6 / HBM_PEAK_GBS, same=same)
    return res


def fmt(d, digits=3):
    return f"{d['median']:.{digits}f} ({d['min']:.{digits}f} - {d['max']:.{digits}f})"


def render(res, box):
    L = ["# Odometry with a local map that carries descriptors: `tools/time_odometry_desc.py`", "", box, "", "Median (minimum - maximum) in ms."]
    f = res.get("frame")
    if f:
        L += ["", f"`KissICP.register_frame(use_descriptors=True)`, scans of {f['points']} points x {f['columns']} {f['dtype']} columns, 100 m "
              f"range, 1 m voxels, {f['frames'] - f['warm']} frames timed after {f['warm']} untimed; the split run synchronises the device between "
              "the stages.", "",
              "| whole call | upload | crop | voxel levels | descriptor-seeded RegisterFrame | download of frame_downsample | map update | sum of the split run |",
              "|---|---|---|---|---|---|---|---|",
              f"| {fmt(f['whole_ms'], 2)} | {fmt(f['upload_deskew'], 2)} | {fmt(f['crop'])} | {fmt(f['voxel_chain'], 2)} | {fmt(f['icp'], 2)} | "
              f"{fmt(f['download'], 2)} | {fmt(f['update'])} | {fmt(f['total'], 2)} |",
              "", f"Local map at the end: {f['map_rows']} rows; the sensor moved 1 m per frame and the last pose's x is {f['end_x']:.3f} m.  The "
              "RegisterFrame column holds the descriptor search, and with it the preparation of the search operand for the WHOLE map: the update "
              "invalidates it, so it is made again every frame (incremental preparation is not built)."]
    u = res.get("update")
    if u:
        L += ["", f"`VoxelHashMap.update` of {NEW_ROWS} new 387-column float32 rows (`vfm_icp_grid_update_src` + `vfm_rows_merge` + the 6-int "
              "read-back), alone and followed by the first `search_device` of 500 queries, against `clear()` + `add_points_device` of the kept and "
              "the new rows + the first `search_device` (no far voxel removed, rows in the container's order).  Both searches prepare the operand "
              "of the whole map.", "",
              "| map rows | voxels | update | update + first search | rebuild + first search | pairs (update / rebuild) |", "|---|---|---|---|---|---|"]
        for size, r in u.items():
            L.append(f"| {r['kept']} | {r['voxels']} | {fmt(r['update_ms'])} | {fmt(r['update_search_ms'])} | {fmt(r['rebuild_search_ms'])} | "
                     f"{r['pairs_update']} / {r['pairs_rebuild']} |")
    m = res.get("merge")
    if m:
        L += ["", f"`vfm_rows_merge` alone (device events around 20 launches): bytes of rows read plus rows written over the time, against the "
              f"specification's HBM peak of {HBM_PEAK_GBS / 1000:.1f} TB/s (a float4 copy reaches about 6.3 TB/s).  At the smaller sizes the rows fit "
              "the 256 MiB last-level cache, so those figures are not HBM rates.", "",
              "| rows | row bytes | src | ms | GB/s | share of the HBM peak | equals the gather |", "|---|---|---|---|---|---|---|"]
        for key, r in m.items():
            L.append(f"| {r['rows']} | {r['row_bytes']} | {key.split('_')[-1]} | {r['ms']:.4f} | {r['gbs']:.0f} | {100 * r['share_of_peak']:.0f} % | {r['same']} |")
    L += ["", "None of these figures is gated by a test."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--json")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "odometry_desc_timing.md"))
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "needs a ROCm device"
        write_step(Path(a.json), dict(frame=frame_step, update=update_step, merge=merge_step)[a.step](), show=600)
        return 0
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    rc, res, box = run_steps(Path(__file__).resolve(), out, (("frame", LIMIT_S), ("update", LIMIT_S), ("merge", LIMIT_S)))
    if res:
        write_report(out, render(res, box), dict(box=box, **res))
    return rc


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python
"""The descriptor-weighted odometry on a device-resident local map (``descriptor_mode="weighted"``, csrc/icp_rows.hip) on one device, in one
session:

    python tools/time_odometry_weighted.py [--out profiles/odometry_weighted_timing.md]

``search``: one launch of the new search (``vfm_icp_step_nearest_rows``) against one of the search it stands beside
(``vfm_icp_step_nearest_desc``, unchanged) on the same inputs in the same process: 7 000 source points against a map of about 200 000 rows
at the cap of 20 (a slab of 50 x 50 x 4 voxels of 1 m offered 40 points a voxel), 16, 64 and 384 descriptor columns.  The rows are made in
float32; the old kernel and the new one read their fp64 image, the new one also the float32 rows themselves -- three runs on the same
values, whose ``tgt`` and ``valid`` have to be equal.  The kernels alternate, device events around every launch, 10 timed after 2 untimed.
``frame``: ``KissICP(descriptor_mode="weighted").register_frame(use_descriptors=True)`` on scans of 20 000 points x (3 + 384) and x (3 + 16)
float32 columns at the default 100 m range -- the whole call, and split into the stages ``KissICP.profile`` gives (the split run
synchronises the device between the stages); profiles/odometry_desc_timing.md has the descriptor-seeded frame at the same scans' size.
``stats``: the norms and flags of a 200 000-row map after an update of 5 000 rows, RECOMPUTED for the whole map (``vfm_icp_rows_stats``,
what ``VoxelHashMap.weighted_operand`` does) against CARRIED through the update (the statistics of the new rows alone, then
``vfm_rows_merge`` of the norms and of the flags as a second and third payload); device events around 20 rounds after 3 untimed.
Host clocks end in a device synchronise.  None of these figures is gated by a test."""
import argparse
import sys
from pathlib import Path

from _timing import median, run_steps, timed, write_report, write_step

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
sys.path.insert(0, str(ROOT))

LIMIT_S = 300
WIDTHS = (16, 64, 384)
SOURCES = 7000
SLAB = (50, 50, 4)
OFFERED = 40
CAP = 20
SCAN_POINTS = 20000
FRAMES = 12
WARM = 2
NEW_ROWS = 5000


def slab_map(width, seed):
    """a "weighted" map of about 200 000 float32 rows at the cap, made on the device"""
    import torch
    from vfmreg.mapping import VoxelHashMap
    VoxelHashMap.quiet = True
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = SLAB[0] * SLAB[1] * SLAB[2] * OFFERED
    size = torch.tensor(SLAB, dtype=torch.float32, device="cuda")
    xyz = torch.rand((n, 3), generator=g, device="cuda") * size
    rows = torch.cat((xyz, torch.randn((n, width), generator=g, device="cuda")), dim=1).contiguous()
    vhm = VoxelHashMap(1.0, 1000.0, CAP, descriptor_mode="weighted")
    vhm.update(rows)
    return vhm, g


def events_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def search_step():
    import numpy as np
    import torch
    from vfmreg import _lib, ops
    lib = _lib.load()
    res = {}
    T = np.eye(4)
    T[:3, 3] = [0.02, -0.01, 0.005]
    for width in WIDTHS:
        vhm, g = slab_map(width, width)
        grid, desc32, norm, has = vhm.weighted_operand()
        pick = torch.randperm(grid.n_kept, generator=g, device="cuda")[:SOURCES]
        src = (grid.pts[pick] + 0.1 * torch.randn((SOURCES, 3), generator=g, device="cuda", dtype=torch.float64)).contiguous()
        sdesc32 = (desc32[pick] + 0.05 * torch.randn((SOURCES, width), generator=g, device="cuda")).contiguous()
        desc64, sdesc64 = desc32.double(), sdesc32.double()
        snorm, shas = ops.icp_rows_stats(sdesc32)
        out = {k: (torch.empty_like(src), torch.empty_like(src), torch.empty(SOURCES, dtype=torch.uint8, device="cuda")) for k in ("old", "new64", "new32")}

        def old():
            moved, tgt, valid = out["old"]
            _lib.check(lib.vfm_icp_step_nearest_desc(src.data_ptr(), SOURCES, T.ctypes.data, moved.data_ptr(), sdesc64.data_ptr(), snorm.data_ptr(),
                                                     shas.data_ptr(), width, grid.keys.data_ptr(), grid.start.data_ptr(), grid.pts.data_ptr(),
                                                     desc64.data_ptr(), norm.data_ptr(), has.data_ptr(), grid.n_voxels, 1.0, 1.0, tgt.data_ptr(),
                                                     valid.data_ptr(), ops._stream()), "icp_step_nearest_desc")

        def new(name, sd, md):
            moved, tgt, valid = out[name]
            ops.icp_step_nearest_rows(src, T, sd, snorm, shas, grid.keys, grid.start, grid.pts, md, norm, has, 1.0, 1.0, src_out=moved, tgt=tgt,
                                      valid=valid)
        runs = (("old", old), ("new64", lambda: new("new64", sdesc64, desc64)), ("new32", lambda: new("new32", sdesc32, desc32)))
        ts = {k: [] for k, _ in runs}
        for i in range(12):
            for name, fn in runs:
                ms = events_ms(fn)
                if i >= 2:
                    ts[name].append(ms)
        same = all(torch.equal(out["old"][j], out[k][j]) for k in ("new64", "new32") for j in range(3))
        counts = (grid.start[1:] - grid.start[:-1]).double()
        res[str(width)] = dict(map_rows=grid.n_kept, voxels=grid.n_voxels, full_voxels=int((counts == CAP).sum()), sources=SOURCES,
                               accepted=int(out["old"][2].sum()), same=bool(same),
                               **{k + "_ms": dict(median=median(v), min=min(v), max=max(v)) for k, v in ts.items()})
    return res


def frame_step():
    import numpy as np
    import torch
    from time_odometry import world as make_world
    from vfmreg.config import load_config
    from vfmreg.kiss_icp import KissICP
    from vfmreg.mapping import VoxelHashMap
    VoxelHashMap.quiet = True
    res = {}
    for width in (384, 16):
        rng = np.random.default_rng(1)
        w = make_world(rng)
        P, phase = rng.normal(0.0, 0.6, (3, width)), rng.uniform(0.0, 2.0 * np.pi, width)
        S = []
        for f in range(FRAMES):
            pos = np.array([1.0 * f, 0.0, 1.8])
            near = np.flatnonzero(np.linalg.norm(w - pos, axis=1) < 105.0)
            pick = rng.choice(near, size=min(SCAN_POINTS, len(near)), replace=False)
            local = (w[pick] - pos + rng.normal(0, 0.01, (len(pick), 3))).astype(np.float32)
            desc = (np.cos(w[pick] @ P + phase) + rng.normal(0.0, 0.02, (len(pick), width))).astype(np.float32)
            S.append(np.ascontiguousarray(np.c_[local, desc]))
        stamps = [rng.uniform(0, 1, len(s)) for s in S]
        r = dict(points=len(S[0]), columns=int(S[0].shape[1]), dtype=str(S[0].dtype), frames=FRAMES, warm=WARM)
        whole, split = [], []
        for profile in (False, True):
            k = KissICP(load_config(), descriptor_mode="weighted")
            k.profile = profile
            for f, (s, t) in enumerate(zip(S, stamps)):
                k.timings = {}
                ms, _ = timed(lambda: k.register_frame(s, t, use_descriptors=True))
                if f >= WARM:
                    (split if profile else whole).append(dict(k.timings, total=ms * 1e-3) if profile else ms)
            torch.cuda.synchronize()
        r["whole_ms"] = dict(median=median(whole), min=min(whole), max=max(whole))
        r["map_rows"] = int(k.local_map.point_cloud_device().shape[0])
        r["end_x"] = float(k.poses[-1][0, 3])
        for key in ("upload_deskew", "crop", "voxel_chain", "icp", "download", "update", "total"):
            v = [1e3 * d.get(key, 0.0) for d in split]
            r[key] = dict(median=median(v), min=min(v), max=max(v))
        res[str(width)] = r
    return res


def stats_step():
    import torch
    from vfmreg import ops
    res = {}
    for width in (16, 384):
        vhm, g = slab_map(width, 100 + width)
        _, desc, norm, has = vhm.weighted_operand()
        nk = desc.shape[0]
        new = torch.randn((NEW_ROWS, width), generator=g, device="cuda")
        n = nk + NEW_ROWS
        count = torch.tensor([n], dtype=torch.int32, device="cuda")
        # as an update leaves it: the old rows in order, a new row after every (nk / NEW_ROWS) of them
        pos = torch.arange(n, device="cuda")
        is_new = ((pos % (n // NEW_ROWS)) == (n // NEW_ROWS - 1)) & (torch.cumsum(((pos % (n // NEW_ROWS)) == (n // NEW_ROWS - 1)).int(), 0) <= NEW_ROWS)
        src = torch.where(is_new, nk + torch.cumsum(is_new.int(), 0) - 1, torch.cumsum((~is_new).int(), 0) - 1).int().contiguous()
        assert int(src.max()) == n - 1 and len(torch.unique(src)) == n
        whole = torch.cat((desc, new))[src.long()].contiguous()          # the rows after the update
        norm_old, flag_old = norm.reshape(-1, 1), has.int().reshape(-1, 1).contiguous()
        norm_out = torch.empty((n, 1), dtype=torch.float64, device="cuda")
        flag_out = torch.empty((n, 1), dtype=torch.int32, device="cuda")
        kept = {}

        def recompute():
            kept["recomputed"] = ops.icp_rows_stats(whole)

        def carry():
            nn, nh = ops.icp_rows_stats(new)
            ops.rows_merge(norm_old, nn.reshape(-1, 1), src, count, out=norm_out)
            ops.rows_merge(flag_old, nh.int().reshape(-1, 1), src, count, out=flag_out)
        ts = dict(recompute=[], carry=[])
        for i in range(23):
            for name, fn in (("recompute", recompute), ("carry", carry)):
                ms = events_ms(fn)
                if i >= 3:
                    ts[name].append(ms)
        same = bool(torch.equal(kept["recomputed"][0], norm_out.reshape(-1)) and torch.equal(kept["recomputed"][1].int(), flag_out.reshape(-1)))
        res[str(width)] = dict(rows=n, new=NEW_ROWS, row_bytes=width * 4, same=same, map_bytes=n * width * 4,
                               **{k + "_ms": dict(median=median(v), min=min(v), max=max(v)) for k, v in ts.items()})
    return res


def fmt(d, digits=3):
    return f"{d['median']:.{digits}f} ({d['min']:.{digits}f} - {d['max']:.{digits}f})"


def render(res, box):
    L = ["# Descriptor-weighted odometry on a device-resident map: `tools/time_odometry_weighted.py`", "", box, "",
         "Median (minimum - maximum) in ms.  None of these figures is gated by a test."]
    s = res.get("search")
    if s:
        L += ["", f"One launch of the search, {SOURCES} source points, 1 m voxels, cap {CAP}, a step transform applied in the launch; device events "
              "around every launch, 10 timed after 2 untimed, the kernels alternating.  `old`: `vfm_icp_step_nearest_desc` (a lane per "
              "neighbour voxel) on fp64 rows; `new`: `vfm_icp_step_nearest_rows` (a lane per candidate) on the same fp64 rows and on the float32 "
              "rows they are the image of.", "",
              "| columns | map rows | voxels (full) | accepted | old, fp64 | new, fp64 | new, fp32 | old / new fp64 | old / new fp32 | same tgt, valid, moved |",
              "|---|---|---|---|---|---|---|---|---|---|"]
        for width, r in s.items():
            L.append(f"| {width} | {r['map_rows']} | {r['voxels']} ({r['full_voxels']}) | {r['accepted']} | {fmt(r['old_ms'])} | {fmt(r['new64_ms'])} | "
                     f"{fmt(r['new32_ms'])} | {r['old_ms']['median'] / r['new64_ms']['median']:.1f} | "
                     f"{r['old_ms']['median'] / r['new32_ms']['median']:.1f} | {r['same']} |")
    f = res.get("frame")
    if f:
        L += ["", "`KissICP(descriptor_mode=\"weighted\").register_frame(use_descriptors=True)`, float32 scans at the 100 m range, 1 m voxels, "
              f"{FRAMES - WARM} frames timed after {WARM} untimed; the split run synchronises the device between the stages.  The descriptor-seeded "
              "frame on scans of this size: profiles/odometry_desc_timing.md.", "",
              "| columns | points | whole call | upload | crop | voxel levels | weighted RegisterFrame | download of frame_downsample | map update | sum of the split run | map rows at the end |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
        for width, r in f.items():
            L.append(f"| 3 + {width} | {r['points']} | {fmt(r['whole_ms'], 2)} | {fmt(r['upload_deskew'], 2)} | {fmt(r['crop'])} | {fmt(r['voxel_chain'], 2)} | "
                     f"{fmt(r['icp'], 2)} | {fmt(r['download'], 2)} | {fmt(r['update'])} | {fmt(r['total'], 2)} | {r['map_rows']} |")
        L += ["", "The RegisterFrame column holds the statistics of the source rows and of the whole map (once per frame) and every iteration's "
              "search, normal equations and read-back."]
    t = res.get("stats")
    if t:
        L += ["", f"The map's norms and flags after an update of {NEW_ROWS} float32 rows: recomputed for the whole map (`vfm_icp_rows_stats`) against "
              "carried through the update (the statistics of the new rows, then `vfm_rows_merge` of the norms and of the flags); device events "
              "around every round, 20 timed after 3 untimed, alternating.", "",
              "| columns | rows | bytes of rows | recomputed | carried | same values |", "|---|---|---|---|---|---|"]
        for width, r in t.items():
            L.append(f"| {width} | {r['rows']} | {r['map_bytes']} | {fmt(r['recompute_ms'])} | {fmt(r['carry_ms'])} | {r['same']} |")
        diff = "; ".join(f"{r['recompute_ms']['median'] - r['carry_ms']['median']:+.3f} ms at {width} columns" for width, r in t.items())
        L += ["", f"The map recomputes (`VoxelHashMap.weighted_operand`).  Recomputed minus carried: {diff} -- against the frames above a few "
              "hundredths of a millisecond either way, so the form without a second and third payload in the update (and without their cases: "
              "mixed precision, the first update of a map `add_points` filled) is the one kept.  At 384 columns the recomputation reads the "
              f"rows at {t['384']['map_bytes'] / t['384']['recompute_ms']['median'] * 1e-9:.2f} TB/s." if "384" in t else ""]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--json")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "odometry_weighted_timing.md"))
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "needs a ROCm device"
        write_step(Path(a.json), dict(search=search_step, frame=frame_step, stats=stats_step)[a.step](), show=600)
        return 0
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    rc, res, box = run_steps(Path(__file__).resolve(), out, (("search", LIMIT_S), ("stats", LIMIT_S), ("frame", LIMIT_S)))
    if res:
        write_report(out, render(res, box), dict(box=box, **res))
    return rc


if __name__ == "__main__":
    sys.exit(main())

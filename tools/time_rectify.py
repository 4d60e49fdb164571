#!/usr/bin/env python
"""The RobotCar camera front end (csrc/camera.hip) at the rig's four frames -- stereo/centre 960 x 1280 (GBRG,
150 rows cropped) and three mono cameras of 1024 x 1024 (RGGB, 200 rows cropped) -- with seeded mosaics and a radial look-up table:

    python tools/time_rectify.py [--out profiles/rectify_timing.md]

* the fused call, ``ops.rectify_bayer`` for the rig, image_subsample 1 and 2;
* the unfused chain on the device: ``demosaic_bilinear`` -> fp64 -> ``undistort_lut`` -> the uint8 cast -> crop, per camera;
* the same chain through scipy on the host (``convolve``, ``map_coordinates``), where scipy is importable, once;
* bytes the fused call must move (mosaic read, table rows of the kept pixels read, RGB written) over its time, against 8 TB/s.

Device times are the time between two device events around ``reps`` back-to-back calls, divided by ``reps``.  One child process under
``timeout``."""
import argparse
import sys
import time
from pathlib import Path

from _timing import median, run_steps, write_report, write_step

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
sys.path.insert(0, str(ROOT))

LIMIT_S = 400
HBM_PEAK_TB_S = 8.0
RIG = (("stereo/centre", 960, 1280, "GBRG", 150), ("mono_left", 1024, 1024, "RGGB", 200), ("mono_right", 1024, 1024, "RGGB", 200),
       ("mono_rear", 1024, 1024, "RGGB", 200))


def radial_table(H, W, k1=0.08):
    """an undistorted pixel's place in the distorted frame under one radial coefficient: [H*W, 2] fp64 (x, y), some of it outside"""
    import numpy as np
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    f = 0.4 * W
    xn, yn = (xx - W / 2) / f, (yy - H / 2) / f
    s = 1.0 + k1 * (xn * xn + yn * yn)
    return np.ascontiguousarray(np.stack([(xn * s * 1.15 * f + W / 2).ravel(), (yn * s * 1.15 * f + H / 2).ravel()], 1))


def event_ms(fn, reps, warm=3):
    """milliseconds per call: device events around ``reps`` back-to-back calls (median of five such windows)"""
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return median(out), min(out)


def step(reps):
    import numpy as np
    import torch
    from tests import rectify_reference as RR
    from vfmreg import ops

    rng = np.random.default_rng(11)
    cams = []
    for name, H, W, pattern, crop in RIG:
        cfa = rng.integers(0, 256, (H, W)).astype(np.uint8)
        lut = radial_table(H, W)
        cams.append(dict(name=name, cfa=cfa, lut=lut, mosaic=torch.from_numpy(cfa).cuda(), table=torch.from_numpy(lut).cuda(), pattern=pattern,
                         crop_bottom=crop))
    res = dict(reps=reps, rig=[list(r) for r in RIG])
    outside = sum(int((~((c["lut"][:, 0] >= 0) & (c["lut"][:, 0] <= c["cfa"].shape[1] - 1) & (c["lut"][:, 1] >= 0)
                         & (c["lut"][:, 1] <= c["cfa"].shape[0] - 1))).sum()) for c in cams)
    res["table_entries_outside"] = outside / sum(c["lut"].shape[0] for c in cams)

    fused_out = {}
    for s in (1, 2):
        recs = [dict(mosaic=c["mosaic"], table=c["table"], pattern=c["pattern"], crop_bottom=c["crop_bottom"], subsample=s,
                     out=torch.empty(((c["cfa"].shape[0] - c["crop_bottom"]) // s, c["cfa"].shape[1] // s, 3), dtype=torch.uint8, device="cuda"))
                for c in cams]
        need = sum((3 * (c["cfa"].shape[0] - c["crop_bottom"]) * c["cfa"].shape[1] + 255) // 256 * 256 for c in cams) if s == 2 else 0
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
        res[f"fused_s{s}_ms"], res[f"fused_s{s}_min_ms"] = event_ms(lambda: ops.rectify_bayer(recs, ws=ws), reps)
        fused_out[s] = [r["out"].cpu().numpy() for r in recs]
        kept = sum((c["cfa"].shape[0] - c["crop_bottom"]) * c["cfa"].shape[1] for c in cams)
        nbytes = sum(c["cfa"].size for c in cams) + 16 * kept + 3 * kept
        if s == 2:
            nbytes += 3 * kept + 3 * kept // 4          # the cropped image read back, the quarter-size image written
        res[f"fused_s{s}_bytes"] = nbytes
        res[f"fused_s{s}_tb_s"] = nbytes / res[f"fused_s{s}_min_ms"] * 1e-9

    def chain():
        outs = []
        for c in cams:
            rgb = ops.undistort_lut(ops.demosaic_bilinear(c["mosaic"], c["pattern"]).double(), c["table"])
            outs.append((rgb[:c["cfa"].shape[0] - c["crop_bottom"]].to(torch.int64) & 255).to(torch.uint8))
        return outs
    res["chain_ms"], res["chain_min_ms"] = event_ms(chain, max(reps // 10, 1))
    res["chain_equals_fused"] = bool(all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(chain(), fused_out[1])))
    # a smaller frame through the numpy restatement: the whole-rig restatement takes minutes on the host
    c = cams[1]
    rows = 64
    small = RR.cast_u8(RR.undistort_lut(RR.demosaic_bilinear(c["cfa"], c["pattern"]), c["lut"]).reshape(-1, 3)[:rows * c["cfa"].shape[1]])
    res["fused_equals_restatement_rows"] = bool(np.array_equal(small, fused_out[1][1].reshape(-1, 3)[:rows * c["cfa"].shape[1]]))
    try:
        from scipy.ndimage import convolve, map_coordinates
    except ImportError:
        res["scipy_ms"] = None
        return res
    k_g = np.array([[0, 1, 0], [1, 4, 1], [0, 1, 0]]) / 4
    k_rb = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]]) / 4
    t0 = time.perf_counter()
    host = []
    for c in cams:
        H, W = c["cfa"].shape
        f = c["cfa"].astype(np.float64)
        mask = {ch: np.zeros((H, W)) for ch in "RGB"}
        for ch, (y, x) in zip(c["pattern"], [(0, 0), (0, 1), (1, 0), (1, 1)]):
            mask[ch][y::2, x::2] = 1
        dem = [convolve(f * mask["R"], k_rb), convolve(f * mask["G"], k_g), convolve(f * mask["B"], k_rb)]
        coords = c["lut"][:, 1::-1].T.reshape(2, H, W)
        und = np.stack([map_coordinates(d, coords, order=1) for d in dem], -1)
        host.append(und.astype(np.uint8)[:H - c["crop_bottom"]])
    res["scipy_ms"] = 1e3 * (time.perf_counter() - t0)
    res["scipy_equals_fused"] = bool(all(np.array_equal(a, b) for a, b in zip(host, fused_out[1])))
    return res


def render(r, box):
    L = ["# The RobotCar camera front end: `tools/time_rectify.py`", "", box, "",
         "One rig: " + ", ".join(f"{n} {h} x {w} ({p}, {c} rows cropped)" for n, h, w, p, c in r["rig"]) + f"; seeded mosaics, a radial "
         f"table with {100 * r['table_entries_outside']:.1f} % of its entries outside the frame.", "",
         "| path | ms per rig (median / minimum) |", "|---|---|",
         f"| `ops.rectify_bayer`, image_subsample 1 (one launch) | {r['fused_s1_ms']:.4f} / {r['fused_s1_min_ms']:.4f} |",
         f"| `ops.rectify_bayer`, image_subsample 2 (two launches) | {r['fused_s2_ms']:.4f} / {r['fused_s2_min_ms']:.4f} |",
         f"| unfused on the device: `demosaic_bilinear` -> fp64 -> `undistort_lut` -> cast -> crop, per camera | {r['chain_ms']:.3f} / "
         f"{r['chain_min_ms']:.3f} |",
         "| scipy on the host (`convolve`, `map_coordinates(order=1)`, `astype`, crop), one run | "
         + (f"{r['scipy_ms']:.0f} |" if r.get("scipy_ms") is not None else "scipy not importable here |"), "",
         f"The fused call must move {r['fused_s1_bytes'] / 1e6:.1f} MB at image_subsample 1 (mosaics, 16-byte table entries of the kept pixels, "
         f"RGB out): {r['fused_s1_tb_s']:.2f} TB/s at its best time, {100 * r['fused_s1_tb_s'] / HBM_PEAK_TB_S:.0f} % of the {HBM_PEAK_TB_S:.0f} "
         f"TB/s peak; {r['fused_s2_bytes'] / 1e6:.1f} MB and {r['fused_s2_tb_s']:.2f} TB/s at image_subsample 2 (the cropped image goes "
         "through the workspace).  These are rates of the call, launches included, not of a kernel; tables and mosaics of one rig "
         "fit the Infinity Cache, so repeated calls on the same buffers need not reach HBM.",
         f"Outputs: unfused chain equals the fused call: {r['chain_equals_fused']}; first rows of mono_left equal the numpy restatement: "
         f"{r['fused_equals_restatement_rows']}" + (f"; scipy's chain equals the fused call: {r['scipy_equals_fused']}" if r.get("scipy_ms") is not None
                                                    else "") + ".", "",
         f"Device events around {r['reps']} back-to-back calls ({max(r['reps'] // 10, 1)} for the unfused chain), median and minimum of five windows."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rectify_timing.md"))
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "needs a ROCm device"
        write_step(Path(a.json), step(a.reps), show=800)
        return 0
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    rc, res, box = run_steps(Path(__file__).resolve(), out, (("", LIMIT_S),))
    if res:
        write_report(out, render(res[""], box), dict(box=box, **res[""]))
    return rc


if __name__ == "__main__":
    sys.exit(main())

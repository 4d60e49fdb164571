#!/usr/bin/env python
"""The Euclidean 1-NN search on narrow rows: VFM_MATCH_EXACT, _FAST and _NARROW side by side, on one device in one process.

    python tools/time_l2_narrow.py [--out profiles/l2_narrow_timing.md]

Two inputs: the FPFH features (33 columns) of ``synth.make_structured_scene(20000, 200000, seed=2)`` -- the scene of
profiles/fpfh_ransac_timing.md, scan pre-voxelised at 0.1 m -- and tools/time_l2.py's random 5000 x 5000 x 33.  Per input and mode: the
forward direction alone and both directions (``ops.match_mutual_l2``), host clocks around calls that end in a device synchronise, median
with minimum and maximum after untimed warm-up calls.  For NARROW also the exact fp64 evaluations per query (vfm_debug_l2_narrow_evals)
and 2 n m Kp over the time of the forward CALL -- scale, map image, sweep and merge together, so a lower bound of the sweep kernel's own
rate -- against the 157.3 TFLOP/s f32 peak.  The three modes must return the same bits; the tool stops if they do not.
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

from _timing import run_steps, timed, write_report, write_step

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))

STEPS = (("", 900),)
PEAK_TF = 157.3
MODES = (("EXACT", 1), ("FAST", 0), ("NARROW", 2))


def spread(fn, reps, warm):
    ts, r = [], None
    for i in range(warm + reps):
        ms, r = timed(fn)
        if i >= warm:
            ts.append(ms)
    ts.sort()
    return dict(median=ts[len(ts) // 2], min=ts[0], max=ts[-1], reps=reps), r


def narrow_evals(a, b):
    import torch
    from vfmreg import _lib
    lib = _lib.load()
    n, m, d = a.shape[0], b.shape[0], a.shape[1]
    nn_ab = torch.empty(n, dtype=torch.int64, device="cuda")
    nn_ba = torch.empty(m, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.vfm_match_mutual_l2_workspace_bytes(n, m, d, 2, 1), dtype=torch.uint8, device="cuda")
    _lib.check(lib.vfm_match_mutual_l2(a.data_ptr(), n, b.data_ptr(), m, d, 2, nn_ab.data_ptr(), None, nn_ba.data_ptr(), ws.data_ptr(),
                                       ws.numel(), torch.cuda.current_stream().cuda_stream), "mutual_l2")
    out = (C.c_int64 * 2)()
    _lib.check(lib.vfm_debug_l2_narrow_evals(ws.data_ptr(), out), "l2_narrow_evals")
    return dict(forward_per_query=out[0] / n, reverse_per_query=out[1] / m, slices_forward=lib.vfm_debug_l2_narrow_slices(n, m),
                slices_reverse=lib.vfm_debug_l2_narrow_slices(m, n))


def measure(a, b, reps_exact, reps):
    import torch
    from vfmreg import ops
    n, m, d = a.shape[0], b.shape[0], a.shape[1]
    res, ref = dict(n=n, m=m, d=d, modes={}), None
    for name, prec in MODES:
        r = reps_exact if name == "EXACT" else reps
        fwd, out_f = spread(lambda: ops.match_mutual_l2(a, b, mutual=False, prec=prec), r, 2)
        both, out_b = spread(lambda: ops.match_mutual_l2(a, b, mutual=True, prec=prec), r, 2)
        got = (out_b[0], out_b[1], out_b[2])
        if ref is None:
            ref = got
        assert all(torch.equal(x, y) for x, y in zip(got, ref)) and torch.equal(out_f[0], ref[0]), f"{name} differs from EXACT"
        res["modes"][name] = dict(forward_ms=fwd, both_ms=both)
    # find_correspondences' mutual filter in one call: NARROW forward, the reverse direction on the n matched rows only
    res["pairs_ms"], _ = spread(lambda: ops.match_mutual_pairs(a, b), reps, 2)
    kp = (d + 1) & ~1
    res["narrow"] = narrow_evals(a, b)
    res["narrow"]["forward_call_tflops"] = 2.0 * n * m * kp / (res["modes"]["NARROW"]["forward_ms"]["median"] * 1e-3) / 1e12
    res["narrow"]["reverse_call_tflops"] = 2.0 * n * m * kp / ((res["modes"]["NARROW"]["both_ms"]["median"] -
                                                               res["modes"]["NARROW"]["forward_ms"]["median"]) * 1e-3) / 1e12
    return res


def step():
    import numpy as np
    import torch
    from vfmreg import synth
    from vfmreg.descriptors import extract_fpfh_features_device
    from vfmreg.voxelization import voxel_down_sample
    sc = synth.make_structured_scene(20000, 200000, seed=2)
    scan = voxel_down_sample(sc["scan"], .1)
    fs = extract_fpfh_features_device(torch.from_numpy(np.ascontiguousarray(scan, dtype=np.float64)).cuda(), .1)[1].float().contiguous()
    fm = extract_fpfh_features_device(torch.from_numpy(sc["map"]).cuda(), .1)[1].float().contiguous()
    out = {"fpfh": measure(fs, fm, 3, 15)}
    g = torch.Generator(device="cuda").manual_seed(1)
    a = torch.randn(5000, 33, device="cuda", generator=g)
    b = torch.randn(5000, 33, device="cuda", generator=g)
    out["random"] = measure(a, b, 7, 31)
    out["sweep"] = sweep()
    out["fpfh_sweep"] = fpfh_sweep(fs, fm)
    return out


def fpfh_sweep(fs, fm):
    """FAST against NARROW on seeded row subsets of the FPFH features: 1/64 ... 1/2 of both sets"""
    import torch
    from vfmreg import ops
    g = torch.Generator(device="cuda").manual_seed(7)
    ps, pm = torch.randperm(fs.shape[0], device="cuda", generator=g), torch.randperm(fm.shape[0], device="cuda", generator=g)
    rows = []
    for frac in (64, 32, 16, 8, 4, 2):
        a, b = fs[ps[:fs.shape[0] // frac]].contiguous(), fm[pm[:fm.shape[0] // frac]].contiguous()
        r = dict(n=a.shape[0], m=b.shape[0])
        for name, prec in MODES[1:]:
            r[name + "_forward_ms"], out = spread(lambda: ops.match_mutual_l2(a, b, mutual=False, prec=prec), 11, 2)
            r[name + "_nn"] = out[0]
        assert torch.equal(r.pop("FAST_nn"), r.pop("NARROW_nn"))
        r["pairs_ms"], _ = spread(lambda: ops.match_mutual_pairs(a, b), 11, 2)
        rows.append(r)
    return rows


SWEEP = (1000, 2000, 5000, 10000, 20000, 50000)


def sweep():
    """FAST against NARROW on random n x n x 33, n rising: where the narrow search starts to pay"""
    import torch
    from vfmreg import ops
    rows = []
    for n in SWEEP:
        g = torch.Generator(device="cuda").manual_seed(n)
        a = torch.randn(n, 33, device="cuda", generator=g)
        b = torch.randn(n, 33, device="cuda", generator=g)
        r = dict(n=n)
        for name, prec in MODES[1:]:
            r[name + "_forward_ms"], _ = spread(lambda: ops.match_mutual_l2(a, b, mutual=False, prec=prec), 21, 2)
            r[name + "_both_ms"], _ = spread(lambda: ops.match_mutual_l2(a, b, mutual=True, prec=prec), 21, 2)
        r["pairs_ms"], _ = spread(lambda: ops.match_mutual_pairs(a, b), 21, 2)
        rows.append(r)
    return rows


def render(res, box):
    L = ["# Exact Euclidean 1-NN on narrow rows: EXACT, FAST and NARROW on one MI355X (`tools/time_l2_narrow.py`)\n",
         f"Device: {box}.  One process; host clocks around `ops.match_mutual_l2` calls that end in a device synchronise (workspace allocation "
         "from torch's caching allocator included, for every mode alike); median [minimum .. maximum] after two untimed warm-up calls.  The "
         "three modes returned the same indices and distances, bit for bit.\n"]
    for key, title in (("fpfh", "FPFH features of `make_structured_scene(20000, 200000, seed=2)`, scan pre-voxelised at 0.1 m"),
                       ("random", "`tools/time_l2.py`'s random rows")):
        r = res[key]
        L.append(f"## {title}: {r['n']} x {r['m']} x {r['d']}\n")
        L.append("| mode | forward alone (ms) | both directions (ms) | calls timed |")
        L.append("|---|---|---|---|")
        for name, _ in MODES:
            f, b = r["modes"][name]["forward_ms"], r["modes"][name]["both_ms"]
            L.append(f"| {name} | {f['median']:.3f} [{f['min']:.3f} .. {f['max']:.3f}] | {b['median']:.3f} [{b['min']:.3f} .. {b['max']:.3f}] | "
                     f"{f['reps']} |")
        p = r["pairs_ms"]
        L.append(f"| `match_mutual_pairs` (NARROW forward + the reverse direction on the matched rows + the filter) | | "
                 f"{p['median']:.3f} [{p['min']:.3f} .. {p['max']:.3f}] | {p['reps']} |")
        w = r["narrow"]
        L.append(f"\nNARROW: {w['forward_per_query']:.2f} exact fp64 evaluations per query forward ({w['slices_forward']} map slices), "
                 f"{w['reverse_per_query']:.2f} per query in the reverse direction ({w['slices_reverse']}).  2 n m Kp over the forward call: "
                 f"{w['forward_call_tflops']:.1f} TFLOP/s = {100 * w['forward_call_tflops'] / PEAK_TF:.1f} % of the {PEAK_TF} TFLOP/s f32 peak; over "
                 f"the reverse direction (both minus forward): {w['reverse_call_tflops']:.1f} TFLOP/s = "
                 f"{100 * w['reverse_call_tflops'] / PEAK_TF:.1f} %.  (Whole calls -- scale, map image, sweep, merge --: lower bounds of the sweep "
                 "kernel's own rate.)\n")
    L.append("## Random n x n x 33, n rising\n")
    L.append("| n | FAST forward | NARROW forward | FAST both | NARROW both | `match_mutual_pairs` (NARROW) |")
    L.append("|---|---|---|---|---|---|")
    cell = lambda v: f"{v['median']:.3f} [{v['min']:.3f} .. {v['max']:.3f}]"
    for r in res["sweep"]:
        L.append(f"| {r['n']} | {cell(r['FAST_forward_ms'])} | {cell(r['NARROW_forward_ms'])} | {cell(r['FAST_both_ms'])} | "
                 f"{cell(r['NARROW_both_ms'])} | {cell(r['pairs_ms'])} |")
    L.append("\n(ms; 21 calls each after two warm-up calls.)\n")
    L.append("## Seeded row subsets of the FPFH features (1/64 ... 1/2 of both sets), forward alone\n")
    L.append("| n x m | FAST forward | NARROW forward | `match_mutual_pairs` (NARROW) |")
    L.append("|---|---|---|---|")
    for r in res["fpfh_sweep"]:
        L.append(f"| {r['n']} x {r['m']} | {cell(r['FAST_forward_ms'])} | {cell(r['NARROW_forward_ms'])} | {cell(r['pairs_ms'])} |")
    L.append("\n(ms; 11 calls each after two warm-up calls.)\n")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "l2_narrow_timing.md"))
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "needs a ROCm device"
        write_step(Path(a.json), step(), show=3000)
        return 0
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    rc, res, box = run_steps(Path(__file__).resolve(), out, STEPS)
    if rc == 0:
        write_report(out, render(res[""], box), dict(box=box, **res[""]))
    return rc


if __name__ == "__main__":
    sys.exit(main())

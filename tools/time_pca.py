#!/usr/bin/env python
"""Descriptor PCA and the colour gate (csrc/pca.hip, ``vfmreg.pca``, ``utils.colour_gate`` / ``filter_map_semantic``) at the map's size,
200 000 x 384 float32 rows resident on the device, against two yardsticks: ``torch.pca_lowrank(niter=4)`` plus a matmul on the same
device (what the reference runs) and the numpy oracle (tests/pca_oracle.py) on the host.

    python tools/time_pca.py [--out profiles/pca_timing.md] [--rows 200000]

Two child processes under ``timeout``: ``kernels`` (the moments, the host eigh, projection + colours, the gate, both yardsticks) and
``filter`` (the whole ``filter_map_semantic`` on a structured scene whose raised surfaces carry descriptors of their own).  The achieved
rate of the fp64 matrix instruction is derived from the Gram kernel's own time (the upper-triangle tiles it multiplies, 2 x 16 x 16 x 4
operations per instruction); its bare issue rate is what tools/probe/f64_mfma_probe.hip prints.  Times are host clocks around calls
that end in a device synchronise.
"""
import argparse
import sys
import time
from pathlib import Path

from _timing import med_of, run_steps, timed, write_report, write_step

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
sys.path.insert(0, str(ROOT))

LIMIT_S = 400
D = 384


def gram_instructions(n, d):
    """v_mfma_f64_16x16x4_f64 instructions of pca_gram_kernel: the tiles I <= J inside d, one per group of four rows -- rounded up to the
    four groups a trip of its loop takes per slab is left out (an upper bound within a few per cent at this size)"""
    tiles = -(-d // 16)
    return tiles * (tiles + 1) // 2 * -(-n // 4)


def kernels(n):
    import numpy as np
    import torch
    from tests import pca_oracle as po
    from vfmreg import ops, pca

    X = po.spectrum_data(3, n, D)
    x = torch.from_numpy(X).cuda()
    res = dict(n=n, d=D)
    lib = ops._lib.load()
    ws = torch.empty(lib.vfm_pca_moments_workspace_bytes(D), dtype=torch.uint8, device=x.device)
    res["moments_workspace_mib"] = ws.numel() / 2 ** 20
    res["moments_ms"], res["moments_min_ms"], (mean, S) = med_of(lambda: ops.pca_moments(x, ws=ws), reps=10, warm=3)
    mean_h, S_h = mean.cpu().numpy(), S.cpu().numpy()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        f = pca.fit_from_moments(mean_h, S_h, 3, n)
        ts.append(1e3 * (time.perf_counter() - t0))
    res["eigh_ms"] = sorted(ts)[2]
    res["fit_ms"], _, _ = med_of(lambda: pca.fit(x, 3), reps=5, warm=1)
    res["gram_gflop"] = 2.0 * 16 * 16 * 4 * gram_instructions(n, D) * 1e-9
    res["gram_tflops_of_moments_time"] = res["gram_gflop"] / res["moments_min_ms"]
    m_d, c_d = torch.from_numpy(f.mean_).cuda(), torch.from_numpy(f.components_).cuda()
    pws = torch.empty(lib.vfm_pca_project_workspace_bytes(), dtype=torch.uint8, device=x.device)

    def project_colours():
        y, zero, lo, hi = ops.pca_project(x, m_d, c_d, ws=pws)
        return ops.pca_colours(y, zero, lo, hi, rgb=True)
    res["project_colours_ms"], res["project_colours_min_ms"], rgb = med_of(project_colours, reps=10, warm=3)
    res["project_gb_s"] = X.nbytes / res["project_colours_min_ms"] * 1e-6
    gate = torch.tensor([[128., 128., 128.], [100., 140., 120.]], dtype=torch.float64, device=x.device)
    res["gate_ms"], res["gate_min_ms"], (idx, counts) = med_of(lambda: ops.colour_gate(rgb, gate, 50.0), reps=10, warm=3)
    res["gate_hits"] = [int(c) for c in counts.cpu()]

    # yardstick 1: what the reference runs, on this device
    def lowrank():
        mu = x.mean(0)
        xc = x - mu
        _, _, V = torch.pca_lowrank(xc, q=3, center=False, niter=4)
        return mu, V

    def lowrank_transform(mu, V):
        y = (x - mu) @ V
        y = y - y.min(0).values
        y = y / y.max(0).values
        return (y * 255.0).to(torch.uint8)
    res["torch_lowrank_fit_ms"], _, (mu, V) = med_of(lowrank, reps=5, warm=2)
    res["torch_transform_ms"], _, _ = med_of(lambda: lowrank_transform(mu, V), reps=10, warm=3)
    cos = np.abs((V.T.cpu().numpy().astype(np.float64) * f.components_).sum(1))
    res["lowrank_abs_cos"] = [float(c) for c in cos]
    # yardstick 2: the numpy oracle on the host
    t0 = time.perf_counter()
    o_mean, o_comps, _ = po.fit(X, 3)
    res["oracle_fit_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    o_rgb = po.colours(po.project_ordered(X, f.mean_, f.components_), X)
    res["oracle_project_colours_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    o_idx = po.gate(o_rgb, gate.cpu().numpy())
    res["oracle_gate_ms"] = 1e3 * (time.perf_counter() - t0)
    res["colours_equal_oracle"] = bool(np.array_equal(o_rgb, rgb.cpu().numpy()))
    got = np.concatenate([idx[c, :int(counts[c])].cpu().numpy() for c in range(2)])
    res["gate_equal_oracle"] = bool(np.array_equal(got, o_idx))
    res["max_component_diff_vs_oracle"] = float(np.abs(o_comps - f.components_).max())
    return res


def filter_step(n):
    import numpy as np
    from vfmreg import pca, synth, utils

    rng = np.random.RandomState(5)
    xyz = synth.make_structured_scene(max(n // 10, 100), n, seed=2)["map"][:, :3]
    n = len(xyz)
    raised = xyz[:, 2] > 0.5
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    coef = np.c_[4.0 * raised, xyz[:, 0] / 15.0, xyz[:, 1] / 30.0]
    local_map = np.c_[xyz, 1.0 + coef @ Q[:, :3].T + 0.01 * rng.standard_normal((n, D))].astype(np.float32)
    holder = pca.DescriptorPCA()
    rgb = holder.run_pca(local_map[:, 3:])
    remove_classes = [np.median(rgb[raised], axis=0, keepdims=True).astype(np.float32)]
    res = dict(n=n, raised=int(raised.sum()), candidates=int(len(utils.colour_gate(rgb, remove_classes[0]))))
    res["first_ms"], out = timed(lambda: utils.filter_map_semantic(local_map, holder, remove_classes, 0.5, np.random.RandomState(42)))
    res["filter_ms"], res["filter_min_ms"], out = med_of(
        lambda: utils.filter_map_semantic(local_map, holder, remove_classes, 0.5, np.random.RandomState(42)), reps=3, warm=0)
    res["kept"] = int(len(out[2]))
    res["run_pca_ms"], _, _ = med_of(lambda: holder.run_pca(local_map[:, 3:]), reps=3, warm=0)
    return res


def render(res, box):
    k, f = res.get("kernels"), res.get("filter")
    L = ["# Descriptor PCA and the colour gate: `tools/time_pca.py`", "", box, ""]
    if k:
        L += [f"{k['n']} x {k['d']} float32 rows resident on the device, three components.", "",
              "| step | this package (median / minimum ms) | torch on the same device, ms | numpy oracle on the host, ms |", "|---|---|---|---|",
              f"| `vfm_pca_moments` (mean + scatter, fp64 matrix cores) | {k['moments_ms']:.2f} / {k['moments_min_ms']:.2f} | | |",
              f"| host `eigh` of the {k['d']} x {k['d']} scatter, sign rule | {k['eigh_ms']:.2f} | | |",
              f"| `pca.fit` (both, with the read-back) | {k['fit_ms']:.2f} | {k['torch_lowrank_fit_ms']:.2f} (`mean`, `pca_lowrank(niter=4)`) | "
              f"{k['oracle_fit_ms']:.0f} |",
              f"| `vfm_pca_project` + `vfm_pca_colours` | {k['project_colours_ms']:.2f} / {k['project_colours_min_ms']:.2f} | "
              f"{k['torch_transform_ms']:.2f} (matmul, min / max, cast; fp32) | {k['oracle_project_colours_ms']:.0f} |",
              f"| `vfm_colour_gate`, two colours ({k['gate_hits']} hits) | {k['gate_ms']:.3f} / {k['gate_min_ms']:.3f} | | {k['oracle_gate_ms']:.1f} |",
              "",
              f"The Gram kernel multiplies {k['gram_gflop']:.1f} GFLOP of fp64 (upper-triangle tiles only); over the whole of `vfm_pca_moments`' "
              f"best time that is {k['gram_tflops_of_moments_time']:.2f} TFLOP/s.  The bare issue rate of `v_mfma_f64_16x16x4_f64` is what "
              "`tools/probe/f64_mfma_probe.hip` prints (`profiles/f64_mfma_probe.txt`).",
              f"Projection + colours read the rows once: {k['project_gb_s']:.0f} GB/s of row data at the best time.",
              f"Moments workspace: {k['moments_workspace_mib']:.1f} MiB.  Colours equal the oracle's under the same fit: "
              f"{k['colours_equal_oracle']}; gate equal: {k['gate_equal_oracle']}; largest component difference to the oracle's fit "
              f"{k['max_component_diff_vs_oracle']:.2g}; |cos| between this fit's components and `pca_lowrank`'s: "
              + ", ".join(f"{c:.6f}" for c in k["lowrank_abs_cos"]) + ".", ""]
    if f:
        L += [f"`utils.filter_map_semantic` on a structured scene of {f['n']} points x (3 + {D}) float32 on the host, {f['raised']} of them on "
              f"raised surfaces with descriptors of their own, {f['candidates']} candidates behind the gate, {f['kept']} rows kept: "
              f"{f['filter_ms']:.0f} ms (best {f['filter_min_ms']:.0f}, first call {f['first_ms']:.0f}), of which `run_pca` with the upload of "
              f"the rows {f['run_pca_ms']:.0f} ms.", ""]
    L += ["Medians of host clocks around calls that end in a device synchronise."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--json")
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pca_timing.md"))
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "needs a ROCm device"
        name, rows = a.step.split(":")
        write_step(Path(a.json), (kernels if name == "kernels" else filter_step)(int(rows)), show=600)
        return 0
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    rc, res, box = run_steps(Path(__file__).resolve(), out, ((f"kernels:{a.rows}", LIMIT_S), (f"filter:{a.rows}", LIMIT_S)))
    res = {name.split(":")[0]: r for name, r in res.items()}
    if res:
        write_report(out, render(res, box), dict(box=box, **res))
    return rc


if __name__ == "__main__":
    sys.exit(main())

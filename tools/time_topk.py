#!/usr/bin/env python
"""The k-best descriptor search (csrc/match_topk.hip, ``ops.match_ip_topk``) timed on one device, next to two yardsticks.

    python tools/time_topk.py [--out profiles/topk_timing.md] [--cases 2000:gaussian,2000:common,20000:gaussian,20000:common]

One child process per case ``N:data`` under ``timeout``; the run stops at the first non-zero status.  N queries among 200 000 map rows
of 384 columns (2000: the reference's query shape; 20 000: C2); ``gaussian`` rows, or ``common``: the same with a shared 2 x Gaussian
vector added to both sides (descriptors that are alike).  Per case, for k in {1, 2, 8}: ``ops.match_ip_topk(prec=FAST)`` with its
``info`` (largest record count of a query, queries decided by the all-pairs kernel, map slices).  The yardsticks, in the same process
on the same inputs:
  (a) ``ops.match_ip_top1(prec=FAST)``, the top-1 search as it stands (this change touches none of its code);
  (b) what a user does without this library: normalise, then ``(qn[i:i+2048] @ bn.T).topk(k)`` in query blocks, in torch.
The one condition: at k = 8, FAST is faster than (b) at both shapes.  The ratios FAST k = 1 : (a) and k = 8 : k = 1 are reported, not
judged: they are what the next change to this kernel is measured against.

Times are host clocks around calls that end in a device synchronise: medians of ten calls after three untimed ones.
"""
import argparse
import sys
from pathlib import Path

from _timing import med_of, run_steps, write_report, write_step

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
sys.path.insert(0, str(ROOT))

LIMIT_S = 300
M, D = 200000, 384
KS = (1, 2, 8)
BLOCK = 2048


def step(case):
    import torch
    from vfmreg import ops
    n, data = case.split(":")
    n = int(n)
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(n, D, generator=g, device="cuda")
    b = torch.randn(M, D, generator=g, device="cuda")
    if data == "common":
        c = 2 * torch.randn(D, generator=g, device="cuda")
        q, b = (q + c).contiguous(), (b + c).contiguous()
    res = dict(n=n, m=M, d=D, data=data, k={})
    ws1 = ops._ws(ops._lib.load().vfm_match_ip_top1_workspace_bytes(n, M, D, ops.FAST), q.device)
    res["top1_ms"], res["top1_min_ms"], (i1, s1) = med_of(lambda: ops.match_ip_top1(q, b, ops.FAST, ws=ws1))
    del ws1

    def torch_topk(k):
        qn, bn = torch.nn.functional.normalize(q, dim=1), torch.nn.functional.normalize(b, dim=1)
        out = [(qn[i:i + BLOCK] @ bn.T).topk(k) for i in range(0, n, BLOCK)]
        return torch.cat([o.indices for o in out]), torch.cat([o.values for o in out])

    for k in KS:
        ws = ops._ws(ops._lib.load().vfm_match_ip_topk_workspace_bytes(n, M, D, k, ops.FAST), q.device)
        ms, mn, (idx, sim, info) = med_of(lambda: ops.match_ip_topk(q, b, k, ops.FAST, ws=ws, return_info=True))
        del ws
        info = info.cpu().tolist()
        tms, tmn, (tidx, tsim) = med_of(lambda: torch_topk(k))
        r = dict(fast_ms=ms, fast_min_ms=mn, max_records=info[0], fallback=info[1], slices=info[2], torch_ms=tms, torch_min_ms=tmn,
                 # the fp32 product orders near-ties as it likes: agreement is reported, not required
                 torch_agrees=float((tidx == idx).float().mean().item()))
        if k == 1:
            r["equals_top1"] = bool(torch.equal(idx[:, 0], i1) and torch.equal(sim[:, 0], s1))
        res["k"][str(k)] = r
    return res


def render(res, box):
    L = ["# Exact k-best descriptor search: `tools/time_topk.py`", "", f"Measured on: {box}", "",
         f"N queries among {M} map rows of {D} columns.  (a) = `ops.match_ip_top1(prec=FAST)`; (b) = normalise + "
         f"`(qn[i:i+{BLOCK}] @ bn.T).topk(k)` in torch.", "",
         "| N | data | k | FAST ms (min) | largest record count | fallback queries | map slices | (a) top-1 ms | FAST : (a) | "
         "(b) torch ms (min) | (b) : FAST | rows equal to (b)'s |", "|" + "---|" * 12]
    verdict = []
    for name in sorted(res, key=lambda c: (int(c.split(":")[0]), c)):
        r = res[name]
        for k in KS:
            x = r["k"][str(k)]
            L.append("| " + " | ".join(str(v) for v in [
                r["n"], r["data"], k, f"{x['fast_ms']:.3f} ({x['fast_min_ms']:.3f})", x["max_records"], x["fallback"], x["slices"],
                f"{r['top1_ms']:.3f}", f"{x['fast_ms'] / r['top1_ms']:.3g}" if k == 1 else "", f"{x['torch_ms']:.3f} ({x['torch_min_ms']:.3f})",
                f"{x['torch_ms'] / x['fast_ms']:.1f}", f"{100 * x['torch_agrees']:.2f} %"]) + " |")
        k1, k8 = r["k"]["1"], r["k"]["8"]
        verdict.append(f"* {r['n']} x {M}, {r['data']}: k = 8 : k = 1 = {k8['fast_ms'] / k1['fast_ms']:.2f}; FAST k = 1 : (a) = "
                       f"{k1['fast_ms'] / r['top1_ms']:.3g} (column 0 equal to (a): {'yes' if k1.get('equals_top1') else 'NO'}); at k = 8 FAST is "
                       f"{k8['torch_ms'] / k8['fast_ms']:.1f} x faster than (b) -- the condition (faster than (b)) is "
                       f"{'MET' if k8['fast_ms'] < k8['torch_ms'] else 'NOT MET'}"
                       f"{'' if k8['torch_ms'] > 10 * k8['fast_ms'] else ', and the gap is below the tenfold one expects of the matrix cores'}.")
    L += [""] + verdict
    L += ["", "Medians of host clocks around calls that end in a device synchronise, ten calls after three untimed ones; every call includes",
          "the normalisation and the operand preparation of both sides (FAST and (a)) or the normalisation of both sides ((b)).  The last column",
          "is the share of (query, rank) entries where torch's fp32 product names the same map row: it orders near-ties by its own rounding."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--json")
    ap.add_argument("--cases", default="2000:gaussian,2000:common,20000:gaussian,20000:common")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "topk_timing.md"))
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "needs a ROCm device"
        write_step(Path(a.json), step(a.step), show=900)
        return 0
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    rc, res, box = run_steps(Path(__file__).resolve(), out, tuple((c, LIMIT_S) for c in a.cases.split(",")))
    if res:
        write_report(out, render(res, box), dict(box=box, **res))
    return rc


if __name__ == "__main__":
    sys.exit(main())

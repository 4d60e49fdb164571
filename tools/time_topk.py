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

``--wide`` times what came after that record instead and writes ``profiles/topk_wide_timing.md`` (the file above stays the record of
its session), again one child process per step:
  wide:N:data   the same table at 768 columns (the 4-wave coarse kernel); ``wide:2000:gaussian`` also times the all-pairs fp64 kernel
                (EXACT) once at k = 8 -- what these widths ran before.  Condition: at k = 8 FAST is faster than (b) at both sizes.
  kept:D        a kept map, 2000 queries among 200 000 rows of D columns, k = 1 and 8: ``ops.match_ip_topk`` (prepares both operands in
                every call), ``ops.match_ip_topk_prepared`` with only the queries prepared per call, and ``vfm_match_prepare`` of the map
                alone.  Condition: the prepared call is faster.  The share of the map preparation's time that the difference recovers is
                reported, not judged.
  ab:NAME       with ``--parent-lib FILE`` (libvfmreg_hip.so built from the parent commit in a directory of its own): the unprepared
                FAST call at 2000 and 20 000 x 200 000 x 384, k = 1 and 8, through the C ABI of the library file alone -- parent, this
                commit, parent again, alternately in one session.  Allowed: the difference between the parent's own two medians.

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


WIDE_D = 768
KEPT_N = 2000


def rows_on_device(n, d, data):
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(n, d, generator=g, device="cuda")
    b = torch.randn(M, d, generator=g, device="cuda")
    if data == "common":
        c = 2 * torch.randn(d, generator=g, device="cuda")
        q, b = (q + c).contiguous(), (b + c).contiguous()
    return q, b


def step_wide(case):
    import torch
    from _timing import timed
    from vfmreg import ops
    _, n, data = case.split(":")
    n, d = int(n), WIDE_D
    q, b = rows_on_device(n, d, data)
    res = dict(n=n, m=M, d=d, data=data, k={})

    def torch_topk(k):
        qn, bn = torch.nn.functional.normalize(q, dim=1), torch.nn.functional.normalize(b, dim=1)
        out = [(qn[i:i + BLOCK] @ bn.T).topk(k) for i in range(0, n, BLOCK)]
        return torch.cat([o.indices for o in out]), torch.cat([o.values for o in out])

    lib = ops._lib.load()
    for k in KS:
        ws = ops._ws(lib.vfm_match_ip_topk_workspace_bytes(n, M, d, k, ops.FAST), q.device)
        ms, mn, (idx, sim, info) = med_of(lambda: ops.match_ip_topk(q, b, k, ops.FAST, ws=ws, return_info=True))
        del ws
        info = info.cpu().tolist()
        tms, tmn, (tidx, tsim) = med_of(lambda: torch_topk(k))
        res["k"][str(k)] = dict(fast_ms=ms, fast_min_ms=mn, max_records=info[0], fallback=info[1], slices=info[2], torch_ms=tms,
                                torch_min_ms=tmn, torch_agrees=float((tidx == idx).float().mean().item()))
        if k == 8 and n == 2000 and data == "gaussian":   # one call: the all-pairs kernel is fp64 on the vector ALUs
            ems, (eidx, esim, _) = timed(lambda: ops.match_ip_topk(q, b, k, ops.EXACT, return_info=True))
            res["exact_ms"] = ems
            res["exact_equal"] = bool(torch.equal(eidx, idx) and torch.equal(esim, sim))
    return res


def step_kept(case):
    import torch
    from vfmreg import ops
    d = int(case.split(":")[1])
    n = KEPT_N
    q, b = rows_on_device(n, d, "gaussian")
    lib = ops._lib.load()
    res = dict(n=n, m=M, d=d, k={})
    bp = ops.PreparedRows(b)
    res["prepare_map_ms"], res["prepare_map_min_ms"], _ = med_of(bp.refresh)
    res["prepare_queries_ms"], _, _ = med_of(lambda: ops.PreparedRows(q))
    for k in (1, 8):
        ws = ops._ws(lib.vfm_match_ip_topk_workspace_bytes(n, M, d, k, ops.FAST), q.device)
        ums, umn, (uidx, usim) = med_of(lambda: ops.match_ip_topk(q, b, k, ops.FAST, ws=ws))
        del ws
        ws = ops._ws(lib.vfm_match_ip_topk_prepared_workspace_bytes(n, d, k), q.device)
        pms, pmn, (pidx, psim) = med_of(lambda: ops.match_ip_topk_prepared(ops.PreparedRows(q), bp, k, ws=ws))
        del ws
        res["k"][str(k)] = dict(unprepared_ms=ums, unprepared_min_ms=umn, prepared_ms=pms, prepared_min_ms=pmn,
                                equal=bool(torch.equal(uidx, pidx) and torch.equal(usim, psim)))
    return res


def step_ab(case, lib_path):
    """the unprepared FAST call through the C ABI of ``lib_path`` alone (no package code: the parent's library is older than it)"""
    import ctypes as C
    import torch
    lib = C.CDLL(lib_path)
    lib.vfm_match_ip_topk_workspace_bytes.restype = C.c_size_t
    lib.vfm_match_ip_topk_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int]
    lib.vfm_match_ip_topk.restype = C.c_int
    lib.vfm_match_ip_topk.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    res = dict(lib=case.split(":")[1], cases={})
    for n in (2000, 20000):
        q, b = rows_on_device(n, D, "gaussian")
        for k in (1, 8):
            ws = torch.empty(lib.vfm_match_ip_topk_workspace_bytes(n, M, D, k, 0), dtype=torch.uint8, device="cuda")
            idx = torch.empty((n, k), dtype=torch.int64, device="cuda")
            sim = torch.empty((n, k), dtype=torch.float32, device="cuda")
            st = torch.cuda.current_stream().cuda_stream

            def call():
                rc = lib.vfm_match_ip_topk(q.data_ptr(), n, b.data_ptr(), M, D, k, 0, idx.data_ptr(), sim.data_ptr(), None, ws.data_ptr(),
                                           ws.numel(), st)
                assert rc == 0, rc
            ms, mn, _ = med_of(call)
            res["cases"][f"{n}:{k}"] = dict(ms=ms, min_ms=mn, checksum=int(idx.sum().item()))
            del ws
    return res


def render_wide(res, box):
    L = ["# k-best search at 768 columns and on kept maps: `tools/time_topk.py --wide`", "", f"Measured on: {box}", "",
         "Medians of host clocks around calls that end in a device synchronise, ten calls after three untimed ones (minimum in brackets).", ""]
    wide = sorted((c for c in res if c.startswith("wide:")), key=lambda c: (int(c.split(":")[1]), c))
    if wide:
        L += [f"## Wide descriptors: N queries among {M} map rows of {WIDE_D} columns", "",
              f"(b) = normalise + `(qn[i:i+{BLOCK}] @ bn.T).topk(k)` in torch on the same device; the last column is the share of (query, rank) "
              "entries where torch's fp32 product names the same map row.", "",
              "| N | data | k | FAST ms (min) | largest record count | fallback queries | map slices | (b) torch ms (min) | (b) : FAST | rows equal to (b)'s |",
              "|" + "---|" * 10]
        verdict = []
        for name in wide:
            r = res[name]
            for k in KS:
                x = r["k"][str(k)]
                L.append("| " + " | ".join(str(v) for v in [
                    r["n"], r["data"], k, f"{x['fast_ms']:.3f} ({x['fast_min_ms']:.3f})", x["max_records"], x["fallback"], x["slices"],
                    f"{x['torch_ms']:.3f} ({x['torch_min_ms']:.3f})", f"{x['torch_ms'] / x['fast_ms']:.1f}", f"{100 * x['torch_agrees']:.2f} %"]) + " |")
            k8 = r["k"]["8"]
            verdict.append(f"* {r['n']} x {M} x {WIDE_D}, {r['data']}: at k = 8 FAST takes {k8['fast_ms']:.3f} ms, (b) {k8['torch_ms']:.3f} ms, ratio "
                           f"{k8['torch_ms'] / k8['fast_ms']:.1f} -- the condition (FAST faster than (b)) is {'MET' if k8['fast_ms'] < k8['torch_ms'] else 'NOT MET'}.")
            if "exact_ms" in r:
                verdict.append(f"* {r['n']} x {M} x {WIDE_D}, k = 8, EXACT (the all-pairs fp64 kernel, what these widths ran before; ONE call): "
                               f"{r['exact_ms']:.1f} ms, {r['exact_ms'] / k8['fast_ms']:.0f} x FAST; answers equal to FAST's: "
                               f"{'yes' if r['exact_equal'] else 'NO'}.")
        L += [""] + verdict + [""]
    kept = sorted(c for c in res if c.startswith("kept:"))
    if kept:
        L += [f"## Kept maps: {KEPT_N} queries among {M} map rows", "",
              "unprepared = `ops.match_ip_topk` (prepares both operands in every call); prepared = `ops.PreparedRows(q)` + "
              "`ops.match_ip_topk_prepared` on a map prepared once; map preparation = `vfm_match_prepare` of the map alone.", "",
              "| d | k | unprepared ms (min) | prepared ms (min) | difference ms | map preparation ms (min) | share recovered | answers equal |",
              "|" + "---|" * 8]
        verdict = []
        for name in kept:
            r = res[name]
            for k in (1, 8):
                x = r["k"][str(k)]
                diff = x["unprepared_ms"] - x["prepared_ms"]
                L.append(f"| {r['d']} | {k} | {x['unprepared_ms']:.3f} ({x['unprepared_min_ms']:.3f}) | {x['prepared_ms']:.3f} ({x['prepared_min_ms']:.3f}) | "
                         f"{diff:.3f} | {r['prepare_map_ms']:.3f} ({r['prepare_map_min_ms']:.3f}) | {100 * diff / r['prepare_map_ms']:.0f} % | "
                         f"{'yes' if x['equal'] else 'NO'} |")
                verdict.append(f"* d = {r['d']}, k = {k}: the condition (prepared faster than unprepared) is "
                               f"{'MET' if x['prepared_ms'] < x['unprepared_ms'] else 'NOT MET'} ({x['unprepared_ms'] / x['prepared_ms']:.2f} x).")
            verdict.append(f"* d = {r['d']}: preparing the {KEPT_N} queries alone takes {r['prepare_queries_ms']:.3f} ms per call.")
        L += [""] + verdict + [""]
    ab = [c for c in ("ab:parent1", "ab:this", "ab:parent2") if c in res]
    if len(ab) == 3:
        L += [f"## No regression of the narrow kernel: unprepared FAST, N x {M} x {D}", "",
              "Through the C ABI of each library file, in the order parent, this commit, parent; margin = the difference between the parent's two "
              "medians (the session's run-to-run noise).", "",
              "| N | k | parent, first ms (min) | this commit ms (min) | parent, second ms (min) | margin ms | this - parents' mean ms | within margin | same answers |",
              "|" + "---|" * 9]
        for c in res["ab:this"]["cases"]:
            p1, t, p2 = (res[a]["cases"][c] for a in ab)
            margin, over = abs(p1["ms"] - p2["ms"]), t["ms"] - 0.5 * (p1["ms"] + p2["ms"])
            n, k = c.split(":")
            L.append(f"| {n} | {k} | {p1['ms']:.3f} ({p1['min_ms']:.3f}) | {t['ms']:.3f} ({t['min_ms']:.3f}) | {p2['ms']:.3f} ({p2['min_ms']:.3f}) | "
                     f"{margin:.3f} | {over:+.3f} | {'yes' if over <= margin else 'NO'} | "
                     f"{'yes' if p1['checksum'] == t['checksum'] == p2['checksum'] else 'NO'} |")
        L.append("")
    return "\n".join(L) + "\n"


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
    ap.add_argument("--out")
    ap.add_argument("--wide", action="store_true", help="the sections of profiles/topk_wide_timing.md instead")
    ap.add_argument("--wide-cases", default="wide:2000:gaussian,wide:2000:common,wide:20000:gaussian,wide:20000:common,kept:384,kept:768")
    ap.add_argument("--parent-lib", help="libvfmreg_hip.so of the parent commit: adds the A/B section")
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "needs a ROCm device"
        if a.step.startswith("wide:"):
            r = step_wide(a.step)
        elif a.step.startswith("kept:"):
            r = step_kept(a.step)
        elif a.step.startswith("ab:"):
            this = ROOT / "vfm-registration_amd" / "vfmreg" / "lib" / "libvfmreg_hip.so"
            r = step_ab(a.step, str(this) if a.step == "ab:this" else a.parent_lib)
        else:
            r = step(a.step)
        write_step(Path(a.json), r, show=900)
        return 0
    out = Path(a.out or ROOT / "profiles" / ("topk_wide_timing.md" if a.wide else "topk_timing.md"))
    out.parent.mkdir(parents=True, exist_ok=True)
    cases = (a.wide_cases if a.wide else a.cases).split(",")
    if a.wide and a.parent_lib:
        cases += ["ab:parent1", "ab:this", "ab:parent2"]
    extra = ("--parent-lib", str(Path(a.parent_lib).resolve())) if a.parent_lib else ()
    rc, res, box = run_steps(Path(__file__).resolve(), out, tuple((c, LIMIT_S) for c in cases if c), extra)
    if res:
        write_report(out, (render_wide if a.wide else render)(res, box), dict(box=box, **res))
    return rc


if __name__ == "__main__":
    sys.exit(main())

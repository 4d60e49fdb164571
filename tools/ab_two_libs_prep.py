#!/usr/bin/env python
"""Several builds of the library in ONE process, their operand preparation at C2 timed alternately at flags 24 (the headline's: fp6 image of
the first d / 2 columns) and 8 (full fp6 image) -- see tools/ab_two_libs_coarse.py.  Also checks that the builds write the same bytes.
A build may be given with a "coarse_variant" code for its preparation form (the same file twice with two codes is two entries):
    python tools/ab_two_libs_prep.py libA.so libB.so:43 libB.so:44 [...]          (files under vfm-registration_amd/vfmreg/lib/)
--cases (first argument): no timing; every row of tests/prep_plan_cases.py that an exported entry serves, at the table's shape and at C2,
through each build with the row's policy in the build's own config: torch.equal of both whole prepared buffers and of the search workspace
(the ranges vfm_match_prepare2_gated_z clears; filled alike before), per row, against the first build.  Both operands carry planted
rows (plant(): NaN, Inf, huge, scaled half, zero), so the paths random rows never take are compared as well."""
import ctypes as C
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
from vfmreg import _lib, synth  # noqa: E402

base = _lib.load()
libs = []
cases_mode = sys.argv[1:2] == ["--cases"]
for arg in sys.argv[2 if cases_mode else 1:]:
    name, _, variant = arg.partition(":")
    l = C.CDLL(str(ROOT / "vfm-registration_amd" / "vfmreg" / "lib" / name))
    for entry in ("vfm_match_prepare", "vfm_match_prepare2", "vfm_match_prepare2_gated", "vfm_match_prepare2_gated_p", "vfm_match_prepare2_gated_z",
                  "vfm_match_prepare2_gated_t"):
        getattr(l, entry).restype, getattr(l, entry).argtypes = _lib.SIGNATURES[entry]
    # the build's own policy object (each loaded file has its own thread binding), bound in front of every timed block
    l.vfm_config_create.argtypes = [C.POINTER(C.c_void_p)]
    l.vfm_config_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    l.vfm_config_use.argtypes = [C.c_void_p]
    l.vfm_config_destroy.argtypes = [C.c_void_p]
    cfg = C.c_void_p()
    assert l.vfm_config_create(C.byref(cfg)) == 0
    if variant:
        assert l.vfm_config_set(cfg, b"coarse_variant", int(variant)) == 0
    libs.append((arg, l, cfg))


def plant(x):
    """Rows that plain randn never draws, in place: a NaN below column d / 2, a NaN at or above it, an Inf, a row scaled by 1e30, a row
    whose first half is scaled by 1e-3 -- one 128-row group each where the operand has that many groups -- and a zero row as the last
    row, in the partly filled last group (tests/test_gpu_mx6.py plants the same kinds)."""
    r, d = x.shape
    groups = (r + 127) // 128
    at = [min((k * groups // 6) * 128 + 3 + k, r - 6 + k) for k in range(5)]   # distinct, in front of the last row
    x[at[0], 5] = float("nan")
    x[at[1], d // 2 + 7] = float("nan")
    x[at[2], 11] = float("inf")
    x[at[3]] *= 1e30
    x[at[4], : d // 2] *= 1e-3
    x[r - 1] = 0.0
    return x


def run_cases():
    """the case table through every build: same bytes as the first one?"""
    sys.path.insert(0, str(ROOT))
    from tests import prep_plan_cases as ppc
    st = torch.cuda.current_stream().cuda_stream
    diff = total = 0
    for shape, (r1, r2) in (("table", (ppc.ROWS1, ppc.ROWS2)), ("C2", (200000, 20000))):
        rows = {}
        for case in ppc.CASES:
            if case.images is None or case.entry in ppc.NO_EXPORT:
                continue
            d, (t1, t2) = case.d, case.dtypes
            if d not in rows:
                rows.clear()   # (one width's operands at a time)
                g = torch.Generator(device="cuda").manual_seed(d)
                rows[d] = [plant(torch.randn(r, d, device="cuda", generator=g)) for r in (r1, r2)]
                rows[d] += [x.half() for x in rows[d]]
            x1, x2 = rows[d][2 * t1], rows[d][1 + 2 * t2]
            n2 = 0 if case.entry in ppc.ONE_OPERAND else r2
            outs = []
            for name, l, _ in libs:
                cfg = C.c_void_p()   # the row's policy in this build's own config
                assert l.vfm_config_create(C.byref(cfg)) == 0
                for k, v in case.cfg:
                    assert l.vfm_config_set(cfg, k.encode(), v) == 0
                l.vfm_config_use(cfg)
                p1 = torch.full((base.vfm_match_prepared_bytes(r1, d),), 0xA5, dtype=torch.uint8, device="cuda")
                p2 = torch.full((base.vfm_match_prepared_bytes(max(n2, 1), d),), 0xA5, dtype=torch.uint8, device="cuda")
                ws = torch.full((base.vfm_match_search_workspace_bytes(r2, r1, d) if case.entry == "gated_z" else 256,), 0xFF, dtype=torch.uint8, device="cuda")
                a = (x1.data_ptr(), r1, p1.data_ptr(), x2.data_ptr(), n2, p2.data_ptr(), d)
                rc = {"prepare": lambda: l.vfm_match_prepare(x1.data_ptr(), r1, d, p1.data_ptr(), st),
                      "prepare2": lambda: l.vfm_match_prepare2(*a, st),
                      "gated": lambda: l.vfm_match_prepare2_gated(*a, st),
                      "gated_p": lambda: l.vfm_match_prepare2_gated_p(*a, case.schedule, st),
                      "gated_z": lambda: l.vfm_match_prepare2_gated_z(*a, case.schedule, ws.data_ptr(), ws.numel(), r2, r1, st),
                      "gated_t": lambda: l.vfm_match_prepare2_gated_t(x1.data_ptr(), t1, r1, p1.data_ptr(), x2.data_ptr(), t2, n2, p2.data_ptr(), d,
                                                                      case.schedule, st)}[case.entry]()
                torch.cuda.synchronize()
                assert rc == 0, (name, case.id)
                l.vfm_config_use(None)
                l.vfm_config_destroy(cfg)
                outs.append((p1, p2, ws))
            same = [all(bool(torch.equal(x, y)) for x, y in zip(outs[0], o)) for o in outs[1:]]
            total += 1
            diff += not all(same)
            print(f"{shape:5s} {case.id:48s} prepared + workspace bytes equal to {libs[0][0]}: {same}", flush=True)
    print(f"--cases: {total} rows, {diff} differ", flush=True)


if cases_mode:
    run_cases()
    sys.exit(0)
n, m, d = 20000, 200000, 384
p = synth.make_pair_device(n, m, d, seed=42)
st = torch.cuda.current_stream().cuda_stream
for flags in (24, 8):
    bufs = {}
    for name, _, _ in libs:
        bufs[name] = (torch.zeros(base.vfm_match_prepared_bytes(n, d), dtype=torch.uint8, device="cuda"),
                      torch.zeros(base.vfm_match_prepared_bytes(m, d), dtype=torch.uint8, device="cuda"))
    acc = {name: [] for name, _, _ in libs}
    for rep in range(12):
        for name, l, cfg in libs:
            qb, bb = bufs[name]
            l.vfm_config_use(cfg)
            call = lambda: l.vfm_match_prepare2_gated_p(p["b_desc"].data_ptr(), m, bb.data_ptr(), p["q_desc"].data_ptr(), n, qb.data_ptr(), d, flags, st)
            for _ in range(3):
                assert call() == 0
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                call()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 2:
                acc[name].append(e0.elapsed_time(e1) / 20)
    ref = bufs[libs[0][0]]
    for name, _, _ in libs:
        v = sorted(acc[name])
        same = all(bool(torch.equal(a, b)) for a, b in zip(ref, bufs[name]))
        print(f"flags {flags:2d}  {name:34s} median {v[len(v) // 2]:.4f} ms   min {v[0]:.4f}   max {v[-1]:.4f}   same bytes as {libs[0][0]}: {same}", flush=True)

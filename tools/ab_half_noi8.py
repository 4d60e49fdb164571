#!/usr/bin/env python
"""VFM_RECORDS_MX6_HALF_FUSED with and without the int8 image (policy key "half_noi8" 0 / 1) in ONE process, alternating, at the
headline's size on D.2 pairs: the preparation alone (flags 24 against 24 | VFM_PREPARE_NO_I8), the finish call alone (events around
vfm_match_search_finish_gated_r behind a fresh coarse pass; records 8 against 8 | VFM_RECORDS_NO_I8) and the bench's pipeline over 20 and
200 steps.  Also checks that both forms return the same idx / sim.    python tools/ab_half_noi8.py [reps] [--no-pipeline]"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from vfmreg import _lib, synth  # noqa: E402
from vfmreg.pipeline import RegistrationPipeline  # noqa: E402

lib = _lib.load()
dev = torch.device("cuda")
n, m, d = 20000, 200000, 384
args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if args else 3
pairs = [synth.make_pair_device(n, m, d, seed=42 + p, device=dev) for p in range(2)]
p = pairs[0]
st = torch.cuda.current_stream().cuda_stream
gate = float(np.nextafter(np.float32(0.8), np.float32(-np.inf)))
FORMS = (("int8 image kept (key 0)", 24, 8), ("no int8 image (key 1)", 24 | 32, 8 | 0x200))


def med(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


bufs = {name: (torch.zeros(lib.vfm_match_prepared_bytes(n, d), dtype=torch.uint8, device=dev),
               torch.zeros(lib.vfm_match_prepared_bytes(m, d), dtype=torch.uint8, device=dev),
               torch.zeros(lib.vfm_match_search_workspace_bytes(n, m, d), dtype=torch.uint8, device=dev),
               torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.float32, device=dev)) for name, _, _ in FORMS}
prep_ms = {name: [] for name, _, _ in FORMS}
fin_ms = {name: [] for name, _, _ in FORMS}
for rep in range(12):
    for name, flags, records in FORMS:
        qb, bb, ws, idx, sim = bufs[name]
        prep = lambda: _lib.check(lib.vfm_match_prepare2_gated_p(p["b_desc"].data_ptr(), m, bb.data_ptr(), p["q_desc"].data_ptr(), n, qb.data_ptr(), d, flags, st))
        for _ in range(3):
            prep()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            prep()
        e1.record()
        torch.cuda.synchronize()
        if rep >= 2:
            prep_ms[name].append(e0.elapsed_time(e1) / 20)
        evs = []
        for it in range(12):
            _lib.check(lib.vfm_match_search_coarse_gated_g(qb.data_ptr(), n, bb.data_ptr(), m, d, ws.data_ptr(), ws.numel(), records, gate, st))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(lib.vfm_match_search_finish_gated_r(p["q_desc"].data_ptr(), qb.data_ptr(), n, p["b_desc"].data_ptr(), bb.data_ptr(), m, d,
                                                           idx.data_ptr(), sim.data_ptr(), ws.data_ptr(), ws.numel(), gate, records, st))
            b.record()
            evs.append((a, b))
        torch.cuda.synchronize()
        if rep >= 2:
            fin_ms[name].append(sum(a.elapsed_time(b) for a, b in evs[2:]) / len(evs[2:]))
same = torch.equal(bufs[FORMS[0][0]][3], bufs[FORMS[1][0]][3]) and torch.equal(bufs[FORMS[0][0]][4].view(torch.int32), bufs[FORMS[1][0]][4].view(torch.int32))
print(f"idx / sim of the two forms equal: {same}   matches: {int((bufs[FORMS[1][0]][3] >= 0).sum())}")
for name, _, _ in FORMS:
    print("preparation alone  %-26s median %.4f ms   min %.4f   max %.4f" % ((name,) + med(prep_ms[name])), flush=True)
for name, _, _ in FORMS:
    print("finish call alone  %-26s median %.4f ms   min %.4f   max %.4f" % ((name,) + med(fin_ms[name])), flush=True)
del bufs
if "--no-pipeline" in sys.argv:
    sys.exit(0)
acc = {}
for rep in range(reps):
    for steps in (20, 200):
        for key in (0, 1):
            pipe = RegistrationPipeline(n, m, d, n_iter=50000, device=dev, overlap_ransac=True, overlap_prepare=True, solve_streams=2, coarse="auto",
                                        config=_lib.Config(half_noi8=key))
            v, msps, cms, res = bench.timed_loop(lib, pipe, pairs, steps, 5, settle=6)
            acc.setdefault((steps, key), []).append((v, cms))
            print(f"rep {rep} {steps:3d} steps  half_noi8 {key} (records {pipe.last_records:#x}, schedule {pipe.last_prep_schedule}): {v:7.1f}/s  "
                  f"coarse kernel in the pipeline {cms:.3f} ms", flush=True)
            del pipe
print("\nsummary (registrations/s: min / median / max over the repetitions; coarse kernel ms: median)")
for (steps, key), rows in acc.items():
    v = sorted(r[0] for r in rows)
    c = sorted(r[1] for r in rows)
    print(f"{steps:3d} steps  half_noi8 {key}: {v[0]:7.1f} / {v[len(v) // 2]:7.1f} / {v[-1]:7.1f}   coarse {c[len(c) // 2]:.3f} ms")

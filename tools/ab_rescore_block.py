#!/usr/bin/env python
"""match_rescore_kernel with 64 and with 256 queries per workgroup (policy key "rescore_block") in ONE process, alternating, at the
headline's size on D.2 pairs: the finish call alone (events around vfm_match_search_finish_gated_r behind a fresh coarse pass, records
8 | VFM_RECORDS_NO_I8; 10 blocks, median and min - max) and the bench's pipeline over 20 and 200 steps.  Also checks that both forms
return the same idx / sim.    python tools/ab_rescore_block.py [reps] [--no-pipeline]"""
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
BLOCKS = (64, 256)
FLAGS, RECORDS = 24 | 32, 8 | 0x200


def med(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


qb = torch.zeros(lib.vfm_match_prepared_bytes(n, d), dtype=torch.uint8, device=dev)
bb = torch.zeros(lib.vfm_match_prepared_bytes(m, d), dtype=torch.uint8, device=dev)
ws = torch.zeros(lib.vfm_match_search_workspace_bytes(n, m, d), dtype=torch.uint8, device=dev)
out = {blk: (torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.float32, device=dev)) for blk in BLOCKS}
_lib.check(lib.vfm_match_prepare2_gated_p(p["b_desc"].data_ptr(), m, bb.data_ptr(), p["q_desc"].data_ptr(), n, qb.data_ptr(), d, FLAGS, st))
fin_ms = {blk: [] for blk in BLOCKS}
for rep in range(12):
    for blk in BLOCKS:
        idx, sim = out[blk]
        with _lib.using(_lib.Config(rescore_block=blk)):
            evs = []
            for it in range(12):
                _lib.check(lib.vfm_match_search_coarse_gated_g(qb.data_ptr(), n, bb.data_ptr(), m, d, ws.data_ptr(), ws.numel(), RECORDS, gate, st))
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                _lib.check(lib.vfm_match_search_finish_gated_r(p["q_desc"].data_ptr(), qb.data_ptr(), n, p["b_desc"].data_ptr(), bb.data_ptr(), m, d,
                                                               idx.data_ptr(), sim.data_ptr(), ws.data_ptr(), ws.numel(), gate, RECORDS, st))
                b.record()
                evs.append((a, b))
            torch.cuda.synchronize()
        if rep >= 2:
            fin_ms[blk].append(sum(a.elapsed_time(b) for a, b in evs[2:]) / len(evs[2:]))
same = torch.equal(out[64][0], out[256][0]) and torch.equal(out[64][1].view(torch.int32), out[256][1].view(torch.int32))
print(f"idx / sim of the two forms equal: {same}   matches: {int((out[256][0] >= 0).sum())}")
for blk in BLOCKS:
    print("finish call alone  rescore_block %3d  median %.4f ms   min %.4f   max %.4f" % ((blk,) + med(fin_ms[blk])), flush=True)
del qb, bb, ws
if "--no-pipeline" in sys.argv:
    sys.exit(0 if same else 1)
acc = {}
for rep in range(reps):
    for steps in (20, 200):
        for blk in BLOCKS:
            pipe = RegistrationPipeline(n, m, d, n_iter=50000, device=dev, overlap_ransac=True, overlap_prepare=True, solve_streams=2, coarse="auto",
                                        config=_lib.Config(rescore_block=blk))
            v, msps, cms, res = bench.timed_loop(lib, pipe, pairs, steps, 5, settle=6)
            acc.setdefault((steps, blk), []).append((v, cms))
            print(f"rep {rep} {steps:3d} steps  rescore_block {blk:3d} (records {pipe.last_records:#x}): {v:7.1f}/s  "
                  f"coarse kernel in the pipeline {cms:.3f} ms", flush=True)
            del pipe
print("\nsummary (registrations/s: min / median / max over the repetitions; coarse kernel ms: median)")
for (steps, blk), rows in acc.items():
    v = sorted(r[0] for r in rows)
    c = sorted(r[1] for r in rows)
    print(f"{steps:3d} steps  rescore_block {blk:3d}: {v[0]:7.1f} / {v[len(v) // 2]:7.1f} / {v[-1]:7.1f}   coarse {c[len(c) // 2]:.3f} ms")
sys.exit(0 if same else 1)

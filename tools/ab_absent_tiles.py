#!/usr/bin/env python
"""A/B of the headline coarse kernel (record kind 8, C2: 625 query tiles in 27 blocks of 24 -- 23 absent sets, all in the last block)
with the absent sets skipped (default) against multiplied as copies of tile 0 (vfm_config "mx6_tune" bit 2), alternating inside one
process: the kernel alone (HIP events around 20 back-to-back calls) and the bench pipeline (20 / 200 steps), median and min - max over
the blocks.  `--sweep`: the slice counts around the launcher's choice with the new kernel, alone and in the pipeline (200 steps).
python tools/ab_absent_tiles.py [blocks] [--sweep]"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
import bench  # noqa: E402
from vfmreg import _lib, synth  # noqa: E402
from vfmreg.pipeline import RegistrationPipeline  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
blocks = int(args[0]) if args else 12
lib = _lib.load()
st = torch.cuda.current_stream().cuda_stream
n, m, d = 20000, 200000, 384
pairs = [synth.make_pair_device(n, m, d, seed=42 + p) for p in range(2)]
p = pairs[0]
qb = torch.empty(lib.vfm_match_prepared_bytes(n, d), dtype=torch.uint8, device="cuda")
bb = torch.empty(lib.vfm_match_prepared_bytes(m, d), dtype=torch.uint8, device="cuda")
ws = torch.empty(lib.vfm_match_search_workspace_bytes(n, m, d), dtype=torch.uint8, device="cuda")
gate = float(np.nextafter(np.float32(0.8), np.float32(-np.inf)))
_lib.check(lib.vfm_match_prepare2_gated_p(p["b_desc"].data_ptr(), m, bb.data_ptr(), p["q_desc"].data_ptr(), n, qb.data_ptr(), d, 24, st))


def alone():
    for _ in range(3):
        _lib.check(lib.vfm_match_search_coarse_gated_g(qb.data_ptr(), n, bb.data_ptr(), m, d, ws.data_ptr(), ws.numel(), 8, gate, st))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        _lib.check(lib.vfm_match_search_coarse_gated_g(qb.data_ptr(), n, bb.data_ptr(), m, d, ws.data_ptr(), ws.numel(), 8, gate, st))
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 20


def summary(v):
    v = sorted(v)
    return f"median {v[len(v) // 2]:9.4f}   min {v[0]:9.4f}   max {v[-1]:9.4f}"


pipe = RegistrationPipeline(n, m, d, n_iter=50000, overlap_ransac=True, overlap_prepare=True, solve_streams=2, coarse="mx6-half")
if "--sweep" in sys.argv:
    for slices in (0, 40, 44, 47, 48, 52, 56, 57, 60, 64):
        ta, tp = [], []
        with _lib.using(_lib.Config(coarse_slices=slices)):
            for rep in range(max(3, blocks // 3)):
                ta.append(alone())
                tp.append(bench.timed_loop(lib, pipe, pairs, 200, 3)[0])
        print(f"slices {slices:2d} (0 = the launcher's): alone ms {summary(ta)} | pipeline 200 steps /s {summary(tp)}", flush=True)
    sys.exit(0)
acc = {tune: {"alone": [], "p20": [], "p200": []} for tune in (0, 4)}
for rep in range(blocks + 2):
    for tune in (0, 4):
        with _lib.using(_lib.Config(mx6_tune=tune)):
            t = alone()
            v20 = bench.timed_loop(lib, pipe, pairs, 20, 3)[0]
            v200 = bench.timed_loop(lib, pipe, pairs, 200, 3)[0]
        if rep >= 2:
            for k, v in (("alone", t), ("p20", v20), ("p200", v200)):
                acc[tune][k].append(v)
for tune in (0, 4):
    print(f"mx6_tune {tune} ({'absent sets skipped' if tune == 0 else 'absent sets multiplied'}):")
    print(f"    coarse call alone, ms       {summary(acc[tune]['alone'])}")
    print(f"    pipeline  20 steps, 1/s     {summary(acc[tune]['p20'])}")
    print(f"    pipeline 200 steps, 1/s     {summary(acc[tune]['p200'])}", flush=True)

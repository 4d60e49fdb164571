#!/usr/bin/env python
"""The two pieces of the persistent-preparation change in ONE process, alternating, inside the bench's pipeline (headline mode, D.2
pairs): A = prep_once_kernel as a persistent grid with the next group's loads under a group's second pass (coarse_variant 44 against
43), B = the search workspace cleared by the preparation and a coarse call without fills (RegistrationPipeline._ws_clean).  20-step
(the driver's form) and 200-step timed loops; per configuration the registrations/s of every repetition and the coarse kernel's
duration between its events.    python tools/ab_prep_persistent.py [reps] [mode ...]"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
import torch  # noqa: E402

import bench  # noqa: E402
from vfmreg import _lib, synth  # noqa: E402
from vfmreg.pipeline import RegistrationPipeline  # noqa: E402

lib = _lib.load()
dev = torch.device("cuda")
n, m, d = 20000, 200000, 384
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
modes = sys.argv[2:] or ["mx6-half"]
pairs = [synth.make_pair_device(n, m, d, seed=42 + p, device=dev) for p in range(2)]
CONFIGS = (("43, coarse call fills (as before)", 43, False), ("A: 44 persistent", 44, False), ("B: 43 + precleared workspace", 43, True),
           ("A + B", 44, True))
acc = {}
for rep in range(reps):
    for mode in modes:
        for steps in (20, 200):
            for name, variant, clean in CONFIGS:
                lib.vfm_debug_set_coarse_variant(variant)
                pipe = RegistrationPipeline(n, m, d, n_iter=50000, device=dev, overlap_ransac=True, overlap_prepare=True, solve_streams=2, coarse=mode)
                pipe._ws_clean = clean
                v, msps, cms, res = bench.timed_loop(lib, pipe, pairs, steps, 5)
                acc.setdefault((mode, steps, name), []).append((v, cms))
                print(f"rep {rep} {mode:10s} {steps:3d} steps  {name:34s}: {v:7.1f}/s  coarse kernel in the pipeline {cms:.3f} ms", flush=True)
                del pipe
lib.vfm_debug_set_coarse_variant(43)
print("\nsummary (registrations/s: min / median / max over the repetitions; coarse kernel ms: median)")
for (mode, steps, name), rows in acc.items():
    v = sorted(r[0] for r in rows)
    c = sorted(r[1] for r in rows)
    print(f"{mode:10s} {steps:3d} steps  {name:34s}: {v[0]:7.1f} / {v[len(v) // 2]:7.1f} / {v[-1]:7.1f}   coarse {c[len(c) // 2]:.3f} ms")

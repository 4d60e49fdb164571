#!/usr/bin/env python
"""Driver for counter and trace passes over VFM_RECORDS_MX6_HALF_FUSED with and without the int8 image (tools/pmc_half_noi8.sh): at the
headline's size on a D.2 pair, a few times each: preparation, coarse pass, finish call -- flags 24 / records 8, then flags 24 | 32 /
records 8 | 0x200.    python tools/time_half_noi8.py [calls]"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
from vfmreg import _lib, synth  # noqa: E402

lib = _lib.load()
n, m, d = 20000, 200000, 384
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 3
p = synth.make_pair_device(n, m, d, seed=42)
qb = torch.empty(lib.vfm_match_prepared_bytes(n, d), dtype=torch.uint8, device="cuda")
bb = torch.empty(lib.vfm_match_prepared_bytes(m, d), dtype=torch.uint8, device="cuda")
ws = torch.empty(lib.vfm_match_search_workspace_bytes(n, m, d), dtype=torch.uint8, device="cuda")
idx = torch.empty(n, dtype=torch.int64, device="cuda")
sim = torch.empty(n, dtype=torch.float32, device="cuda")
st = torch.cuda.current_stream().cuda_stream
gate = float(np.nextafter(np.float32(0.8), np.float32(-np.inf)))
for flags, records in ((24, 8), (24 | 32, 8 | 0x200)):
    for _ in range(calls):
        _lib.check(lib.vfm_match_prepare2_gated_p(p["b_desc"].data_ptr(), m, bb.data_ptr(), p["q_desc"].data_ptr(), n, qb.data_ptr(), d, flags, st))
        _lib.check(lib.vfm_match_search_coarse_gated_g(qb.data_ptr(), n, bb.data_ptr(), m, d, ws.data_ptr(), ws.numel(), records, gate, st))
        _lib.check(lib.vfm_match_search_finish_gated_r(p["q_desc"].data_ptr(), qb.data_ptr(), n, p["b_desc"].data_ptr(), bb.data_ptr(), m, d,
                                                       idx.data_ptr(), sim.data_ptr(), ws.data_ptr(), ws.numel(), gate, records, st))
    torch.cuda.synchronize()
    print(f"flags {flags} records {records:#x}: {int((idx >= 0).sum())} matches", flush=True)

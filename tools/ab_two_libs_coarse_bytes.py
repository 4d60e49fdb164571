#!/usr/bin/env python
"""Two builds of the library in ONE process, every inner-product case of the coarse dispatch table (tests/match_dispatch_cases.py: the
"ip" and "gated" entries, the padding cases included) run by each on buffers of its own: the search workspace is pre-filled with 0xA5,
and after the coarse call the WHOLE workspace, after the finish call idx / sim, must be equal byte for byte between the builds.
A coarse kernel that files its records or survivors through atomics leaves them in an order that differs from run to run of ONE build,
so where the builds differ the first build runs the case again: a case whose two runs of the same build differ is reported as such,
not as a difference between the builds, and its workspaces are compared once more as multisets of 32-bit words -- equal where the same
records or survivors were filed in another order (the fused kinds), not necessarily where the set itself depends on the timing (the sparse
fp16 records: rows within a window of the query's running maximum AT THAT TIME).
python tools/ab_two_libs_coarse_bytes.py libA.so libB.so      (names under vfm-registration_amd/vfmreg/lib/)"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
sys.path.insert(0, str(ROOT))
from vfmreg import _lib  # noqa: E402

from tests import match_dispatch_cases as mdc  # noqa: E402

FUNCS = ("vfm_config_create", "vfm_config_destroy", "vfm_config_set", "vfm_config_use", "vfm_match_prepared_bytes", "vfm_match_prepare",
         "vfm_match_prepare2_gated_p", "vfm_match_search_workspace_bytes", "vfm_match_search_coarse", "vfm_match_search_finish",
         "vfm_match_search_coarse_gated_g", "vfm_match_search_finish_gated_r")


def load(name):
    lib = C.CDLL(str(ROOT / "vfm-registration_amd" / "vfmreg" / "lib" / name))
    for fn in FUNCS:
        getattr(lib, fn).restype, getattr(lib, fn).argtypes = _lib.SIGNATURES[fn]
    return lib


def run(lib, case, q, b):
    """(workspace after the coarse call, idx, sim) of the case under its config, every buffer this run's own"""
    n, d = q.shape
    m = b.shape[0]
    st = torch.cuda.current_stream().cuda_stream
    cfg = C.c_void_p()
    assert lib.vfm_config_create(C.byref(cfg)) == 0
    for k, v in case.cfg:
        assert lib.vfm_config_set(cfg, k.encode(), v) == 0
    assert lib.vfm_config_use(cfg) == 0
    try:
        qb = torch.full((lib.vfm_match_prepared_bytes(n, d),), 0xA5, dtype=torch.uint8, device="cuda")
        bb = torch.full((lib.vfm_match_prepared_bytes(m, d),), 0xA5, dtype=torch.uint8, device="cuda")
        ws = torch.full((lib.vfm_match_search_workspace_bytes(n, m, d),), 0xA5, dtype=torch.uint8, device="cuda")
        idx = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        sim = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        if case.gated:
            flags = mdc.PREPARE_MX6 if case.records in mdc.MX6_KINDS else 0
            assert lib.vfm_match_prepare2_gated_p(b.data_ptr(), m, bb.data_ptr(), q.data_ptr(), n, qb.data_ptr(), d, flags, st) == 0
            assert lib.vfm_match_search_coarse_gated_g(qb.data_ptr(), n, bb.data_ptr(), m, d, ws.data_ptr(), ws.numel(), case.records, mdc.GATE, st) == 0
            after_coarse = ws.clone()
            assert lib.vfm_match_search_finish_gated_r(q.data_ptr(), qb.data_ptr(), n, b.data_ptr(), bb.data_ptr(), m, d, idx.data_ptr(), sim.data_ptr(),
                                                       ws.data_ptr(), ws.numel(), mdc.GATE, case.records, st) == 0
        else:
            assert lib.vfm_match_prepare(q.data_ptr(), n, d, qb.data_ptr(), st) == 0 and lib.vfm_match_prepare(b.data_ptr(), m, d, bb.data_ptr(), st) == 0
            assert lib.vfm_match_search_coarse(qb.data_ptr(), n, bb.data_ptr(), m, d, ws.data_ptr(), ws.numel(), st) == 0
            after_coarse = ws.clone()
            assert lib.vfm_match_search_finish(q.data_ptr(), qb.data_ptr(), n, b.data_ptr(), bb.data_ptr(), m, d, idx.data_ptr(), sim.data_ptr(),
                                               ws.data_ptr(), ws.numel(), st) == 0
        torch.cuda.synchronize()
        return after_coarse, idx, sim
    finally:
        lib.vfm_config_use(None)
        lib.vfm_config_destroy(cfg)


def main():
    _lib.load()   # (torch's HIP runtime first)
    name_a, name_b = sys.argv[1:3]
    lib_a, lib_b = load(name_a), load(name_b)
    cases = [c for c in mdc.CASES + mdc.PADDING_CASES if c.entry in ("ip", "gated")]
    differ_ws = differ_out = unstable = 0
    for case in cases:
        q, b = (torch.from_numpy(x).cuda() for x in mdc.make(case.d, case.n, case.m, seed=case.d + case.n + case.m))
        ws_a, idx_a, sim_a = run(lib_a, case, q, b)
        ws_b, idx_b, sim_b = run(lib_b, case, q, b)
        same_ws = torch.equal(ws_a, ws_b)
        same_out = torch.equal(idx_a, idx_b) and torch.equal(sim_a, sim_b)
        note = ""
        if not same_ws:
            ws_a2, _, _ = run(lib_a, case, q, b)
            if torch.equal(ws_a, ws_a2):
                differ_ws += 1
                note = f"WORKSPACE DIFFERS ({int((ws_a != ws_b).sum())} bytes)"
            else:
                unstable += 1
                words = [torch.sort(w[:w.numel() // 4 * 4].view(torch.int32)).values for w in (ws_a, ws_b, ws_a2)]
                note = (f"workspace differs between two runs of {name_a} too ({int((ws_a != ws_a2).sum())} bytes; {int((ws_a != ws_b).sum())} against "
                        f"{name_b}); as multisets of words: the builds {'equal' if torch.equal(words[0], words[1]) else 'not equal'}, "
                        f"the two runs of {name_a} {'equal' if torch.equal(words[0], words[2]) else 'not equal'}")
        if not same_out:
            differ_out += 1
            note += " IDX / SIM DIFFER"
        print(f"{case.id:64s} ws {'equal' if same_ws else 'NOT equal'}  idx/sim {'equal' if same_out else 'NOT equal'}  {note}", flush=True)
    print(f"cases {len(cases)}  workspace differs between the builds {differ_ws}  idx / sim differ {differ_out}  "
          f"not reproducible within one build {unstable}", flush=True)
    return 1 if differ_ws or differ_out else 0


if __name__ == "__main__":
    sys.exit(main())

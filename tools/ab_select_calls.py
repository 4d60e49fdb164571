"""A/B of two builds of the library on the calls that run the candidate-selection kernels (csrc/match_select.h): the gated search at
20 000 x 200 000 x 384 (a synth D.2 pair, gate 0.8) under the record kinds BEST, TOP2, HALF, MX6, MX6_TOP2 and MX6_HALF -- BEST and MX6
once more under "coarse_variant" 20, the general kernel -- and the FAST Euclidean search at tools/time_l2.py's 5000 x 5000 x 33 (fp16
records: match_select_kernel) and 5000 x 50 000 x 384 (int8 records: match_select_l2_kernel).  As tools/ab_exact_calls.py: each
build runs in its own process (the .so cannot be swapped in-process), alternating, on the same box.  Per run and case: the median of
10 finish calls between device events after 3 warm-up calls, each behind a fresh coarse pass (the Euclidean search has one entry: the
whole call), then one search with match_stats = 1: a checksum of idx, of the bits of sim and the 64 counters of vfm_debug_match_stats.
    python tools/ab_select_calls.py libvfmreg_hip_parent.so libvfmreg_hip.so"""
import json, subprocess, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
CHILD = r'''
import ctypes as C, json, sys
from pathlib import Path
ROOT = Path(sys.argv[1]); sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
import numpy as np, torch
from vfmreg import _lib
_lib.LIB_PATH = ROOT / "vfm-registration_amd" / "vfmreg" / "lib" / sys.argv[2]
from vfmreg import ops, synth
lib = _lib.load()
n, m, d = 20000, 200000, 384
p = synth.make_pair_device(n, m, d, seed=42)
q, b = p["q_desc"], p["b_desc"]
qb = torch.empty(lib.vfm_match_prepared_bytes(n, d), dtype=torch.uint8, device="cuda")
bb = torch.empty(lib.vfm_match_prepared_bytes(m, d), dtype=torch.uint8, device="cuda")
ws = torch.empty(lib.vfm_match_search_workspace_bytes(n, m, d), dtype=torch.uint8, device="cuda")
idx = torch.empty(n, dtype=torch.int64, device="cuda")
sim = torch.empty(n, dtype=torch.float32, device="cuda")
st = torch.cuda.current_stream().cuda_stream
gate = float(np.nextafter(np.float32(0.8), np.float32(-np.inf)))
def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64).to(torch.int64).sum().item()
def median_ms(timed, before=lambda: None):
    ms = []
    for i in range(13):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); timed(); e1.record(); torch.cuda.synchronize()
        if i >= 3: ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2]
BEST, TOP2, HALF, MX6, MX6_TOP2, MX6_HALF = 0, 1, 3, 5, 6, 7
CASES = [("BEST", BEST, 0), ("BEST/v20", BEST, 20), ("TOP2", TOP2, 0), ("TOP2/v20", TOP2, 20), ("HALF", HALF, 0), ("MX6", MX6, 0), ("MX6/v20", MX6, 20),
         ("MX6_TOP2", MX6_TOP2, 0), ("MX6_HALF", MX6_HALF, 0)]
out = {}
for name, records, variant in CASES:
    def coarse():
        _lib.check(lib.vfm_match_search_coarse_gated_g(qb.data_ptr(), n, bb.data_ptr(), m, d, ws.data_ptr(), ws.numel(), records, gate, st))
    def finish():
        _lib.check(lib.vfm_match_search_finish_gated_r(q.data_ptr(), qb.data_ptr(), n, b.data_ptr(), bb.data_ptr(), m, d, idx.data_ptr(),
                                                       sim.data_ptr(), ws.data_ptr(), ws.numel(), gate, records, st))
    with _lib.using(_lib.Config(coarse_variant=variant)):
        _lib.check(lib.vfm_match_prepare2_gated_p(b.data_ptr(), m, bb.data_ptr(), q.data_ptr(), n, qb.data_ptr(), d, 8 if records >= MX6 else 0, st))
        ms = median_ms(finish, coarse)
    with _lib.using(_lib.Config(coarse_variant=variant, match_stats=1)):
        coarse(); finish()
        stats = (C.c_int32 * 64)()
        _lib.check(lib.vfm_debug_match_stats(ws.data_ptr(), n, m, C.cast(stats, C.c_void_p)))
    out[name] = {"median_ms": ms, "checksum": [int((idx >= 0).sum()), bits(idx), bits(sim)] + list(stats)}
g = torch.Generator(device="cuda").manual_seed(1)
for name, (n2, m2, d2) in (("l2 d33", (5000, 5000, 33)), ("l2 d384", (5000, 50000, 384))):
    a5, b5 = torch.randn(n2, d2, device="cuda", generator=g), torch.randn(m2, d2, device="cuda", generator=g)
    res = []
    def call():
        res[:] = ops.match_mutual_l2(a5, b5, prec=ops.FAST)
    ms = median_ms(call)
    out[name] = {"median_ms": ms, "checksum": [bits(t) for t in res if t is not None]}
print(json.dumps(out))
'''
libs = sys.argv[1:]
runs = {l: [] for l in libs}
for rep in range(3):
    for l in libs:
        r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), l], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:   # a build that fails ends the comparison: nothing further is started on the device
            sys.exit(f"{l}: exit status {r.returncode}\n{r.stderr[-2000:]}")
        runs[l].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(f"run {rep + 1} of {l} done", flush=True)
for name in runs[libs[0]][0]:
    for l in libs:
        ms = [r[name]["median_ms"] for r in runs[l]]
        print(f"{name:9s} {l:28s} " + " ".join(f"{v:9.4f}" for v in ms) + f"   median {sorted(ms)[1]:9.4f} ms")
    sums = {json.dumps(r[name]["checksum"]) for l in libs for r in runs[l]}
    print(f"{name:9s} idx, sim and the 64 counters equal in every run of every build: {len(sums) == 1}   {runs[libs[0]][0][name]['checksum'][:3]}")
    if len(sums) != 1:
        for l in libs:
            for r in runs[l]:
                print(f"          {l}: {r[name]['checksum']}")

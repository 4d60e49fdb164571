"""A/B of two builds of the library on the calls that end in the all-pairs fp64 decision (csrc/match_exact.h): match_ip_top1(EXACT) and
match_ip_topk(EXACT, k = 8) at 2 000 x 200 000 x 384, match_mutual_l2(prec=EXACT) at tools/time_l2.py's 5000 x 5000 x 33 -- and
prec=NARROW there, whose sweep kernels use the same order.  As
tools/ab_libs.py: each build runs in its own process (the .so cannot be swapped in-process), alternating, on the same box.  Per run
and call: the median of 10 calls between device events after 3 warm-up calls, and a checksum of the outputs (equal answers).
    python tools/ab_exact_calls.py libvfmreg_hip_parent.so libvfmreg_hip.so"""
import json, subprocess, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
CHILD = r'''
import json, sys
from pathlib import Path
ROOT = Path(sys.argv[1]); sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
import torch
from vfmreg import _lib
_lib.LIB_PATH = ROOT / "vfm-registration_amd" / "vfmreg" / "lib" / sys.argv[2]
from vfmreg import ops
g = torch.Generator(device="cuda").manual_seed(1)
q, b = torch.randn(2000, 384, device="cuda", generator=g), torch.randn(200000, 384, device="cuda", generator=g)
a5, b5 = torch.randn(5000, 33, device="cuda", generator=g), torch.randn(5000, 33, device="cuda", generator=g)
calls = {"top1": lambda: ops.match_ip_top1(q, b, ops.EXACT), "topk8": lambda: ops.match_ip_topk(q, b, 8, ops.EXACT),
         "l2": lambda: ops.match_mutual_l2(a5, b5, prec=ops.EXACT), "l2n": lambda: ops.match_mutual_l2(a5, b5, prec=ops.NARROW)}
out = {}
for name, call in calls.items():
    for _ in range(3):
        res = call()
    ms = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); res = call(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    bits = [t.view(torch.int32 if t.dtype == torch.float32 else torch.int64).to(torch.int64).sum().item() for t in res if t is not None]
    out[name] = {"median_ms": ms[len(ms) // 2], "checksum": bits}
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
for name in runs[libs[0]][0]:
    for l in libs:
        ms = [r[name]["median_ms"] for r in runs[l]]
        print(f"{name:6s} {l:28s} " + " ".join(f"{v:9.4f}" for v in ms) + f"   median {sorted(ms)[1]:9.4f} ms   checksum {runs[l][0][name]['checksum']}")
    print(f"{name:6s} same answers in every run of every build: {len({json.dumps(r[name]['checksum']) for l in libs for r in runs[l]}) == 1}")

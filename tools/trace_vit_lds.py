#!/usr/bin/env python
"""Inside the LDS-tiled residual GEMMs (proj, fc2) of a ViT forward at N images: per workgroup the time in the k loop and in the epilogue
(residual read-modify-write, fp16 copy, LayerNorm statistics), from the kernel's own trace (start / end of loop / end, 100 MHz)."""
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
from vfmreg import _lib  # noqa: E402
from vfmreg import vit as V  # noqa: E402

rng = np.random.default_rng(0)
nimg = int(sys.argv[1]) if len(sys.argv) > 1 else 90
imgs = torch.from_numpy(rng.integers(1, 255, (nimg, 1200, 1600, 3), dtype=np.uint8)).cuda()
buf = torch.zeros((2, 4096, 4), dtype=torch.int64, device="cuda")
cfg = _lib.Config().set("vit_trace_buffer", buf.data_ptr())
# depth 1: the LAST residual GEMM of the forward is the block's fc2; with VFM_ONLY_PROJ=1 the MLP is skipped by reading after a
# forward whose weights make fc2 the traced launch anyway -- the two are told apart by the k-steps the kernel records
if os.environ.get("VFM_ONLY_PROJ") == "1":   # the proj launch instead of fc2 (both are the LDS-tiled residual kernel)
    cfg.set("vit_trace_fused", 2)
model = V.ViTS14(V.random_weights(0, depth=1), 1200, 1600)
with _lib.using(cfg):
    for _ in range(3):
        buf.zero_()
        model.forward(imgs)
torch.cuda.synchronize()
both = buf.cpu().numpy()
live = both[0][:, 0] > 0
t = both[0][live]
cyc = both[1][live].astype(np.float64)
t0 = t[:, 0].min()
start, loop_end, end, ks = (t[:, 0] - t0) / 100.0, (t[:, 1] - t0) / 100.0, (t[:, 2] - t0) / 100.0, t[:, 3]
print(f"{nimg} images: {len(t)} workgroups traced, k-steps {sorted(set(int(k) for k in ks))}")
print(f"  start: median {np.median(start):.1f} us, max {start.max():.1f}; kernel end {end.max():.1f} us")
print(f"  k loop: min / median / max {np.min(loop_end - start):.1f} / {np.median(loop_end - start):.1f} / {np.max(loop_end - start):.1f} us")
print(f"  epilogue: min / median / max {np.min(end - loop_end):.1f} / {np.median(end - loop_end):.1f} / {np.max(end - loop_end):.1f} us")
from collections import Counter, defaultdict
place = both[1][live][:, 2]
xcc = (place >> 32) & 0xf
hw = place & 0xffffffff
cu = (xcc << 8) | (((hw >> 13) & 0x7) << 4) | ((hw >> 8) & 0xf)      # (XCC, shader engine, compute unit)
per_cu = Counter(int(c) for c in cu)
print(f"  compute units used: {len(per_cu)}; workgroups per unit: {sorted(Counter(per_cu.values()).items())}")
by_n = defaultdict(list)
for c, lo, en in zip(cu, loop_end - start, end):
    by_n[per_cu[int(c)]].append((lo, en))
for k in sorted(by_n):
    v = np.array(by_n[k])
    print(f"    units with {k} workgroup(s): k loop median {np.median(v[:, 0]):.1f} us (max {v[:, 0].max():.1f}), end median {np.median(v[:, 1]):.1f} us (max {v[:, 1].max():.1f})")
lp = loop_end - start
print("    k loop median per XCC: " + ", ".join(f"{int(x)}: {np.median(lp[xcc == x]):.1f}" for x in sorted(set(int(v) for v in xcc))))
three = np.array([per_cu[int(c)] == 3 for c in cu])
slow_cu = sorted(((np.median(lp[cu == c]), int(c)) for c in set(int(v) for v in cu[three])), reverse=True)[:8]
print("    slowest units (k loop median us, XCC / SE / CU): " + ", ".join(f"{t:.1f} @ {c >> 8}/{(c >> 4) & 7}/{c & 15}" for t, c in slow_cu))
se = (cu >> 4) & 7
print("    k loop median per shader engine (all XCCs): " + ", ".join(f"{int(x)}: {np.median(lp[se == x]):.1f}" for x in sorted(set(int(v) for v in se))))
cuix = cu & 15
print("    k loop median per CU index within its engine: " + ", ".join(f"{int(x)}: {np.median(lp[cuix == x]):.1f}" for x in sorted(set(int(v) for v in cuix))))
cyc[:, 2] = 0
ns = ks / 2.0
print("  counter ticks per stage of the last wave, median over the workgroups: DMA wait %.0f, LDS wait + barrier %.0f, - %.0f, fragment reads + MFMAs + DMA issue %.0f"
      % tuple(np.median(cyc[:, i] / ns) for i in range(4)))
slow = (loop_end - start) > np.quantile(loop_end - start, 0.9)
print("  the slowest tenth of the workgroups: DMA wait %.0f, LDS wait + barrier %.0f, - %.0f, fragment reads + MFMAs + DMA issue %.0f"
      % tuple(np.median(cyc[slow, i] / ns[slow]) for i in range(4)))
q = np.quantile(end, [0.1, 0.5, 0.9, 1.0])
print(f"  workgroup end times: 10 % {q[0]:.1f}, 50 % {q[1]:.1f}, 90 % {q[2]:.1f}, last {q[3]:.1f} us")

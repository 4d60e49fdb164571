#!/usr/bin/env python
"""Builds of the library side by side on the ViT forward (files under vfm-registration_amd/vfmreg/lib/), as tools/ab_two_libs_prep.py does
for the operand preparation.  The rows are every policy of tests/vit_plan_cases.py at the three shapes of tests/test_gpu_vit_plan.py
(depth 1) and the default policy at 6 and 24 images of 1200 x 1600 (depth 12).
    --cases libA.so libB.so ...     both builds in ONE process, row by row into workspaces filled alike: torch.equal of the tokens and of the
                                    whole workspace against the first build
    --sequence lib.so               one forward per row and nothing else: run it under `rocprofv3 --kernel-trace --output-format csv`
    --diff a.csv b.csv              the ordered (kernel, grid, workgroup, LDS bytes) lists of two such traces against each other
    --time libA.so libB.so [n ...]  the depth-12 forward at n images (6 84 168), the builds alternating, five timed blocks of each
A build without the "vit_trace_buffer" key (before the plan) gets the pointer through its "vit_gemm" code pair: that branch of bind() is
for comparing against such a build and is dead once none is around."""
import csv
import ctypes as C
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vfm-registration_amd"))
sys.path.insert(0, str(ROOT))


def diff(a, b):
    def launches(path):
        rows = [r for r in csv.DictReader(open(path)) if "vit_" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        return [(r["Kernel_Name"], r["Grid_Size_X"], r["Workgroup_Size_X"], r["LDS_Block_Size"]) for r in rows]
    la, lb = launches(a), launches(b)
    bad = [(i, x, y) for i, (x, y) in enumerate(zip(la, lb)) if x != y]
    print(f"{len(la)} and {len(lb)} ViT launches; {len(bad)} positions differ")
    kinds = {}
    for _, x, y in bad:
        kinds[(x, y)] = kinds.get((x, y), 0) + 1
    for (x, y), n in sorted(kinds.items(), key=lambda kv: -kv[1]):
        print(f"  {n} x  {x}\n   ->   {y}")


if sys.argv[1:2] == ["--diff"]:
    diff(*sys.argv[2:4])
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from tests import vit_plan_cases as vpc  # noqa: E402
from vfmreg import _lib, vit as V  # noqa: E402

base = _lib.load()
mode, names = sys.argv[1], [a for a in sys.argv[2:] if a.endswith(".so")]
libs = []
for name in names:
    l = C.CDLL(str(ROOT / "vfm-registration_amd" / "vfmreg" / "lib" / name))
    l.vfm_vit_forward.restype, l.vfm_vit_forward.argtypes = _lib.SIGNATURES["vfm_vit_forward"]
    l.vfm_config_create.argtypes = [C.POINTER(C.c_void_p)]
    l.vfm_config_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    l.vfm_config_use.argtypes = [C.c_void_p]
    l.vfm_config_destroy.argtypes = [C.c_void_p]
    libs.append((name, l))
trace = torch.zeros(2 * 4096 * 4 + 4096, dtype=torch.int64, device="cuda")   # every traced kernel's record layout fits


def bind(l, policy):
    """the row's policy in this build's own config, bound to the thread"""
    cfg = C.c_void_p()
    assert l.vfm_config_create(C.byref(cfg)) == 0
    for k, v in policy:
        if k == "vit_trace_buffer":
            v = trace.data_ptr()
            if l.vfm_config_set(cfg, k.encode(), v) != 0:   # a build before the plan: the two halves of the pointer
                for code, half in ((-11, v & 0xFFFFFFFF), (-12, v >> 32)):
                    assert l.vfm_config_set(cfg, b"vit_gemm", (code << 32) | half) == 0
        else:
            assert l.vfm_config_set(cfg, k.encode(), v) == 0, k
    l.vfm_config_use(cfg)
    return cfg


def unbind(l, cfg):
    l.vfm_config_use(None)
    l.vfm_config_destroy(cfg)


def forward(l, model, imgs, out, ws):
    B, H, W, _ = imgs.shape
    rc = l.vfm_vit_forward(C.byref(model.cfg), model.blob.data_ptr(), imgs.data_ptr(), B, H, W, out.data_ptr(), ws.data_ptr(), ws.numel(),
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


def setup(s, seed=3):
    model = V.ViTS14(V.random_weights(seed=seed, dim=s.dim, depth=s.depth, mlp=s.mlp), s.H, s.W)
    imgs = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (s.B, s.H, s.W, 3), dtype=np.uint8)).cuda()
    nws = base.vfm_vit_workspace_bytes(C.byref(model.cfg), s.B)
    return model, imgs, nws


def rows():
    policies = list(dict.fromkeys(c.cfg for c in vpc.CASES))
    for name, s in vpc.GPU_SHAPES.items():
        yield name, s, policies
    for B in (6, 24):
        yield f"vit-s-{B}", vpc.VITS(B), [()]


if mode == "--time":
    counts = [int(a) for a in sys.argv[2:] if a.isdigit()] or [6, 84, 168]
    for B in counts:
        model, imgs, nws = setup(vpc.VITS(B))
        out = torch.empty((B, 16, model.patch_w, 384), device="cuda")
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
        reps = 200 if B <= 12 else 20
        blocks = {name: [] for name, _ in libs}
        for block in range(6):
            for name, l in libs:
                for _ in range(3):
                    forward(l, model, imgs, out, ws)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    forward(l, model, imgs, out, ws)
                e1.record()
                torch.cuda.synchronize()
                if block:   # (the first block of each build warms the device up)
                    blocks[name].append(e0.elapsed_time(e1) / reps)
        for name, _ in libs:
            v = sorted(blocks[name])
            print(f"{B:3d} images  {name:28s} blocks {' '.join(f'{x:.4f}' for x in blocks[name])} ms   median {v[len(v) // 2]:.4f}   slowest {v[-1]:.4f}", flush=True)
    sys.exit(0)

total = differ = 0
for tag, s, policies in rows():
    model, imgs, nws = setup(s)
    out = torch.empty((s.B, 16, model.patch_w, s.dim), device="cuda")
    for policy in policies:
        got = []
        for name, l in libs:
            ws = torch.full((nws,), 0x5A, dtype=torch.uint8, device="cuda")
            out.fill_(float("nan"))
            cfg = bind(l, policy)
            forward(l, model, imgs, out, ws)
            torch.cuda.synchronize()
            unbind(l, cfg)
            got.append((out.clone().view(torch.int32), ws))
        if mode == "--cases":
            same = [all(bool(torch.equal(x, y)) for x, y in zip(got[0], g)) for g in got[1:]]
            total += 1
            differ += not all(same)
            print(f"{tag:8s} {dict(policy)!s:110s} tokens + workspace equal to {libs[0][0]}: {same}", flush=True)
if mode == "--cases":
    print(f"--cases: {total} rows, {differ} differ", flush=True)

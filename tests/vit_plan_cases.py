"""The case table of the ViT forward's plan (csrc/vit_plan.h: resolve_vit), shared by tests/test_vit_plan.py (CPU: the read-back
vfm_debug_vit_plan), tests/test_gpu_vit_plan.py (the forced forms through a real forward) and tools/ab_two_libs_vit.py (kernel sequence and
bytes against another build).  WHICH kernel a row expects at each stage was worked by hand from vfm_vit_forward and launch_gemm<EPI> as they
stood BEFORE the plan existed -- the ladders with their decisions inline -- and is written out here stage by stage, never asked of the
resolver; the helpers below only spell a chosen kernel's name and put the shape into that launcher's grid expression.

The arithmetic behind the default-policy rows, ViT-S at 1200 x 1600 (21 patch columns, 337 tokens, 11 token tiles per image, 6 heads) on 256
compute units, B images: tiles = 11 B, groups = ceil(tiles / 4).
  fused QKV   per_xcd = ceil(6 B / 8), rounds = ceil(per_xcd / 32), last = per_xcd - 32 (rounds - 1); on: B >= 24 and (rounds >= 3 or
              rounds == 1 or 4 last >= 32).  B = 24: 18, 1 round; 42: 32, 1 round; 44: 33, last 1; 48: 36, last 4; 54: 41, last 9;
              84: 63, last 31; 86: 65, 3 rounds
  fused MLP   rounds = ceil(groups / 256); on: rounds >= 2 and 5 groups >= 4 rounds 256.  B = 84: 231 groups, 1 round; 144: 396, 1980 < 2048;
              156: 429, 2145 >= 2048; 168: 462; 192: 528, 3 rounds, 2640 < 3072; 252: 693, 3465 >= 3072
  token-stationary QKV / fc1   on: groups >= 192 and (groups % 256 == 0 or 4 (groups % 256) >= 768).  B = 69: 190; 70: 193; 93: 256; 94: 259
              (3 in the second round); 96: 264 (8); and the two-tile form (default) since 1152 / 64, 1536 / 64 >= 8 and 24 k-steps % 4 == 0
  LDS-tiled   groups x (N / 128) >= 256: N = 384 (patch, proj, fc2) from 86 groups, QKV (1152) from 29, fc1 (1536) from 22"""
from __future__ import annotations

from typing import NamedTuple, Optional

CUS = 256
TRACE_BUFFER = 0x7F0012345600   # (a device address the resolver never dereferences)
KP = 608                        # 3 x 14 x 14 = 588 padded to 32


def cdiv(a, b):
    return -(-a // b)


class Shape(NamedTuple):
    dim: int
    mlp: int
    depth: int
    B: int
    H: int
    W: int

    @property
    def heads(self):
        return self.dim // 64

    @property
    def patch_w(self):
        return int((14 * 16) / self.H * self.W / 14)   # vfmreg/vit.py, ViTS14.__init__

    @property
    def qt(self):       # token tiles per image
        return cdiv(16 * self.patch_w + 1, 32)

    @property
    def tiles(self):
        return self.B * self.qt

    @property
    def groups(self):
        return cdiv(self.tiles, 4)


VITS = lambda B, depth=12: Shape(384, 1536, depth, B, 1200, 1600)   # noqa: E731  (11 tiles)
# the shapes of tests/test_gpu_vit_plan.py: a partial last group of four tiles (55) and B x heads no multiple of 8; 13 tiles; ViT-B width, 9 tiles
GPU_SHAPES = {"s-11t": Shape(384, 1536, 1, 5, 560, 700), "s-13t": Shape(384, 1536, 1, 9, 1200, 1800), "b-9t": Shape(768, 3072, 1, 2, 560, 600)}


# ---- a chosen kernel -> "<name>@<grid>x<block>+<lds>", each with the grid expression of the launcher that used to hold it
def _n(s, epi):
    return {"PATCH": s.dim, "QKV": 3 * s.dim, "RESID": s.dim, "GELU": s.mlp}[epi]


def D(s, epi, nt=1, pf=8, wpw=1, xcd=1):           # launch_gemm_cfg<EPI, NT, PF>
    cols = _n(s, epi) // (32 * nt)
    grid = 8 * cdiv(cdiv(s.tiles, 8) * cols, wpw) if xcd else cdiv(s.tiles * cols, wpw)
    return f"vit_gemm_kernel<{epi},{nt},{pf}>@{grid}x{64 * wpw}+0"


def L(s, epi, kb=2, ns=3, dbg=False):              # VIT_LDS(KB, NS)
    grid = 8 * cdiv(s.groups, 8) * (_n(s, epi) // 128)
    return f"vit_gemm_lds_kernel<{epi},{kb},{ns}{',dbg' if dbg else ''}>@{grid}x256+{ns * 8 * kb * 1024}"


def WIDE(s, dbg=False):                            # the 128 x 384 form (RESID, N = 384)
    return f"vit_gemm_lds_kernel<RESID,2,4,3,8{',dbg' if dbg else ''}>@{8 * cdiv(s.groups, 8)}x512+131072"


def A(s, epi, nw=12, nt=False):                    # VIT_ASTAT(NW) / the 112 case
    return f"vit_gemm_astat_kernel<{epi},{nw},6{',nt' if nt else ''}>@{s.groups}x{64 * nw}+{4 * (s.dim // 16) * 1024}"


def A2(s, epi):
    return f"vit_gemm_astat2_kernel<{epi},8,4>@{s.groups}x512+{4 * (s.dim // 16) * 1024}"


def AT(s, xcd=1):                                  # VIT_ATT, per tile
    grid = 8 * cdiv(cdiv(s.tiles, 8) * s.heads, 4) if xcd else cdiv(s.B * s.heads * s.qt, 4)
    return f"vit_attention_kernel<{s.qt}>@{grid}x256+0"


def ATL(s):                                        # VIT_ATT, K / V^T through the LDS
    return f"vit_attention_lds_kernel<{s.qt}>@{s.B * s.heads * cdiv(s.qt, 4)}x256+{s.qt * 4096 + 16384}"


def F(s):                                          # VIT_FQA
    return f"vit_qkv_attention_kernel<{s.qt}>@{8 * cdiv(s.B * s.heads, 8)}x256+{48 * 1024 + 2 * s.qt * 4096 + s.qt * 32 * 8}"


def MLP(s):
    return f"vit_mlp_kernel@{s.groups}x256+{144 * 1024 + 2 * 1536 * 4}"


def PRE(s, patch=True):
    M = s.tiles * 32
    return f"vit_preprocess_patch_kernel@{M}x256+0" if patch else f"vit_preprocess_kernel@{cdiv(M * (KP // 16) * 2, 256)}x256+0"


class Case(NamedTuple):
    id: str
    shape: Shape
    cfg: tuple                 # ((policy key, value), ...) beside the factory settings
    cus: int
    stages: tuple              # pre, patch, qkv, att, proj, fc1, fc2: a launch, or None where the stage is inside the kernel before it
    launches: int
    trace: Optional[str]
    W: int                     # the source width the resolver is told


# the forced forms of tests/test_gpu_vit_stages.py (BASE, GEMM, ATT): the GPU tests run every one of them
BASE = dict(vit_fused_qkv=-1, vit_fused_mlp=-1, vit_astat_min=-1, vit_lds_min_wg=0, vit_att_lds_min=0)
GEMM = {"direct": {}, "lds": dict(vit_lds_min_wg=1), "lds-wide": dict(vit_lds_min_wg=1, vit_wide_tile=1),
        "astat": dict(vit_astat_min=1, vit_astat_two=0), "astat2": dict(vit_astat_min=1, vit_astat_two=1)}
ATT = {"per-tile": {}, "lds": dict(vit_att_lds_min=1), "fused": dict(vit_fused_qkv=1)}
FORCED = {f"gemm={k}": {**BASE, **v} for k, v in GEMM.items()}
FORCED.update({f"att={k}": {**BASE, **v} for k, v in ATT.items() if k != "per-tile"})
FORCED["mlp=fused"] = {**BASE, "vit_fused_mlp": 1}
FORCED["qkv+mlp=fused"] = {**BASE, "vit_fused_qkv": 1, "vit_fused_mlp": 1}


def _cases():
    out = []

    def add(tag, s, stages, cfg=(), cus=CUS, trace=None, W=None):
        cfg = tuple(dict(cfg).items())
        stages = tuple(stages)
        assert len(stages) == 7
        per_block = sum(x is not None for x in stages[2:])
        out.append(Case(tag, s, cfg, cus, stages, 2 + s.depth * per_block + 1, trace, s.W if W is None else W))

    def block(s, patch, qkv, att, proj, fc1, fc2, pre=True):
        return (PRE(s, pre), patch, qkv, att, proj, fc1, fc2)

    # ---- the default policy, ViT-S at 1200 x 1600 (the arithmetic is in the module's docstring)
    s = VITS(6)      # one scan: 17 groups, nothing reaches 256 workgroups; 63 launches
    add("default-B6", s, block(s, D(s, "PATCH"), D(s, "QKV"), ATL(s), D(s, "RESID"), D(s, "GELU"), D(s, "RESID")))
    assert out[-1].launches == 63
    s = VITS(23)     # 64 groups: QKV and fc1 LDS-tiled, not yet fused
    add("default-B23", s, block(s, D(s, "PATCH"), L(s, "QKV"), ATL(s), D(s, "RESID"), L(s, "GELU"), D(s, "RESID")))
    s = VITS(24)     # fused QKV from 24 images on
    add("default-B24", s, block(s, D(s, "PATCH"), F(s), None, D(s, "RESID"), L(s, "GELU"), D(s, "RESID")))
    for B in (42, 54):      # 116 / 149 groups: every GEMM LDS-tiled; a full first round / a second round at least a quarter full
        s = VITS(B)
        add(f"default-B{B}", s, block(s, L(s, "PATCH"), F(s), None, L(s, "RESID"), L(s, "GELU"), L(s, "RESID")))
    for B in (44, 48):      # a second round of 1 / 4 workgroups per XCD: the two kernels
        s = VITS(B)
        add(f"default-B{B}", s, block(s, L(s, "PATCH"), L(s, "QKV"), ATL(s), L(s, "RESID"), L(s, "GELU"), L(s, "RESID")))
    for B, stationary in ((69, False), (70, True), (84, True), (86, True), (93, True), (94, False), (96, False), (144, False), (192, False)):
        s = VITS(B)         # fused QKV throughout; fc1 token-stationary (two tiles per wave) where its rounds are full
        add(f"default-B{B}", s, block(s, L(s, "PATCH"), F(s), None, L(s, "RESID"), A2(s, "GELU") if stationary else L(s, "GELU"), L(s, "RESID")))
    for B in (156, 168, 252):   # fused MLP: two rounds and more with a full last one (168: the token-stationary rule holds too, fc1 is inside)
        s = VITS(B)
        add(f"default-B{B}", s, block(s, L(s, "PATCH"), F(s), None, L(s, "RESID"), MLP(s), None))
    # ... the token-stationary QKV where the stage is not fused away
    for B, stationary in ((69, False), (70, True), (93, True), (94, False), (96, False)):
        s = VITS(B)
        add(f"two-kernels-B{B}", s, block(s, L(s, "PATCH"), A2(s, "QKV") if stationary else L(s, "QKV"), ATL(s), L(s, "RESID"),
                                          A2(s, "GELU") if stationary else L(s, "GELU"), L(s, "RESID")), cfg=dict(vit_fused_qkv=-1))
    # ... on other devices: 128 compute units -- 36 images = 99 groups fill one round (396 >= 384), 84 = 231 groups are two rounds (1155 >= 1024)
    s = VITS(36)
    add("cus128-B36", s, block(s, L(s, "PATCH"), F(s), None, L(s, "RESID"), A2(s, "GELU"), L(s, "RESID")), cus=128)
    add("cus256-B36", s, block(s, L(s, "PATCH"), F(s), None, L(s, "RESID"), L(s, "GELU"), L(s, "RESID")))
    s = VITS(84)
    add("cus128-B84", s, block(s, L(s, "PATCH"), F(s), None, L(s, "RESID"), MLP(s), None), cus=128)
    # ... the "vit_fused_*" overrides: from n images on, never
    s = VITS(6)
    add("fused-qkv-from-6", s, block(s, D(s, "PATCH"), F(s), None, D(s, "RESID"), D(s, "GELU"), D(s, "RESID")), cfg=dict(vit_fused_qkv=6))
    add("fused-qkv-from-7", s, block(s, D(s, "PATCH"), D(s, "QKV"), ATL(s), D(s, "RESID"), D(s, "GELU"), D(s, "RESID")), cfg=dict(vit_fused_qkv=7))
    add("fused-mlp-from-6", s, block(s, D(s, "PATCH"), D(s, "QKV"), ATL(s), D(s, "RESID"), MLP(s), None), cfg=dict(vit_fused_mlp=6))
    s = VITS(168)
    add("never-fused-B168", s, block(s, L(s, "PATCH"), A2(s, "QKV"), ATL(s), L(s, "RESID"), A2(s, "GELU"), L(s, "RESID")),
        cfg=dict(vit_fused_qkv=-1, vit_fused_mlp=-1))

    # ---- 13 token tiles: the fused QKV kernel is refused whatever the key says (30 groups: QKV and fc1 reach 256 workgroups)
    s = Shape(384, 1536, 12, 9, 1200, 1800)
    for tag, cfg in (("default", {}), ("fused-qkv-1", dict(vit_fused_qkv=1))):
        add(f"13-tiles-{tag}", s, block(s, D(s, "PATCH"), L(s, "QKV"), ATL(s), D(s, "RESID"), L(s, "GELU"), D(s, "RESID")), cfg=cfg)
    s = Shape(384, 1536, 12, 24, 1200, 1800)   # (24 images: the policy's threshold)
    add("13-tiles-B24", s, block(s, D(s, "PATCH"), L(s, "QKV"), ATL(s), D(s, "RESID"), L(s, "GELU"), D(s, "RESID")))
    # ---- dim 768 / mlp 3072: no fused kernel, and no token-stationary one (128 rows x 768 channels = 192 KiB)
    s = Shape(768, 3072, 12, 2, 560, 600)
    for tag, cfg in (("default", {}), ("all-on", dict(vit_fused_qkv=1, vit_fused_mlp=1, vit_astat_min=1))):
        add(f"vit-b-{tag}", s, block(s, D(s, "PATCH"), D(s, "QKV"), ATL(s), D(s, "RESID"), D(s, "GELU"), D(s, "RESID")), cfg=cfg)
    add("vit-b-lds", s, block(s, L(s, "PATCH"), L(s, "QKV"), ATL(s), L(s, "RESID"), L(s, "GELU"), L(s, "RESID")),
        cfg=dict(vit_lds_min_wg=1, vit_wide_tile=1))   # (the 128 x 384 form is for N = 384)
    s = Shape(768, 3072, 12, 30, 560, 600)             # 68 groups x 6 = 408 workgroups at N = 768
    add("vit-b-B30", s, block(s, L(s, "PATCH"), L(s, "QKV"), ATL(s), L(s, "RESID"), L(s, "GELU"), L(s, "RESID")), cfg=dict(vit_astat_min=1))
    # ---- dim 128 / mlp 256 (tests/test_gpu_vit.py): N = 128 ... 384 all LDS-tiled from one workgroup on; the token-stationary kernel takes
    # QKV (12 channel tiles: twelve waves, too few for the two-tile form) and not fc1 (8 channel tiles)
    s = Shape(128, 256, 2, 9, 300, 400)
    add("dim128-lds", s, block(s, L(s, "PATCH"), L(s, "QKV"), ATL(s), L(s, "RESID"), L(s, "GELU"), L(s, "RESID")), cfg=dict(vit_lds_min_wg=1))
    add("dim128-astat", s, block(s, D(s, "PATCH"), A(s, "QKV"), ATL(s), D(s, "RESID"), D(s, "GELU"), D(s, "RESID")), cfg=dict(vit_astat_min=1))

    # ---- every forced form of tests/test_gpu_vit_stages.py at the three shapes of the GPU test
    for name, s in GPU_SHAPES.items():
        small = s.dim == 384
        d = (D(s, "PATCH"), D(s, "QKV"), AT(s), D(s, "RESID"), D(s, "GELU"), D(s, "RESID"))
        lds = (L(s, "PATCH"), L(s, "QKV"), AT(s), L(s, "RESID"), L(s, "GELU"), L(s, "RESID"))
        forms = {
            "gemm=direct": d,
            "gemm=lds": lds,
            "gemm=lds-wide": (lds[0], lds[1], lds[2], WIDE(s), lds[4], WIDE(s)) if small else lds,
            "gemm=astat": (d[0], A(s, "QKV"), d[2], d[3], A(s, "GELU"), d[5]) if small else d,
            "gemm=astat2": (d[0], A2(s, "QKV"), d[2], d[3], A2(s, "GELU"), d[5]) if small else d,
            "att=lds": (d[0], d[1], ATL(s), d[3], d[4], d[5]),
            "att=fused": (d[0], F(s), None, d[3], d[4], d[5]) if small and s.qt <= 12 else d,
            "mlp=fused": (d[0], d[1], d[2], d[3], MLP(s), None) if small else d,
            "qkv+mlp=fused": ((d[0], F(s), None, d[3], MLP(s), None) if s.qt <= 12 else (d[0], d[1], d[2], d[3], MLP(s), None)) if small else d,
        }
        assert set(forms) == set(FORCED)
        for form, stages in forms.items():
            add(f"{name}-{form}", s, block(s, *stages), cfg=FORCED[form])

    # ---- the single keys, one scan of ViT-S
    s = VITS(6)
    base = dict(patch=D(s, "PATCH"), qkv=D(s, "QKV"), att=ATL(s), proj=D(s, "RESID"), fc1=D(s, "GELU"), fc2=D(s, "RESID"))

    def one(tag, cfg, pre=True, trace=None, W=None, **changed):
        add(tag, s, block(s, pre=pre, **{**base, **changed}), cfg=cfg, trace=trace, W=W)

    # "vit_lds_shape" with the LDS-tiled kernel everywhere: the stages of four k-steps leave the patch embedding (38 k-steps) to the direct kernel
    for shape in (23, 24, 25, 26, 42, 43, 99):
        kb, ns = (shape // 10, shape % 10) if shape != 99 else (2, 3)   # (an unknown shape: 23)
        one(f"lds-shape-{shape}", dict(vit_lds_min_wg=1, vit_lds_shape=shape), patch=D(s, "PATCH") if kb == 4 else L(s, "PATCH", kb, ns),
            qkv=L(s, "QKV", kb, ns), proj=L(s, "RESID", kb, ns), fc1=L(s, "GELU", kb, ns), fc2=L(s, "RESID", kb, ns))
    # "vit_astat_nw", one channel tile per wave: QKV has 36 channel tiles, fc1 48 -- a count that does not divide them is twelve; 4 divides
    # both and is no instantiation: twelve waves as well
    for nw, q, f in ((0, 12, 12), (6, 6, 6), (8, 12, 8), (12, 12, 12), (16, 12, 16), (5, 12, 12), (4, 12, 12)):
        one(f"astat-nw-{nw}", dict(vit_astat_min=1, vit_astat_two=0, vit_astat_nw=nw), qkv=A(s, "QKV", q), fc1=A(s, "GELU", f))
    one("astat-nw-112", dict(vit_astat_min=1, vit_astat_two=0, vit_astat_nw=112), qkv=A(s, "QKV", 12, nt=True), fc1=A(s, "GELU", 12, nt=True))
    one("astat-nw-112-two", dict(vit_astat_min=1, vit_astat_nw=112), qkv=A2(s, "QKV"), fc1=A2(s, "GELU"))
    one("astat-min-17", dict(vit_astat_min=17), qkv=A2(s, "QKV"), fc1=A2(s, "GELU"))     # 17 groups
    one("astat-min-18", dict(vit_astat_min=18))
    # the direct kernel's tile: "vit_cfg_narrow" for N <= 512 (patch, proj, fc2), "vit_cfg_wide" above
    one("cfg-narrow-116", dict(vit_cfg_narrow=116), patch=D(s, "PATCH", 1, 16), proj=D(s, "RESID", 1, 16), fc2=D(s, "RESID", 1, 16))
    one("cfg-narrow-208", dict(vit_cfg_narrow=208), patch=D(s, "PATCH", 2, 8), proj=D(s, "RESID", 2, 8), fc2=D(s, "RESID", 2, 8))
    one("cfg-wide-116", dict(vit_cfg_wide=116), qkv=D(s, "QKV", 1, 16), fc1=D(s, "GELU", 1, 16))
    one("cfg-wide-208", dict(vit_cfg_wide=208), qkv=D(s, "QKV", 2, 8), fc1=D(s, "GELU", 2, 8))
    one("cfg-unknown", dict(vit_cfg_narrow=300, vit_cfg_wide=-1))
    for wpw in (2, 4):
        one(f"wpw-{wpw}", dict(vit_wpw=wpw), **{k: D(s, e, wpw=wpw) for k, e in (("patch", "PATCH"), ("qkv", "QKV"), ("proj", "RESID"),
                                                                                 ("fc1", "GELU"), ("fc2", "RESID"))})
    one("wpw-4-wide-208", dict(vit_wpw=4, vit_cfg_wide=208), patch=D(s, "PATCH", wpw=4), qkv=D(s, "QKV", 2, 8, wpw=4), proj=D(s, "RESID", wpw=4),
        fc1=D(s, "GELU", 2, 8, wpw=4), fc2=D(s, "RESID", wpw=4))
    one("xcd-0", dict(vit_xcd=0, vit_att_lds_min=0), att=AT(s, xcd=0),
        **{k: D(s, e, xcd=0) for k, e in (("patch", "PATCH"), ("qkv", "QKV"), ("proj", "RESID"), ("fc1", "GELU"), ("fc2", "RESID"))})
    one("att-per-tile", dict(vit_att_lds_min=0), att=AT(s))
    one("att-lds-from-7", dict(vit_att_lds_min=7), att=AT(s))
    one("att-lds-from-6", dict(vit_att_lds_min=6))
    one("preprocess-unit", dict(vit_preprocess_patch=0), pre=False)
    one("preprocess-one-column", {}, pre=False, W=1)   # the per-patch kernel reads two source columns
    # ---- the trace buffer goes to ONE launch: the stage "vit_trace_fused" names, where that stage runs the kernel that keeps a trace
    buf = dict(vit_trace_buffer=TRACE_BUFFER)
    lds_all = dict(patch=L(s, "PATCH"), qkv=L(s, "QKV"), proj=L(s, "RESID"), fc1=L(s, "GELU"), fc2=L(s, "RESID"))
    one("trace-0-nothing-traceable", {**buf})
    one("trace-0-astat-fc1", {**buf, "vit_astat_min": 1, "vit_astat_two": 0}, trace="fc1", qkv=A(s, "QKV"), fc1=A(s, "GELU"))
    one("trace-0-lds-fc2", {**buf, "vit_lds_min_wg": 1}, trace="fc2", **{**lds_all, "fc2": L(s, "RESID", dbg=True)})
    one("trace-0-lds-wide-fc2", {**buf, "vit_lds_min_wg": 1, "vit_wide_tile": 1}, trace="fc2", **{**lds_all, "proj": WIDE(s), "fc2": WIDE(s, dbg=True)})
    one("trace-0-astat-before-lds", {**buf, "vit_lds_min_wg": 1, "vit_astat_min": 1, "vit_astat_two": 0}, trace="fc1",
        **{**lds_all, "qkv": A(s, "QKV"), "fc1": A(s, "GELU")})
    one("trace-0-astat2-keeps-none", {**buf, "vit_lds_min_wg": 1, "vit_astat_min": 1}, trace="fc2",
        **{**lds_all, "qkv": A2(s, "QKV"), "fc1": A2(s, "GELU"), "fc2": L(s, "RESID", dbg=True)})
    one("trace-0-no-buffer", dict(vit_lds_min_wg=1), **lds_all)
    one("trace-1-fused-qkv", {**buf, "vit_trace_fused": 1, "vit_fused_qkv": 1}, trace="qkv", qkv=F(s), att=None)
    one("trace-1-two-kernels", {**buf, "vit_trace_fused": 1, "vit_lds_min_wg": 1}, **lds_all)
    one("trace-2-lds-proj", {**buf, "vit_trace_fused": 2, "vit_lds_min_wg": 1}, trace="proj", **{**lds_all, "proj": L(s, "RESID", dbg=True)})
    one("trace-2-direct", {**buf, "vit_trace_fused": 2})
    one("trace-3-mlp", {**buf, "vit_trace_fused": 3, "vit_fused_mlp": 1, "vit_lds_min_wg": 1}, trace="fc1",
        **{**lds_all, "fc1": MLP(s), "fc2": None})
    one("trace-3-two-kernels", {**buf, "vit_trace_fused": 3, "vit_lds_min_wg": 1}, **lds_all)
    one("trace-4-unknown", {**buf, "vit_trace_fused": 4, "vit_lds_min_wg": 1, "vit_fused_qkv": 1, "vit_fused_mlp": 1},
        **{**lds_all, "qkv": F(s), "att": None, "fc1": MLP(s), "fc2": None})
    return out


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)

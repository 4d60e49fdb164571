"""The ViT forward's plan on the device: under every forced form of tests/vit_plan_cases.py, at its three shapes (a partial last group of
four token tiles with B x heads no multiple of 8; 13 token tiles; ViT-B width), one depth-1 forward into a sentinel-filled workspace runs
what the read-back vfm_debug_vit_plan says it runs -- q / k / V^T stay unwritten exactly under vit_qkv_attention_kernel, h exactly under
vit_mlp_kernel --, gives the tokens of the direct-kernel forward bit for bit, and with a trace buffer bound hands it to the planned launch
and no other: only that kernel's region of the buffer changes, whatever "vit_trace_fused" says."""
import ctypes as C

import numpy as np
import pytest

from tests import vit_plan_cases as vpc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT = 0x5A
TRACE_WORDS = 2 * 4096 * 4 + 1024          # the LDS-tiled kernel's [2][4096][4] and a margin behind it
_cache = {}


def _model(name):
    """(model, images, tokens of the direct-kernel forward) of a shape, built once"""
    if name not in _cache:
        from vfmreg import _lib
        from vfmreg import vit as V
        s = vpc.GPU_SHAPES[name]
        w = V.random_weights(seed=29, dim=s.dim, depth=s.depth, mlp=s.mlp)
        imgs = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (s.B, s.H, s.W, 3), dtype=np.uint8)).cuda()
        model = V.ViTS14(w, s.H, s.W, device="cuda")
        assert model.patch_w == s.patch_w
        with _lib.using(_lib.Config(**vpc.FORCED["gemm=direct"])):
            direct = model.forward(imgs).clone()
        torch.cuda.synchronize()
        assert torch.isfinite(direct).all()
        _cache[name] = (model, imgs, direct)
    return _cache[name]


def _traced_words(plan):
    """the words of the trace buffer the planned launch may write: (lo, hi) ranges by the kernel's own record layout"""
    if plan["trace"] is None:
        return []
    kernel, rest = plan[plan["trace"]].split("@")
    grid = int(rest.split("x")[0])
    if kernel.startswith("vit_gemm_lds_kernel"):           # [2][4096][4]: stamps, and counters + placement
        return [(0, 4 * grid), (4 * 4096, 4 * 4096 + 4 * grid)]
    words = {"vit_gemm_astat_kernel": 4, "vit_qkv_attention_kernel": 16, "vit_mlp_kernel": 8}[kernel.split("<")[0]]
    return [(0, words * grid)]


@pytest.mark.parametrize("form", sorted(vpc.FORCED))
@pytest.mark.parametrize("name", sorted(vpc.GPU_SHAPES))
def test_a_forward_runs_its_plan(name, form):
    from vfmreg import _lib
    lib = _lib.load()
    model, imgs, direct = _model(name)
    s = vpc.GPU_SHAPES[name]
    table = {c.id: c for c in vpc.CASES}[f"{name}-{form}"]
    offs, nbytes = (C.c_int64 * 8)(), (C.c_int64 * 8)()
    _lib.check(lib.vfm_debug_vit_workspace_layout(C.byref(model.cfg), s.B, offs, nbytes), "vit_workspace_layout")
    ws = model._ws[(s.B, 0)]
    part = {n: ws[offs[i]:offs[i] + nbytes[i]] for i, n in enumerate(("x", "a", "xh", "stats", "h", "q", "k", "vt"))}
    trace = torch.empty(TRACE_WORDS, dtype=torch.int64, device="cuda")
    seen = set()
    for fused in (0, 1, 2, 3):
        cfg = _lib.Config(**vpc.FORCED[form]).set("vit_trace_buffer", trace.data_ptr()).set("vit_trace_fused", fused)
        with _lib.using(cfg):
            plan = _lib.vit_plan(model.cfg, s.B, s.W)
            assert [plan[st] and plan[st].replace(",dbg>", ">") for st in _lib.VIT_STAGES] == list(table.stages), (plan, table.stages)
            ws.fill_(SENT)
            trace.fill_(-1)
            out = model.forward(imgs)
        torch.cuda.synchronize()
        unwritten = {n for n, v in part.items() if bool((v == SENT).all())}
        assert ({"q", "k", "vt"} <= unwritten) == plan["qkv"].startswith("vit_qkv_attention_kernel") == (plan["att"] is None), (fused, unwritten)
        assert ("h" in unwritten) == plan["fc1"].startswith("vit_mlp_kernel") == (plan["fc2"] is None), (fused, unwritten)
        assert unwritten <= {"q", "k", "vt", "h"}
        assert torch.equal(out, direct), (fused, float((out - direct).abs().max()))
        changed = trace != -1
        for lo, hi in _traced_words(plan):
            assert bool(changed[lo:hi].any()), (fused, plan["trace"], lo, hi)
            changed[lo:hi] = False
        assert not bool(changed.any()), (fused, plan["trace"], torch.nonzero(changed)[:8].tolist())
        seen.add(plan["trace"])
    expected = {None}   # which stages a form can hand the buffer to
    if s.dim == 384:
        expected |= {"gemm=astat": {"fc1"}, "gemm=lds": {"fc2", "proj"}, "gemm=lds-wide": {"fc2", "proj"}, "mlp=fused": {"fc1"},
                     "att=fused": {"qkv"} if s.qt <= 12 else set(), "qkv+mlp=fused": {"qkv", "fc1"} if s.qt <= 12 else {"fc1"}}.get(form, set())
    elif form in ("gemm=lds", "gemm=lds-wide"):
        expected |= {"fc2", "proj"}
    assert seen == expected, (seen, expected)

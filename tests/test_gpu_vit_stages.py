"""csrc/vit.hip stage by stage against tests/vit_stages.py (fp64), every stage fed with what the DEVICE left in the workspace for it
(vfm_debug_vit_workspace_layout), under the bounds derived there -- and the attention kernels at every token-tile count.

How a stage's input survives a forward.  Depth-1 models; a LayerScale of exactly 0 keeps the residual stream as it was (fma(0, v, x) = x),
so three forwards of the same images under the same kernel policy isolate every stage:
    A  ls1 = ls2 = 0   x, xh, stats are the patch embedding's; q, k, V^T, the attention output a and the hidden h are computed from them
    B  ls1 != 0, ls2 = 0   x = x_A + ls1 (a W_proj^T + b): the proj stage, from a and x_A
    C  ls1 = 0, ls2 != 0   x = x_A + ls2 (h W_fc2^T + b): the fc2 stage, from h and x_A
(the kernels are deterministic: x_A is what B and C started from).  Under vit_fused_qkv q, k, V^T are never written (the workspace is filled
with a sentinel first, and the test asserts they were not): the kernel's a is held to the PLAIN attention bound from the q, k, V^T that the
two-kernel run of the same forward left -- the fused kernel states them bit-equal, and a bound composed from the QKV stage's would admit a
wrong mask or scale.  Under vit_fused_mlp h is never written: x_C likewise under the plain fc2 bound from the two-kernel run's h.  The pixels the preprocessing wrote are read through a probe model with a one-hot patch
embedding.  Every comparison prints ``STAGE <stage> <case> err/bound=<worst ratio>`` (profiles/vit_stage_bounds.md keeps a run's figures)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import vit_stages as VS  # noqa: E402
from tests.test_vit_stages import checkerboard, smooth_images, stage_case, stage_weights as _weights  # noqa: E402

BASE = dict(vit_fused_qkv=-1, vit_fused_mlp=-1, vit_astat_min=-1, vit_lds_min_wg=0, vit_att_lds_min=0)
GEMM = {"direct": {}, "lds": dict(vit_lds_min_wg=1), "lds-wide": dict(vit_lds_min_wg=1, vit_wide_tile=1),
        "astat": dict(vit_astat_min=1, vit_astat_two=0), "astat2": dict(vit_astat_min=1, vit_astat_two=1)}
ATT = {"per-tile": {}, "lds": dict(vit_att_lds_min=1), "fused": dict(vit_fused_qkv=1)}


def _config(**kv):
    from vfmreg import _lib
    cfg = _lib.Config()
    for k, v in {**BASE, **kv}.items():
        cfg.set(k, v)
    return cfg


def _forward(w, imgs, patch_h=16, **kv):
    """one forward -> (tokens, the workspace's buffers in plain layouts, the packed operands)"""
    from vfmreg import _lib
    from vfmreg import vit as V
    lib = _lib.load()
    B, H, W, _ = imgs.shape
    model = V.ViTS14(w, H, W, device="cuda", patch_h=patch_h)
    SENT = 0x5A   # the workspace starts as a sentinel: what a forward did not write is seen
    model._ws[(B, 0)] = torch.full((lib.vfm_vit_workspace_bytes(C.byref(model.cfg), B),), SENT, dtype=torch.uint8, device="cuda")
    with _lib.using(_config(**kv)):
        out = model.forward(torch.from_numpy(imgs).cuda())
    torch.cuda.synchronize()
    ws = model._ws[(B, 0)].cpu().numpy()
    offs, nbytes = (C.c_int64 * 8)(), (C.c_int64 * 8)()
    _lib.check(lib.vfm_debug_vit_workspace_layout(C.byref(model.cfg), B, offs, nbytes), "vit_workspace_layout")
    assert offs[7] + nbytes[7] == ws.size == lib.vfm_vit_workspace_bytes(C.byref(model.cfg), B)
    raw = {n: ws[offs[i]:offs[i] + nbytes[i]] for i, n in enumerate(("x", "a", "xh", "stats", "h", "q", "k", "vt"))}
    P = VS.pack(w, patch_h, model.patch_w)
    D, Tp, heads, mlp = P["D"], P["Tp"], P["heads"], w["blocks.0.mlp.fc1.weight"].shape[0]
    M = B * Tp
    h16 = lambda n: raw[n].view(np.float16)   # noqa: E731
    sx, sq = VS.stats_to_rows(raw["stats"].view(np.float32), M, D)
    unwritten = {n for n, v in raw.items() if (v == SENT).all()}
    r = {"unwritten": unwritten, "x": raw["x"].view(np.float32)[:M * D].reshape(B, Tp, D).astype(np.float64),
         "a": VS.frag_to_rows(h16("a"), M, D).astype(np.float64), "xh": VS.frag_to_rows(h16("xh"), M, D).astype(np.float64),
         "sx": sx.astype(np.float64), "sq": sq.astype(np.float64), "h": VS.frag_to_rows(h16("h"), M, mlp).astype(np.float64),
         "q": VS.qk_to_rows(h16("q"), B, heads, Tp).astype(np.float64), "k": VS.qk_to_rows(h16("k"), B, heads, Tp).astype(np.float64),
         "vt": VS.vt_to_rows(h16("vt"), B, heads, Tp).astype(np.float64)}
    return out.cpu().numpy().astype(np.float64), r, P


def _stage(stage, case, dev, ref, bound, sel=None):
    """worst |dev - ref| / bound over the selected elements: printed, then asserted <= 1"""
    assert np.isfinite(dev).all(), (stage, case)
    ratio = np.abs(dev - ref) / np.maximum(bound, 1e-300)
    if sel is not None:
        ratio = ratio[sel]
    worst = float(ratio.max())
    print(f"STAGE {stage:12s} {case:60s} err/bound={worst:.3f}")
    assert worst <= 1.0, (stage, case, worst)
    return worst


def _with_ls(w, ls1, ls2):
    w = dict(w)
    w["blocks.0.ls1.gamma"] = np.where(ls1, w["blocks.0.ls1.gamma"], 0).astype(np.float32)
    w["blocks.0.ls2.gamma"] = np.where(ls2, w["blocks.0.ls2.gamma"], 0).astype(np.float32)
    return w


def _check_padding_and_stats(case, r, P, B):
    T, Tp, D = P["T"], P["Tp"], P["D"]
    x = r["x"]
    assert (x[:, T:] == 0).all() and (r["xh"].reshape(B, Tp, D)[:, T:] == 0).all(), "padded token rows are not exactly zero"
    (sx, sq), (bx, bq), xh, bh = VS.stats_stage(x.reshape(-1, D))
    _stage("xh", case, r["xh"], xh, bh)
    _stage("stats.sum", case, r["sx"], sx, bx + 1e-300)
    _stage("stats.sumsq", case, r["sq"], sq, bq + 1e-300)


def _check_qkv_attention(case, r, P, B, fused, two=None):
    """fused: `two` is the two-kernel run of the same forward (its q, k, V^T are what vit_qkv_attention_kernel keeps in the compute unit)"""
    T, Tp, D, heads = P["T"], P["Tp"], P["D"], P["heads"]
    blk = P["blocks"][0]
    if fused:
        assert {"q", "k", "vt"} <= r["unwritten"], "vit_fused_qkv: q / k / V^T were written -- the two kernels ran"
        assert np.array_equal(two["xh"], r["xh"]) and np.array_equal(two["sx"], r["sx"]) and np.array_equal(two["sq"], r["sq"])
        out, ob = VS.attention_stage(two["q"], two["k"], two["vt"], T)
        _stage("att(fused)", case, r["a"].reshape(B, Tp, D), out, ob)
        # include/vfmreg.h states "the same bits as the two kernels": a wrong mask, scale or rounding point in the fused kernel alone is
        # then seen whatever its size (the two-kernel run itself is held to the stage bounds by the tests of that path)
        assert np.array_equal(two["a"], r["a"]), (case, float(np.abs(two["a"] - r["a"]).max()))
        return
    assert not ({"q", "k", "vt"} & r["unwritten"]), "q / k / V^T were not written"
    y, yb = VS.qkv_stage(r["xh"], r["sx"], r["sq"], blk["qkv"])
    yq, yk, yv = VS.split_qkv(y, B, Tp, heads)
    bq, bk, bv = VS.split_qkv(yb, B, Tp, heads)
    _stage("qkv.q", case, r["q"], yq, bq)
    _stage("qkv.k", case, r["k"], yk, bk)
    _stage("qkv.vt", case, r["vt"], yv, bv)   # (padded key rows: b' alone -- r = 1e3, S = 0)
    out, ob = VS.attention_stage(r["q"], r["k"], r["vt"], T)
    _stage("attention", case, r["a"].reshape(B, Tp, D), out, ob)


def _two_kernels(kv):
    return {k: v for k, v in kv.items() if k not in ("vit_fused_qkv", "vit_fused_mlp")}


def _check_block(case, w, imgs, patch_h=16, qkv_fused=False, mlp_fused=False, **kv):
    """forwards A, B, C of one depth-1 model under one kernel policy: every stage of the block and the final LayerNorms"""
    B = imgs.shape[0]
    if qkv_fused:
        kv["vit_fused_qkv"] = 1
    if mlp_fused:
        kv["vit_fused_mlp"] = 1
    outA, rA, P = _forward(_with_ls(w, False, False), imgs, patch_h, **kv)
    T, Tp, D = P["T"], P["Tp"], P["D"]
    blk = P["blocks"][0]
    real = np.arange(Tp) < T
    assert np.array_equal(rA["x"][:, 0], np.broadcast_to(P["cls_pos"][0], (B, D))), "row 0 is not cls + pos[0]"
    _check_padding_and_stats(case + " A", rA, P, B)
    two = _forward(_with_ls(w, False, False), imgs, patch_h, **_two_kernels(kv))[1] if qkv_fused else None
    _check_qkv_attention(case, rA, P, B, qkv_fused, two)
    if mlp_fused:
        assert "h" in rA["unwritten"], "vit_fused_mlp: h was written -- the two kernels ran"
    else:
        h, hb = VS.fc1_stage(rA["xh"], rA["sx"], rA["sq"], blk["fc1"])
        _stage("fc1+gelu", case, rA["h"], h, hb)
    z, zb = VS.final_stage(rA["x"], P)
    _stage("final", case, outA.reshape(z.shape), z, zb)
    x0 = rA["x"].reshape(-1, D)
    # B: proj + LayerScale + residual from the device's own attention output
    outB, rB, PB = _forward(_with_ls(w, True, False), imgs, patch_h, **kv)
    assert np.array_equal(rB["a"], rA["a"])   # (the same stream in front of the block: the kernels are deterministic)
    xr, xb = VS.resid_stage(rB["a"], x0, PB["blocks"][0]["proj"])
    _stage("proj", case, rB["x"], xr.reshape(B, Tp, D), xb.reshape(B, Tp, D), sel=(slice(None), real))
    _check_padding_and_stats(case + " B", rB, P, B)
    # C: fc2 + LayerScale + residual from the device's own hidden activations (or, fused, through fc1 from xh and stats)
    outC, rC, PC = _forward(_with_ls(w, False, True), imgs, patch_h, **kv)
    fc2 = PC["blocks"][0]["fc2"]
    if mlp_fused:   # the hidden activations of the two-kernel run of the same forward, themselves held to the fc1 bound
        assert "h" in rC["unwritten"]
        two = _forward(_with_ls(w, False, True), imgs, patch_h, **{**kv, "vit_fused_mlp": -1})[1]
        h, hb = VS.fc1_stage(rA["xh"], rA["sx"], rA["sq"], blk["fc1"])
        _stage("fc1+gelu", case + " (two-kernel run)", two["h"], h, hb)
        xr, xb = VS.resid_stage(two["h"], x0, fc2)
        _stage("fc2(fused)", case, rC["x"], xr.reshape(B, Tp, D), xb.reshape(B, Tp, D), sel=(slice(None), real))
        # fc2 sums 1536 terms: its worst-case bound would admit a slightly wrong GELU inside vit_mlp_kernel alone; the header states the same
        # bits as the two kernels, whose h and x are held to the fc1 and fc2 bounds here
        _stage("fc2", case + " (two-kernel run)", two["x"], xr.reshape(B, Tp, D), xb.reshape(B, Tp, D), sel=(slice(None), real))
        assert np.array_equal(two["x"], rC["x"]), (case, float(np.abs(two["x"] - rC["x"]).max()))
    else:
        xr, xb = VS.resid_stage(rC["h"], x0, fc2)
        _stage("fc2", case, rC["x"], xr.reshape(B, Tp, D), xb.reshape(B, Tp, D), sel=(slice(None), real))
    _check_padding_and_stats(case + " C", rC, P, B)
    z, zb = VS.final_stage(rC["x"], P)
    _stage("final", case + " C", outC.reshape(z.shape), z, zb)


@pytest.mark.parametrize("xcd", (1, 0))
@pytest.mark.parametrize("gemm", list(GEMM))
def test_block_stages_under_every_gemm_kernel(gemm, xcd):
    """every stage of a block through the direct, LDS-tiled (128 x 128 and 128 x 384), token-stationary (one / two channel tiles per wave)
    GEMM kernels, with and without the XCD mapping; 5 images x 288 padded tokens: the last group of four token tiles is partial"""
    imgs = smooth_images(np.random.default_rng(5), 5, 224, 14 * 17)
    _check_block(f"gemm={gemm} xcd={xcd}", _weights("plain"), imgs, vit_xcd=xcd, **GEMM[gemm])


@pytest.mark.parametrize("kind", ("offset4", "offset100", "outliers", "lowvar"))
def test_statistics_and_their_consumers_on_hard_rows(kind):
    imgs = smooth_images(np.random.default_rng(6), 2, 224, 14 * 9)
    _check_block(f"rows={kind}", _weights(kind), imgs)
    _check_block(f"rows={kind} fused", _weights(kind), imgs, qkv_fused=True, mlp_fused=True)


@pytest.mark.parametrize("att", list(ATT))
@pytest.mark.parametrize("kind", ("uniform", "peaked", "underflow"))
def test_attention_on_scores_that_speak(kind, att):
    _tile_case(att, 16, 11, 3, kinds=(kind,))   # 177 tokens: 15 padded keys


@pytest.mark.parametrize("mlp_fused", (False, True))
@pytest.mark.parametrize("qkv_fused", (False, True))
def test_block_stages_under_the_fused_kernels(qkv_fused, mlp_fused):
    imgs = smooth_images(np.random.default_rng(8), 3, 300, 400)   # a down-sampling resize in front
    for xcd in (1, 0):
        _check_block(f"fused_qkv={int(qkv_fused)} fused_mlp={int(mlp_fused)} xcd={xcd}", _weights("plain", seed=4), imgs,
                     qkv_fused=qkv_fused, mlp_fused=mlp_fused, vit_xcd=xcd)


# ------------------------------------------------------------------------------------------------------------ every token-tile count
def _tile_case(att, patch_h, pw, B, kinds=("plain", "uniform")):
    """'plain' and 'uniform' (every score equal, the padded rows of V^T unlike the real ones: tests/test_vit_stages.py, center_v, where the
    CPU test shows one unmasked key at > 100x the bound on these inputs); the per-tile kernel with and without the XCD mapping"""
    for kind in kinds:
        w, imgs = stage_case(kind, patch_h, pw, B)
        w = _with_ls(w, False, False)
        for xcd in ((1, 0) if att == "per-tile" else (1,)):
            _, r, P = _forward(w, imgs, patch_h, vit_xcd=xcd, **ATT[att])
            fused = att == "fused" and P["Tp"] // 32 <= 12   # (above: the fall-back to the two kernels, q, k, V^T written and checked)
            two = _forward(w, imgs, patch_h, vit_xcd=xcd)[1] if fused else None
            _check_qkv_attention(f"att={att} xcd={xcd} T={P['T']} tiles={P['Tp'] // 32} B={B} {kind}", r, P, B, fused, two)


@pytest.mark.parametrize("tiles", range(1, 17))
@pytest.mark.parametrize("att", ("per-tile", "lds"))
def test_attention_at_every_tile_count(att, tiles):
    """16 patch rows x pw columns, pw = 1 .. 31: Tp / 32 = 1 .. 16, every NKT of vit_attention_kernel / vit_attention_lds_kernel (query
    groups of 1, 2, 3 and 4 tiles), B = 1 and 3"""
    for pw in (2 * tiles - 2, 2 * tiles - 1):
        if pw >= 1:
            for B in (1, 3):
                _tile_case(att, 16, pw, B)


@pytest.mark.parametrize("tiles", range(1, 17))
def test_fused_qkv_attention_at_every_tile_count(tiles):
    """vit_qkv_attention_kernel at NKT = 1 .. 12; at 13 .. 16 tiles vit_fused_qkv = 1 must still be right, through the two kernels"""
    for pw in (2 * tiles - 2, 2 * tiles - 1):
        if pw >= 1:
            for B in (1, 3):
                _tile_case("fused", 16, pw, B)


@pytest.mark.parametrize("att", list(ATT))
@pytest.mark.parametrize("T,patch_h,pw", ((64, 3, 21), (33, 2, 16), (512, 7, 73)))
def test_attention_at_token_counts_through_patch_h(T, patch_h, pw, att):
    """T = 64: no padded key at all; T = 33: one real key in the last tile, 31 padded; T = 512: the largest the ABI admits"""
    assert patch_h * pw + 1 == T
    _tile_case(att, patch_h, pw, 2)


def test_513_tokens_are_refused():
    from vfmreg import vit as V
    w = _weights("plain")
    model = V.ViTS14(w, 224, 448, device="cuda")   # 16 x 32 patches + cls
    assert model.patch_w == 32
    out = torch.zeros((1, 16, 32, 384), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        model.forward(torch.zeros((1, 224, 448, 3), dtype=torch.uint8, device="cuda"), out=out)
    torch.cuda.synchronize()
    assert not out.any()   # refused, not run


# ------------------------------------------------------------------------------------------------------------ preprocess, patch embedding
def _probe_weights():
    """one-hot patch embedding, dim 640 (all 588 k in one forward), bias 0, cls + pos 0, LayerScale 0: x[m][n] IS the fp16 pixel k(n)"""
    from vfmreg import vit as V
    w = V.random_weights(seed=1, dim=640, depth=1, mlp=128)
    W = np.zeros((640, 588), np.float32)
    W[np.arange(640), np.arange(640) % 588] = 1.0
    w["patch_embed.proj.weight"] = W.reshape(640, 3, 14, 14)
    for k in ("patch_embed.proj.bias", "cls_token", "pos_embed", "blocks.0.ls1.gamma", "blocks.0.ls2.gamma"):
        w[k] = np.zeros_like(w[k])
    return w


def _device_pixels(imgs, patch_h, patch_kernel):
    _, r, P = _forward(_probe_weights(), imgs, patch_h, vit_preprocess_patch=patch_kernel)
    x = r["x"]
    assert (x[:, 0] == 0).all() and (x[:, P["T"]:] == 0).all()
    pix = x[:, 1:P["T"], :588]
    assert np.array_equal(pix, VS.f16(pix)) and np.array_equal(x[:, 1:P["T"], 588:], pix[..., :52])
    return pix, P


def _images(kind, B, H, W):
    if kind == "zeros":
        return np.zeros((B, H, W, 3), np.uint8)
    if kind == "full":
        return np.full((B, H, W, 3), 255, np.uint8)
    if kind == "checker":
        return checkerboard(B, H, W)
    return np.random.default_rng(H * W).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("patch_kernel", (1, 0))
@pytest.mark.parametrize("H,W", ((1200, 1600), (700, 820), (224, 14 * 9), (100, 37), (16, 2), (150, 211)))
def test_preprocessing_pixel_by_pixel(H, W, patch_kernel):
    """down-sampling, identity, up-sampling (sy < 0 clamped, x0 = W - 1), W = 2, W odd; noise, pure 0, pure 255 and a checkerboard"""
    for kind in ("noise", "zeros", "full", "checker"):
        imgs = _images(kind, 2, H, W)
        pix, P = _device_pixels(imgs, 16, patch_kernel)
        ref, bound = VS.preprocess_stage(imgs, 16, P["pw"])
        _stage("preprocess", f"{H}x{W} {kind} patch_kernel={patch_kernel}", pix, ref, bound)


@pytest.mark.parametrize("gemm", ("direct", "lds"))
def test_patch_embedding_from_the_device_pixels(gemm):
    w = _weights("plain", seed=9)
    for (H, W) in ((700, 820), (100, 37)):
        imgs = _images("noise", 3, H, W)
        pix, _ = _device_pixels(imgs, 16, 1)
        _, r, P = _forward(_with_ls(w, False, False), imgs, **GEMM[gemm])
        x, xb = VS.patch_embed_stage(pix, P, 3)
        T = P["T"]
        assert np.array_equal(r["x"][:, 0], np.broadcast_to(P["cls_pos"][0], (3, 384)))   # cls + pos[0] reaches row 0 only, as loaded
        assert (r["x"][:, T:] == 0).all() and (r["xh"].reshape(3, -1, 384)[:, T:] == 0).all()
        _stage("patch-embed", f"{H}x{W} gemm={gemm}", r["x"][:, 1:T], x[:, 1:T], xb[:, 1:T])


# ------------------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_where_the_output_depends_on_attention():
    """LayerScale 1, proj of norm O(1), two blocks: tolerance = 4 x the gap between the fp16 model accumulated in fp32 and in fp64 (both on
    the CPU, tests/test_vit_stages.py asserts that the softmax-scale and unmasked-key faults are outside it for these inputs)"""
    from tests import test_vit_stages as TS
    from vfmreg import vit as V
    w, imgs = TS.e2e_case()
    f64, gap = TS.e2e_gap(w, imgs)
    for name, kv in (("two kernels", {}), ("fused", dict(vit_fused_qkv=1, vit_fused_mlp=1))):
        model = V.ViTS14(w, imgs.shape[1], imgs.shape[2], device="cuda", patch_h=TS.E2E_CASE["patch_h"])
        from vfmreg import _lib
        with _lib.using(_config(**kv)):
            out = model.forward(torch.from_numpy(imgs).cuda()).cpu().numpy()
        err = float(np.abs(out - f64).max())
        print(f"STAGE end-to-end   {name:60s} err={err:.3g} gap={gap:.3g} err/(4 gap)={err / (TS.E2E_K * gap):.3f}")
        assert err <= TS.E2E_K * gap, (name, err, gap)

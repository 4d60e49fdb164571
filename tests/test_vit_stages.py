"""tests/vit_stages.py on the CPU: the fp64 stage chain is anchored to oracle.vit_reference, the layout helpers invert the kernels' layouts,
and every planted fault leaves its stage's derived bound while the correct stage, evaluated in fp32, stays inside (no GPU involved)."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import vit_stages as VS  # noqa: E402


def smooth_images(rng, B, H, W):
    low = rng.uniform(0, 255, (B, H // 40 + 2, W // 40 + 2, 3)).astype(np.float32)
    up = torch.nn.functional.interpolate(torch.from_numpy(low).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)
    up = up + 12.0 * torch.randn(up.shape, generator=torch.Generator().manual_seed(1))
    return up.clamp(0, 255).permute(0, 2, 3, 1).to(torch.uint8).contiguous().numpy()


def checkerboard(B, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    img = (((yy + xx) & 1) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(img[None, :, :, None], (B, H, W, 3)))


def attention_sensitive_weights(seed=31, dim=384, depth=2, mlp=1536):
    """LayerScale 1 and a proj of norm O(1): the output depends on what attention computes; a V bias of 3, which the padded key rows
    of V^T carry alone: a key that escapes the mask is seen."""
    from vfmreg import vit as V
    w = V.random_weights(seed=seed, dim=dim, depth=depth, mlp=mlp)
    for l in range(depth):
        w[f"blocks.{l}.ls1.gamma"][:] = 1.0
        w[f"blocks.{l}.ls2.gamma"][:] = 1.0
        w[f"blocks.{l}.attn.qkv.bias"][2 * dim:] += 3.0
    return w


def stage_weights(kind, seed=3):
    """depth-1 ViT-S weights whose stages speak (the GPU stage tests and the sensitivity test below use the same): 'plain'; 'offset4' /
    'offset100': rows with a common offset of 4x / 100x their spread (the cancellation of sum x^2 - (sum x)^2 / D); 'outliers': six channels
    at 50-200x; 'lowvar': rows of variance ~1e-4 (the LayerNorm eps matters); 'uniform': q = 0, every score equal, on the 'outliers' rows
    (see center_v); 'peaked' / 'underflow': scores x4 / x12."""
    from vfmreg import vit as V
    if kind in ("outliers", "uniform"):
        w, _ = V.dinov2_like_weights(seed=seed, dim=384, depth=1, mlp=1536, layerscale_range=(0.5, 1.0))
    else:
        w = V.random_weights(seed=seed, dim=384, depth=1, mlp=1536)
    w["blocks.0.ls1.gamma"][:] = np.random.default_rng(seed).uniform(0.5, 1.0, 384)
    w["blocks.0.ls2.gamma"][:] = np.random.default_rng(seed + 1).uniform(0.5, 1.0, 384)
    if kind in ("offset4", "offset100"):
        off = 4.0 if kind == "offset4" else 100.0   # the stream's spread is ~1 (patch embedding + bias + position embedding)
        w["patch_embed.proj.bias"] += off
        w["cls_token"] += off
    elif kind == "lowvar":
        for k in ("patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "pos_embed"):
            w[k] = (w[k] * 0.01).astype(np.float32)
    elif kind == "uniform":
        w["blocks.0.attn.qkv.weight"][:384] = 0
        w["blocks.0.attn.qkv.bias"][:384] = 0
    elif kind in ("peaked", "underflow"):
        w["blocks.0.attn.qkv.weight"][:768] *= 4.0 if kind == "peaked" else 12.0
    return w


def center_v(w, imgs, patch_h):
    """The V bias that makes the REAL rows of V mean-free for these images.  A padded key row of V^T is b' = b + W beta alone (its xh and
    statistics are zero); a real row is W (n gamma) + b' with n the normalised token.  No bias can be planted in the padded rows only, but
    with mean_real(W n gamma) + b' = 0 the padded rows are what the real ones are NOT: -mean(W n gamma).  On rows dominated by a few
    outlier channels n is nearly the same vector for every token, so the real rows are small and the padded rows are not: a key that escapes
    the mask moves the output by |b'| / (T + 1) while the bound follows the small real values."""
    B, H, W, _ = imgs.shape
    pw = int((14 * patch_h) / H * W / 14)
    P = VS.pack(w, patch_h, pw)
    pix, _ = VS.preprocess_stage(imgs, patch_h, pw)
    x, _ = VS.patch_embed_stage(VS.f16(pix), P, B)
    x = x[:, :P["T"]].reshape(-1, P["D"])
    n = (x - x.mean(-1, keepdims=True)) / np.sqrt(x.var(-1, keepdims=True) + 1e-6)
    g = lambda k: np.asarray(w[k], dtype=np.float64)   # noqa: E731
    Wv = g("blocks.0.attn.qkv.weight")[768:]
    proj = (n * g("blocks.0.norm1.weight")) @ Wv.T
    w = dict(w)
    b = g("blocks.0.attn.qkv.bias").copy()
    b[768:] = -proj.mean(0) - Wv @ g("blocks.0.norm1.bias")
    w["blocks.0.attn.qkv.bias"] = b.astype(np.float32)
    return w


def stage_case(kind, patch_h, pw, B, seed=3):
    """(weights, images) of one attention case of the GPU stage tests: no resize (H = 14 patch_h, W = 14 pw)"""
    imgs = smooth_images(np.random.default_rng(pw), B, 14 * patch_h, 14 * pw)
    w = stage_weights(kind, seed)
    return (center_v(w, imgs, patch_h) if kind == "uniform" else w), imgs


E2E_CASE = dict(B=1, H=150, W=200, patch_h=16)   # 16 x 21 patches: 337 tokens, 15 padded keys
E2E_K = 4                                         # tolerance = 4 x the CPU-measured fp32-vs-fp64 gap of the fp16 model (MFMA order, hardware functions)


def e2e_case():
    w = attention_sensitive_weights()
    imgs = smooth_images(np.random.default_rng(12), E2E_CASE["B"], E2E_CASE["H"], E2E_CASE["W"])
    return w, imgs


def e2e_gap(w, imgs):
    f64 = VS.forward_chain(w, imgs, E2E_CASE["patch_h"], rounding=True, acc=np.float64)
    f32 = VS.forward_chain(w, imgs, E2E_CASE["patch_h"], rounding=True, acc=np.float32)
    return f64, float(np.abs(f64 - f32).max())


def test_chain_without_rounding_reproduces_the_oracle():
    """every rounding point off: the stage chain IS oracle.vit_reference up to the oracle's own fp32 arithmetic (2.3e-5 on the 12-block
    ViT-S below; asserted <= 5e-5)"""
    from oracle import oracle as orc
    from vfmreg import vit as V
    for (seed, dim, depth, mlp, B, H, W, ph) in ((0, 384, 12, 1536, 2, 300, 400, 16), (5, 128, 2, 256, 1, 150, 130, 16), (6, 128, 1, 256, 2, 90, 333, 3)):
        w = V.random_weights(seed=seed, dim=dim, depth=depth, mlp=mlp)
        imgs = smooth_images(np.random.default_rng(seed), B, H, W)
        ref = orc.vit_reference(w, imgs, patch_h=ph)
        got = VS.forward_chain(w, imgs, ph, rounding=False)
        assert got.shape == ref.shape
        err = np.abs(got - ref).max()
        print("chain vs oracle", (dim, depth, B, H, W, ph), "max abs", err)
        assert err <= 5e-5, err


def test_layout_helpers_round_trip():
    from vfmreg import vit as V
    rng = np.random.default_rng(0)
    for (M, K) in ((32, 16), (96, 64), (64, 608), (352, 384)):
        A = rng.standard_normal((M, K)).astype(np.float16)
        fr = VS.rows_to_frag(A)
        assert np.array_equal(VS.frag_to_rows(fr, M, K), A)
        for (r, k) in ((0, 0), (M - 1, K - 1), (33 % M, 9), (M // 2, K // 2 + 3)):
            assert fr[VS.frag_index(r, k, K // 16)] == A[r, k]
    for (N, K, km) in ((384, 588, 32), (100, 50, 16), (33, 17, 16), (1152, 384, 16)):   # to_frag_f16 pads ragged sizes with zeros
        Wt = rng.standard_normal((N, K)).astype(np.float32)
        fr = V.to_frag_f16(Wt, km)
        Np_, Kp = -(-N // 32) * 32, -(-K // km) * km
        back = VS.frag_to_rows(fr, Np_, Kp)
        assert np.array_equal(back[:N, :K], Wt.astype(np.float16)) and not back[N:].any() and not back[:, K:].any()
    q = rng.standard_normal((2, 3, 64, 64)).astype(np.float16)
    assert np.array_equal(VS.qk_to_rows(VS.rows_to_qk(q), 2, 3, 64), q)
    vt = rng.standard_normal((2, 3, 64, 96)).astype(np.float16)
    assert np.array_equal(VS.vt_to_rows(VS.rows_to_vt(vt), 2, 3, 96), vt)
    st = rng.standard_normal((64, 12, 2)).astype(np.float32)
    sx, sq = VS.stats_to_rows(st, 64, 384)
    assert np.array_equal(sx, st[..., 0]) and np.array_equal(sq, st[..., 1])


def _block_inputs(seed=3, B=2, patch_h=16, pw=5):
    """a depth-1 model's operands and a patch-embedded stream to feed the stages with"""
    from vfmreg import vit as V
    w = V.random_weights(seed=seed, dim=384, depth=1, mlp=1536)
    P = VS.pack(w, patch_h, pw)
    imgs = smooth_images(np.random.default_rng(seed), B, 14 * patch_h, 14 * pw)
    pix, _ = VS.preprocess_stage(imgs, patch_h, pw)
    x, _ = VS.patch_embed_stage(VS.f16(pix), P, B)
    x = VS.f32(x)
    (sx, sq), _, xh, _ = VS.stats_stage(x.reshape(-1, 384))
    return w, P, x, VS.f16(xh), VS.f32(sx), VS.f32(sq)


def _outside(fault, ref, bound):
    return float((np.abs(fault - ref) / bound).max())


def test_correct_stages_in_fp32_stay_inside_their_bounds():
    """the stage arithmetic in fp32 (numpy / BLAS; libm in place of the hardware functions) must satisfy the bounds derived for fp32"""
    w, P, x, xh, sx, sq = _block_inputs()
    B, Tp, heads, T = x.shape[0], P["Tp"], P["heads"], P["T"]
    blk = P["blocks"][0]
    f = np.float32
    # QKV in fp32
    y, bound = VS.qkv_stage(xh, sx, sq, blk["qkv"])
    mean = (sx.astype(f).sum(-1) * f(1 / 384))[:, None]
    var = np.maximum(sq.astype(f).sum(-1)[:, None] * f(1 / 384) - mean * mean, f(0))
    a = (f(1) / np.sqrt(var + f(1e-6))).astype(f)
    Wh, b, c = blk["qkv"]
    y32 = (xh.astype(f) @ Wh.astype(f).T) * a + ((-(a * mean)) * c.astype(f)[None, :] + b.astype(f)[None, :])
    r = _outside(VS.f16(y32), y, bound)
    print("fp32 qkv err / bound", r)
    assert r <= 1.0
    # attention in fp32
    q, k, vt = VS.split_qkv(VS.f16(y), B, Tp, heads)
    out, bound = VS.attention_stage(q, k, vt, T)
    s = np.einsum("bhqd,bhkd->bhqk", q.astype(f), k.astype(f))[..., :T]
    sc = f(0.125 * 1.44269504088896340736)
    p = np.exp2(s * sc - s.max(-1, keepdims=True) * sc).astype(f)
    o = np.einsum("bhqk,bhdk->bhqd", p.astype(np.float16).astype(f), vt[..., :T].astype(f)) * (f(1) / p.sum(-1, dtype=f))[..., None]
    r = _outside(VS.f16(o.transpose(0, 2, 1, 3).reshape(B, Tp, -1)), out, bound)
    print("fp32 attention err / bound", r)
    assert r <= 1.0
    # fc1 + GELU in fp32
    h, bound = VS.fc1_stage(xh, sx, sq, blk["fc1"])
    Wh, b, c = blk["fc1"]
    y32 = (xh.astype(f) @ Wh.astype(f).T) * a + ((-(a * mean)) * c.astype(f)[None, :] + b.astype(f)[None, :])
    h32 = (f(0.5) * y32 * (f(1) + torch.erf(torch.from_numpy(y32 * f(math.sqrt(0.5)))).numpy())).astype(f)
    r = _outside(VS.f16(h32), h, bound)
    print("fp32 fc1 + gelu err / bound", r)
    assert r <= 1.0
    # proj in fp32
    a16 = VS.f16(out).reshape(-1, 384)
    xo, bound = VS.resid_stage(a16, x.reshape(-1, 384), blk["proj"])
    Wp, bp, g1 = blk["proj"]
    x32 = x.reshape(-1, 384).astype(f) + g1.astype(f)[None, :] * (a16.astype(f) @ Wp.astype(f).T + bp.astype(f)[None, :])
    r = _outside(x32, xo, bound)
    print("fp32 proj err / bound", r)
    assert r <= 1.0
    # final in fp32
    z, bound = VS.final_stage(x, P)
    t = torch.from_numpy(x[:, 1:T].astype(f))
    nw, nb, cw, cb = (torch.from_numpy(v.astype(f)) for v in P["final"])
    z32 = torch.nn.functional.layer_norm(torch.nn.functional.layer_norm(t, (384,), nw, nb, 1e-6), (384,), cw, cb, 1e-5).numpy()
    r = _outside(z32, z, bound)
    print("fp32 final err / bound", r)
    assert r <= 1.0


def _lattice(v, frac=0.45):
    """fp32 values that all sit `frac` of an fp16 spacing above an fp16 number: their fp16 roundings err in ONE direction"""
    g = np.asarray(v, dtype=np.float64).astype(np.float16)
    return VS.f32(g.astype(np.float64) + frac * np.spacing(np.abs(g)).astype(np.float64))


def _offset_rows(offset, sigma, M=64, D=384, seed=7):
    """rows with a common offset and a spread, on the lattice above (the statistic faults are errors of mu c: visible when the roundings of
    the fp16 copy do not average out), their fp16 copy and their fp32 slice sums"""
    rng = np.random.default_rng(seed)
    x = _lattice(offset + sigma * rng.standard_normal((M, D)))
    (sx, sq), _, _, _ = VS.stats_stage(x)
    return x, VS.f16(x), VS.f32(sx), VS.f32(sq)


def _positive_folded(c_from_rounded=True, N=128, D=384, seed=8):
    """a folded weight with rows of one sign (c = sum |W'|: as large as the weight allows) on the lattice, gamma = 1, beta = 0"""
    rng = np.random.default_rng(seed)
    Wf = _lattice(0.01 + 0.05 * np.abs(rng.standard_normal((N, D))))
    return VS.folded(Wf, 0.05 * rng.standard_normal(N), np.ones(D), np.zeros(D), c_from_rounded=c_from_rounded)


def test_every_planted_fault_leaves_its_stage_bound():
    """Each fault against the correct stage, on the CPU.  The inputs are those that make the fault speak: an up-sampled checkerboard,
    rows of small variance for the LayerNorm eps, and -- constructed, not what a forward produces -- rows with a common offset of 4x their
    spread whose fp16 roundings do not average out, against a folded weight of one sign, for mu and c (on a forward's own rows these two
    faults are errors of a few fp32 units: test_gpu_inputs_see_the_faults says what the GPU tests' inputs see)."""
    w, P, x, xh, sx, sq = _block_inputs()
    B, Tp, heads, T = x.shape[0], P["Tp"], P["heads"], P["T"]
    blk = P["blocks"][0]
    y, yb = VS.qkv_stage(xh, sx, sq, blk["qkv"])
    q, k, vt = VS.split_qkv(VS.f16(y), B, Tp, heads)
    out, ob = VS.attention_stage(q, k, vt, T)
    ratios = {}
    assert T < Tp   # (padded rows of k, V^T carry b': not zero)
    ratios["unmasked key"] = _outside(VS.attention_stage(q, k, vt, T, n_keys=T + 1)[0], out, ob)
    ratios["softmax scale 1/8.1"] = _outside(VS.attention_stage(q, k, vt, T, scale=1 / 8.1)[0], out, ob)
    h, hb = VS.fc1_stage(xh, sx, sq, blk["fc1"])
    ratios["tanh GELU"] = _outside(VS.fc1_stage(xh, sx, sq, blk["fc1"], gelu=VS.gelu_tanh)[0], h, hb)
    # LayerNorm eps: rows whose variance (4e-4) is small enough for 1e-5 - 1e-6 to matter beside it
    xs, xsh, ssx, ssq = _offset_rows(0.0, 0.02)
    for name in ("qkv", "fc1"):
        stage = VS.qkv_stage if name == "qkv" else VS.fc1_stage
        good, gb = stage(xsh, ssx, ssq, blk[name])
        ratios[f"LN eps 1e-5 ({name})"] = _outside(stage(xsh, ssx, ssq, blk[name], eps=1e-5)[0], good, gb)
    # mu from the fp16 copy, c from the unrounded weight: offset 4x the spread
    xo, xoh, osx, osq = _offset_rows(1.5, 0.375)
    good, gb = VS.qkv_stage(xoh, osx, osq, _positive_folded())
    ratios["mu from xh"] = _outside(VS.qkv_stage(xoh, osx, osq, _positive_folded(), mu_override=xoh.mean(-1))[0], good, gb)
    ratios["c from the unrounded weight"] = _outside(VS.qkv_stage(xoh, osx, osq, _positive_folded(c_from_rounded=False))[0], good, gb)
    # the last bilinear tap not clamped: an up-sampling resize of a checkerboard
    img = checkerboard(1, 100, 37)
    pix, pb = VS.preprocess_stage(img, 16, 5)
    ratios["last tap not clamped"] = _outside(VS.preprocess_stage(img, 16, 5, clamp_last_tap=False)[0], pix, pb)
    for name, r in ratios.items():
        print(f"fault {name}: worst |fault - ref| / bound = {r:.3g}")
    for name, r in ratios.items():
        assert r > 1.0, (name, r)


def _stage_chain(w, imgs, patch_h):
    B, H, W, _ = imgs.shape
    pw = W // 14
    P = VS.pack(w, patch_h, pw)
    pix, _ = VS.preprocess_stage(imgs, patch_h, pw)
    x, _ = VS.patch_embed_stage(VS.f16(pix), P, B)
    x = VS.f32(x).reshape(-1, 384)
    (sx, sq), _, _, _ = VS.stats_stage(x)
    return P, VS.f16(x), VS.f32(sx), VS.f32(sq)


@pytest.mark.parametrize("pw", (1, 11, 23, 30, 31))
def test_gpu_inputs_see_the_faults(pw):
    """the inputs tests/test_gpu_vit_stages.py gives the device, through the same bounds, with the fault planted in the CPU stage: one
    unmasked padded key must leave the attention bound in the 'uniform' case at every token count up to the largest of the sweep
    (T = 497) and in the 'plain' case; the softmax scale and the tanh GELU in the 'plain' case"""
    res = {}
    for kind in ("uniform", "plain"):
        w, imgs = stage_case(kind, 16, pw, 1)
        P, xh, sx, sq = _stage_chain(w, imgs, 16)
        blk, T = P["blocks"][0], P["T"]
        y, _ = VS.qkv_stage(xh, sx, sq, blk["qkv"])
        q, k, vt = VS.split_qkv(VS.f16(y), 1, P["Tp"], P["heads"])
        out, ob = VS.attention_stage(q, k, vt, T)
        res[kind + " unmasked"] = _outside(VS.attention_stage(q, k, vt, T, n_keys=T + 1)[0], out, ob)
        if kind == "plain":
            res["plain scale"] = _outside(VS.attention_stage(q, k, vt, T, scale=1 / 8.1)[0], out, ob)
            h, hb = VS.fc1_stage(xh, sx, sq, blk["fc1"])
            res["plain tanh"] = _outside(VS.fc1_stage(xh, sx, sq, blk["fc1"], gelu=VS.gelu_tanh)[0], h, hb)
    print(f"GPU inputs, T = {16 * pw + 1}:", {k_: round(v, 2) for k_, v in res.items()})
    for name, r in res.items():
        assert r > 1.0, (pw, name, r)


def test_attention_sensitive_end_to_end_tolerance_excludes_the_attention_faults():
    """the end-to-end case of tests/test_gpu_vit_stages.py: its tolerance is 4 x the gap between the fp16 model accumulated in fp32 and in
    fp64 (both computed here, no kernel), and for these very inputs a wrong softmax scale and one unmasked key are outside it"""
    w, imgs = e2e_case()
    f64, gap = e2e_gap(w, imgs)
    tol = E2E_K * gap
    out = {}
    for fault in ("scale", "unmasked"):
        out[fault] = float(np.abs(VS.forward_chain(w, imgs, E2E_CASE["patch_h"], faults=(fault,)) - f64).max())
    print(f"attention-sensitive e2e: fp32-vs-fp64 gap {gap:.3g}, tolerance {tol:.3g}, faults {out}")
    assert gap > 0
    for fault, e in out.items():
        assert e > tol, (fault, e, tol)

"""The ViT forward of csrc/vit.hip restated stage by stage in fp64 (numpy), with the error bound of every stage.

Each ``*_stage`` function takes the arrays the kernel of that stage reads (already holding the kernel's operand values: fp16 operands as
fp64 numbers that ARE fp16 values, fp32 parameters as fp64 numbers that ARE fp32 values), and returns ``(ref, bound)``: the exact result of
the stage on those operands and the admissible |device - ref| per element.  Nothing is inherited from the stage before: the GPU tests feed
every stage with what the device itself left in the workspace.

Where the kernels round (csrc/vit.hip at this commit), and what the reference does there
  * preprocess (vit_preprocess_kernel / vit_preprocess_patch_kernel): fp32 throughout, ``sh = (float)H / (float)Hr``, source index
    ``sh (o + 0.5) - 0.5`` clamped below at 0, ``y0`` clamped at H - 1, ``y1 = y0 + (y0 < H - 1)``; ``(r - mean) / std`` stored as fp16
    (``v[e] = (_Float16)(...)`` / ``vals[c * 196 + tid] = (_Float16)(...)``).  Reference: exact, one fp16 store.
  * patch embedding (EPI_PATCH in epi_tile): fp16 x fp16 MFMA, fp32 accumulator, ``acc + bias`` then ``+ cls_pos[t]`` in fp32; row t = 0 is
    ``cls_pos[0]`` as loaded; rows t >= T are the zeros of epi_load.  Output x is fp32; ``xh = to_half4(o)`` is the fp16 copy of that very
    fp32 value; ``stats`` = (sum o, sum o^2) over 32 channels in fp32.
  * folded LN + QKV / fc1 (ln_stats_load, EPI_QKV / EPI_GELU): the twelve slice sums added in fp32, ``mean = sx * invD``,
    ``var = max(fma(sq, invD, -mean^2), 0)``, ``a = v_rsq_f32(var + 1e-6)``, ``nb = -(a mean)``; ``y = fma(acc, a, fma(nb, c, b'))`` in fp32,
    stored as fp16 by to_half4 (QKV) or after gelu2 (fc1).  mu comes from the fp32 stream's sums, never from xh; c is the row sum of the
    weight AS ROUNDED to fp16 (vfmreg/vit.py, folded).
  * attention (att_softmax and the three kernels that call it): scores in fp32 from fp16 q, k; keys >= T set to -3e38;
    ``p = v_exp_f32(fma(s, scale, -(max scale)))`` with scale = log2(e) / 8; the sum of the UNROUNDED p in fp32, ``inv = 1.0f / sum``;
    p rounded to fp16 by pack_f16x2 for the P.V MFMA; ``O * inv`` stored as fp16.
  * proj / fc2 (EPI_RESID): ``v = acc + bias``, ``o = fma(gamma, v, x)`` in fp32; x, xh, stats as for the patch embedding.
  * final (vit_final_kernel): fp32, two-pass LayerNorm (eps 1e-6), cls dropped, two-pass ChannelNorm (eps 1e-5), fp32 output.

The bound (every term derived, none tuned against a kernel's output), u = 2^-24 the fp32 unit roundoff, for an element stored as fp16:
    |out - ref| <= 2^-11 |ref|  (the store)  +  2^-10 |ref|  (one flipped rounding)  +  c_acc u sum_k |a_k| |b_k|  +  eps_fn
and without the two fp16 terms for fp32 outputs.  c_acc is the STANDARD worst-case bound of a length-K fp32 accumulation in any order,
K u (Higham, Accuracy and Stability, 3.1; gamma_K ~ K u), plus one u per fp32 operation of the epilogue; it is not sqrt(K)-scaled.
eps_fn: v_rcp_f32, v_rsq_f32, v_exp_f32 1 ulp (2^-23 relative) each; the A&S 7.1.26 erf 1.5e-7 absolute.  Where a stage divides by a
difference that cancels (the variance from sum x^2 - (sum x)^2 / D) the lost bits are carried through explicitly (``_ln_terms``).
fp16 subnormals: a store below 2^-14 has absolute error 2^-25, added where values can be that small.
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24          # fp32 unit roundoff
H_STORE = 2.0 ** -11    # fp16 store (round to nearest)
H_FLIP = 2.0 ** -10     # one flipped fp16 rounding: a full fp16 spacing
H_SUB = 2.0 ** -25      # half the smallest fp16 subnormal
ULP = 2.0 ** -23        # "1 ulp" of an fp32 hardware function, relative
ERF_ABS = 1.5e-7        # Abramowitz & Stegun 7.1.26
MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])


def f16(x):
    """round to fp16 (nearest even, subnormals kept), back in fp64"""
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def half_bound(ref):
    """the two fp16 terms of the bound"""
    return (H_STORE + H_FLIP) * np.abs(ref) + H_SUB


# --------------------------------------------------------------------------------------------------------------- layouts
def frag_index(row, k, ksteps):
    """csrc/vit.hip frag_index: half index of element (row, k) of a fragment-tiled matrix with `ksteps` k-steps of 16"""
    tile, p, s, h, e = row >> 5, row & 31, k >> 4, (k >> 3) & 1, k & 7
    return ((((tile * ksteps + s) * 2 + h) * 32 + p) * 8 + e)


def rows_to_frag(A):
    """[M][K] (M % 32 == 0, K % 16 == 0) -> flat fragment tiles [M/32][K/16][2][32][8]"""
    M, K = A.shape
    assert M % 32 == 0 and K % 16 == 0
    return np.ascontiguousarray(A.reshape(M // 32, 32, K // 16, 2, 8).transpose(0, 2, 3, 1, 4)).reshape(-1)


def frag_to_rows(buf, M, K):
    """inverse of rows_to_frag (and of vfmreg.vit.to_frag_f16 for its padded shape)"""
    assert M % 32 == 0 and K % 16 == 0
    t = np.asarray(buf).reshape(-1)[:M * K].reshape(M // 32, K // 16, 2, 32, 8)
    return np.ascontiguousarray(t.transpose(0, 3, 1, 2, 4)).reshape(M, K)


def qk_to_rows(buf, B, heads, Tp):
    """q or k: per (image, head) a fragment-tiled [Tp][64] -> [B][heads][Tp][64]"""
    t = np.asarray(buf).reshape(-1)[:B * heads * Tp * 64].reshape(B * heads, Tp * 64)
    return np.stack([frag_to_rows(r, Tp, 64) for r in t]).reshape(B, heads, Tp, 64)


def rows_to_qk(A):
    B, heads, Tp, _ = A.shape
    return np.concatenate([rows_to_frag(A[b, h]) for b in range(B) for h in range(heads)])


def vt_to_rows(buf, B, heads, Tp):
    """V^T: per (image, head) a fragment-tiled [64][Tp] -> [B][heads][64][Tp]"""
    t = np.asarray(buf).reshape(-1)[:B * heads * Tp * 64].reshape(B * heads, Tp * 64)
    return np.stack([frag_to_rows(r, 64, Tp) for r in t]).reshape(B, heads, 64, Tp)


def rows_to_vt(A):
    B, heads, _, Tp = A.shape
    return np.concatenate([rows_to_frag(A[b, h]) for b in range(B) for h in range(heads)])


def stats_to_rows(buf, M, D):
    """[M][D/32][2] -> (sum x [M][D/32], sum x^2 [M][D/32])"""
    t = np.asarray(buf).reshape(-1)[:M * (D // 32) * 2].reshape(M, D // 32, 2)
    return t[..., 0].copy(), t[..., 1].copy()


# --------------------------------------------------------------------------------------------------------------- parameters
def interpolate_pos_embed(pos_embed, h, w):
    from oracle import oracle as orc
    return np.asarray(orc.interpolate_pos_embed(pos_embed, h, w), dtype=np.float64).reshape(-1, np.asarray(pos_embed).shape[-1])


def folded(W, b, gamma, beta, c_from_rounded=True):
    """vfmreg/vit.py::folded: (W' as fp16 values, b' fp32, c fp32).  c_from_rounded=False plants the fault 'c summed from the unrounded weight'."""
    W, b, gamma, beta = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (W, b, gamma, beta))
    Wf = f32(W * gamma[None, :])
    Wh = f16(Wf)
    return Wh, f32(b + W @ beta), f32((Wh if c_from_rounded else Wf).sum(1))


def pack(w, patch_h, pw, rounding=True):
    """The operand values the kernels read.  rounding=False: the fp32 weights themselves, LayerNorm still folded (exact algebra)."""
    g = lambda k: np.asarray(w[k], dtype=np.float32).astype(np.float64)   # noqa: E731
    r16 = f16 if rounding else (lambda a: np.asarray(a, dtype=np.float64))
    D = g("patch_embed.proj.weight").shape[0]
    pos = interpolate_pos_embed(w["pos_embed"], patch_h, pw)
    cls_pos = pos.copy()
    cls_pos[0] += g("cls_token").reshape(-1)
    P = {"D": D, "heads": D // 64, "patch_h": patch_h, "pw": pw, "T": patch_h * pw + 1, "patch_w": r16(g("patch_embed.proj.weight").reshape(D, -1)),
         "patch_b": g("patch_embed.proj.bias"), "cls_pos": f32(cls_pos) if rounding else cls_pos, "blocks": []}
    P["Tp"] = -(-P["T"] // 32) * 32
    l = 0
    while f"blocks.{l}.norm1.weight" in w:
        p = f"blocks.{l}."
        blk = {}
        for name, lin, nrm in (("qkv", "attn.qkv", "norm1"), ("fc1", "mlp.fc1", "norm2")):
            if rounding:
                blk[name] = folded(g(p + lin + ".weight"), g(p + lin + ".bias"), g(p + nrm + ".weight"), g(p + nrm + ".bias"))
            else:
                Wf = g(p + lin + ".weight") * g(p + nrm + ".weight")[None, :]
                blk[name] = (Wf, g(p + lin + ".bias") + g(p + lin + ".weight") @ g(p + nrm + ".bias"), Wf.sum(1))
        blk["proj"] = (r16(g(p + "attn.proj.weight")), g(p + "attn.proj.bias"), g(p + "ls1.gamma"))
        blk["fc2"] = (r16(g(p + "mlp.fc2.weight")), g(p + "mlp.fc2.bias"), g(p + "ls2.gamma"))
        P["blocks"].append(blk)
        l += 1
    P["final"] = tuple(g(k) for k in ("norm.weight", "norm.bias", "channel_norm.weight", "channel_norm.bias"))
    return P


# --------------------------------------------------------------------------------------------------------------- 1. preprocess
def preprocess_stage(img, patch_h, pw, clamp_last_tap=True):
    """img uint8 [B][H][W][3] -> (pixels [B][Np][588] in im2col order k = c 196 + py 14 + px, unrounded; bound for the fp16 value the
    kernel stores).  clamp_last_tap=False plants the fault: the second tap is x0 + 1 / y0 + 1 whatever the border (reads past the row).

    The kernel's source coordinate is fp32: s = fl(fl(sh fl(o + 0.5)) - 0.5) with sh = fl(H / Hr), three roundings on a quantity <= s + 1,
    |ds| <= 3 u (s + 1).  Bilinear interpolation is continuous and piecewise linear in s with slope <= G = the largest difference of two
    neighbouring pixels (/ 255) of that image and channel, also across a cell border, so the coordinate costs <= ds G.  The interpolation
    itself is 12 fp32 roundings of quantities <= 1 (1 / 255, four products, two weights, five multiply-adds); (r - mean) / std adds
    u mean (the constant) / std and 2 u |ref|."""
    img = np.asarray(img)
    B, H, W, _ = img.shape
    Hr, Wr = 14 * patch_h, 14 * pw
    x = img.astype(np.float64) / 255.0

    def taps(n_out, n_in):
        s = np.maximum((n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5, 0.0)
        i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
        i1 = i0 + ((i0 < n_in - 1) if clamp_last_tap else 1)
        return s, i0, i1, s - i0
    sy, y0, y1, ly = taps(Hr, H)
    sx, x0, x1, lx = taps(Wr, W)
    flat = np.concatenate([x.reshape(B, H * W, 3), np.ones((B, W + 2, 3))], 1)   # an unclamped tap reads on in memory (here: ones)
    at = lambda yy, xx: flat[:, (yy[:, None] * W + xx[None, :]).reshape(-1)].reshape(B, Hr, Wr, 3)   # noqa: E731
    wy, wx = ly[None, :, None, None], lx[None, None, :, None]
    r = (1 - wy) * ((1 - wx) * at(y0, x0) + wx * at(y0, x1)) + wy * ((1 - wx) * at(y1, x0) + wx * at(y1, x1))
    ref = (r - MEAN) / STD
    Gy = np.abs(np.diff(x, axis=1)).max(axis=(1, 2)) if H > 1 else np.zeros((B, 3))
    Gx = np.abs(np.diff(x, axis=2)).max(axis=(1, 2)) if W > 1 else np.zeros((B, 3))
    e_r = 3 * U * (sy + 1)[None, :, None, None] * Gy[:, None, None, :] + 3 * U * (sx + 1)[None, None, :, None] * Gx[:, None, None, :] + 12 * U
    bound = half_bound(ref) + (e_r + U * MEAN) / STD + 2 * U * np.abs(ref)

    def im2col(a):   # [B][Hr][Wr][3] -> [B][Np][c 196 + py 14 + px]
        return a.reshape(B, patch_h, 14, pw, 14, 3).transpose(0, 1, 3, 5, 2, 4).reshape(B, patch_h * pw, 588)
    return im2col(ref), im2col(bound)


# --------------------------------------------------------------------------------------------------------------- GEMM pieces
def _gemm(A, W, dA=None):
    """A [M][K], W [N][K] -> (A W^T, sum_k |a||w| (+ what an uncertainty dA of A can move))"""
    S = A @ W.T
    mag = np.abs(A) @ np.abs(W).T
    extra = (dA @ np.abs(W).T) if dA is not None else 0.0
    return S, mag, extra


def patch_embed_stage(pix16, P, B):
    """pix16 [B][Np][588] fp16 values -> x [B][Tp][D] (fp32 output).  K = 588 products and sums in any order: (K + 2) u of the magnitudes
    (accumulation, + bias, + cls_pos)."""
    T, Tp, D = P["T"], P["Tp"], P["D"]
    S, mag, _ = _gemm(pix16.reshape(-1, 588), P["patch_w"])
    x = np.zeros((B, Tp, D))
    bd = np.zeros((B, Tp, D))
    x[:, 1:T] = S.reshape(B, T - 1, D) + P["patch_b"] + P["cls_pos"][None, 1:]
    bd[:, 1:T] = (588 + 2) * U * (mag.reshape(B, T - 1, D) + np.abs(P["patch_b"]) + np.abs(P["cls_pos"][None, 1:]))
    x[:, 0] = P["cls_pos"][0]
    return x, bd


def stats_stage(x):
    """x [M][D] (the device's fp32 stream) -> ((sum x, sum x^2) per 32-channel slice, their bounds, xh and its bound).  32 terms in any
    order: 32 u sum |x|; the squares carry one more rounding each: 33 u sum x^2.  xh is ONE rounding of the fp32 value: 2^-11 |x|, no flip."""
    M, D = x.shape
    xs = x.reshape(M, D // 32, 32)
    return (xs.sum(-1), (xs * xs).sum(-1)), (32 * U * np.abs(xs).sum(-1), 33 * U * (xs * xs).sum(-1)), x.copy(), H_STORE * np.abs(x) + H_SUB


def _ln_terms(sx, sq, D, eps, mu_override=None):
    """mean, r = rsqrt(var + eps) from the slice sums as ln_stats_load forms them, and the relative error of r / absolute error of mean.
    nsl slice sums added (nsl u each of sum |.|), mean = sx invD (invD rounded + the product: 2 u), mean^2 (2 x mean's + 1 u), the fma
    (1 u), var + eps (1 u), v_rsq_f32 (1 ulp).  d var / (var + eps) goes through r = (var + eps)^-1/2 exactly, not to first order."""
    nsl = sx.shape[-1]
    mean = sx.sum(-1) / D if mu_override is None else mu_override
    msq = sq.sum(-1) / D
    var = np.maximum(msq - mean * mean, 0.0)
    d_mean = (nsl + 2) * U * np.abs(sx).sum(-1) / D
    d_var = (nsl + 3) * U * msq + 2 * np.abs(mean) * d_mean + d_mean ** 2 + 2 * U * mean * mean + U * (var + eps)
    rel = d_var / (var + eps)
    assert (rel < 0.5).all(), "row statistics too ill-conditioned for a bound"
    d_r = (1.0 - rel) ** -0.5 - 1.0 + ULP
    return mean, 1.0 / np.sqrt(var + eps), d_mean, d_r


def folded_ln_gemm_stage(xh, sx, sq, Wh, b, c, eps=1e-6, mu_override=None):
    """y = r (xh W'^T - mu c) + b' in fp32 BEFORE its fp16 store -> (y, fp32 error of y).  K = D: K u on sum |xh| |W'|; then the epilogue:
    the error of r on both products, the error of mu on c, three roundings (nb, two fmas) on the three magnitudes."""
    M, D = xh.shape
    S, mag, _ = _gemm(xh, Wh)
    mean, r, d_mean, d_r = _ln_terms(sx, sq, D, eps, mu_override)
    mean, r, d_mean, d_r = (a[:, None] for a in (mean, r, d_mean, d_r))
    y = r * (S - mean * c[None, :]) + b[None, :]
    big = r * (np.abs(S) + np.abs(mean * c[None, :]))
    e = d_r * big + r * (D * U * mag + d_mean * np.abs(c)[None, :]) + 3 * U * (big + np.abs(b)[None, :])
    return y, e


def qkv_stage(xh, sx, sq, blk_qkv, eps=1e-6, mu_override=None):
    """-> (y [M][3D] unrounded, bound of the fp16 q | k | v the kernel stores)"""
    y, e = folded_ln_gemm_stage(xh, sx, sq, *blk_qkv, eps=eps, mu_override=mu_override)
    return y, half_bound(y) + e


def split_qkv(y, B, Tp, heads):
    """[B Tp][3D] -> q, k [B][heads][Tp][64], vt [B][heads][64][Tp]"""
    t = y.reshape(B, Tp, 3, heads, 64)
    return t[:, :, 0].transpose(0, 2, 1, 3), t[:, :, 1].transpose(0, 2, 1, 3), t[:, :, 2].transpose(0, 2, 3, 1)


def gelu_erf(y):
    return 0.5 * y * (1.0 + np.vectorize(math.erf)(y / math.sqrt(2.0)))


def gelu_tanh(y):
    return 0.5 * y * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (y + 0.044715 * y ** 3)))


def fc1_stage(xh, sx, sq, blk_fc1, eps=1e-6, gelu=gelu_erf):
    """-> (h [M][mlp] unrounded, bound of the stored fp16).  |gelu'| <= 1.13 carries y's fp32 error; erf: 1.5e-7 (A&S 7.1.26) + the
    hardware functions under it -- v_rcp_f32 through five Horner steps of a polynomial with p t <= 1 (6 ulp), v_exp_f32 and the two
    roundings of its argument, |arg| e^arg <= 0.37 (2 ulp), seven fma roundings on quantities <= 1.5 (11 u): 16 x 2^-24 --; 3 u on the result."""
    y, e = folded_ln_gemm_stage(xh, sx, sq, *blk_fc1, eps=eps)
    h = gelu(y)
    return h, half_bound(h) + 1.13 * e + 0.5 * np.abs(y) * (ERF_ABS + 16 * U) + 3 * U * np.abs(h)


# --------------------------------------------------------------------------------------------------------------- attention
def attention_stage(q, k, vt, T, scale=0.125, n_keys=None, round_p=False, dq=None, dk=None, dv=None):
    """q, k [B][heads][Tp][64], vt [B][heads][64][Tp] fp16 values -> (out [B][Tp][heads 64], bound of the stored fp16).
    Keys < T only (n_keys = T + 1 plants the unmasked padded key; scale = 1 / 8.1 the wrong scale).  round_p: p rounded to fp16 before
    P.V as the kernel does (the model chain); the bound is against the unrounded p and carries 2^-11 p for it.
    dq, dk, dv: element-wise uncertainty of the inputs (the fused kernel: the QKV stage bound).

    Per query: a_j = log2(e) scale (s_j - max) has error <= scale' (64 u sum |q||k| + ds_j) + 2 u |s_j| scale' + u |a_j| (what is common to
    all keys -- the rounded max, its product with the scale -- cancels in p / sum p); p_j then has relative error
    eps = 2^(max_j da_j) - 1 + 1 ulp (v_exp_f32).  numerator: sum_j |v_j| (p_j (eps + 2^-11) + 2^-25) + Tp u sum p |v| + sum p |dv|;
    denominator: relative eps + T u; 1 / sum and the product: 2 u."""
    B, heads, Tp, _ = q.shape
    nk = T if n_keys is None else n_keys
    s = np.einsum("bhqd,bhkd->bhqk", q, k)
    smag = np.einsum("bhqd,bhkd->bhqk", np.abs(q), np.abs(k))
    ds = 0.0
    if dq is not None:
        ds = np.einsum("bhqd,bhkd->bhqk", dq, np.abs(k) + dk) + np.einsum("bhqd,bhkd->bhqk", np.abs(q), dk)
    s, smag = s[..., :nk], smag[..., :nk]
    ds = ds[..., :nk] if dq is not None else 0.0
    sc = scale * math.log2(math.e)
    a = sc * (s - s.max(-1, keepdims=True))
    p = np.exp2(a)
    da = sc * (64 * U * smag + ds) + 2 * U * np.abs(s) * sc + U * np.abs(a)
    eps = (np.exp2(da.max(-1)) - 1.0 + ULP)[..., None]                      # [b][h][q][1]
    v = vt[..., :nk]                                                        # [b][h][d][k]
    pn = f16(p) if round_p else p
    psum = p.sum(-1)[..., None]
    out = np.einsum("bhqk,bhdk->bhqd", pn, v) / psum
    pv = np.einsum("bhqk,bhdk->bhqd", p, np.abs(v))
    num_err = pv * (eps + H_STORE + Tp * U) + H_SUB * np.abs(v).sum(-1)[:, :, None, :]
    if dv is not None:
        num_err = num_err + np.einsum("bhqk,bhdk->bhqd", p, dv[..., :nk])
    bound = num_err / psum + np.abs(out) * (eps + (nk + 2) * U)
    to_rows = lambda t: t.transpose(0, 2, 1, 3).reshape(B, Tp, heads * 64)   # noqa: E731
    out, bound = to_rows(out), to_rows(bound)
    return out, half_bound(out) + bound


# --------------------------------------------------------------------------------------------------------------- residual GEMMs, final
def resid_stage(A16, x_in, blk, dA=None):
    """x_in + gamma (A W^T + bias) for the real rows (the caller masks padding) -> (x, bound), fp32 output: (K + 1) u on the accumulation
    and the bias, one fma rounding on the result, and gamma x what the operand's uncertainty dA can move (the fused MLP kernel)."""
    Wh, b, gam = blk
    K = A16.shape[1]
    S, mag, extra = _gemm(A16, Wh, dA)
    x = x_in + gam[None, :] * (S + b[None, :])
    bound = np.abs(gam)[None, :] * ((K + 1) * U * (mag + np.abs(b)[None, :]) + extra) + U * np.abs(x) + U * np.abs(gam[None, :] * (S + b[None, :]))
    return x, bound


def final_stage(x, P, eps1=1e-6, eps2=1e-5):
    """x [B][Tp][D] -> tokens [B][Np][D] (fp32).  Two two-pass LayerNorms in fp32: each normalised value carries (D + 4) u relative from its
    mean and variance sums plus 1 ulp of rsqrtf, the affine 2 u; the second LayerNorm sees the first one's error divided by its own
    standard deviation.  Stated as a relative-to-magnitude bound on both steps."""
    nw, nb, cw, cb = P["final"]
    D = x.shape[-1]
    t = x[:, 1:P["T"]]

    def ln(v, w, b, eps, dv):
        mu = v.mean(-1, keepdims=True)
        c = v - mu
        var = (c * c).mean(-1, keepdims=True)
        r = 1.0 / np.sqrt(var + eps)
        n = c * r
        # error of c: u |v| + D u mean|v| + dv (and the mean of dv); of r: relative (D + 3) u + ULP + what dv moves the variance by
        dc = U * np.abs(v) + (D + 1) * U * np.abs(v).mean(-1, keepdims=True) + dv + dv.mean(-1, keepdims=True)
        dr = (D + 3) * U + ULP + (2 * np.abs(c) * dc).mean(-1, keepdims=True) / (var + eps) / 2
        dn = dc * r + np.abs(n) * dr + U * np.abs(n)
        return n * w + b, dn * np.abs(w) + 2 * U * (np.abs(n * w) + np.abs(b))
    y, dy = ln(t, nw, nb, eps1, np.zeros_like(t))
    z, dz = ln(y, cw, cb, eps2, dy)
    return z, dz


# --------------------------------------------------------------------------------------------------------------- the chain
def forward_chain(w, img, patch_h=16, rounding=True, acc=np.float64, faults=()):
    """All stages chained -> tokens [B][patch_h][pw][D].  rounding: the kernels' fp16 rounding points on / off (off: the exact forward of
    the fp32 weights).  acc: np.float64, or np.float32 = the same fp16 model with every product accumulated in fp32 by the BLAS (the noise
    floor of an end-to-end comparison).  faults: any of 'unmasked', 'tanh', 'ln_eps', 'scale' -- a planted wrong kernel."""
    img = np.asarray(img)
    B, H, W, _ = img.shape
    pw = int((14 * patch_h) / H * W / 14)
    P = pack(w, patch_h, pw, rounding)
    T, Tp, D, heads = P["T"], P["Tp"], P["D"], P["heads"]
    r16 = f16 if rounding else (lambda a_: a_)
    mm = lambda A_, W_: (A_.astype(acc) @ W_.astype(acc).T).astype(np.float64)   # noqa: E731
    eps = 1e-5 if "ln_eps" in faults else 1e-6
    pix, _ = preprocess_stage(img, patch_h, pw)
    x = np.zeros((B, Tp, D))
    x[:, 1:T] = mm(r16(pix).reshape(-1, 588), P["patch_w"]).reshape(B, T - 1, D) + P["patch_b"] + P["cls_pos"][None, 1:]
    x[:, 0] = P["cls_pos"][0]

    def ln_gemm(xv, Wh, b, c):
        xv = xv.reshape(-1, D)
        mean = xv.mean(-1, keepdims=True)
        var = np.maximum((xv * xv).mean(-1, keepdims=True) - mean * mean, 0.0)
        return (mm(r16(xv), Wh) - mean * c[None, :]) / np.sqrt(var + eps) + b[None, :]
    real = (np.arange(Tp) < T)[None, :, None]
    for blk in P["blocks"]:
        q, k, vt = split_qkv(r16(ln_gemm(x, *blk["qkv"])), B, Tp, heads)
        s = np.stack([[mm(q[b, h], k[b, h]) for h in range(heads)] for b in range(B)])
        nk = T + 1 if ("unmasked" in faults and T < Tp) else T
        sc = (1 / 8.1 if "scale" in faults else 0.125) * math.log2(math.e)
        p = np.exp2(sc * (s[..., :nk] - s[..., :nk].max(-1, keepdims=True)))
        pn = r16(p)
        o = np.stack([[mm(pn[b, h], vt[b, h][:, :nk]) for h in range(heads)] for b in range(B)]) / p.sum(-1)[..., None]
        a = r16(o.transpose(0, 2, 1, 3).reshape(B * Tp, D))
        Wp, bp, g1 = blk["proj"]
        x = np.where(real, x + (g1[None, :] * (mm(a, Wp) + bp[None, :])).reshape(B, Tp, D), 0.0)
        h = r16((gelu_tanh if "tanh" in faults else gelu_erf)(ln_gemm(x, *blk["fc1"])))
        W2, b2, g2 = blk["fc2"]
        x = np.where(real, x + (g2[None, :] * (mm(h, W2) + b2[None, :])).reshape(B, Tp, D), 0.0)
    out, _ = final_stage(x, P)
    return out.reshape(B, patch_h, pw, D)

// vit_plan.h -- what a ViT forward launches, resolved ONCE from the model, the batch and the calling thread's policy.  vfm_vit_forward
// (vit.hip) walks the plan through its launch table; the read-back vfm_debug_vit_plan prints it.  Host-only C++, no HIP call in here.
#pragma once
#include <stdint.h>

#include <string>

#include "../../include/vfmreg.h"
#include "config.h"

int vfm_fail(int code, const char* fmt, ...);

namespace vitplan {

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

enum VitEpi { VIT_EPI_PATCH = 0, VIT_EPI_QKV, VIT_EPI_RESID, VIT_EPI_GELU };   // = enum Epi of vit.hip

// the GEMM kernels' forms, each instantiated per epilogue (the token-stationary ones for QKV and GELU only)
enum VitGemmForm {
    VIT_DIRECT_1_8, VIT_DIRECT_1_16, VIT_DIRECT_2_8,   // vit_gemm_kernel<EPI, NT, PF>
    VIT_LDS,                                           // vit_gemm_lds_kernel<EPI, KB, NS>: + 2 * (index of the shape in 23 24 25 26 42 43) + DBG
    VIT_LDS_WIDE = VIT_LDS + 12,                       // vit_gemm_lds_kernel<EPI, 2, 4, 3, 8>: + DBG
    VIT_ASTAT_6 = VIT_LDS_WIDE + 2, VIT_ASTAT_8, VIT_ASTAT_12, VIT_ASTAT_16,   // vit_gemm_astat_kernel<EPI, NW, 6>
    VIT_ASTAT_12_NT,                                   // ... <EPI, 12, 6, true>
    VIT_ASTAT2,                                        // vit_gemm_astat2_kernel<EPI, 8, 4>
    VIT_GEMM_FORMS
};
enum VitInst {   // one per kernel instantiation the forward can launch; vit.hip's launch table is indexed by it
    VIT_NONE = -1,                         // the stage is inside another stage's kernel
    VIT_PRE_UNIT, VIT_PRE_PATCH,
    VIT_GEMM,                              // + 4 * VitGemmForm + VitEpi
    VIT_ATT = VIT_GEMM + 4 * VIT_GEMM_FORMS,   // vit_attention_kernel<NKT>: + NKT - 1 (1 .. 16)
    VIT_ATT_LDS = VIT_ATT + 16,            // vit_attention_lds_kernel<NKT>: + NKT - 1 (1 .. 16)
    VIT_FQA = VIT_ATT_LDS + 16,            // vit_qkv_attention_kernel<NKT>: + NKT - 1 (1 .. 12)
    VIT_MLP = VIT_FQA + 12,                // vit_mlp_kernel
    VIT_INST_COUNT
};
constexpr int VIT_LDS_SHAPES[6] = {23, 24, 25, 26, 42, 43};   // k-steps per stage x 10 + stages
constexpr int VIT_MLP_LDS = 144 * 1024 + 2 * 1536 * 4;

// an instantiation spelled from its template arguments
inline std::string vit_inst_name(int inst) {
    const auto n = [](int v) { return std::to_string(v); };
    if (inst == VIT_PRE_UNIT) return "vit_preprocess_kernel";
    if (inst == VIT_PRE_PATCH) return "vit_preprocess_patch_kernel";
    if (inst == VIT_MLP) return "vit_mlp_kernel";
    if (inst >= VIT_FQA) return "vit_qkv_attention_kernel<" + n(inst - VIT_FQA + 1) + ">";
    if (inst >= VIT_ATT_LDS) return "vit_attention_lds_kernel<" + n(inst - VIT_ATT_LDS + 1) + ">";
    if (inst >= VIT_ATT) return "vit_attention_kernel<" + n(inst - VIT_ATT + 1) + ">";
    static const char* const epi[4] = {"PATCH", "QKV", "RESID", "GELU"};
    const int form = (inst - VIT_GEMM) / 4;
    const std::string e = epi[(inst - VIT_GEMM) % 4];
    switch (form) {
        case VIT_DIRECT_1_8: return "vit_gemm_kernel<" + e + ",1,8>";
        case VIT_DIRECT_1_16: return "vit_gemm_kernel<" + e + ",1,16>";
        case VIT_DIRECT_2_8: return "vit_gemm_kernel<" + e + ",2,8>";
        case VIT_LDS_WIDE: return "vit_gemm_lds_kernel<" + e + ",2,4,3,8>";
        case VIT_LDS_WIDE + 1: return "vit_gemm_lds_kernel<" + e + ",2,4,3,8,dbg>";
        case VIT_ASTAT_6: return "vit_gemm_astat_kernel<" + e + ",6,6>";
        case VIT_ASTAT_8: return "vit_gemm_astat_kernel<" + e + ",8,6>";
        case VIT_ASTAT_12: return "vit_gemm_astat_kernel<" + e + ",12,6>";
        case VIT_ASTAT_16: return "vit_gemm_astat_kernel<" + e + ",16,6>";
        case VIT_ASTAT_12_NT: return "vit_gemm_astat_kernel<" + e + ",12,6,nt>";
        case VIT_ASTAT2: return "vit_gemm_astat2_kernel<" + e + ",8,4>";
    }
    const int shape = VIT_LDS_SHAPES[(form - VIT_LDS) / 2];
    return "vit_gemm_lds_kernel<" + e + "," + n(shape / 10) + "," + n(shape % 10) + ((form - VIT_LDS) % 2 ? ",dbg>" : ">");
}

struct VitLaunch {
    int inst = VIT_NONE;   // VitInst
    int grid = 0, block = 0, lds_bytes = 0;
    bool trace = false;    // this launch, and no other, gets the policy's trace buffer
    int hot_a = 0;         // GemmArgs::hot_a of the launch (tools; the LDS-tiled kernel reads it)
};
enum VitStage { VIT_ST_PRE, VIT_ST_PATCH, VIT_ST_QKV, VIT_ST_ATT, VIT_ST_PROJ, VIT_ST_FC1, VIT_ST_FC2, VIT_STAGES };
inline const char* vit_stage_name(int s) {
    static const char* const names[VIT_STAGES] = {"pre", "patch", "qkv", "att", "proj", "fc1", "fc2"};
    return names[s];
}
// One launch per stage.  QKV and attention are one launch under the fused kernel (att: VIT_NONE), fc1 and fc2 one under vit_mlp_kernel
// (fc2: VIT_NONE).  A block's launches are the same for every layer: the plan holds one block's worth.
struct VitPlan {
    VitLaunch st[VIT_STAGES];
    int launches = 0;              // of the whole forward, vit_final_kernel included
    int trace_stage = -1;          // VitStage of the launch with `trace`, -1: none
    int xcd_map = 0;               // "vit_xcd": GemmArgs::xcd_map of every launch, and the per-tile attention kernel's
};

// Wave tile (NT x 32 channels) and prefetch depth (PF k-steps) of the direct kernel.  Round 2 measurements on 6 x 1200 x 1600
// (tools/ab_vit.py, profiles/r02_pmc_vit.json): a wave lives ~2.5 us inside kernels that take 10-17 us -- the forward is bound by the
// ~5 us floor of each of its 87 launches, not by L2 latency or bandwidth: PF = 8 / 16 / 24 make no difference, 32-channel
// tiles everywhere (twice the waves) give 0.76 instead of 0.82 ms, 64 x 64 wave tiles and row-complete workgroups with the
// LayerNorm fused into the epilogue (63 launches, but 66 workgroups per GEMM) gave 1.04 ms and were removed again.
inline VitLaunch resolve_gemm(int epi, int M, int N, int KS, const VfmConfig& c, int cus) {
    VitLaunch l;
    const int tiles = M / 32, groups = cdiv(tiles, 4);
    if (epi == VIT_EPI_QKV || epi == VIT_EPI_GELU) {
        const int nw = c.vit_astat_nw == 112 ? 112 : (c.vit_astat_nw > 0 && (N / 32) % c.vit_astat_nw == 0 ? c.vit_astat_nw : 12);
        // The token-stationary kernel, one workgroup per compute unit: it pays when its rounds are full.  vit_astat_min > 0: from that many
        // groups on whatever the fill (tools); 0 (default): when the last round of `cus` workgroups is at least three quarters full and
        // there is at least one such round -- 69 ... 93 images of 1200 x 1600 at a time on 256 compute units (tools/ab_vit_astat.py:
        // 48 images 2.19 -> 2.30 ms, 84: 3.35 -> 3.22, 93: 3.60 -> 3.49, 96 = 264 groups, eight of them alone in a second round: 3.95 -> 4.58)
        const int last_round = groups % cus;
        const bool full_rounds = groups >= (3 * cus) / 4 && (last_round == 0 || 4 * last_round >= 3 * cus);
        const bool want = c.vit_astat_min > 0 ? groups >= c.vit_astat_min : (c.vit_astat_min == 0 && full_rounds);
        if (want && 4 * KS * 1024 <= 128 * 1024 && (nw == 112 || (N / 32) % nw == 0)) {   // (128 rows of A fit the LDS)
            l.grid = groups; l.lds_bytes = 4 * KS * 1024;
            if (c.vit_astat_two && (N / 64) >= 8 && N % 64 == 0 && KS % 4 == 0) {   // two channel tiles per wave, eight waves (round 5)
                l.inst = VIT_GEMM + 4 * VIT_ASTAT2 + epi; l.block = 512;
                return l;
            }
            // (As the ladder did: a "vit_astat_nw" that divides the channel tiles and is no instantiation -- 4, say -- passes the test above
            //  and takes the twelve-wave kernel WITHOUT (N / 32) % 12 == 0 being asked; tests/vit_plan_cases.py, astat-nw-4, pins it.)
            const int form = nw == 6 ? VIT_ASTAT_6 : nw == 112 ? VIT_ASTAT_12_NT   // (112, A/B: twelve waves, non-temporal output stores)
                             : nw == 8 ? VIT_ASTAT_8 : nw == 16 ? VIT_ASTAT_16 : VIT_ASTAT_12;
            l.inst = VIT_GEMM + 4 * form + epi;
            l.block = 64 * (nw == 6 || nw == 8 || nw == 16 ? nw : 12);
            return l;
        }
    }
    if (N % 128 == 0 && c.vit_lds_min_wg > 0 && KS % (c.vit_lds_shape / 10 == 4 ? 4 : 2) == 0) {   // (whole stages of 2 or 4 k-steps)
        if (groups * (N / 128) >= c.vit_lds_min_wg) {
            l.hot_a = c.vit_hot_a;
            if (epi == VIT_EPI_RESID && N == 384 && c.vit_wide_tile && KS % 2 == 0) {   // one workgroup per 128 tokens x all 384 channels (NG = 3)
                l.inst = VIT_GEMM + 4 * VIT_LDS_WIDE + epi;
                l.grid = 8 * cdiv(groups, 8); l.block = 512;
                l.lds_bytes = 4 * 16 * 2 * 1024;   // NS = 4 stages of (4 + 12) x KB = 2 KiB: 128 KiB
                return l;
            }
            int shape = 0;   // (an unknown "vit_lds_shape": 23)
            for (int i = 1; i < 6; ++i)
                if (c.vit_lds_shape == VIT_LDS_SHAPES[i]) shape = i;
            l.inst = VIT_GEMM + 4 * (VIT_LDS + 2 * shape) + epi;
            l.grid = 8 * cdiv(groups, 8) * (N / 128);   // every XCD: ceil(groups / 8) token groups x channel groups
            l.block = 256;
            l.lds_bytes = (VIT_LDS_SHAPES[shape] % 10) * 8 * (VIT_LDS_SHAPES[shape] / 10) * 1024;
            return l;
        }
    }
    const int cfg = N <= 512 ? c.vit_cfg_narrow : c.vit_cfg_wide;
    const int form = cfg == 116 ? VIT_DIRECT_1_16 : cfg == 208 ? VIT_DIRECT_2_8 : VIT_DIRECT_1_8, nt = cfg == 208 ? 2 : 1;
    // waves per workgroup: one -- the waves share nothing, and single waves are spread over more compute units (one scan, N = 384: 648 waves
    // were 168 workgroups); tools/ab_vit_wpw.py: 6 / 12 / 24 images 0.62 / 0.865 / 1.444 ms with four waves per workgroup, 0.62 / 0.845 / 1.425 with one
    const int wpw = c.vit_wpw > 0 ? c.vit_wpw : 1;
    l.inst = VIT_GEMM + 4 * form + epi;
    // "vit_xcd": every XCD gets ceil(tiles / 8) token tiles' worth of workgroups
    l.grid = c.vit_xcd ? 8 * cdiv(cdiv(tiles, 8) * (N / (32 * nt)), wpw) : cdiv(tiles * (N / (32 * nt)), wpw);
    l.block = 64 * wpw;
    return l;
}

// W: the source images' width (the one-workgroup-per-patch preprocessing needs two columns).  Every refusal of a forward that does not
// depend on its pointers is made here, once.
inline int resolve_vit(const vfm_vit_config& m, int B, int W, const VfmConfig& c, int cus, VitPlan& p) {
    p = VitPlan{};
    if (!(m.dim % 64 == 0 && m.dim == m.heads * 64 && m.dim <= 1024)) return vfm_fail(VFM_EINVAL, "vit: dim must be heads*64 and <= 1024");
    if (!(m.mlp_dim % 64 == 0 && m.depth >= 1 && m.depth <= 64)) return vfm_fail(VFM_EINVAL, "vit: bad mlp_dim / depth");
    if (!(m.patch == 14 && m.patch_h >= 1 && m.patch_w >= 1 && B >= 1)) return vfm_fail(VFM_EINVAL, "vit: bad patch grid");
    const int64_t T64 = (int64_t)m.patch_h * m.patch_w + 1;
    if (T64 > 512) return vfm_fail(VFM_EINVAL, "vit: at most 512 tokens per image supported (got %lld)", (long long)T64);
    const int D = m.dim, mlp = m.mlp_dim, heads = m.heads, Tp = cdiv((int)T64, 32) * 32, qt = Tp / 32;
    // (the GEMM epilogues address every activation buffer with 32-bit byte offsets and find a token tile's image by a 20-bit reciprocal)
    const uint64_t M64 = (uint64_t)B * (uint64_t)Tp;
    if (!(M64 * (uint64_t)(mlp > 3 * D ? mlp : 3 * D) * 4u < (1ull << 32) && M64 / 32 < 65536 &&
          (M64 / 32) * ((1u << 20) / (unsigned)qt + 1u) < (1ull << 32)))   // (the reciprocal's product is 32-bit in the kernels)
        return vfm_fail(VFM_EINVAL, "vit: batch of %d images too large for one call", B);
    const int M = (int)M64, KP = cdiv(3 * m.patch * m.patch, 32) * 32, groups = cdiv(M / 32, 4);
    p.xcd_map = c.vit_xcd;

    VitLaunch& pre = p.st[VIT_ST_PRE];
    pre.block = 256;
    if (c.vit_preprocess_patch && KP <= 640 && W >= 2) {
        pre.inst = VIT_PRE_PATCH; pre.grid = M;
    } else {   // round 1's kernel: a thread per fragment unit; padded token rows stay exactly zero in the residual stream
        pre.inst = VIT_PRE_UNIT; pre.grid = (int)(((int64_t)M * (KP / 16) * 2 + 255) / 256);
    }
    p.st[VIT_ST_PATCH] = resolve_gemm(VIT_EPI_PATCH, M, D, KP / 16, c, cus);

    // QKV + attention per (image, head) in one workgroup (vit_qkv_attention_kernel).  "vit_fused_qkv": n > 0 from n images on, -1 never,
    // 0 (default) the policy: one workgroup per compute unit, B x heads of them, an eighth per XCD in rounds of 32 -- from 24 images on
    // (below, the two kernels' many small workgroups fill the chip better) unless a second round would be less than a quarter full
    // (profiles/r06_ab_vit_fused_qkv_sweep.txt: 42 images -12.6 %, 44: +1.7 %, 48: +0.2 %, 54: -2.1 %, 84: -11 %, 86: -3.7 %; three
    // rounds and more: -4 ... -9 % wherever the last one ends)
    bool fused_qkv = false;
    if (D == 384 && qt <= 12) {
        const int per_xcd = cdiv(B * heads, 8), rounds = cdiv(per_xcd, 32), last = per_xcd - 32 * (rounds - 1);
        const int k = c.vit_fused_qkv;
        fused_qkv = k > 0 ? B >= k : (k == 0 && B >= 24 && (rounds >= 3 || rounds == 1 || 4 * last >= 32));
    }
    // fc1 -> GELU -> fc2 in one workgroup per 128 tokens (vit_mlp_kernel).  "vit_fused_mlp": n > 0 from n images on, -1 never, 0 (default)
    // the policy: one workgroup per compute unit whose loop moves nothing through HBM and whose epilogue moves everything -- a single round runs
    // in lockstep and ends level with the two kernels; from two rounds on the workgroups drift apart and it wins, IF the last round is full
    // (profiles/r06_ab_vit_fused_mlp_sweep.txt: 84 images 0 %, 144: +1.5 %, 156: -1.9 %, 168: -5.3 %, 180: -6.8 %, 192: +5.4 %, 252: -8.9 %)
    bool fused_mlp = false;
    if (D == 384 && mlp == 1536) {
        const int rounds = cdiv(groups, cus), k = c.vit_fused_mlp;
        fused_mlp = k > 0 ? B >= k : (k == 0 && rounds >= 2 && 5 * groups >= 4 * rounds * cus);
    }
    VitLaunch& qkv = p.st[VIT_ST_QKV];
    VitLaunch& att = p.st[VIT_ST_ATT];
    if (fused_qkv) {
        qkv.inst = VIT_FQA + qt - 1;
        qkv.grid = 8 * cdiv(B * heads, 8); qkv.block = 256;
        qkv.lds_bytes = 48 * 1024 + 2 * qt * 4096 + qt * 32 * 8;
    } else {
        qkv = resolve_gemm(VIT_EPI_QKV, M, 3 * D, D / 16, c, cus);
        att.block = 256;
        // K / V^T of an (image, head) shared by four query tiles through the LDS from "vit_att_lds_min" images on (0: never): at one scan the
        // one-wave-per-tile kernel's 396 waves spread over the chip win, at batches the shared form reads a quarter of the L2 bytes
        if (c.vit_att_lds_min > 0 && B >= c.vit_att_lds_min) {
            att.inst = VIT_ATT_LDS + qt - 1;
            att.grid = B * heads * ((qt + 3) / 4);
            att.lds_bytes = qt * 4096 + 16384;
        } else {
            att.inst = VIT_ATT + qt - 1;
            att.grid = c.vit_xcd ? 8 * cdiv(cdiv(M / 32, 8) * heads, 4) : cdiv(B * heads * qt, 4);
        }
    }
    p.st[VIT_ST_PROJ] = resolve_gemm(VIT_EPI_RESID, M, D, D / 16, c, cus);
    VitLaunch& fc1 = p.st[VIT_ST_FC1];
    if (fused_mlp) {   // (the file's second compile part)
        fc1.inst = VIT_MLP;
        fc1.grid = groups; fc1.block = 256; fc1.lds_bytes = VIT_MLP_LDS;
    } else {
        fc1 = resolve_gemm(VIT_EPI_GELU, M, mlp, D / 16, c, cus);
        p.st[VIT_ST_FC2] = resolve_gemm(VIT_EPI_RESID, M, D, mlp / 16, c, cus);
    }
    int per_block = 0;
    for (int s = VIT_ST_QKV; s < VIT_STAGES; ++s) per_block += p.st[s].inst != VIT_NONE;
    p.launches = 2 + m.depth * per_block + 1;

    // The tools' trace buffer goes to ONE launch of a block, named by "vit_trace_fused": 0 the token-stationary fc1 (one channel tile per
    // wave: the two-tile kernel keeps no trace), or else the LDS-tiled fc2; 1 vit_qkv_attention_kernel; 2 the LDS-tiled proj;
    // 3 vit_mlp_kernel.  Every other launch gets a null pointer.  The LDS-tiled kernel keeps its trace in its DBG twin.
    if (c.vit_astat_dbg) {
        const auto form_of = [&](int s) { return p.st[s].inst >= VIT_GEMM && p.st[s].inst < VIT_ATT ? (p.st[s].inst - VIT_GEMM) / 4 : -1; };
        const auto lds_tiled = [&](int s) { return form_of(s) >= VIT_LDS && form_of(s) < VIT_ASTAT_6; };
        const auto astat_one = [&](int s) { return form_of(s) >= VIT_ASTAT_6 && form_of(s) <= VIT_ASTAT_12_NT; };
        int s = -1;
        switch (c.vit_trace_fused) {
            case 0: s = astat_one(VIT_ST_FC1) ? VIT_ST_FC1 : lds_tiled(VIT_ST_FC2) ? VIT_ST_FC2 : -1; break;
            case 1: s = fused_qkv ? VIT_ST_QKV : -1; break;
            case 2: s = lds_tiled(VIT_ST_PROJ) ? VIT_ST_PROJ : -1; break;
            case 3: s = fused_mlp ? VIT_ST_FC1 : -1; break;
        }
        if (s >= 0) {
            p.st[s].trace = true;
            if (lds_tiled(s)) p.st[s].inst += 4;   // its DBG twin
            p.trace_stage = s;
        }
    }
    return VFM_OK;
}

// the plan as one line of text (include/vfmreg_debug.h, vfm_debug_vit_plan)
inline std::string vit_plan_line(const VitPlan& p) {
    std::string line;
    for (int s = 0; s < VIT_STAGES; ++s) {
        const VitLaunch& l = p.st[s];
        line += std::string(s ? " " : "") + vit_stage_name(s) + "=";
        line += l.inst == VIT_NONE ? std::string("-")
                                   : vit_inst_name(l.inst) + "@" + std::to_string(l.grid) + "x" + std::to_string(l.block) + "+" + std::to_string(l.lds_bytes);
    }
    return line + " launches=" + std::to_string(p.launches) + " trace=" + (p.trace_stage < 0 ? "none" : vit_stage_name(p.trace_stage));
}

}  // namespace vitplan

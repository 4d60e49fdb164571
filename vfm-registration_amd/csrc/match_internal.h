// match_internal.h -- declarations shared by the translation units of the matcher (csrc/match_*.hip): constants, the
// argument block and device helpers of the coarse kernels, the layout of prepared operands and search workspaces, and the
// host functions that cross translation units.  Kernels live in anonymous namespaces of the file that launches them.
#pragma once
#include "common.h"
#include "../../include/vfmreg_debug.h"

#include <type_traits>
#include <vector>

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx8 __attribute__((ext_vector_type(8)));
typedef int intx16 __attribute__((ext_vector_type(16)));

#define GLOBAL_AS __attribute__((address_space(1)))
#define LDS_AS __attribute__((address_space(3)))

namespace vfmm {

constexpr int TILE_ROWS = 32;     // rows per fragment tile
constexpr int CHUNK_ROWS = 128;   // map rows per partial record (4 tiles)
constexpr int ROW_PAD = 256;      // prepared operands are padded to a multiple of this
constexpr int QBLOCK = 256;       // queries per workgroup of the coarse kernel (8 waves x 32)
// LDS ring depth in tiles: a step consumes 2 tiles; 6 buffers = 2 steps in flight (d <= 384),
// 4 buffers = 1 step in flight when a tile is 32 KiB (d = 512): 160 KiB of LDS per CU.
constexpr int ring_depth(int ksteps) { return ksteps <= 24 ? 6 : 4; }
constexpr int CAND_CAP_MAX = 2048;  // candidate entries a query can hold = min(#chunks, this), a multiple of 64 (cand_cap());
                                    // beyond it the query is decided by the all-pairs kernel.  At C2 (1563 chunks) the cap
                                    // cannot be exceeded: every chunk fits in the list.
constexpr int REFINE_MIN = 3;     // queries with this many candidate entries (or a whole-chunk entry) go through the fp32 refinement
constexpr int REFINE_MIN_I8 = 8;  // the same threshold for the row lists of the int8 pass (match_rescan_kernel)
constexpr int REFINE_KEEP = 64;   // rows a query may keep after the refinement
// candidate queries a map chunk can collect for the chunk-major int8 rescan (the rest: query-major): sized per search from the
// queries per chunk -- 128 per average query share, at least 1024 (C2: 1664; the reverse direction of a Euclidean search, 200 000
// queries on 157 chunks: 65 536; round 2's fixed 512 sent such searches through the 48-KB-per-candidate query-major path)
__host__ __device__ inline int rescan_bin_cap(int64_t npad, int64_t nchunks) {
    int64_t c = (128 * npad / (nchunks > 0 ? nchunks : 1) + 63) / 64 * 64;
    return (int)(c < 1024 ? 1024 : (c > 65536 ? 65536 : c));
}
// One counter per 128-byte line: device-scope atomics are resolved at the memory side, line by line -- 1563 counters in 49
// consecutive lines took ~0.3 ns per atomic whatever the number of threads (select_best: 64 us of 122 at 250 000 candidates, 283 of
// 345 at 920 000).
constexpr int BIN_CNT_STRIDE = 32;
constexpr int RESCAN_SLICE = 256;    // bin entries one workgroup of match_rescan_chunk_kernel takes (grid.y slices a long bin; 1024 until the end of round 4: the longest workgroups -- 32 blocks of 2.6 us -- were the kernel, 155 -> 140 us at 590 queries per chunk; 128 pays more prologues than it balances)
// Half-width pass, device-side guard: a search whose bound leaves more than this many (query, chunk) pairs per query -- descriptors
// that are all alike: every chunk survives -- does not rescan them (31 million 128-row rescans at C2: 171 ms) but falls through,
// inside the same _finish call, to match_gatepass_kernel: one full-width int8 MFMA pass with the gate as hit test (2-3 ms).
// SearchWs::fb_count[7] is the flag (half_guard_kernel); the host policy (vfmreg/pipeline.py) leaves the mode on the same figure.
constexpr int HALF_GUARD_PER_QUERY = 48;
constexpr int HALF_GUARD_FLAG = 7;   // index into fb_count
enum { MX6_BEST = 0, MX6_TOP2 = 1, MX6_FUSE = 2 };   // KIND of match_coarse_mx6q2_kernel
constexpr int MX6_LTAB = 256;       // per-chunk constants of a workgroup's slice kept in the LDS (resolve_coarse keeps slices this short)
constexpr int MX6_LCAP = 2047;      // FUSE: survivors a workgroup can list (+ the header = 8 KiB)
constexpr int MX6_SURV_SLOT_WORDS = MX6_LCAP + 4;   // fused fp6 half-width pass: a workgroup's survivor slot = header (4 words) + up to MX6_LCAP entries
constexpr int MX6_GRID_SLOT = 32;    // fb_count[.]: workgroups of the fused fp6 half-width kernel = survivor slots match_bin_survivors_kernel walks
constexpr int FUSE_BIN_SATURATE_X = 8;  // fused form: a chunk that collected this many times its bin capacity stops recording (and raises the flag)
constexpr int FILTER_LDS_ROWS = 1024;  // sparse fp16 records a query can hold (= SearchWs::rcap; match_filter_refine_kernel keeps them in LDS)
constexpr int SPARSE_LREC_CAP = 1536;  // records a workgroup of the sparse coarse kernel buffers in LDS (12 KiB)
constexpr float COARSE_OFFSET = 2.0f;   // accumulators start here: every coarse score is a
                                        // positive normal float, so uint order == float order
constexpr float DEFAULT_WINDOW = 2.5e-3f;  // >= 2E, E = proven |coarse - exact| bound
constexpr int I8_OFFSET = 1 << 30;  // int8 coarse pass: accumulators start here (scores positive: uint order == int order)
constexpr int I8_GROUP = 128;       // rows that share one quantisation step (= CHUNK_ROWS: a record never mixes two steps)
static_assert(I8_GROUP == 128, "match_select_kernel and the coarse records assume 128-row groups");

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// ---------------------------------------------------------------------------------------------
// prepared operand layout: [inv: rows_pad floats][tiles: rows_pad/32 x (d/16 ksteps) x 64 x 16 B]
// unit (tile, s, h, p) = 8 fp16 = row (tile*32+p), k = 16 s + 8 h .. +7  at uint4 index
// tile*(d/16*64) + s*64 + h*32 + p : exactly the register image of one 32x32x16 MFMA operand.
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline int cand_cap(int64_t map_rows_padded) {
    int64_t c = (map_rows_padded / 128 + 63) / 64 * 64;
    return (int)(c < 64 ? 64 : (c > CAND_CAP_MAX ? CAND_CAP_MAX : c));
}
__host__ __device__ inline int64_t rows_padded(int64_t rows) { return (rows + ROW_PAD - 1) / ROW_PAD * ROW_PAD; }

// sum of squares in the oracle's order: lane l owns the float4 chunks c with c % 64 == l
// (ascending c, ascending element inside a chunk), then an xor butterfly.  d <= 1024.
template <bool STREAM = false>
__device__ __forceinline__ float row_sumsq_wave(const float* __restrict__ row, int d, float4 (&v)[4]) {
    const int lane = lane_id();
    const int nchunks = d >> 2;
    float p = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < nchunks) {
            if constexpr (STREAM) {  // read-once data: do not displace the coarse pass' map slice from L2
                const float* pc = row + 4 * c;
                x.x = __builtin_nontemporal_load(pc);
                x.y = __builtin_nontemporal_load(pc + 1);
                x.z = __builtin_nontemporal_load(pc + 2);
                x.w = __builtin_nontemporal_load(pc + 3);
            } else {
                x = reinterpret_cast<const float4*>(row)[c];
            }
            float t;
            t = x.x * x.x; p = p + t;
            t = x.y * x.y; p = p + t;
            t = x.z * x.z; p = p + t;
            t = x.w * x.w; p = p + t;
        }
        v[i] = x;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_xor(p, off);
    return p;
}

__device__ __forceinline__ float inv_norm_from_sumsq(float nr) {
    // faiss: const float inv_nr = 1.0 / sqrtf(nr);  (double divide, rounded to float)
    if (!(nr > 0.0f)) return 0.0f;
    float s = sqrtf(nr);  // __builtin_sqrtf: correctly rounded (HIP default); __fsqrt_rn is the native approximation
    return (float)(1.0 / (double)s);
}

// ---------------------------------------------------------------------------------------------
// coarse pass
// ---------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if constexpr (N == 18) asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
    else if constexpr (N == 24) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    else static_assert(N < 0, "unsupported vmcnt");
}

// LDS-DMA, 16 B per lane: LDS destination = wave-uniform byte address in M0 + lane * 16.
// Issued from inline asm so that hipcc neither counts it nor drains it (it would place an
// s_waitcnt vmcnt(0) in front of the next ds_read); completion is tracked by wait_vmcnt<N>().
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst_uniform) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gsrc), "s"(lds_dst_uniform)
        : "memory");
}

// The same, 4 B per lane: LDS destination = M0 + lane * 4 (a gather of one dword per lane).
__device__ __forceinline__ void glds4(const void* gsrc, unsigned lds_dst_uniform) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dword %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gsrc), "s"(lds_dst_uniform)
        : "memory");
}

__device__ __forceinline__ unsigned umed3(unsigned a, unsigned b, unsigned c) {
    return max(min(a, b), min(max(a, b), c));
}

// per-row / per-group quantisation data of the two operands of an int8 pass (qerr == NULL: fp16 records)
struct I8Bounds {
    const float* qerr;   // [npad] E of every query row
    const float* qstep;  // [npad / 128] step of the query's group
    const float* bstep;  // [nchunks] step of the map chunk
    const float* berr;   // [nchunks] maximum E of the map chunk
    int top2;            // records: 0 = best score per (query, chunk), 1 = packed top-2 with the best row's index
};
// Euclidean mode of the int8 finish stage (row A6, match_l2i8.hip; qn == NULL: inner-product mode).  The int8 image holds the
// NORMALISED rows, so the proven bound  cosU = s_q s_c S + A + B_c  bounds the cosine; with the commonly scaled norms |a~|, |b~|
// (<= 1) the Euclidean score  a~.b~ - |b~|^2 / 2  of a row is at most  qn * bn * max(cosU, 0) - bn^2 / 2 + slack  (slack covers
// the fp32 roundings of the norms: (d + 16) 2^-22).  Map rows are SORTED by norm, so a chunk's norms span a narrow [lo, hi].
struct L2Terms {
    const float* qn;   // [npad] |a~| per query
    const float* bn;   // [mpad] |b~| per map row, in the (sorted) row order of the int8 image
    float slack;
};
__device__ __forceinline__ float l2_upper_row(float qn, float bn, float cosU, float slack) {
    return __builtin_fmaf(qn * bn, fmaxf(cosU, 0.0f), -0.5f * bn * bn) + slack;
}

// float <-> unsigned key with the same order (0 = below every float: the memset value of "nothing published")
__device__ __forceinline__ unsigned float_key(float f) {
    const int k = __float_as_int(f);
    return (unsigned)(k >= 0 ? k : k ^ 0x7FFFFFFF) ^ 0x80000000u;
}
__device__ __forceinline__ float key_float(unsigned u) {
    if (u == 0u) return -__builtin_inff();
    const int k = (int)(u ^ 0x80000000u);
    return __int_as_float(k >= 0 ? k : k ^ 0x7FFFFFFF);
}

struct CoarseArgs {
    const uint4* Qh;     // query fragment tiles
    const uint4* Bh;     // map fragment tiles
    uint2* partials;     // [nchunks][npad]
    int nq_tiles;        // valid 32-query tiles
    int nchunks;         // map chunks (128 rows)
    long long m_valid;   // real map rows
    int npad;            // padded query count (row stride of partials)
    int nqb;             // query blocks (256 queries)
    int nslices;         // map slices
    unsigned* qmax;      // [npad] running coarse maximum per query (value bits only), zeroed per search
    int first_pad_chunk; // chunks >= this contain zero-padded map rows: excluded from qmax
    const float* row_bias;  // [padded map rows] added to the accumulator start of that row, or NULL
                            // (Euclidean search for d > 510: -|b~|^2 / 2; match_coarse_r_kernel only)
    // sparse row-level records (match_coarse_pipe_kernel<., true>): every (query, map row) whose coarse score is
    // within `window` of the query's running maximum at that time -- a superset of the rows within `window` of the
    // final maximum, which is all the exact decision needs
    const float* qinv;   // [npad] 1/|query row| (0 for zero rows: they record nothing, match_rescore_kernel decides them)
    // seed units (sparse path): the first seed_parts * seed_chunks chunks of the map are taken by short workgroups at the
    // head of the grid, seed_parts per query block, so that every later unit of a query block starts from a published
    // maximum (a fresh running maximum breaks records at rate ~1/k per row; with 55 slices, 15 % of the units used to
    // start unseeded and the record-breaking phase cost the kernel 5 %)
    int seed_parts, seed_chunks, nseed_pad;
    unsigned* rec_cnt;   // [npad] records appended per query (may exceed rcap: overflow)
    uint2* rec;          // [npad][rcap] (map row, score bits)
    int rcap;
    float window;
    I8Bounds ib;         // int8 pass: qmax receives float_key(lower bound of the query's exact maximum) instead of score bits
    // half-width pass with the selection fused into the coarse kernel (VFM_RECORDS_HALF_FUSED): no records are written --
    // a (query, chunk) pair whose bound reaches `gate` goes straight into the chunk's bin (or, past the bin, the query's list)
    float gate;
    int64_t n_valid;        // real queries
    const float* qrest;     // [npad] |second half of the normalised query|, rounded up
    const float* grest;     // [nchunks] its maximum over the chunk's rows
    unsigned* bin_cnt;      // [nchunks * BIN_CNT_STRIDE], zeroed per search
    int* bins;              // [nchunks][bin_cap]
    int bin_cap;
    int* cand_cnt;          // [npad], zeroed per search (entries of the query's own list)
    unsigned* cand;         // [npad][cap]
    int cap;
    int* survivors;         // fb_count + 5: the search's load figure
    unsigned long long* qbest;   // VFM_RECORDS_MX6_PILOT: [npad] (float_key(lower bound) << 32 | chunk) of the query's best chunk, by 64-bit atomicMax (NULL: not kept)
    int tune;               // (A/B, vfm_config "mx6_tune") bit 0: waves 4 - 7 of a workgroup of the fp6 kernel at s_setprio 1; bit 2: absent query sets are multiplied (as copies of tile 0)
    unsigned* surv;         // VFM_RECORDS_MX6_HALF_FUSED / _MX6_FUSED: a slot of MX6_SURV_SLOT_WORDS words per workgroup (in the record buffer)
};

// XCD-aware unit mapping shared by the coarse kernels: workgroup b runs on XCD b % 8 (observed, speed
// only); every XCD gets one contiguous range of (slice-major) units so that co-resident workgroups stream
// the same map slice through that XCD's L2.  Unit = (query block qb, map slice); tiles [4 c0, 4 c1).
struct CoarseUnit {
    int qb, c0, ntiles;
};
__device__ __forceinline__ CoarseUnit coarse_unit(const CoarseArgs& a) {
    const int total = a.nqb * a.nslices;
    int bid = blockIdx.x;
    const int seed_total = a.seed_parts * a.seed_chunks;  // chunks [0, seed_total) belong to the seed units
    if (bid < a.nseed_pad) {  // nseed_pad is a multiple of 8: the XCD phase of the remaining grid is unchanged
        CoarseUnit u;
        u.qb = bid / a.seed_parts;
        u.c0 = (bid - u.qb * a.seed_parts) * a.seed_chunks;
        u.ntiles = (u.qb < a.nqb) ? a.seed_chunks * 4 : 0;  // padding workgroups of the seed round: nothing to do
        return u;
    }
    bid -= a.nseed_pad;
    const int xcd = bid & 7, within = bid >> 3;
    const int qn = total >> 3, rn = total & 7;
    const int unit = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + within;
    const int slice = unit / a.nqb;
    CoarseUnit u;
    u.qb = unit - slice * a.nqb;
    const int rest = a.nchunks - seed_total;
    u.c0 = seed_total + (int)(((long long)slice * rest) / a.nslices);
    const int c1 = seed_total + (int)(((long long)(slice + 1) * rest) / a.nslices);
    u.ntiles = (c1 - u.c0) * 4;
    return u;
}

// One accumulator element into the running top-2 of its chunk: 3 VALU ops, branch-free.  code = 16 * tile
// in chunk + accumulator register; zero-padded map rows (score exactly 2.0) are NOT masked here:
// match_select_kernel ignores padded chunks for the maximum and rescans them exactly.
__device__ __forceinline__ void coarse_fold_bits(unsigned& s1, unsigned& s2, unsigned bits, int code) {
    const unsigned pk = (bits & 0xFFFFFFC0u) | (unsigned)(63 - code);
    s2 = umed3(s1, s2, pk);
    s1 = max(s1, pk);
}
__device__ __forceinline__ void coarse_fold(unsigned& s1, unsigned& s2, float v, int code) { coarse_fold_bits(s1, s2, __float_as_uint(v), code); }
__device__ __forceinline__ void coarse_fold(unsigned& s1, unsigned& s2, int v, int code) { coarse_fold_bits(s1, s2, (unsigned)v, code); }
__device__ __forceinline__ unsigned score_bits(float v) { return __float_as_uint(v); }
__device__ __forceinline__ unsigned score_bits(int v) { return (unsigned)v; }

// End of a 128-row chunk: merge the two half-waves and emit the chunk's top-2 for the 32 queries of tile
// qt (chunk < 0: the dummy fold of the very first step, nothing is stored); resets the running pair.
__device__ __forceinline__ unsigned coarse_emit_chunk(const CoarseArgs& a, unsigned& s1, unsigned& s2, unsigned& runmax,
                                                      int qt, int chunk) {
    const int lane = lane_id(), hi = lane >> 5;
    const unsigned o1 = __shfl_xor(s1, 32), o2 = __shfl_xor(s2, 32);
    const bool own = (s1 > o1) || (s1 == o1 && hi == 0);
    const unsigned w1 = own ? s1 : o1;
    const int wh = own ? hi : (1 - hi);
    const unsigned w2 = max(max(s2, o2), min(s1, o1));
    const int code = 63 - (int)(w1 & 63u);
    const int li = (code >> 4) * 32 + (code & 3) + 8 * ((code & 15) >> 2) + 4 * wh;  // row inside the chunk
    if (lane < 32 && qt < a.nq_tiles && chunk >= 0) {
        // int8 pass: [query tile][chunk][32] (a query tile's records are one contiguous stream for match_select_top2_kernel);
        // fp16 pass: [chunk][npad]
        const size_t at = a.ib.qerr ? ((size_t)qt * a.nchunks + (size_t)chunk) * 32 + lane : (size_t)chunk * a.npad + (size_t)qt * 32 + lane;
        a.partials[at] = make_uint2((w1 & ~127u) | (unsigned)li, w2);
        if (chunk < a.first_pad_chunk) runmax = max(runmax, w1 & ~127u);
    }
    s1 = 0u;
    s2 = 0u;
    return w1 & ~127u;  // the chunk's best score, low 7 bits dropped (all lanes)
}

// int8 pass: the chunk's BEST VALUE only -- one VALU op per accumulator element instead of three (with the packed top-2 the
// fold had become the kernel's limiter: the int8 MFMA halves the matrix time per element -- 5 VALU ops per MFMA, matrix pipe
// 56 % busy) and a 4-byte record.  Which rows of a candidate chunk matter is found by match_refine_kernel's int8 rescan.
__device__ __forceinline__ unsigned coarse_emit_chunk_best(const CoarseArgs& a, unsigned& s1, int qt, int chunk) {
    const int lane = lane_id();
    const unsigned w1 = max(s1, (unsigned)__shfl_xor(s1, 32));
    // layout [query tile][chunk][32]: a wave's records of consecutive chunks are consecutive 128-byte lines, and
    // match_select_kernel reads each query tile as one contiguous stream
    if (lane < 32 && qt < a.nq_tiles && chunk >= 0)
        reinterpret_cast<unsigned*>(a.partials)[((size_t)qt * a.nchunks + (size_t)chunk) * 32 + lane] = w1;
    s1 = 0u;
    return w1;
}

// the common scale of a Euclidean search (l2_maxnorm_kernel leaves the largest fp32 sum of squares of both sets in max_bits):
// 2^-k with 2^k >= sqrt(max sum of squares) * 1.01 (the fp32 sums above are good to ~1e-6)
__device__ __forceinline__ float l2_scale(const unsigned* max_bits) {
    const float mx = __uint_as_float(*max_bits);
    if (!(mx > 0.f) || !(mx < 3.0e38f)) return 1.0f;
    const float s = sqrtf(mx) * 1.01f;
    int e;
    (void)frexpf(s, &e);  // s = f * 2^e, f in [0.5, 1)  =>  2^e > s
    return ldexpf(1.0f, -e);
}

// (wave_argmax and the rest of the fp64 decision: match_exact.h)

// =============================================================================================
// host side
// =============================================================================================
struct Prepared {
    float* inv;
    uint4* tiles;
    // int8 image (i8_capable(d); prep_chunk_kernel)
    float* err;       // E per row
    float* gstep;     // quantisation step per group of 128 rows
    float* gerr;      // maximum E per group
    uint4* tiles8;    // int8 fragment tiles
    uint4* tiles8h;   // int8 fragment tiles of the first d / 2 columns
    float* rest;      // per row: |second half of the normalised row|_2, rounded up
    float* grest;     // its maximum per group
    // fp6 image (mx6_width(d); prep_chunk_kernel<., ., true>, written on request: VFM_PREPARE_MX6)
    uint4* tiles6;    // MX fp6 (e2m3) fragment tiles of the 32x32x64 scaled MFMA
    float* err6;      // per row: |v - dequantised row|_2 rounded up, plus the slack of the pass's fp32 / fixed-point arithmetic
    float* gerr6;     // its maximum per group
    float* gstep6;    // MX6_FIX_STEP for every group (the records are fixed-point: I8Bounds needs a step per group)
    float* err6h;     // per row: the same residual norm over the FIRST d / 2 columns only -- what the half-width pass multiplies
    float* gerr6h;    // its maximum per group
    // the int8 image once more, ROW-major (d bytes per row), for operands of at most ROWS8_MAX_ROWS rows -- scans: the chunk-major
    // rescan gathers 32 queries' k-steps per LDS-DMA instruction, and from the fragment tiles that is 64 different 128-byte lines per
    // instruction (a query's 16-byte units lie 512 bytes apart), from rows 32 lines that the block's other k-steps touch again
    unsigned char* rows8;
    size_t bytes;
};
constexpr int64_t ROWS8_MAX_ROWS = 131072;

// widths the int8 coarse pass exists for (match_coarse_pipe_kernel<d/32, false, true>; d = 128 has too few k-steps for the
// fragment ring)
inline bool i8_capable(int d) { return d == 256 || d == 384 || d == 512 || d == 640 || d == 768; }
// widths the fp6 pass (VFM_RECORDS_MX6) has a kernel for: two resident query sets of d / 64 x 8 registers
inline bool mx6_width(int d) { return d == 256 || d == 384; }
// widths whose HALF-width pass has an fp6 kernel (d / 128 k-steps of queries in registers): the fp6 image exists for these
inline bool mx6_half_width(int d) { return d == 256 || d == 384 || d == 512 || d == 768; }
constexpr float MX6_FIX_STEP = 0.0009765625f;   // 2^-10: an fp6 record is ceil(score * 2^20) -- "integer score" x step x step
// ---------------------------------------------------------------------------------------------
// fp6 image (VFM_PREPARE_MX6), dense since round 4.  Lane l of v_mfma_scale_f32_32x32x64_f8f6f4 holds, for row l & 31 of a 32-row
// tile, the 32 columns 64 s + 32 (l >> 5) ... of k-step s as 32 consecutive 6-bit codes = 24 bytes, and one E8M0 scale per
// k-step.  A stored tile (KS = d / 64 k-steps):
//     [scale plane 0: 64 lanes x 8 B -- byte s of lane l = scale of k-step s < 8]
//     [k-step 0: plane A = 64 lanes x 16 B (code bytes 0 .. 15) | plane B = 64 lanes x 8 B (code bytes 16 .. 23)] [k-step 1] ...
//     [scale plane 1 (KS > 8 only): k-steps 8 ..]
// so a wave's fragment of a k-step is one ds_read_b128 at 16-byte stride + one ds_read_b64 at 8-byte stride -- both free of bank
// conflicts (MI355X_MICROARCH.md, LDS; round 3's 16-byte units with 8 spare bytes cost 35 % of the LDS cycles in conflicts and a
// third more bytes to stage) -- and the scales + the first KS / 2 k-steps, what the half-width pass reads, are a PREFIX of the tile.
// ---------------------------------------------------------------------------------------------
constexpr int MX6_SCALE_PLANE = 512;
constexpr int MX6_KSTEP_BYTES = 1536;
__host__ __device__ constexpr int mx6_tile_bytes(int ks) { return MX6_SCALE_PLANE + ks * MX6_KSTEP_BYTES + (ks > 8 ? MX6_SCALE_PLANE : 0); }
__host__ __device__ inline size_t mx6_code_a(int s, int lane) { return (size_t)MX6_SCALE_PLANE + (size_t)s * MX6_KSTEP_BYTES + (size_t)lane * 16; }
__host__ __device__ inline size_t mx6_code_b(int s, int lane) { return (size_t)MX6_SCALE_PLANE + (size_t)s * MX6_KSTEP_BYTES + 1024 + (size_t)lane * 8; }
__host__ __device__ inline size_t mx6_scale_at(int ks, int s, int lane) {
    return (s < 8 ? 0 : (size_t)MX6_SCALE_PLANE + (size_t)ks * MX6_KSTEP_BYTES) + (size_t)lane * 8 + (size_t)(s & 7);
}
// one lane's operand of a k-step of v_mfma_scale_f32_32x32x64_f8f6f4 in e2m3: 32 codes in six registers (the instruction reads v[n:n+5])
struct Mx6Frag {
    int c[6];
};
// k-step S (0 .. 7) of the scaled MFMA: xs / ys hold the lane's eight E8M0 scales, byte S & 3 of .x (S < 4) or .y (a kernel that
// multiplies four k-steps at the most leaves .y unset: it is never read)
template <int S>
__device__ __forceinline__ floatx16 mfma_mx6(const Mx6Frag& x, const uint2& xs, const Mx6Frag& y, const uint2& ys, floatx16 c) {
    intx8 a, b;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        a[i] = x.c[i];
        b[i] = y.c[i];
    }
    a[6] = a[7] = b[6] = b[7] = 0;   // not read: cbsz = blgp = 2 (e2m3) takes six registers per operand
#ifdef VFM_ABL_NOSCALE   // (timing experiment, tools/ablate6.py: the unscaled instruction -- results are garbage)
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 2, 2, 0, 0, 0, 0);
#else
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 2, 2, S & 3, (int)(S < 4 ? xs.x : xs.y), S & 3,
                                                           (int)(S < 4 ? ys.x : ys.y));
#endif
}

inline Prepared carve_prepared(void* p, int64_t rows, int d) {
    VfmCarver c(p);
    Prepared r;
    const int64_t rp = rows_padded(rows);
    r.inv = c.take<float>((size_t)rp);
    r.tiles = c.take<uint4>((size_t)rp / TILE_ROWS * (size_t)(d / 16) * 64);
    r.err = nullptr;
    r.gstep = r.gerr = nullptr;
    r.tiles8 = nullptr;
    r.tiles8h = nullptr;
    r.rest = r.grest = nullptr;
    r.tiles6 = nullptr;
    r.err6 = r.gerr6 = r.gstep6 = nullptr;
    r.err6h = r.gerr6h = nullptr;
    r.rows8 = nullptr;
    if (i8_capable(d)) {  // behind the fp16 image: the Euclidean path carves the same layout and ignores the rest
        r.err = c.take<float>((size_t)rp);
        r.gstep = c.take<float>((size_t)rp / I8_GROUP);
        r.gerr = c.take<float>((size_t)rp / I8_GROUP);
        r.tiles8 = c.take<uint4>((size_t)rp / TILE_ROWS * (size_t)(d / 32) * 64);
        // half-width pass (VFM_RECORDS_HALF): the int8 image of the first d / 2 columns as tiles of their own, the norm of
        // the OTHER half of every normalised row (rounded up) and its maximum per 128-row group
        r.tiles8h = c.take<uint4>((size_t)rp / TILE_ROWS * (size_t)(d / 64) * 64);
        r.rest = c.take<float>((size_t)rp);
        r.grest = c.take<float>((size_t)rp / I8_GROUP);
        if (mx6_half_width(d)) {   // the fp6 image: 24 bytes of codes per (row, 64 columns) + the block scales (mx6_tile_bytes)
            r.tiles6 = c.take<uint4>((size_t)rp / TILE_ROWS * (size_t)(mx6_tile_bytes(d / 64) / 16));
            r.err6 = c.take<float>((size_t)rp);
            r.gerr6 = c.take<float>((size_t)rp / I8_GROUP);
            r.gstep6 = c.take<float>((size_t)rp / I8_GROUP);
            r.err6h = c.take<float>((size_t)rp);
            r.gerr6h = c.take<float>((size_t)rp / I8_GROUP);
        }
        if (rp <= ROWS8_MAX_ROWS) r.rows8 = c.take<unsigned char>((size_t)rp * (size_t)d);
    }
    r.bytes = c.used();
    return r;
}

struct SearchWs {
    uint2* partials;
    int* cand_cnt;
    unsigned* cand;
    int cap;  // entries per query in `cand`
    unsigned* rec_cnt;  // sparse records of the coarse pass (see CoarseArgs)
    uint2* rec;
    int rcap;
    int* fb_count;
    int* fb_list;
    unsigned* qmax;
    unsigned* bin_cnt;  // int8 pass, best-score records: candidate queries per map chunk ...
    unsigned* hit_cnt;  // rows match_rescan_chunk_kernel appended to a query's list, one counter per 128-byte line (added to cand_cnt by
                        // match_rescan_close_kernel): the lists' own lengths sit 32 to a line, and a line is what the memory side serialises
    int* bins;          // ... and the queries themselves, bin_cap per chunk (match_rescan_chunk_kernel)
    int bin_cap;        // rescan_bin_cap(npad, chunks)
    unsigned long long* qbest;   // [npad] VFM_RECORDS_MX6_PILOT: the query's best chunk (CoarseArgs::qbest); inside the zeroed region
    float* cand_up;     // [npad][cap] upper bound of the exact score of the rows match_rescan_chunk_kernel appended (same positions as
                        // `cand`; other entries' slots are never read): match_refine_kernel drops rows below the list's best lower bound
    size_t bytes;
};

// The survivor slots of the fused fp6 kinds, one per workgroup: the most map slices and the most query blocks the record buffer is sized
// for.  carve_search sizes it by them and resolve_coarse refuses a launch beyond them.
inline int64_t surv_slot_slices(int64_t nchunks) {
    const int64_t slices = nchunks / 8 < 1 ? 1 : (nchunks / 8 > 64 ? 64 : nchunks / 8);   // at most min(64, chunks / 8) slices, at least one
    const int64_t tab = (nchunks + 254) / 255;   // (a slice's per-chunk constants fit the kernel's LDS table: <= 255 chunks)
    return slices < tab ? tab : slices;
}
inline int64_t surv_slot_qblocks(int64_t npad) { return npad / 512 + 1; }

inline SearchWs carve_search(void* p, int64_t n, int64_t m) {
    VfmCarver c(p);
    SearchWs w;
    const int64_t npad = rows_padded(n), mpad = rows_padded(m);
    // the records of a coarse pass: per (chunk, query) 8 bytes -- or, for the fused fp6 half-width pass (which writes none), one slot
    // of MX6_SURV_SLOT_WORDS words per workgroup: surv_slot_qblocks x surv_slot_slices of them
    {
        const size_t nch = (size_t)(mpad / CHUNK_ROWS);
        const size_t slots = (size_t)surv_slot_qblocks(npad) * (size_t)surv_slot_slices((int64_t)nch) * (size_t)MX6_SURV_SLOT_WORDS;   // 4-byte words
        const size_t recs = nch * (size_t)npad;                                                  // 8-byte records
        w.partials = c.take<uint2>(recs > (slots + 1) / 2 ? recs : (slots + 1) / 2);
    }
    w.cand_cnt = c.take<int>((size_t)npad);
    w.cap = cand_cap(mpad);
    w.cand = c.take<unsigned>((size_t)npad * (size_t)w.cap);
    w.fb_list = c.take<int>((size_t)npad);
    // zeroed before every search by ONE memset (search_zero_bytes): [fb_count (64, padded to 256 B) | qmax (npad) |
    // rec_cnt (npad) | bin_cnt (chunks padded to 64, x BIN_CNT_STRIDE) | hit_cnt (npad x BIN_CNT_STRIDE)]; npad is a multiple of 256, so the arrays are contiguous under the
    // carver's 256-byte alignment
    w.fb_count = c.take<int>(64);
    w.qmax = c.take<unsigned>((size_t)npad);
    w.rec_cnt = c.take<unsigned>((size_t)npad);
    w.bin_cnt = c.take<unsigned>((size_t)((mpad / CHUNK_ROWS + 63) / 64 * 64) * BIN_CNT_STRIDE);
    w.hit_cnt = c.take<unsigned>((size_t)npad * BIN_CNT_STRIDE);
    w.qbest = c.take<unsigned long long>((size_t)npad);   // (the last array of the region search_zero_bytes covers)
    w.bin_cap = rescan_bin_cap(npad, mpad / CHUNK_ROWS);
    w.bins = c.take<int>((size_t)(mpad / CHUNK_ROWS) * (size_t)w.bin_cap);
    w.rcap = FILTER_LDS_ROWS;
    w.rec = c.take<uint2>((size_t)npad * (size_t)w.rcap);
    w.cand_up = c.take<float>((size_t)npad * (size_t)w.cap);
    w.bytes = c.used();
    return w;
}

inline size_t search_zero_bytes(int64_t n, int64_t m) {
    const int64_t npad = rows_padded(n), mpad = rows_padded(m);
    return 256 + 2 * (size_t)npad * sizeof(unsigned) + (size_t)((mpad / CHUNK_ROWS + 63) / 64 * 64) * BIN_CNT_STRIDE * sizeof(unsigned) +
           (size_t)npad * BIN_CNT_STRIDE * sizeof(unsigned) + (size_t)npad * sizeof(unsigned long long);
}

// Descriptor rows as the caller stores them (round 5, BASELINE.json configs[4] "fp16 descriptor storage"): fp32 -- the reference's layout
// behind VoxelHashMap.cpp:469-482 -- or fp16 (VFM_ROWS_F16: half the bytes of a resident map and of the preparation's read), every
// element widened to fp32 as it is loaded; from there on the arithmetic is the fp32 path's, operation for operation -- the oracle of an
// fp16 operand is the oracle of its widened rows.  A `const float*` converts implicitly (f16 = 0).
struct Rows {
    const void* p;
    int f16;
    __host__ __device__ Rows() : p(nullptr), f16(0) {}
    __host__ __device__ Rows(const float* x) : p(x), f16(0) {}
    __host__ __device__ Rows(const void* x, int is_f16) : p(x), f16(is_f16) {}
#if defined(__HIPCC__)
    typedef _Float16 rows_half4 __attribute__((ext_vector_type(4)));
    // four consecutive elements from element index e (a multiple of 4)
    __device__ __forceinline__ float4 ld4(int64_t e) const {
        if (f16) {
            const rows_half4 h = *reinterpret_cast<const rows_half4*>(static_cast<const _Float16*>(p) + e);
            return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
        }
        return *reinterpret_cast<const float4*>(static_cast<const float*>(p) + e);
    }
    // the same, streamed (read-once rows of the preparation: do not displace the coarse pass' map slice from the L2)
    __device__ __forceinline__ float4 ld4_nt(int64_t e) const {
        if (f16) {
            const unsigned* pc = reinterpret_cast<const unsigned*>(static_cast<const _Float16*>(p) + e);
            unsigned w[2] = {__builtin_nontemporal_load(pc), __builtin_nontemporal_load(pc + 1)};
            rows_half4 h;
            __builtin_memcpy(&h, w, 8);
            return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
        }
        const float* pc = static_cast<const float*>(p) + e;
        return make_float4(__builtin_nontemporal_load(pc), __builtin_nontemporal_load(pc + 1), __builtin_nontemporal_load(pc + 2),
                           __builtin_nontemporal_load(pc + 3));
    }
    __device__ __forceinline__ float ld1(int64_t e) const {
        return f16 ? (float)static_cast<const _Float16*>(p)[e] : static_cast<const float*>(p)[e];
    }
#endif
};


// ---------------------------------------------------------------------------------------------
// The instantiations of the coarse kernels, one list per kernel family, one entry each: X(family, template arguments).  These lists are
// ALL that names an instantiation: the enum CoarseInst, the table resolve_coarse looks its choice up in, the names of
// vfm_debug_last_coarse_kernel / _coarse_kernel_names / _coarse_plan (match_api.hip spells them from the arguments) and the switch of each
// match_coarse_*.hip that turns an enum value into its __global__ function are generated from them -- so a name without a kernel, or a
// kernel the plan cannot name, does not exist.
// ---------------------------------------------------------------------------------------------
// match_coarse_pipe_kernel<KSTEPS, SPARSE>
#define VFM_COARSE_PIPE_INSTS(X) X(PIPE, 8, false) X(PIPE, 8, true) X(PIPE, 16, false) X(PIPE, 16, true) X(PIPE, 24, false) X(PIPE, 24, true)
// match_coarse_kernel<KSTEPS, QSETS>
#define VFM_COARSE_V_INSTS(X) X(V, 8, 1) X(V, 8, 2) X(V, 16, 1) X(V, 16, 2) X(V, 24, 1) X(V, 24, 2) X(V, 32, 1)
// match_coarse_r_kernel<KSTEPS, QSETS, NBUF, BIAS>
#define VFM_COARSE_R_INSTS(X) X(R, 40, 1, 3, false) X(R, 40, 1, 3, true) X(R, 48, 1, 3, false) X(R, 48, 1, 3, true)
// match_coarse_i8_kernel<KSTEPS, T, TOP2, LOW>: the half-width pass (LOW = false), then full width
#define VFM_COARSE_I8_INSTS(X)                                                                                                         \
    X(I8, 4, 4, false, false) X(I8, 6, 4, false, false) X(I8, 8, 4, false, false) X(I8, 10, 4, false, false) X(I8, 12, 4, false, false) \
    X(I8, 8, 2, false, true) X(I8, 8, 4, false, true) X(I8, 8, 4, true, true) X(I8, 12, 2, false, true) X(I8, 12, 4, false, true)       \
    X(I8, 12, 4, true, true) X(I8, 16, 2, false, true) X(I8, 16, 2, true, true) X(I8, 20, 2, false, true) X(I8, 20, 2, true, true)      \
    X(I8, 24, 2, false, true) X(I8, 24, 2, true, true)
// match_coarse_i8q2_kernel<KSTEPS, TOP2, LOW, FUSE>
#define VFM_COARSE_I8Q2_INSTS(X)                                                                                                   \
    X(I8Q2, 4, false, false, true) X(I8Q2, 6, false, false, true) X(I8Q2, 4, false, false, false) X(I8Q2, 6, false, false, false)  \
    X(I8Q2, 8, false, false, false) X(I8Q2, 10, false, false, false) X(I8Q2, 12, false, false, false)                              \
    X(I8Q2, 8, false, true, false) X(I8Q2, 8, true, true, false) X(I8Q2, 12, false, true, false) X(I8Q2, 12, true, true, false)
// match_coarse_mx6q2_kernel<KS6, KIND, LOW, IMG_KS6, RING, T, NS>
#define VFM_COARSE_MX6_INSTS(X)                                                                                                      \
    X(MX6, 3, MX6_FUSE, false, 6, 5, 4, 3) X(MX6, 3, MX6_FUSE, false, 6, 4, 4, 3)                                                    \
    X(MX6, 6, MX6_FUSE, false, 6, 4, 4, 2) X(MX6, 4, MX6_FUSE, false, 4, 4, 4, 2)                                                    \
    X(MX6, 3, MX6_FUSE, false, 6, 3, 8, 2) X(MX6, 2, MX6_FUSE, false, 4, 3, 8, 2)                                                    \
    X(MX6, 6, MX6_FUSE, false, 12, 4, 4, 2) X(MX6, 4, MX6_FUSE, false, 8, 4, 4, 2) X(MX6, 3, MX6_FUSE, false, 6, 4, 4, 2)            \
    X(MX6, 2, MX6_FUSE, false, 4, 4, 4, 2)                                                                                           \
    X(MX6, 6, MX6_BEST, false, 12, 4, 4, 2) X(MX6, 4, MX6_BEST, false, 8, 4, 4, 2) X(MX6, 3, MX6_BEST, false, 6, 4, 4, 2)            \
    X(MX6, 2, MX6_BEST, false, 4, 4, 4, 2)                                                                                           \
    X(MX6, 6, MX6_TOP2, true, 6, 4, 4, 2) X(MX6, 6, MX6_BEST, true, 6, 4, 4, 2) X(MX6, 4, MX6_TOP2, true, 4, 4, 4, 2) X(MX6, 4, MX6_BEST, true, 4, 4, 4, 2)
#define VFM_COARSE_INSTS_F16(X) VFM_COARSE_PIPE_INSTS(X) VFM_COARSE_V_INSTS(X) VFM_COARSE_R_INSTS(X)
#define VFM_COARSE_INSTS_I8(X) VFM_COARSE_I8_INSTS(X) VFM_COARSE_I8Q2_INSTS(X)
#define VFM_COARSE_INSTS(X) VFM_COARSE_INSTS_F16(X) VFM_COARSE_INSTS_I8(X) VFM_COARSE_MX6_INSTS(X)
// the enum value of an instantiation, and its case label (a switch over CoarseInst has no default: every value is named in it)
#define VFM_CI_PIPE(k, s) CI_PIPE_##k##_##s
#define VFM_CI_V(k, q) CI_V_##k##_##q
#define VFM_CI_R(k, q, nb, b) CI_R_##k##_##q##_##nb##_##b
#define VFM_CI_I8(k, t, t2, lo) CI_I8_##k##_##t##_##t2##_##lo
#define VFM_CI_I8Q2(k, t2, lo, f) CI_I8Q2_##k##_##t2##_##lo##_##f
#define VFM_CI_MX6(k, kind, lo, img, ring, t, ns) CI_##kind##_##k##_##lo##_##img##_##ring##_##t##_##ns
#define VFM_CI(family, ...) VFM_CI_##family(__VA_ARGS__)
#define VFM_CI_CASE(family, ...) case VFM_CI(family, __VA_ARGS__):
#define VFM_CI_ENUM(family, ...) VFM_CI(family, __VA_ARGS__),
#define VFM_CI_ARGS(family, ...) {CF_##family, {__VA_ARGS__}},
enum CoarseFamily : unsigned char { CF_PIPE, CF_V, CF_R, CF_I8, CF_I8Q2, CF_MX6 };
enum CoarseInst : unsigned char { VFM_COARSE_INSTS(VFM_CI_ENUM) CI_COUNT };
struct CoarseInstArgs {
    unsigned char family;   // CoarseFamily
    short a[7];             // the template arguments, in order (the rest 0)
};
constexpr CoarseInstArgs k_coarse_insts[CI_COUNT] = {VFM_COARSE_INSTS(VFM_CI_ARGS)};
// the instantiation of `family` with these template arguments, or -1
inline int coarse_inst(int family, int a0, int a1 = 0, int a2 = 0, int a3 = 0, int a4 = 0, int a5 = 0, int a6 = 0) {
    const int want[7] = {a0, a1, a2, a3, a4, a5, a6};
    for (int i = 0; i < CI_COUNT; ++i) {
        bool same = k_coarse_insts[i].family == family;
        for (int j = 0; same && j < 7; ++j) same = k_coarse_insts[i].a[j] == want[j];
        if (same) return i;
    }
    return -1;
}
// Dynamic LDS of a shape, one function per kernel family: what the launch asks for (resolve_coarse) and what must fit a compute unit's
// 160 KiB (the static_assert below the functions; every kernel asserts the same of the ring it lays out)
constexpr int pipe_lds(int ksteps, bool sparse) { return 6 * ksteps * 1024 + (sparse ? SPARSE_LREC_CAP * 8 + 16 : 0); }
constexpr int v_lds(int ksteps) { return ring_depth(ksteps) * ksteps * 1024; }
constexpr int r_lds(int ksteps, int nbuf) { return nbuf * ksteps * 1024; }
constexpr int i8_lds(int ksteps, int t) { return 3 * t * ksteps * 1024; }
constexpr int i8q2_lds(int ksteps) { return 12 * ksteps * 1024; }
constexpr int mx6_lds(int ks6, int kind, int ring, int t) {
    const int ring_bytes = ring * t * (MX6_SCALE_PLANE + ks6 * MX6_KSTEP_BYTES) + MX6_LTAB * 8;   // the tiles' prefix the pass reads, and the table
    // FUSE: entries the workgroup's list holds (the slot in global memory is MX6_LCAP + 4 words for every shape; d = 768's ring leaves 4 KiB)
    const int lcap = ring_bytes + (MX6_LCAP + 1) * 4 <= 160 * 1024 ? MX6_LCAP : 1023;
    return ring_bytes + (kind == MX6_FUSE ? (lcap + 1) * 4 : 0);
}
constexpr int coarse_inst_lds(const CoarseInstArgs& k) {
    return k.family == CF_PIPE ? pipe_lds(k.a[0], k.a[1]) : k.family == CF_V ? v_lds(k.a[0]) : k.family == CF_R ? r_lds(k.a[0], k.a[2])
         : k.family == CF_I8 ? i8_lds(k.a[0], k.a[1]) : k.family == CF_I8Q2 ? i8q2_lds(k.a[0]) : mx6_lds(k.a[0], k.a[1], k.a[4], k.a[5]);
}
// threads per workgroup: 8 waves; match_coarse_kernel 512 / QSETS; match_coarse_r_kernel 4 waves
constexpr int coarse_inst_block(const CoarseInstArgs& k) { return k.family == CF_V ? 512 / k.a[1] : k.family == CF_R ? 256 : 512; }
constexpr bool coarse_lds_fits() {
    for (int i = 0; i < CI_COUNT; ++i)
        if (coarse_inst_lds(k_coarse_insts[i]) > 160 * 1024) return false;
    return true;
}
static_assert(coarse_lds_fits(), "an instantiation's ring exceeds the LDS");

// size and policy rules of the passes (match_api.hip)
bool use_sparse(int d, int64_t n, int64_t m);
bool use_i8(int d, int64_t n, int64_t m, bool gated);

// ---------------------------------------------------------------------------------------------
// What a search does, resolved ONCE from what the caller passed and the calling thread's vfm_cfg(): do_search_coarse, do_search_finish
// and the read-back vfm_debug_search_plan all branch on this and on nothing else, so the two stages cannot disagree.
// ---------------------------------------------------------------------------------------------
// the two chunk counts of a map of m rows: the 128-row chunks that hold at least one row, and the chunks of the map padded to ROW_PAD
// rows (what the kernels walk: one more when the first count is odd)
inline int64_t chunks_with_rows(int64_t m) { return (m + CHUNK_ROWS - 1) / CHUNK_ROWS; }
inline int64_t chunks_padded(int64_t m) { return rows_padded(m) / CHUNK_ROWS; }

enum SearchPass { PASS_F16_DENSE, PASS_F16_SPARSE, PASS_I8, PASS_MX6 };
enum SearchBounds { BOUNDS_NONE, BOUNDS_I8, BOUNDS_MX6, BOUNDS_MX6_HALF };   // i8_bounds / mx6_bounds / mx6_bounds_half
// the finish stage's launches (do_search_finish runs plan.steps in order; finish_step_name spells them)
enum FinishStep : unsigned char {
    FIN_FILTER_REFINE, FIN_PILOT_BIN, FIN_PILOT_RESCAN, FIN_BIN_SURVIVORS, FIN_SELECT_HALF, FIN_SELECT_TOP2, FIN_SELECT_BEST, FIN_SELECT,
    FIN_HALF_GUARD, FIN_GUARD_FALLBACK, FIN_RESCAN, FIN_GATEPASS, FIN_RESCAN_CHUNK, FIN_RESCAN_CHUNK_MX6H, FIN_RESCAN_CLOSE, FIN_REFINE,
    FIN_RESCORE, FIN_EXACT
};
inline const char* finish_step_name(FinishStep s) {
    static const char* const names[] = {"match_filter_refine_kernel", "match_pilot_bin_kernel", "match_rescan_chunk_kernel", "match_bin_survivors_kernel",
                                        "match_select_half_kernel", "match_select_top2_kernel", "match_select_best_kernel", "match_select_kernel",
                                        "half_guard_kernel", "match_guard_fallback_kernel", "match_rescan_kernel", "match_gatepass_kernel",
                                        "match_rescan_chunk_kernel", "match_rescan_chunk_mx6h_kernel", "match_rescan_close_kernel", "match_refine_kernel",
                                        "match_rescore_kernel", "match_exact_kernel"};
    return names[s];
}
struct SearchPlan {
    int pass = PASS_F16_DENSE;
    int kind = VFM_RECORDS_F16;   // the kind the search runs as, after every fallback (VFM_RECORDS_F16: an fp16 pass)
    bool half = false;            // the coarse pass multiplies the first d / 2 columns
    bool fused = false;           // ... and does the selection itself: the gate is needed at the coarse call already
    bool top2 = false;            // packed top-2 records
    bool pilot = false;           // VFM_RECORDS_MX6_PILOT: the coarse pass notes every query's best chunk
    bool gate_test = false;       // behind the selection the gate itself is the hit test (half-width and fused kinds): needs a finite gate
    bool use_bins = false;        // the chunk-major rescan walks the chunks' bins
    bool no_i8 = false;           // VFM_RECORDS_NO_I8: nothing may read the int8 image
    int bounds = BOUNDS_NONE;     // of the records: the coarse kernel's and the selection's (the int8 rescans use i8_bounds)
    FinishStep steps[12] = {};
    int nsteps = 0;
    bool quantised() const { return pass == PASS_I8 || pass == PASS_MX6; }
};

// records: as passed (a kind, VFM_RECORDS_NO_I8 beside it or not).  A combination no kernel serves is refused here, once.
inline int resolve_search(SearchPlan& p, int records, int d, int64_t n, int64_t m, bool gated, bool inner_product) {
    p = SearchPlan{};
    p.no_i8 = (records & VFM_RECORDS_NO_I8) != 0;
    int kind = records & ~VFM_RECORDS_NO_I8;
    if (kind < VFM_RECORDS_BEST || kind > VFM_RECORDS_MX6_FUSED) return vfm_fail(VFM_EINVAL, "search: unknown record kind %d", records);
    auto add = [&p](FinishStep s) { p.steps[p.nsteps++] = s; };
    if (inner_product && kind != VFM_RECORDS_F16 && use_i8(d, n, m, gated)) {
        if (!gated) kind = VFM_RECORDS_TOP2;  // no feedback loop behind an ungated call: the robust record kind
        // The fallbacks.  The fused kinds and the pilot need the chunk-major rescan behind them: several queries per map chunk.
        // The fp6 kernels and the fused int8 kernel hold 64 queries per wave: more than 2048 queries, d = 256 / 384 (the one-set
        // kernels have no fp6 form; half width in fp6: 512 / 768 too, and such operands carry no int8 half image).
        const bool many = n >= 4 * chunks_with_rows(m), q2 = n > 2048;
        if (kind == VFM_RECORDS_HALF_FUSED && !((d == 256 || d == 384) && q2 && many)) kind = VFM_RECORDS_HALF;
        if ((kind == VFM_RECORDS_MX6_PILOT || kind == VFM_RECORDS_MX6_FUSED) && !many) kind = VFM_RECORDS_MX6;
        if ((kind == VFM_RECORDS_MX6 || kind == VFM_RECORDS_MX6_PILOT || kind == VFM_RECORDS_MX6_FUSED) && !(mx6_width(d) && q2)) kind = VFM_RECORDS_BEST;
        if (kind == VFM_RECORDS_MX6_TOP2 && !(mx6_width(d) && q2)) kind = VFM_RECORDS_TOP2;
        if ((kind == VFM_RECORDS_MX6_HALF || kind == VFM_RECORDS_MX6_HALF_FUSED) && !(mx6_half_width(d) && q2)) kind = VFM_RECORDS_BEST;
        if (kind == VFM_RECORDS_MX6_HALF_FUSED && !many) kind = VFM_RECORDS_MX6_HALF;
        p.kind = kind;
        p.pass = kind >= VFM_RECORDS_MX6 ? PASS_MX6 : PASS_I8;
        p.half = kind == VFM_RECORDS_HALF || kind == VFM_RECORDS_HALF_FUSED || kind == VFM_RECORDS_MX6_HALF || kind == VFM_RECORDS_MX6_HALF_FUSED;
        p.fused = kind == VFM_RECORDS_HALF_FUSED || kind == VFM_RECORDS_MX6_HALF_FUSED || kind == VFM_RECORDS_MX6_FUSED;
        p.top2 = kind == VFM_RECORDS_TOP2 || kind == VFM_RECORDS_MX6_TOP2;
        p.pilot = kind == VFM_RECORDS_MX6_PILOT;
        p.gate_test = p.half || p.fused;
        p.bounds = p.pass == PASS_I8 ? BOUNDS_I8 : (p.half ? BOUNDS_MX6_HALF : BOUNDS_MX6);
    } else if (inner_product && use_sparse(d, n, m)) {
        p.pass = PASS_F16_SPARSE;
    }
    // any other kind -- asked for, or what this shape makes of the one asked for -- reads the int8 image that was not written
    if (p.no_i8 && !(gated && p.kind == VFM_RECORDS_MX6_HALF_FUSED && mx6_width(d)))
        return vfm_fail(VFM_EINVAL, "search: VFM_RECORDS_NO_I8 needs a search that runs as VFM_RECORDS_MX6_HALF_FUSED at d = 256 / 384 (records %d, n %lld, m %lld, d %d)",
                        records, (long long)n, (long long)m, d);
    if (!inner_product) return VFM_OK;   // (the Euclidean search finishes in match_l2.hip)
    if (p.pass == PASS_F16_SPARSE) {
        add(FIN_FILTER_REFINE);
    } else if (!p.quantised()) {
        add(FIN_SELECT);
        add(FIN_REFINE);
    } else {
        const int variant = vfm_cfg().select_variant;
        const bool best = !p.top2 && !p.gate_test && variant != 1;
        // Best-score records with many queries per map chunk: the rescan runs chunk-major.  A fused kind has no choice: its coarse kernel
        // -- or match_bin_survivors_kernel -- has filed the survivors in the bins already, and a search that does not rescan the bins
        // reports every one of those queries as below the gate ("coarse_variant" 21; and n between four times the two chunk counts).
        p.use_bins = p.fused || ((best || p.gate_test) && variant != 2 && n >= 4 * chunks_padded(m));
        if (p.pilot && p.use_bins) {
            add(FIN_PILOT_BIN);
            add(FIN_PILOT_RESCAN);
        }
        if (p.fused) {   // nothing to select; the fp6 coarse kernel has left the survivors in its workgroups' slots
            if (p.pass == PASS_MX6) add(FIN_BIN_SURVIVORS);
        } else {
            add(p.gate_test ? FIN_SELECT_HALF : (p.top2 && variant != 1) ? FIN_SELECT_TOP2 : best ? FIN_SELECT_BEST : FIN_SELECT);
        }
        if (p.gate_test) add(FIN_HALF_GUARD);
        if (p.no_i8) {   // survivors rescanned on the fp6 half image; guard up: every live query to the all-pairs kernel
            add(FIN_GUARD_FALLBACK);
            add(FIN_RESCAN_CHUNK_MX6H);
            add(FIN_RESCAN_CLOSE);
        } else {         // candidate chunks -> candidate rows on the int8 image; guard up: one full-width gate pass
            add(FIN_RESCAN);
            if (p.gate_test) add(FIN_GATEPASS);
            if (p.use_bins) add(FIN_RESCAN_CHUNK);
            add(FIN_RESCAN_CLOSE);
            add(FIN_REFINE);
        }
    }
    add(FIN_RESCORE);
    add(FIN_EXACT);
    return VFM_OK;
}
// a finite gate where the plan tests against it: at the coarse call for the fused kinds, at the finish call for every gate-tested kind
inline int check_plan_gate(bool needed, float gate, const char* who) {
    if (needed && !(gate > -__builtin_inff())) return vfm_fail(VFM_EINVAL, "%s: the half-width and fused record kinds need a finite gate", who);
    return VFM_OK;
}

// ---------------------------------------------------------------------------------------------
// Which coarse kernel a plan's coarse pass launches and on what grid, resolved ONCE: do_search_coarse and l2i8_search hand the result to
// launch_coarse, the read-back vfm_debug_coarse_plan prints it.  Host arithmetic on the shape, the calling thread's vfm_cfg() and the
// compute-unit count the caller passes; no HIP call in here.
// ---------------------------------------------------------------------------------------------
struct CoarseLaunch {
    int inst = 0;          // CoarseInst
    bool seeded = false;   // the sparse pipelined kernel with seed units at the head of its grid: a launch argument, not a template one -- but a
                           // different grid and a different first round, so it goes by a second name ("pipe<24,sparse>+seed")
    int nqb = 0, nslices = 0, seed_parts = 0, seed_chunks = 0, nseed_pad = 0, tune = 0;   // CoarseArgs' fields of the same names
    int block = 0, lds = 0;   // threads per workgroup, bytes of dynamic LDS
    int grid() const { return nseed_pad + nqb * nslices; }
};

inline int choose_slices(int nqb, int nchunks) {
    if (vfm_cfg().force_slices > 0) return vfm_cfg().force_slices < nchunks ? vfm_cfg().force_slices : nchunks;
    // Fill 256 CUs with whole "rounds" of workgroups (tail efficiency).  Every (query block, slice) unit re-reads its 256
    // queries (196 KB), so HBM / Infinity-Cache traffic grows with the slice count (C2: 55 slices 1.45 GB per launch).
    // Round 2 sweep at C2 with the seeded sparse kernel (registrations/s in the pipeline): 14-16 slices 349, 21: 367,
    // 29: 366, 35: 367, 42: 365, 48: 364, 55: 364 -- flat from ~8 rounds on.  So: among the counts within 1 % of the best
    // tail efficiency take the SMALLEST that still gives >= 8 rounds (29 at C2); without such a count, the most efficient.
    int best_s = 1;
    double best_eff = -1.0;
    const int smax = nchunks < 64 ? nchunks : 64;
    auto eff_of = [&](int s, long long* rounds_out) {
        const long long total = (long long)nqb * s;
        const long long rounds = (total + 255) / 256;
        if (rounds_out) *rounds_out = rounds;
        return (double)total / (double)(rounds * 256);
    };
    for (int s = 1; s <= smax; ++s) {
        if (nchunks / s < 8 && s > 1) break;  // keep >= 32 tiles per workgroup
        const double eff = eff_of(s, nullptr);
        if (eff > best_eff + 1e-9) {
            best_eff = eff;
            best_s = s;
        }
    }
    for (int s = 1; s < best_s; ++s) {
        long long rounds;
        const double eff = eff_of(s, &rounds);
        if (rounds >= 8 && eff >= best_eff - 0.01) return s;
    }
    return best_s;
}

// row_bias: the launch adds CoarseArgs::row_bias (Euclidean search, d > 510); compute_units: of the device the launch goes to
inline int resolve_coarse(CoarseLaunch& l, const SearchPlan& p, int d, int64_t n, int64_t m, bool row_bias, int compute_units) {
    l = CoarseLaunch{};
    const VfmConfig& cfg = vfm_cfg();
    const int npad = (int)rows_padded(n), nchunks = (int)chunks_padded(m), nq_tiles = (int)((n + TILE_ROWS - 1) / TILE_ROWS);
    const bool top2 = p.top2;
    int inst;
    if (row_bias && d != 640 && d != 768) return vfm_fail(VFM_EINVAL, "row bias needs the 4-wave coarse kernel (K = 640 / 768), got %d", d);
    if (!p.quantised()) {   // the fp16 pass, d in {128, ..., 768}
        const int ks = d / 16;
        const bool sparse = p.pass == PASS_F16_SPARSE;
        l.nqb = npad / (d > 512 ? 128 : QBLOCK);   // queries per workgroup: 8 waves x 32 or 4 x 64; the 4-wave kernel of d > 512 4 x 32
        l.nslices = choose_slices(l.nqb, nchunks);
        if (d > 512) inst = coarse_inst(CF_R, ks, 1, 3, row_bias);
        else if (d > 384) inst = coarse_inst(CF_V, ks, 1);   // d = 512: 2 x 128 query VGPRs would not fit; 8-wave kernel, ring of 4: 3.45 ms at C2 x 512 (4-wave kernel: 4.42 ms)
        else if (cfg.coarse_qsets == 1 || cfg.coarse_qsets == 2) inst = coarse_inst(CF_V, ks, cfg.coarse_qsets);
        else inst = coarse_inst(CF_PIPE, ks, sparse);   // 0, 3
        if (inst < 0) return vfm_fail(VFM_EINVAL, "FAST matching supports d in {128,256,384,512,640,768}, got %d", d);
        if (sparse && cfg.seed_units && nchunks >= 256 && l.nqb <= 256) {  // seed units: one short round at the head of the grid
            l.seed_parts = 256 / l.nqb < 4 ? 256 / l.nqb : 4;
            l.seed_chunks = 5;
            l.nseed_pad = (l.nqb * l.seed_parts + 7) / 8 * 8;
            l.nslices = choose_slices(l.nqb, nchunks - l.seed_parts * l.seed_chunks);
        }
    } else if (p.pass == PASS_I8) {   // KSTEPS = d / 32 (the half-width kinds: the image of the first d / 2 columns, d / 64)
        // 64 resident queries per wave: 11-15 % faster than the one-set kernel from ~3000 queries on (C2: 1.09 vs 1.23 ms;
        // 1500 x 100 000: 0.059 vs 0.056 ms -- half as many, twice as large workgroups); variants 10 / 12 = one set, A/B.
        // The half-width pass has them at every width (d / 2 columns are at most 384), the fused one (d = 256 / 384, more than 2048
        // queries: resolve_search) nothing else
        const bool q2 = p.fused || ((p.half || d <= 384) && n > 2048 && cfg.coarse_qsets == 0);
        const bool t2 = cfg.coarse_qsets == 10;  // variant 10 (A/B): 2 tiles per step at every width
        l.nqb = q2 ? (nq_tiles + 15) / 16 : npad / QBLOCK;  // 8 waves x 64 / x 32 queries at every width
        l.nslices = choose_slices(l.nqb, nchunks);
        if (q2) inst = coarse_inst(CF_I8Q2, p.half ? d / 64 : d / 32, top2, !p.half, p.fused);
        else if (p.half) inst = coarse_inst(CF_I8, d / 64, 4, false, false);   // one query set per wave: few queries (variants 10 / 12: every size, A/B)
        else inst = coarse_inst(CF_I8, d / 32, d <= 384 && (top2 || !t2) ? 4 : 2, top2, true);
    } else {   // the fp6 pass: d = 256 / 384 (full width) or 256 / 384 / 512 / 768 (half width) and more than 2048 queries (resolve_search)
        const bool half = p.half, fuse = p.fused;   // (fuse && !half: VFM_RECORDS_MX6_FUSED, the full-width pass with the gate test in its epilogue)
        const bool ns3 = half && fuse && d == 384 && cfg.mx6_ns3 && cfg.mx6_t4;   // three query tiles per wave: 768 queries per workgroup
        l.nqb = ns3 ? (nq_tiles + 23) / 24 : (nq_tiles + 15) / 16;
        l.nslices = choose_slices(l.nqb, nchunks);
        if (half && cfg.force_slices == 0) {
            // the half-width kernel's workgroups are short, and shorter ones let the other stages of a pipeline in: ~7.5 rounds of 256
            // workgroups instead of choose_slices' 5 (tools/sweep_slices.py, C2, 200 steps: 48 slices 1548 against 32 slices 1475
            // registrations/s; the full-width fp6 kernel and the int8 kernels are flat from 32 on)
            int s = (int)((1600 + l.nqb - 1) / l.nqb);   // (round 4, tools/sweep_slices_r4.py, fused kernel: 40 / 44 slices 1764 / 1762, 48: 1740, 57: 1690 registrations/s over 200 steps)
            const int smax = nchunks / 8 < 64 ? nchunks / 8 : 64;
            s = s > smax ? smax : s;
            s = s < 1 ? 1 : s;
            // Round 6: the workgroups are equal and a compute unit holds one, so the kernel lasts ceil(workgroups / units) rounds whatever the last
            // round holds (tools/sweep_slices_r6.py, the kernel alone at C2, 27 query blocks: 60 slices = 6.33 rounds 0.388 ms; 56 = 5.9 rounds
            // 0.370; 47 = 4.96 rounds 0.367; 19 slices = 2.004 rounds 0.445).  Near the count above, take the slice count whose last round is
            // (almost) full -- at most 4 above, 12 below; in the pipeline 56 against 60 is +1 % over 200 steps, even in the 20-step form.
            {
                const int cus = compute_units;
                int best = s;
                double best_fill = 0.0;
                for (int t = (s + 4 < smax ? s + 4 : smax); t >= 1 && t >= s - 12; --t) {
                    const long long wg = (long long)l.nqb * t, rounds = (wg + cus - 1) / cus;
                    const double fill = (double)wg / (double)(rounds * cus);
                    if (fill >= 0.975) {   // the largest such count (short workgroups let the pipeline's other stages in)
                        best = t;
                        best_fill = 2.0;
                        break;
                    }
                    if (fill > best_fill) {
                        best_fill = fill;
                        best = t;
                    }
                }
                s = best;
            }
            l.nslices = s < 1 ? 1 : s;
        }
        while ((nchunks + l.nslices - 1) / l.nslices + 1 > MX6_LTAB && l.nslices < nchunks) ++l.nslices;   // a slice's constants fit the LDS table
        if (fuse && (l.nqb > surv_slot_qblocks(npad) || l.nslices > surv_slot_slices(nchunks)))   // (what carve_search sized the slots for)
            return vfm_fail(VFM_EINVAL, "search_coarse: %d x %d survivor slots exceed the workspace (n %d chunks %d)", l.nqb, l.nslices, npad, nchunks);
        // Two chunks per barrier (T = 8, ring of 3 x 8 tiles: 84 / 120 KiB at d = 256 / 384) is built, parity-tested and measured: 0.415 ms
        // against 0.419 alone, 1715 against 1725 registrations/s in the pipeline (tools/ab_r4.py) -- the barrier share the ablations
        // show (tools/ablate6.py: -10 % without barrier and staging) does not come back by halving the barriers, and the larger ring
        // leaves the side kernels less LDS.  One chunk per barrier stays the default; vfm_debug_set_coarse_variant(31) selects T = 8.
        const bool t8 = half && fuse && (d == 384 || d == 256) && !cfg.mx6_t4 && l.nslices <= nchunks / 2;
        l.tune = cfg.mx6_tune;
        const int ring = ns3 ? ((cfg.mx6_tune & 2) ? 5 : 4) : t8 ? 3 : 4;   // (A/B, three-tile shape) a ring of five steps
        inst = coarse_inst(CF_MX6, half ? d / 128 : d / 64, fuse ? MX6_FUSE : top2 ? MX6_TOP2 : MX6_BEST, !half && !fuse, d / 64, ring, t8 ? 8 : 4, ns3 ? 3 : 2);
    }
    if (inst < 0) return vfm_fail(VFM_EINVAL, "search_coarse: no coarse kernel for d = %d, record kind %d", d, p.kind);
    l.inst = inst;
    l.seeded = l.nseed_pad != 0;
    l.block = coarse_inst_block(k_coarse_insts[inst]);
    l.lds = coarse_inst_lds(k_coarse_insts[inst]);
    return VFM_OK;
}
inline I8Bounds i8_bounds(const Prepared& Q, const Prepared& B, bool on, int top2 = 0) {
    return on ? I8Bounds{Q.err, Q.gstep, B.gstep, B.gerr, top2 == VFM_RECORDS_TOP2 ? 1 : 0} : I8Bounds{nullptr, nullptr, nullptr, nullptr, 0};
}
// bounds of the fp6 records (selection only: the rescans score the int8 image and use i8_bounds)
inline I8Bounds mx6_bounds(const Prepared& Q, const Prepared& B, int top2 = 0) { return I8Bounds{Q.err6, Q.gstep6, B.gstep6, B.gerr6, top2}; }
// ... of the half-width fp6 kinds: the residual norms over the columns the pass multiplies (tighter, and all a VFM_PREPARE_MX6_HALF
// operand carries: its full-width E is infinite)
inline I8Bounds mx6_bounds_half(const Prepared& Q, const Prepared& B) { return I8Bounds{Q.err6h, Q.gstep6, B.gstep6, B.gerr6h, 0}; }
// ... of the records a plan's coarse pass writes (SearchPlan::bounds)
inline I8Bounds plan_bounds(const SearchPlan& p, const Prepared& Q, const Prepared& B) {
    if (p.bounds == BOUNDS_MX6_HALF) return mx6_bounds_half(Q, B);
    if (p.bounds == BOUNDS_MX6) return mx6_bounds(Q, B, p.top2 ? 1 : 0);
    return i8_bounds(Q, B, p.bounds == BOUNDS_I8, p.top2 ? 1 : 0);
}
// everything of the argument block but the launch geometry (nqb, nslices, the seed units, tune: launch_coarse sets them from a CoarseLaunch;
// the finish stage reads none of them)
CoarseArgs coarse_args(const Prepared& Q, const Prepared& B, const SearchWs& w, int64_t n, int64_t m);

// match_prep.hip
// What do_search_coarse clears in front of a coarse pass, as two ranges of whole 16-byte units: a preparation that runs just before on
// another stream can clear them on its way (vfm_match_prepare2_gated_z) and the coarse call be told so (VFM_RECORDS_WS_CLEAN).
struct PrepZero {
    uint4* a = nullptr;   // [fb_count, fb_count + search_zero_bytes)
    size_t na = 0;
    uint4* b = nullptr;   // cand_cnt[0 .. npad)
    size_t nb = 0;
};
inline PrepZero prep_zero(void* ws, int64_t n, int64_t m) {
    const SearchWs w = carve_search(ws, n, m);
    PrepZero z;
    z.a = reinterpret_cast<uint4*>(w.fb_count);
    z.na = search_zero_bytes(n, m) / 16;               // (256 + multiples of npad = 256 k bytes)
    z.b = reinterpret_cast<uint4*>(w.cand_cnt);
    z.nb = (size_t)rows_padded(n) * sizeof(int) / 16;
    return z;
}
// ---------------------------------------------------------------------------------------------
// What a preparation does, resolved ONCE from what the caller passed and the calling thread's vfm_cfg(): the launcher (match_prep.hip,
// do_prepare2 / do_prepare_perm) walks plan.launches and the read-back vfm_debug_prepare_plan prints them.  No HIP call in here: a
// grid is a RULE, turned into a number at launch.
//
// Which kernels.  d = 128 has no int8 image: prep_rows_kernel (fp16 tiles).  Elsewhere prep_chunk_kernel holds a 128-row group in the
// registers of 16 fat waves, one workgroup per compute unit: <true, 2> writes both images from one read (d <= 384; 144 KB of LDS),
// <false, 2 | 3> the int8 image alone, the fp16 image then by prep_rows_kernel.  With the fp6 image (VFM_PREPARE_MX6) at d = 256 / 384
// the form is vfm_cfg().prep_form ("coarse_variant" 40, 41, 43, 44; tools/ab_prep_r5.py, ab_prep_r6.py, DESIGN.md R6.2 and the section
// on the persistent form): 3 (default since round 6) prep_once_kernel -- one read of fp32 rows, the fp16 copy of a wave's tile in
// registers, two short workgroups per compute unit; 4 the same kernel as a persistent grid with the next group's loads under a group's
// second pass; 1 prep_stream_kernel, built to run BESIDE a coarse workgroup of round 4 (332 of a SIMD's 512 registers, 90 KiB), every
// row read twice; anything else, and fp16 rows under every form, prep_chunk_kernel<false, 2, true, 8>.  d = 512 / 768 get the fp6 image
// by kernels of their own behind the int8 one; d = 128 / 640 have none and ignore the flag.
// ---------------------------------------------------------------------------------------------
enum PrepInst : unsigned char {   // one per kernel instantiation in match_prep.hip; prep_inst_name and launch_prepare's switch follow this order
    PREP_ROWS, PREP_CHUNK_BOTH, PREP_CHUNK_2, PREP_CHUNK_3, PREP_CHUNK_MX6,
    PREP_STREAM,                        // + 2 (d == 384) + half
    PREP_ONCE = PREP_STREAM + 4,        // + 4 (d == 384) + 2 half + persist
    PREP_ONCE_NOI8 = PREP_ONCE + 8,     // + 2 (d == 384) + persist
    PREP_MX6_ROWS_16 = PREP_ONCE_NOI8 + 4, PREP_MX6_ROWS_32, PREP_MX6_GROUP, PREP_INST_COUNT
};
inline const char* prep_inst_name(int inst) {
    static const char* const names[PREP_INST_COUNT] = {
        "prep_rows_kernel", "prep_chunk_kernel<true,2>", "prep_chunk_kernel<false,2>", "prep_chunk_kernel<false,3>", "prep_chunk_kernel<false,2,true,8>",
        "prep_stream_kernel<256,full>", "prep_stream_kernel<256,half>", "prep_stream_kernel<384,full>", "prep_stream_kernel<384,half>",
        "prep_once_kernel<256,full,short>", "prep_once_kernel<256,full,persist>", "prep_once_kernel<256,half,short>", "prep_once_kernel<256,half,persist>",
        "prep_once_kernel<384,full,short>", "prep_once_kernel<384,full,persist>", "prep_once_kernel<384,half,short>", "prep_once_kernel<384,half,persist>",
        "prep_once_kernel<256,half,short,noi8>", "prep_once_kernel<256,half,persist,noi8>", "prep_once_kernel<384,half,short,noi8>",
        "prep_once_kernel<384,half,persist,noi8>", "prep_mx6_rows_kernel<16>", "prep_mx6_rows_kernel<32>", "prep_mx6_group_kernel"};
    return names[inst];
}
// workgroups of a launch: one per n padded rows of both operands (128: per group, 32: per tile); or, never more than the groups, one
// per compute unit, two per compute unit of the stream's mask, or n
enum PrepGridRule : unsigned char { PREP_GRID_ROWS, PREP_GRID_CU, PREP_GRID_2CU_STREAM, PREP_GRID_N };
enum PrepZeroAt : unsigned char { PREP_ZERO_NONE, PREP_ZERO_INSIDE, PREP_ZERO_BEHIND };   // INSIDE: the one-read kernel clears the ranges; BEHIND: prep_zero_kernel
struct PrepLaunch {
    int inst;       // PrepInst
    bool half6;     // PrepOut::mx6_half of the launch (the fp6 kernels under VFM_PREPARE_MX6_HALF)
    int block, lds;
    int rule, n;    // PrepGridRule and its n
};
struct PrepPlan {
    bool f16 = false, i8 = false, fp6 = false, fp6_half = false;   // the images written (fp6_half: of the first d / 2 columns only)
    PrepLaunch launches[4] = {};
    int nlaunches = 0;
    int zero = PREP_ZERO_NONE;
};

// entry: a VFM_PREP_ENTRY_* (include/vfmreg_debug.h); schedule, row types: as passed; rows2 = 0: no second operand; zero: search
// workspace ranges ride along.  Every refusal of a preparation is made here, once.
inline int resolve_prepare(PrepPlan& p, int entry, int schedule, int d, int64_t rows1, int dtype1, int64_t rows2, int dtype2, bool zero) {
    p = PrepPlan{};
    const bool single = entry == VFM_PREP_ENTRY_PREPARE || entry == VFM_PREP_ENTRY_PERM;
    const bool gated = entry >= VFM_PREP_ENTRY_GATED && entry <= VFM_PREP_ENTRY_GATED_T;
    const bool scheduled = entry >= VFM_PREP_ENTRY_GATED_P && entry <= VFM_PREP_ENTRY_GATED_T;
    if (entry < VFM_PREP_ENTRY_PREPARE || entry > VFM_PREP_ENTRY_ONESHOT) return vfm_fail(VFM_EINVAL, "prepare: unknown entry %d", entry);
    if (!(rows1 > 0 && (single ? rows2 == 0 : rows2 > 0) && d % 128 == 0 && d >= 128 && d <= 768))
        return vfm_fail(VFM_EINVAL, "%s: d must be in {128,256,384,512,640,768}", entry == VFM_PREP_ENTRY_PREPARE ? "prepare" : "prepare2");
    if (entry == VFM_PREP_ENTRY_PERM && !i8_capable(d)) return vfm_fail(VFM_EINVAL, "prepare(perm): no int8 image for d = %d", d);
    VFM_CHECK_ARG((dtype1 == VFM_ROWS_F32 || dtype1 == VFM_ROWS_F16) && (dtype2 == VFM_ROWS_F32 || dtype2 == VFM_ROWS_F16) &&
                      (entry == VFM_PREP_ENTRY_GATED_T || (dtype1 == VFM_ROWS_F32 && dtype2 == VFM_ROWS_F32)), "prepare2: unknown row type");
    const int flags = VFM_PREPARE_MX6 | VFM_PREPARE_MX6_HALF | VFM_PREPARE_NO_I8;
    const int mode = schedule & ~flags;   // the low bits: the chunk kernel's grid and nothing else
    VFM_CHECK_ARG(scheduled ? mode >= VFM_PREPARE_DEFAULT && mode <= VFM_PREPARE_INTERLEAVED : schedule == 0, "prepare2: unknown schedule %d", schedule);
    const bool no_i8 = (schedule & VFM_PREPARE_NO_I8) != 0;
    const bool half6 = (schedule & VFM_PREPARE_MX6_HALF) != 0;               // (implies VFM_PREPARE_MX6)
    const bool mx6 = half6 || (schedule & VFM_PREPARE_MX6) != 0;
    const bool any_f16 = dtype1 == VFM_ROWS_F16 || (rows2 > 0 && dtype2 == VFM_ROWS_F16);
    const int form = vfm_cfg().prep_form;
    const bool once = mx6 && mx6_width(d) && !any_f16 && (form == 3 || form == 4);
    if (no_i8) {   // prep_once_kernel<., true, ., true> or nothing: no other form leaves the int8 image out
        VFM_CHECK_ARG(entry != VFM_PREP_ENTRY_GATED_T, "prepare2: VFM_PREPARE_NO_I8 is for fp32 rows (vfm_match_prepare2_gated_p / _z)");
        VFM_CHECK_ARG((schedule & VFM_PREPARE_MX6) && half6, "prepare2: VFM_PREPARE_NO_I8 needs VFM_PREPARE_MX6 | VFM_PREPARE_MX6_HALF (schedule %d)", schedule);
        VFM_CHECK_ARG(mx6_width(d), "prepare2: VFM_PREPARE_NO_I8 exists for d = 256 / 384, got %d", d);
    }
    // (map, scan): where the search of x2 in x1 runs a quantised pass, the fp16 image is never read.  fp16 rows are widened on load by
    // prep_chunk_kernel and prep_mx6_rows_kernel only: the int8 and fp6 images of the gated family
    const bool want_f16 = entry == VFM_PREP_ENTRY_PERM ? false : (gated || entry == VFM_PREP_ENTRY_ONESHOT) ? !use_i8(d, rows2, rows1, gated) : true;
    if (any_f16 && (want_f16 || !i8_capable(d)))
        return vfm_fail(VFM_EINVAL, "prepare: fp16 rows are taken by the gated int8 / fp6 searches (d in {256 .. 768}, more queries than the fp16 pass' limit)");
    if (no_i8 && !(once && rows2 > 0))
        return vfm_fail(VFM_EINVAL, "prepare: VFM_PREPARE_NO_I8 needs VFM_PREPARE_MX6_HALF, d = 256 / 384, fp32 rows of both operands and the "
                                    "one-read preparation (prep_form 3 / 4)");
    auto add = [&p](int inst, bool h6, int block, int lds, int rule, int n) { p.launches[p.nlaunches++] = PrepLaunch{inst, h6, block, lds, rule, n}; };
    auto add_rows = [&] { add(PREP_ROWS, false, 256, d * 64, PREP_GRID_ROWS, TILE_ROWS); };
    p.zero = !zero ? PREP_ZERO_NONE : once ? PREP_ZERO_INSIDE : PREP_ZERO_BEHIND;
    p.f16 = want_f16 || !i8_capable(d);
    if (!i8_capable(d)) {
        add_rows();
        return VFM_OK;
    }
    p.i8 = !no_i8;
    p.fp6 = mx6 && mx6_half_width(d);
    p.fp6_half = p.fp6 && half6;
    // prep_chunk_kernel's grid: DEFAULT the "prep_grid" key, PERSISTENT one per compute unit, INTERLEAVED one per group
    const int knob = mode == VFM_PREPARE_DEFAULT ? vfm_cfg().prep_grid : (mode == VFM_PREPARE_PERSISTENT ? 0 : -1);
    const int crule = knob > 0 ? PREP_GRID_N : (knob < 0 ? PREP_GRID_ROWS : PREP_GRID_CU), cn = knob > 0 ? knob : I8_GROUP;
    const int d384 = d == 384;
    if (once) {   // the persistent form: "prep_grid" n > 0, or two workgroups per compute unit of the stream's mask
        const int persist = form == 4, n = vfm_cfg().prep_grid;
        add(no_i8 ? PREP_ONCE_NOI8 + 2 * d384 + persist : PREP_ONCE + 4 * d384 + 2 * half6 + persist, half6, 256, 0,
            !persist ? PREP_GRID_ROWS : (n > 0 ? PREP_GRID_N : PREP_GRID_2CU_STREAM), persist && n > 0 ? n : I8_GROUP);
    } else if (mx6 && mx6_width(d) && form == 1 && !any_f16) {
        add(PREP_STREAM + 2 * d384 + half6, half6, 256, 0, PREP_GRID_ROWS, I8_GROUP);
    } else if (mx6 && mx6_width(d)) {
        add(PREP_CHUNK_MX6, half6, 512, I8_GROUP * (d * 3 + d / 8 + 16), crule, cn);
    } else if (want_f16 && d <= 384) {
        add(PREP_CHUNK_BOTH, false, 1024, I8_GROUP * d * 3, crule, cn);
        return VFM_OK;
    } else {
        add(d <= 512 ? PREP_CHUNK_2 : PREP_CHUNK_3, false, 1024, I8_GROUP * d, crule, cn);
    }
    if (want_f16) add_rows();
    if (p.fp6 && !mx6_width(d)) {   // d = 512, 768: 16 / 8 rows per workgroup, then the groups' maxima (four groups per workgroup)
        add(d == 512 ? PREP_MX6_ROWS_16 : PREP_MX6_ROWS_32, half6, 256, (d == 512 ? 16 : 8) * d * 4, PREP_GRID_ROWS, d == 512 ? 16 : 8);
        add(PREP_MX6_GROUP, half6, 256, 0, PREP_GRID_ROWS, 4 * I8_GROUP);
    }
    return VFM_OK;
}

// one or two operands (rows2 = 0: one) as `entry` with `schedule` prepares them; zero: ranges of a search workspace to clear on `st`
// with the preparation (none by default)
int do_prepare2(int entry, int schedule, Rows x1, int64_t rows1, void* prepared1, Rows x2, int64_t rows2, void* prepared2, int d,
                hipStream_t st, PrepZero zero = PrepZero{});
// int8 image alone of ONE operand whose row r is x[perm[r]] (perm == NULL: identity) -- the Euclidean search prepares its map
// sorted by norm and the queries of its reverse direction gathered by the forward result
int do_prepare_perm(const float* x, int64_t rows, const int* perm, int d, void* prepared, hipStream_t st);
// match_api.hip: the coarse kernel `l` names on the grid it gives, for arguments prepared by do_search_coarse (sets a's launch geometry)
int launch_coarse(const CoarseLaunch& l, CoarseArgs& a, hipStream_t st);
// ... and the one frame every launch goes through: dynamic LDS allowed once per device, the profiling events around the launch
typedef void (*CoarseKernel)(CoarseArgs);
int launch_coarse_kernel(CoarseKernel kernel, const char* what, const CoarseLaunch& l, const CoarseArgs& a, hipStream_t st);
// match_coarse_f16.hip / _i8.hip / _mx6.hip: the instantiations of each file's families
int launch_coarse_f16(const CoarseLaunch& l, const CoarseArgs& a, hipStream_t st);
int launch_coarse_int8(const CoarseLaunch& l, const CoarseArgs& a, hipStream_t st);
int launch_coarse_mx6(const CoarseLaunch& l, const CoarseArgs& a, hipStream_t st);
// match_api.hip
int do_search_coarse(const void* qprep, int64_t n, const void* bprep, int64_t m, int d, void* ws, hipStream_t st,
                     bool bias_from_map_inv = false, bool inner_product = false, bool gated = false, int records = 0,
                     float gate = -__builtin_inff(), bool ws_clean = false);
// match_finish.hip
int do_search_finish(Rows q, const void* qprep, int64_t n, Rows b, const void* bprep, int64_t m, int d,
                     int64_t* idx_out, float* sim_out, void* ws, hipStream_t st, bool gated = false,
                     float gate = -__builtin_inff(), int records = 0);
int launch_select_dense(const SearchWs& w, const CoarseArgs& a, const float* qinv, int64_t n, hipStream_t st);
// candidate chunks (bins / lists of a selection kernel) -> candidate rows: query-major + chunk-major int8 rescans and the
// closing pass (over-long lists to the all-pairs fallback); l2.qn != NULL: the Euclidean hit test, qmax = float_key(qlow)
int launch_i8_rescans(const SearchWs& w, const CoarseArgs& a, const Prepared& Q, const Prepared& B, int64_t n, int64_t m, int d,
                      bool use_bins, L2Terms l2, hipStream_t st);
int probe_half_select(const SearchPlan& plan, const void* qprep, int64_t n, const void* bprep, int64_t m, int d, void* ws, float gate, hipStream_t st);
int exact_ip_top1(const float* q, int64_t n, const float* b, int64_t m, int d, int64_t* idx_out, float* sim_out, void* ws,
                  hipStream_t st);
// inv_out[r] = 1 / |row r of x| in fp32, the sum of squares in the oracle's order (orc_sumsq_f32), any d >= 1; zero rows get 1
int launch_inv_norm(const float* x, int64_t rows, int d, float* inv_out, hipStream_t st);
// match_l2_narrow.hip (VFM_MATCH_NARROW, d <= VFM_L2_NARROW_MAX_D): one direction of the f32-MFMA Euclidean search -- query i = row
// (qperm ? qperm[i] : i) of q, among the m rows of b -- in a workspace of l2n_dir_bytes(nq, m, d); max_bits as l2_maxnorm_kernel left it
// for BOTH sets; *evals (device) is incremented by the number of exact evaluations
int l2n_slices(int64_t nq, int64_t m);
size_t l2n_dir_bytes(int64_t nq, int64_t m, int d);
int l2n_search(const float* q, const int* qperm, int64_t nq, const float* b, int64_t m, int d, const unsigned* max_bits, int64_t* nn,
               double* d2, void* ws_dir, unsigned long long* evals, hipStream_t st);

}  // namespace vfmm

// match_topk.hip -- exact k-best inner-product search (include/vfmreg.h: vfm_match_ip_topk): what
// faiss::IndexFlatIP::search(n, x, k, D, I) answers on L2-normalised rows, 1 <= k <= VFM_MATCH_TOPK_MAX, decided in fp64.
//
// Semantics.  Rows are normalised in fp32 as the top-1 search normalises them; the score of a pair is the fp64 sum of the products
// of the two normalised rows in ascending column (oracle/vfm_oracle.c, orc_dot_f64); a query's answer is sorted by (score
// descending, map index ascending); sim = (float)score; with m < k the last k - m columns are (-1, -FLT_MAX), the padding of a
// faiss inner-product heap.  Column 0 is what vfm_match_ip_top1 returns.
//
// EXACT (any d >= 1): all pairs in fp64 on the vector ALUs (match_topk_exact_kernel), one workgroup per query, a sorted list of
// VFM_MATCH_TOPK_MAX entries per thread, then k rounds of a workgroup-wide arg-max over the lists' heads.  The score chain, the
// order and the arg-max are the top-1 search's own (match_exact.h), and so is 1 / |row| (launch_inv_norm, match_finish.hip).
//
// FAST (d = 128 / 256 / 384 / 640 / 768, at most 2^24 padded map rows; anything else given FAST runs EXACT, as the top-1 entry point
// falls back -- d = 512 is the one width of the top-1 search's fp16 kernels left without a k-best form; vfm_match_ip_topk_prepared,
// the same search on operands prepared beforehand, refuses such a shape instead):
//   coarse   match_topk_coarse_kernel<d / 16, waves>: v_mfma_f32_32x32x16_f16 on the fragment images vfm_match_prepare writes.  Up to
//            d = 384 in the shape of match_coarse_kernel<KSTEPS, 1> (match_coarse_f16.hip): 8 waves x 32 resident queries, map tiles
//            through an LDS ring of 6 by LDS-DMA, two tiles (64 map rows) per step; d = 640 / 768 in the shape of
//            match_coarse_r_kernel<KSTEPS, 1, 3>: 4 waves, one tile per step, ring of 3 (TopkShape below: the two forms and the
//            wide form's accumulation order and error bound).  Accumulators started at COARSE_OFFSET so that uint order == float order.
//            A lane holds ONE query's scores for 16 of a tile's 32 rows and keeps the k best coarse scores it has seen in a sorted
//            list of registers.  The list's smallest entry, tau, is a lower bound of the query's final k-th best coarse score c_k (the
//            k-th best of a subset never exceeds the k-th best of the whole).  Per step the epilogue is one max per accumulator
//            element; only when the step's maximum reaches tau - window does the slow path walk the 32 elements, append
//            (map row, score bits) for every element >= tau - window to the query's record list (workgroup buffer in LDS, flushed to
//            global after the last step) and insert into the lane's list.  tau is published per query with a device-scope atomicMax
//            and re-read (device-scope load) in the slow path, so every workgroup of the query -- other map slices, the other
//            half-wave -- starts from and tightens one bound; the map is walked in growing launches with the exact bound of the prefix
//            taken from the records in between (match_topk_bound_kernel; see vfm_match_ip_topk below), so that every slice starts seeded.  Rows at or beyond m (zero padding, score exactly 2.0) are neither
//            inserted nor recorded; zero query rows record nothing.
//   finish   match_topk_finish_kernel: per query, every record scored exactly in fp64, the k best selected under the tie rule.  A
//            query whose record count exceeded MATCH_TOPK_RECORD_CAP is decided by match_topk_exact_kernel, restricted to those
//            queries, inside the same call.
//
// Completeness.  tau only grows and never exceeds c_k, so every row with coarse score >= c_k - window is recorded.  A row that is not
// recorded has coarse score < c_k - window, and with window >= 2E (E = the proven |coarse - exact| bound) its exact
// score is below c_k - E.  Each of the (at least) k rows whose coarse score is >= c_k has an exact score >= c_k - E.  So an
// unrecorded row's exact score is strictly below the exact scores of k recorded rows: it cannot be in the answer, ties included.
//
// LDS-DMA and the slow path: the DMA is issued from inline asm (glds16) and tracked by wait_vmcnt<0>() in front of every step's
// barrier -- always 0, so that the slow path's global atomics and loads, which the compiler counts on the same counter, cannot shift
// what a non-zero count would mean.  The record slot comes from an LDS atomic; the publishing atomicMax does not return; the one
// returning access (the re-read of tau) makes the wave wait for the tiles in flight, which is why it sits in the slow path only.
#include "match_exact.h"

#include <cfloat>

namespace vfmm {
namespace {

constexpr int TOPK_MAX = VFM_MATCH_TOPK_MAX;
constexpr int TOPK_RECORD_CAP = FILTER_LDS_ROWS;   // records a query can hold (MATCH_TOPK_RECORD_CAP of vfmreg/ops.py)
constexpr int TOPK_LREC_CAP = SPARSE_LREC_CAP;     // records a coarse workgroup buffers in LDS
constexpr int TOPK_NBUF = 6;                       // LDS ring, tiles
constexpr int TOPK_SEED_CHUNKS = 16;               // map chunks of the first, one-slice launch of the coarse pass
constexpr int TOPK_FAST_MAX_D = 768;               // widest row FAST serves (match_topk_finish_kernel keeps a query row in LDS)
static_assert(TOPK_MAX == 8, "the lanes' lists and the threads' lists are eight registers");
static_assert(TOPK_RECORD_CAP >= 1024, "record cap");

// counters of a call (zeroed with rec_cnt and tau by one memset)
enum { CNT_FALLBACK = 0, CNT_MAXREC = 1, CNT_WORDS = 64 };

struct TopkWs {
    int* counters;       // [CNT_WORDS]
    unsigned* rec_cnt;   // [npad] records appended per query (may exceed the cap: overflow)
    unsigned* tau;       // [npad] published lower bound of the query's k-th best coarse score (score bits)
    int* fb_list;        // [npad] queries for the all-pairs kernel
    uint2* rec;          // [npad][TOPK_RECORD_CAP] (map row, coarse score bits)
    size_t zero_bytes;   // counters | rec_cnt | tau
    size_t bytes;
};
inline TopkWs carve_topk(void* p, int64_t n) {
    VfmCarver c(p);
    TopkWs w;
    const int64_t npad = rows_padded(n);
    w.counters = c.take<int>(CNT_WORDS);   // 256 bytes; npad is a multiple of 256: the three arrays are contiguous
    w.rec_cnt = c.take<unsigned>((size_t)npad);
    w.tau = c.take<unsigned>((size_t)npad);
    w.zero_bytes = c.used();
    w.fb_list = c.take<int>((size_t)npad);
    w.rec = c.take<uint2>((size_t)npad * TOPK_RECORD_CAP);
    w.bytes = c.used();
    return w;
}

struct TopkArgs {
    const uint4* Qh;     // query fragment tiles
    const uint4* Bh;     // map fragment tiles
    const float* qinv;   // [npad] 1 / |query row| (0: zero row)
    int nq_tiles, nqb;
    int chunk0, nchunks, nslices;   // this launch: map chunks [chunk0, chunk0 + nchunks) in nslices slices
    long long m_valid, n_valid;
    int k;
    float window;
    unsigned* tau;
    unsigned* rec_cnt;
    uint2* rec;
};

// The two forms of the coarse kernel, by the number of waves of a workgroup (32 resident queries each):
//   8 waves (d = 128 / 256 / 384)  two waves per SIMD; a step is two map tiles (a lane sees 32 elements), ring of six tiles;
//   4 waves (d = 640 / 768)        the shape of match_coarse_r_kernel<48 | 40, 1, 3> (match_coarse_f16.hip): one wave per SIMD and
//                                  the whole 512-register file -- the query fragments alone are 192 registers at d = 768 --; a step
//                                  is ONE map tile (48 KiB at d = 768; a lane sees 16 elements and refreshes its bound twice as
//                                  often), ring of three tiles.  The k-steps alternate between two accumulator chains, the first
//                                  started at COARSE_OFFSET and the second at 0, added before the epilogue: the accumulation
//                                  order of the top-1 wide kernel, whose bound E < 1.15e-3 at 48 k-steps (40
//                                  k-steps at d = 640 stay below it) gives 2E < 2.3e-3 <= DEFAULT_WINDOW = 2.5e-3 -- no packed row
//                                  index in the score here, so nothing is added to it.
// Either ring is three steps deep: the tiles of step i in use, those of step i + 1 landed, those of step i + 2 staged behind the
// barrier of step i into the slots step i - 1 read.  Everything after the accumulation is one copy.
template <int NWAVES>
struct TopkShape {
    static_assert(NWAVES == 8 || NWAVES == 4, "8 waves x 2 tiles per step, or 4 waves x 1");
    static constexpr int TPS = NWAVES == 8 ? 2 : 1;   // map tiles per step
    static constexpr int NBUF = 3 * TPS;              // LDS ring, tiles
    static constexpr int SPLIT = NWAVES == 8 ? 1 : 2; // accumulator chains per tile
    static constexpr int QROWS = NWAVES * 32;         // queries of a workgroup
    static constexpr int lds_bytes(int ksteps) { return NBUF * ksteps * 1024 + TOPK_LREC_CAP * 8 + 16; }
};
static_assert(TopkShape<8>::NBUF == TOPK_NBUF && TopkShape<8>::QROWS == QBLOCK, "the 8-wave form is the top-1 search's block");
static_assert(TopkShape<4>::lds_bytes(48) == 159760 && TopkShape<4>::lds_bytes(48) <= 160 * 1024,
              "d = 768: three 48 KiB tiles and the record buffer fit the 160 KiB of a compute unit, and no more");

template <int KSTEPS, int NWAVES>
__global__ __launch_bounds__(NWAVES * 64) void match_topk_coarse_kernel(TopkArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Shape = TopkShape<NWAVES>;
    constexpr int TILE_U4 = KSTEPS * 64;
    constexpr int TILE_BYTES = TILE_U4 * 16;
    constexpr int PASSES = KSTEPS / NWAVES;   // 1 KiB pieces per wave per tile
    constexpr int TPS = Shape::TPS, NBUF = Shape::NBUF, SPLIT = Shape::SPLIT;
    constexpr int NE = 16 * TPS;              // accumulator elements of a lane per step
    static_assert(KSTEPS % NWAVES == 0 && (NWAVES == 8 ? KSTEPS <= 24 : KSTEPS == 40 || KSTEPS == 48), "d = 128, 256, 384 | 640, 768");
    static_assert(Shape::lds_bytes(KSTEPS) <= 160 * 1024, "ring and record buffer must fit the LDS");

    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // unit = (query block, map slice), slice-major: the workgroups that run together stream the same map slice
    const int slice = blockIdx.x / a.nqb, qb = blockIdx.x - slice * a.nqb;
    const int c0 = a.chunk0 + (int)(((long long)slice * a.nchunks) / a.nslices);
    const int c1 = a.chunk0 + (int)(((long long)(slice + 1) * a.nchunks) / a.nslices);
    const int ntiles = (c1 - c0) * 4;   // >= 4: a slice holds at least one chunk
    const int t0 = c0 * 4;
    const int qt = qb * NWAVES + wave;  // this wave's 32-query tile

    const unsigned lds_base = (unsigned)(uintptr_t)(LDS_AS unsigned char*)smem;
    auto stage = [&](int it_s) {
        const uint4* src = a.Bh + (size_t)(t0 + it_s) * TILE_U4;
        const unsigned dst = lds_base + (unsigned)((it_s % NBUF) * TILE_BYTES);
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int piece = p * NWAVES + wave;
            glds16(src + piece * 64 + lane, __builtin_amdgcn_readfirstlane(dst + (unsigned)piece * 1024u));
        }
    };

    half8 qf[KSTEPS];   // the wave's queries stay in registers for the whole slice
    {
        const uint4* qsrc = a.Qh + (size_t)(qt < a.nq_tiles ? qt : 0) * TILE_U4 + lane;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            uint4 v = qsrc[s * 64];
            qf[s] = *reinterpret_cast<half8*>(&v);
        }
    }
#pragma unroll
    for (int i = 0; i < 2 * TPS; ++i) stage(i);   // (a slice has at least four tiles)

    uint2* lrec = reinterpret_cast<uint2*>(smem + NBUF * TILE_BYTES);   // [TOPK_LREC_CAP] (query in block << 24 | row, score bits)
    unsigned* lrec_count = reinterpret_cast<unsigned*>(lrec + TOPK_LREC_CAP);
    if (threadIdx.x == 0) *lrec_count = 0u;   // visible after the first barrier below

    // the lane's query, its list (descending; the first 8 - k slots hold a sentinel above every score, so that L[7] is the k-th best
    // of the rows this lane has seen, 0 until there are k) and its bound
    const long long qi = (long long)qt * 32 + (lane & 31);
    const bool live = qt < a.nq_tiles && qi < a.n_valid && a.qinv[qi] != 0.0f;   // (a zero row scores 2.0 everywhere: fixed answer)
    unsigned L[TOPK_MAX];
#pragma unroll
    for (int i = 0; i < TOPK_MAX; ++i) L[i] = i < TOPK_MAX - a.k ? 0xFFFFFFFFu : 0u;
    unsigned tau = 0u;
    // published by other workgroups of the query (any stale value is valid).  Device-scope load: a plain load could be served
    // from this XCD's own L2 and keep returning the zero it cached at the start of the launch.
    if (live) tau = __hip_atomic_load(a.tau + qi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    auto thr_of = [&](unsigned t) -> unsigned {
        if (!live) return 0xFFFFFFFFu;   // nothing passes
        const float f = __uint_as_float(t) - a.window;
        return f > 0.0f ? __float_as_uint(f) : 1u;   // (1: every real score -- masked padding rows are 0)
    };
    unsigned thr = thr_of(tau);
    const int half4 = 4 * (lane >> 5);

    for (int it = 0; it < ntiles; it += TPS) {
        // every DMA issued so far has landed: the tiles of this step (issued two steps ago) and of the next
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (it + 2 * TPS < ntiles) {   // into the slots of the previous step's tiles: their last read retired before this barrier
#pragma unroll
            for (int t = 0; t < TPS; ++t) stage(it + 2 * TPS + t);
        }
        const uint4* buf[TPS];
        floatx16 acc[TPS][SPLIT];
#pragma unroll
        for (int t = 0; t < TPS; ++t) {
            buf[t] = reinterpret_cast<const uint4*>(smem + ((it + t) % NBUF) * TILE_BYTES) + lane;
#pragma unroll
            for (int c = 0; c < SPLIT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][c][r] = c == 0 ? COARSE_OFFSET : 0.f;
        }
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            uint4 v[TPS];
#pragma unroll
            for (int t = 0; t < TPS; ++t) v[t] = buf[t][s * 64];
#pragma unroll
            for (int t = 0; t < TPS; ++t)
                acc[t][s % SPLIT] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<half8*>(&v[t]), qf[s], acc[t][s % SPLIT], 0, 0, 0);
        }
        // accumulator register r of a lane: map row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the tile, query lane & 31
        const long long row0 = ((long long)t0 + it) * TILE_ROWS;
        unsigned x[NE];
#pragma unroll
        for (int t = 0; t < TPS; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) x[16 * t + r] = __float_as_uint(SPLIT == 2 ? acc[t][0][r] + acc[t][SPLIT - 1][r] : acc[t][0][r]);
        if (row0 + TPS * TILE_ROWS > a.m_valid) {   // wave-uniform, the last tiles of the map only: zero padding out of the way
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const long long row = row0 + (e >> 4) * TILE_ROWS + (e & 3) + 8 * ((e & 15) >> 2) + half4;
                if (row >= a.m_valid) x[e] = 0u;
            }
        }
        unsigned smax = 0u;
#pragma unroll
        for (int e = 0; e < NE; ++e) smax = max(smax, x[e]);
        if (smax >= thr) {   // rare after warm-up (never for a lane that is not live)
            const unsigned ql = (unsigned)(wave * 32 + (lane & 31));
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                if (x[e] >= thr) {
                    const unsigned row = (unsigned)(row0 + (e >> 4) * TILE_ROWS + (e & 3) + 8 * ((e & 15) >> 2) + half4);
                    const unsigned slot = atomicAdd(lrec_count, 1u);
                    if (slot < (unsigned)TOPK_LREC_CAP) {
                        lrec[slot] = make_uint2((ql << 24) | row, x[e]);
                    } else {   // buffer full (a fresh bound meeting a duplicate-rich map): straight to the list
                        const unsigned gs = atomicAdd(a.rec_cnt + qi, 1u);
                        if (gs < (unsigned)TOPK_RECORD_CAP) a.rec[(size_t)qi * TOPK_RECORD_CAP + gs] = make_uint2(row, x[e]);
                    }
                    if (x[e] > L[TOPK_MAX - 1]) {
                        unsigned v = x[e];
#pragma unroll
                        for (int i = 0; i < TOPK_MAX; ++i) {
                            const unsigned hi = max(L[i], v);
                            v = min(L[i], v);
                            L[i] = hi;
                        }
                    }
                }
            }
            if (L[TOPK_MAX - 1] > tau) {
                tau = L[TOPK_MAX - 1];
                atomicMax(a.tau + qi, tau);   // result unused: no return value to wait for
            }
            tau = max(tau, __hip_atomic_load(a.tau + qi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            thr = thr_of(tau);
        }
    }
    // flush the workgroup's records to the per-query lists (no DMA in flight any more)
    __syncthreads();
    const unsigned cnt = min(*lrec_count, (unsigned)TOPK_LREC_CAP);
    for (unsigned i = threadIdx.x; i < cnt; i += NWAVES * 64) {
        const uint2 r = lrec[i];
        const size_t q = (size_t)qb * Shape::QROWS + (r.x >> 24);
        const unsigned gs = atomicAdd(a.rec_cnt + q, 1u);
        if (gs < (unsigned)TOPK_RECORD_CAP) a.rec[q * TOPK_RECORD_CAP + gs] = make_uint2(r.x & 0xFFFFFFu, r.y);
    }
}

// ---------------------------------------------------------------------------------------------
// the exact decision
// ---------------------------------------------------------------------------------------------
// The score of a pair is dot_norm_any_f64 (match_exact.h): the chain of orc_dot_f64 on the fp32-normalised rows, for rows of any width.
// a thread's k best pairs, best first: (score descending, map row ascending); j < 0: empty slot
struct TopList {
    double s[TOPK_MAX];
    long long j[TOPK_MAX];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < TOPK_MAX; ++i) {
            s[i] = 0.0;
            j[i] = -1;
        }
    }
    __device__ __forceinline__ void insert(double sc, long long row) {
#pragma unroll
        for (int i = 0; i < TOPK_MAX; ++i) {
            if (decided_before(sc, row, s[i], j[i])) {
                const double ts = s[i];
                const long long tj = j[i];
                s[i] = sc;
                j[i] = row;
                sc = ts;
                row = tj;
            }
        }
    }
    __device__ __forceinline__ void pop() {
#pragma unroll
        for (int i = 0; i + 1 < TOPK_MAX; ++i) {
            s[i] = s[i + 1];
            j[i] = j[i + 1];
        }
        j[TOPK_MAX - 1] = -1;
    }
};

// k rounds of a workgroup-wide arg-max (256 threads) over the heads of the threads' lists: the winner pops.  Every map row sits in
// at most one list.  red_s / red_j: [2][4] in LDS.
__device__ __forceinline__ void block_emit_topk(TopList& T, int k, double* red_s, long long* red_j, int64_t* __restrict__ idx_row,
                                                float* __restrict__ sim_row) {
    for (int r = 0; r < k; ++r) {
        double s = T.s[0];
        long long j = T.j[0];
        // (the buffers alternate: round r + 1 writes the other pair while a late thread still reads this one)
        block_argmax(s, j, red_s + (r & 1) * 4, red_j + (r & 1) * 4);
        if (threadIdx.x == 0) {
            idx_row[r] = j >= 0 ? j : -1;
            sim_row[r] = j >= 0 ? (float)s : -FLT_MAX;   // the padding of a faiss inner-product heap
        }
        if (j >= 0 && T.j[0] == j) T.pop();
    }
}

// all pairs of the queries in `list` (NULL: all n queries), one workgroup per query at a time
__global__ __launch_bounds__(256) void match_topk_exact_kernel(const float* __restrict__ q, const float* __restrict__ invq,
                                                               const float* __restrict__ b, const float* __restrict__ invb, int64_t n,
                                                               int64_t m, int d, int k, const int* __restrict__ list,
                                                               const int* __restrict__ list_count, int64_t* __restrict__ idx_out,
                                                               float* __restrict__ sim_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* qn = reinterpret_cast<float*>(smem);
    __shared__ double red_s[8];
    __shared__ long long red_j[8];
    const int64_t count = list ? (int64_t)*list_count : n;
    for (int64_t e = blockIdx.x; e < count; e += gridDim.x) {
        const int64_t qi = list ? (int64_t)list[e] : e;
        const float iq = invq[qi];
        __syncthreads();
        for (int c = threadIdx.x; c < d; c += 256) qn[c] = q[qi * (int64_t)d + c] * iq;
        __syncthreads();
        TopList T;
        T.clear();
        for (long long j = threadIdx.x; j < m; j += 256) T.insert(dot_norm_any_f64(qn, Rows(b), j * (int64_t)d, invb[j], d), j);
        block_emit_topk(T, k, red_s, red_j, idx_out + qi * k, sim_out + qi * k);
    }
}

// the recorded rows of every query: exact scores, the k best
__global__ __launch_bounds__(256) void match_topk_finish_kernel(const float* __restrict__ q, const float* __restrict__ invq,
                                                                const float* __restrict__ b, const float* __restrict__ invb, int64_t n,
                                                                int64_t m, int d, int k, const unsigned* __restrict__ rec_cnt,
                                                                const uint2* __restrict__ rec, int* __restrict__ counters,
                                                                int* __restrict__ fb_list, int64_t* __restrict__ idx_out,
                                                                float* __restrict__ sim_out) {
    __shared__ float qn[TOPK_FAST_MAX_D];
    __shared__ double red_s[8];
    __shared__ long long red_j[8];
    const int64_t qi = blockIdx.x;
    const float iq = invq[qi];
    const unsigned cnt = rec_cnt[qi];
    if (threadIdx.x == 0 && cnt) atomicMax(counters + CNT_MAXREC, (int)min(cnt, 0x7FFFFFFFu));
    if (iq == 0.0f) {   // zero query: every score is 0.0, the lowest rows in index order
        if (threadIdx.x < k) {
            const bool have = (int64_t)threadIdx.x < m;
            idx_out[qi * k + threadIdx.x] = have ? (int64_t)threadIdx.x : -1;
            sim_out[qi * k + threadIdx.x] = have ? 0.0f : -FLT_MAX;
        }
        return;
    }
    if (cnt > (unsigned)TOPK_RECORD_CAP) {   // some records were dropped: all pairs of this query
        if (threadIdx.x == 0) fb_list[atomicAdd(counters + CNT_FALLBACK, 1)] = (int)qi;
        return;
    }
    for (int c = threadIdx.x; c < d; c += 256) qn[c] = q[qi * (int64_t)d + c] * iq;
    __syncthreads();
    TopList T;
    T.clear();
    for (unsigned i = threadIdx.x; i < cnt; i += 256) {
        const long long j = (long long)rec[(size_t)qi * TOPK_RECORD_CAP + i].x;
        T.insert(dot_norm_any_f64(qn, Rows(b), j * (int64_t)d, invb[j], d), j);
    }
    block_emit_topk(T, k, red_s, red_j, idx_out + qi * k, sim_out + qi * k);
}

// Between two launches of the coarse pass: the k-th best coarse score among a query's records.  The records hold every row of the
// map prefix walked so far whose score is within the window of the prefix's k-th best -- its k best rows among them -- so this IS the
// prefix's k-th best: the bound one workgroup would have reached alone, where a lane's own list knows 1 / (2 x slices) of the rows.
// One wave per query; a query with fewer than k records, or more than the cap (the all-pairs kernel decides it), keeps its bound.
__global__ __launch_bounds__(256) void match_topk_bound_kernel(int64_t n, int k, const unsigned* __restrict__ rec_cnt,
                                                               const uint2* __restrict__ rec, unsigned* __restrict__ tau) {
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= n) return;
    const unsigned cnt = rec_cnt[qi];
    if (cnt < (unsigned)k || cnt > (unsigned)TOPK_RECORD_CAP) return;
    const int lane = lane_id();
    unsigned L[TOPK_MAX];   // the lane's best scores, descending (0: empty -- every score is a positive float)
#pragma unroll
    for (int i = 0; i < TOPK_MAX; ++i) L[i] = 0u;
    for (unsigned i = lane; i < cnt; i += 64) {
        unsigned v = rec[(size_t)qi * TOPK_RECORD_CAP + i].y;
#pragma unroll
        for (int j = 0; j < TOPK_MAX; ++j) {
            const unsigned hi = max(L[j], v);
            v = min(L[j], v);
            L[j] = hi;
        }
    }
    unsigned kth = 0u;
    for (int r = 0; r < k; ++r) {   // k rounds over the lists' heads: the lowest lane that holds the maximum pops
        kth = L[0];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) kth = max(kth, (unsigned)__shfl_xor(kth, off));
        const unsigned long long holders = __ballot(L[0] == kth);
        if (lane == __ffsll((long long)holders) - 1) {
#pragma unroll
            for (int j = 0; j + 1 < TOPK_MAX; ++j) L[j] = L[j + 1];
            L[TOPK_MAX - 1] = 0u;
        }
    }
    if (lane == 0 && kth) atomicMax(tau + qi, kth);
}

__global__ void topk_pad_kernel(int64_t total, int64_t* __restrict__ idx_out, float* __restrict__ sim_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        idx_out[i] = -1;
        sim_out[i] = -FLT_MAX;
    }
}

// info_out: largest record count of a query, queries decided by the all-pairs kernel, map slices, 0
__global__ void topk_info_kernel(const int* __restrict__ counters, int fallback_all, int nslices, int32_t* __restrict__ info_out) {
    info_out[0] = counters ? counters[CNT_MAXREC] : 0;
    info_out[1] = counters ? counters[CNT_FALLBACK] : fallback_all;
    info_out[2] = nslices;
    info_out[3] = 0;
}

template <int KSTEPS, int NWAVES>
int launch_topk_coarse(const TopkArgs& a, hipStream_t st) {
    const int lds = TopkShape<NWAVES>::lds_bytes(KSTEPS);
    static std::atomic<unsigned long long> done{0ull};
    int dev = 0;
    (void)hipGetDevice(&dev);
    VFM_TRY(vfm_allow_dynamic_lds(reinterpret_cast<const void*>(&match_topk_coarse_kernel<KSTEPS, NWAVES>), lds, dev, done));
    hipLaunchKernelGGL((match_topk_coarse_kernel<KSTEPS, NWAVES>), dim3((unsigned)(a.nqb * a.nslices)), dim3(NWAVES * 64), lds, st, a);
    VFM_CHECK_LAUNCH("match_topk_coarse_kernel");
    return VFM_OK;
}
inline int launch_topk_coarse(int d, const TopkArgs& a, hipStream_t st) {
    switch (d) {
        case 128: return launch_topk_coarse<8, 8>(a, st);
        case 256: return launch_topk_coarse<16, 8>(a, st);
        case 384: return launch_topk_coarse<24, 8>(a, st);
        case 640: return launch_topk_coarse<40, 4>(a, st);
        case 768: return launch_topk_coarse<48, 4>(a, st);
    }
    return vfm_fail(VFM_EINVAL, "match_topk: no coarse kernel for d = %d", d);
}
inline bool topk_wide(int d) { return d > 384; }   // the 4-wave form: 128 queries per workgroup

inline bool topk_fast_shape(int64_t m, int d) {   // (a record holds the row in 24 bits)
    return (d == 128 || d == 256 || d == 384 || d == 640 || d == 768) && m >= 1 && rows_padded(m) <= (1ll << 24);
}
inline size_t topk_exact_bytes(int64_t n, int64_t m) {
    return vfm_align_up((size_t)n * sizeof(float), 256) + vfm_align_up((size_t)m * sizeof(float), 256) + 256;
}
constexpr int TOPK_EXACT_MAX_D = 8192;   // a normalised query row in 32 KiB of LDS

inline bool topk_args_ok(int64_t n, int64_t m, int d, int k, int prec_mode) {
    return n >= 0 && m >= 0 && d >= 1 && k >= 1 && k <= TOPK_MAX && (prec_mode == VFM_MATCH_FAST || prec_mode == VFM_MATCH_EXACT) &&
           m < (1ll << 31) - 256 && n < (1ll << 31) - 256;
}
inline size_t topk_bytes(int64_t n, int64_t m, int d, int prec_mode) {
    if (prec_mode == VFM_MATCH_FAST && topk_fast_shape(m, d) && n > 0)
        return vfm_match_prepared_bytes(n, d) + vfm_match_prepared_bytes(m, d) + carve_topk(nullptr, n).bytes;
    return topk_exact_bytes(n, m);
}

// FAST after the operands' preparation -- what vfm_match_ip_topk and vfm_match_ip_topk_prepared share: the counters cleared, the
// coarse launches with the bound kernel between them, the finish, the all-pairs kernel for the overflowed queries, the read-back
int run_topk_fast(const float* q, const Prepared& Q, int64_t n, const float* b, const Prepared& B, int64_t m, int d, int k,
                  const TopkWs& w, int64_t* idx_out, float* sim_out, int32_t* info_out, hipStream_t st) {
    const unsigned egrid = (unsigned)(n < 4096 ? n : 4096);
    VFM_CHECK_HIP(hipMemsetAsync(w.counters, 0, w.zero_bytes, st));
    TopkArgs a;
    a.Qh = Q.tiles;
    a.Bh = B.tiles;
    a.qinv = Q.inv;
    a.nq_tiles = (int)((n + TILE_ROWS - 1) / TILE_ROWS);
    a.nqb = (int)(rows_padded(n) / (topk_wide(d) ? TopkShape<4>::QROWS : TopkShape<8>::QROWS));
    a.m_valid = m;
    a.n_valid = n;
    a.k = k;
    a.window = DEFAULT_WINDOW;
    a.tau = w.tau;
    a.rec_cnt = w.rec_cnt;
    a.rec = w.rec;
    // Launches.  Workgroups that run at the same time seed each other only weakly -- a lane publishes the k-th best of ITS rows --
    // and a fresh bound records ~k (1 + ln(rows / k)) rows per half-wave: 64 unseeded slices would fill a query's list with warm-up
    // alone (tools/sim_topk_records.py: 1166 records per query at 200 000 rows where one slice leaves 210).  So the map is walked in
    // launches that each take three times the chunks already done -- TOPK_SEED_CHUNKS in one slice first --, every one sliced by the
    // top-1 search's rule (choose_slices: whole rounds of workgroups, at least 8 chunks per slice), and between two launches
    // match_topk_bound_kernel sets every query's bound to the k-th best score of the prefix.  Every slice then starts where a single
    // workgroup would stand at the start of the launch: the record counts stay those of one slice (same tool: 213 at 200 000 rows).
    const int total_chunks = (int)chunks_padded(m);
    int max_slices = 0;
    for (int done = 0; done < total_chunks;) {
        const int want = done ? 3 * done : TOPK_SEED_CHUNKS;
        a.chunk0 = done;
        a.nchunks = total_chunks - done < want ? total_chunks - done : want;
        a.nslices = done ? choose_slices(a.nqb, a.nchunks) : 1;
        if (a.nslices > max_slices) max_slices = a.nslices;
        VFM_TRY(launch_topk_coarse(d, a, st));
        done += a.nchunks;
        if (done < total_chunks) {
            hipLaunchKernelGGL(match_topk_bound_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, n, k, (const unsigned*)w.rec_cnt,
                               (const uint2*)w.rec, w.tau);
            VFM_CHECK_LAUNCH("match_topk_bound_kernel");
        }
    }
    hipLaunchKernelGGL(match_topk_finish_kernel, dim3((unsigned)n), dim3(256), 0, st, q, (const float*)Q.inv, b, (const float*)B.inv, n, m, d,
                       k, (const unsigned*)w.rec_cnt, (const uint2*)w.rec, w.counters, w.fb_list, idx_out, sim_out);
    VFM_CHECK_LAUNCH("match_topk_finish_kernel");
    hipLaunchKernelGGL(match_topk_exact_kernel, dim3(egrid < 256u ? egrid : 256u), dim3(256), ((size_t)d * 4 + 15) & ~(size_t)15, st, q,
                       (const float*)Q.inv, b, (const float*)B.inv, n, m, d, k, (const int*)w.fb_list,
                       (const int*)(w.counters + CNT_FALLBACK), idx_out, sim_out);
    VFM_CHECK_LAUNCH("match_topk_exact_kernel");
    if (info_out) {
        hipLaunchKernelGGL(topk_info_kernel, dim3(1), dim3(1), 0, st, (const int*)w.counters, 0, max_slices, info_out);
        VFM_CHECK_LAUNCH("topk_info_kernel");
    }
    return VFM_OK;
}

}  // namespace
}  // namespace vfmm

using namespace vfmm;

VFM_EXPORT size_t vfm_match_ip_topk_workspace_bytes(int64_t n, int64_t m, int d, int k, int prec_mode) {
    if (!topk_args_ok(n, m, d, k, prec_mode)) return 0;
    return topk_bytes(n, m, d, prec_mode);
}

VFM_EXPORT int vfm_match_ip_topk(const float* q, int64_t n, const float* b, int64_t m, int d, int k, int prec_mode, int64_t* idx_out,
                                 float* sim_out, int32_t* info_out, void* ws, size_t ws_bytes, vfm_stream_t stream) {
    VFM_CHECK_ARG(k >= 1 && k <= TOPK_MAX, "match_topk: k must be in 1 .. %d, got %d", TOPK_MAX, k);
    VFM_CHECK_ARG(idx_out && sim_out, "match_topk: null output");
    VFM_CHECK_ARG(d >= 1, "match_topk: d must be at least 1, got %d", d);
    VFM_CHECK_ARG(prec_mode == VFM_MATCH_FAST || prec_mode == VFM_MATCH_EXACT, "match_topk: unknown prec_mode %d", prec_mode);
    VFM_CHECK_ARG(n >= 0 && m >= 0 && m < (1ll << 31) - 256 && n < (1ll << 31) - 256, "match_topk: bad row counts (n=%lld m=%lld)",
                  (long long)n, (long long)m);
    if (n == 0) return VFM_OK;   // nothing to answer, nothing written
    if (!ws || ws_bytes < topk_bytes(n, m, d, prec_mode)) return vfm_fail(VFM_EWORKSPACE, "match_topk: workspace too small");
    VFM_CHECK_ARG(q && (b || m == 0), "match_topk: null operand");
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = n * (int64_t)k;
    if (m == 0) {   // every column is padding
        hipLaunchKernelGGL(topk_pad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, idx_out, sim_out);
        if (info_out) hipLaunchKernelGGL(topk_info_kernel, dim3(1), dim3(1), 0, st, (const int*)nullptr, 0, 0, info_out);
        VFM_CHECK_LAUNCH("topk_pad_kernel");
        return VFM_OK;
    }
    const unsigned egrid = (unsigned)(n < 4096 ? n : 4096);
    if (!(prec_mode == VFM_MATCH_FAST && topk_fast_shape(m, d))) {
        VFM_CHECK_ARG(d <= TOPK_EXACT_MAX_D, "match_topk: d must be at most %d, got %d", TOPK_EXACT_MAX_D, d);
        VfmCarver c(ws);
        float* invq = c.take<float>((size_t)n);
        float* invb = c.take<float>((size_t)m);
        VFM_TRY(launch_inv_norm(q, n, d, invq, st));
        VFM_TRY(launch_inv_norm(b, m, d, invb, st));
        hipLaunchKernelGGL(match_topk_exact_kernel, dim3(egrid), dim3(256), ((size_t)d * 4 + 15) & ~(size_t)15, st, q, (const float*)invq, b,
                           (const float*)invb, n, m, d, k, (const int*)nullptr, (const int*)nullptr, idx_out, sim_out);
        VFM_CHECK_LAUNCH("match_topk_exact_kernel");
        if (info_out) {   // no records, every query by the all-pairs kernel, no slices
            hipLaunchKernelGGL(topk_info_kernel, dim3(1), dim3(1), 0, st, (const int*)nullptr, (int)n, 0, info_out);
            VFM_CHECK_LAUNCH("topk_info_kernel");
        }
        return VFM_OK;
    }
    // FAST: prepare both operands (fp16 fragment images + 1 / |row|), then run_topk_fast
    unsigned char* p = static_cast<unsigned char*>(ws);
    void* qprep = p;
    void* bprep = p + vfm_match_prepared_bytes(n, d);
    const TopkWs w = carve_topk(p + vfm_match_prepared_bytes(n, d) + vfm_match_prepared_bytes(m, d), n);
    VFM_TRY(do_prepare2(VFM_PREP_ENTRY_PREPARE2, 0, q, n, qprep, b, m, bprep, d, st));
    const Prepared Q = carve_prepared(qprep, n, d), B = carve_prepared(bprep, m, d);
    return run_topk_fast(q, Q, n, b, B, m, d, k, w, idx_out, sim_out, info_out, st);
}

// the FAST search on operands prepared beforehand (include/vfmreg.h): no all-pairs fallback for a shape without a kernel
VFM_EXPORT size_t vfm_match_ip_topk_prepared_workspace_bytes(int64_t n, int d, int k) {
    if (!topk_args_ok(n, 1, d, k, VFM_MATCH_FAST) || !topk_fast_shape(1, d)) return 0;
    return carve_topk(nullptr, n).bytes;
}

VFM_EXPORT int vfm_match_ip_topk_prepared(const float* q, const void* q_prepared, int64_t n, const float* b, const void* b_prepared,
                                          int64_t m, int d, int k, int64_t* idx_out, float* sim_out, int32_t* info_out, void* ws,
                                          size_t ws_bytes, vfm_stream_t stream) {
    VFM_CHECK_ARG(k >= 1 && k <= TOPK_MAX, "match_topk_prepared: k must be in 1 .. %d, got %d", TOPK_MAX, k);
    VFM_CHECK_ARG(idx_out && sim_out, "match_topk_prepared: null output");
    VFM_CHECK_ARG(n >= 0 && m >= 0 && m < (1ll << 31) - 256 && n < (1ll << 31) - 256, "match_topk_prepared: bad row counts (n=%lld m=%lld)",
                  (long long)n, (long long)m);
    VFM_CHECK_ARG(topk_fast_shape(m, d), "match_topk_prepared: no kernel for this shape (d=%d must be 128, 256, 384, 640 or 768; m=%lld "
                  "must be 1 .. 2^24 padded rows)", d, (long long)m);
    if (n == 0) return VFM_OK;   // nothing to answer, nothing written
    VFM_CHECK_ARG(q && q_prepared && b && b_prepared, "match_topk_prepared: null operand");
    const TopkWs w = carve_topk(ws, n);
    if (!ws || ws_bytes < w.bytes) return vfm_fail(VFM_EWORKSPACE, "match_topk_prepared: workspace too small");
    const Prepared Q = carve_prepared(const_cast<void*>(q_prepared), n, d), B = carve_prepared(const_cast<void*>(b_prepared), m, d);
    return run_topk_fast(q, Q, n, b, B, m, d, k, w, idx_out, sim_out, info_out, (hipStream_t)stream);
}

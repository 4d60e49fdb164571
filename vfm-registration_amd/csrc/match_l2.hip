// match_l2.hip -- exact Euclidean nearest neighbours both ways (row A6: find_correspondences, registration_node.py:482-538)
// on the fp16 coarse pass: common power-of-two scale, the norm term in two appended fp16 columns (or a row bias in the
// accumulator start), fp64 decision in the oracle's order ("Row A6").  Rows of at most 64 columns have a search of
// their own on the f32 MFMA (VFM_MATCH_NARROW, match_l2_narrow.hip); the entry points below route to it.
#include <hipcub/hipcub.hpp>

#include "match_exact.h"
#include "match_select.h"

namespace vfmm {
namespace {

// ---------------------------------------------------------------------------------------------
// exact Euclidean 1-NN (find_correspondences, registration_node.py:485-496): one workgroup per
// query row, fp64 squared distance, sequential k, ties -> lowest index
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nn_l2_kernel(const float* __restrict__ a, int64_t n, const float* __restrict__ b,
                                                    int64_t m, int d, const int* __restrict__ list,
                                                    const int* __restrict__ list_count, int64_t* __restrict__ nn,
                                                    double* __restrict__ d2, const int* __restrict__ qperm = nullptr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* qa = reinterpret_cast<float*>(smem);
    double* rs = reinterpret_cast<double*>(smem + (((size_t)d * 4 + 15) & ~(size_t)15));
    long long* rj = reinterpret_cast<long long*>(rs + 4);
    const int64_t count = list ? (int64_t)*list_count : n;  // list: the queries whose candidate list overflowed
    for (int64_t e = blockIdx.x; e < count; e += gridDim.x) {
        const int64_t qi = list ? (int64_t)list[e] : e;
        __syncthreads();
        const int64_t qsrc = qperm ? (int64_t)qperm[qi] : qi;   // (query qi is row qperm[qi] of a)
        for (int k = threadIdx.x; k < d; k += 256) qa[k] = a[qsrc * (int64_t)d + k];
        __syncthreads();
        double best = 0.0;
        long long bj = -1;
        for (long long j = threadIdx.x; j < m; j += 256) {
            const double acc = l2_dist_f64(qa, b + j * (int64_t)d, d);
            if (bj < 0 || acc < best) {   // (a thread's j ascends: an equal distance never replaces an earlier row)
                best = acc;
                bj = j;
            }
        }
        // arg-min: negate so that the arg-max applies (x -> -x is exact)
        double neg = -best;
        block_argmax(neg, bj, rs, rj);   // (rs / rj are rewritten behind the two barriers at the top of the next query)
        if (threadIdx.x == 0) {
            nn[qi] = bj;
            if (d2) d2[qi] = -neg;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// FAST Euclidean 1-NN (row A6): the arg-min of |a - b|^2 = |a|^2 + |b|^2 - 2 a.b over b is the arg-max
// of f(b) = a~.b~ - |b~|^2 / 2 for any common scale (x~ = x * 2^-k, k chosen so that every row norm of
// BOTH sets is <= 1: power of two, so the scaling is exact).  f comes out of the same fp16 MFMA coarse
// pass as the cosine search by appending two columns to the fragment tiles: the map row carries
// (-hi, -lo) with hi + lo = |b~|^2 / 2 split into two fp16 values (error 2^-22), the query row
// carries (1, 1); the padded K is the next multiple of 128 >= d + 2.  |coarse - f| <= E as before
// (operand rounding (2u + u^2) |a~| |b~| <= 9.8e-4, subnormal flush < 1e-6, norm term < 1e-6), so the
// same window / select apply; the decision among the candidates is the oracle's fp64 squared
// distance (sequential k), ties -> lowest index.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void l2_maxnorm_row(const float* __restrict__ x, int64_t r, int d, unsigned* __restrict__ max_bits) {
    float p = 0.f;
    for (int k = lane_id(); k < d; k += 64) {
        const float v = x[r * (int64_t)d + k];
        p += v * v;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p += __shfl_xor(p, off);
    // p >= 0: bit order == value order; only a row that raises the maximum touches it
    if (lane_id() == 0 && __float_as_uint(p) > __hip_atomic_load(max_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(max_bits, __float_as_uint(p));
}
__global__ __launch_bounds__(256) void l2_maxnorm_kernel(const float* __restrict__ x, int64_t rows, int d,
                                                         unsigned* __restrict__ max_bits) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    l2_maxnorm_row(x, r, d, max_bits);
}
// both sets in one launch (the narrow search: a 5000 x 5000 call is a handful of launches long)
__global__ __launch_bounds__(256) void l2_maxnorm2_kernel(const float* __restrict__ a, int64_t n, const float* __restrict__ b, int64_t m, int d,
                                                          unsigned* __restrict__ max_bits) {
    const int64_t na = (n + 3) / 4;
    const bool second = (int64_t)blockIdx.x >= na;
    const int64_t r = ((int64_t)blockIdx.x - (second ? na : 0)) * 4 + (threadIdx.x >> 6);
    if (r >= (second ? m : n)) return;
    l2_maxnorm_row(second ? b : a, r, d, max_bits);
}

// (l2_scale: match_internal.h -- shared with the f32 search of match_l2_narrow.hip)

// one workgroup (4 waves) per 32-row tile; role 0 = query (extra columns 1, 1), 1 = map (-hi, -lo)
// aug = 1: the norm term travels in two appended columns (d + 2 <= kp); aug = 0 (d > 510, kp = d rounded up
// to 128): no extra columns, the MAP role stores -|b~|^2 / 2 per row in inv_out instead -- the coarse kernel
// adds it to the accumulator start of that row (CoarseArgs::row_bias)
__global__ __launch_bounds__(256) void l2_prep_kernel(const float* __restrict__ x, int64_t rows, int d, int kp,
                                                      const unsigned* __restrict__ max_bits, int role, int aug,
                                                      float* __restrict__ inv_out, uint4* __restrict__ tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tile = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const float scale = l2_scale(max_bits);
    _Float16* img = reinterpret_cast<_Float16*>(smem);
    for (int pr = wave; pr < TILE_ROWS; pr += 4) {
        const int64_t r = (int64_t)tile * TILE_ROWS + pr;
        const bool valid = r < rows;
        float nb2 = 0.f;
        for (int k = lane; k < kp; k += 64) {
            float v = 0.f;
            if (valid && k < d) {
                v = x[r * (int64_t)d + k] * scale;
                nb2 += v * v;
            }
            if (!aug || k < d || k >= d + 2) img[(((k >> 4) * 2 + ((k >> 3) & 1)) * 32 + pr) * 8 + (k & 7)] = (_Float16)v;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) nb2 += __shfl_xor(nb2, off);
        if (aug && lane < 2) {
            const float h = 0.5f * nb2;
            const _Float16 hi = (_Float16)h;
            const _Float16 lo = (_Float16)(h - (float)hi);
            _Float16 e = (_Float16)0.f;
            if (valid) e = (role == 0) ? (_Float16)1.0f : (lane == 0 ? (_Float16)(-(float)hi) : (_Float16)(-(float)lo));
            const int k = d + lane;
            img[(((k >> 4) * 2 + ((k >> 3) & 1)) * 32 + pr) * 8 + (k & 7)] = e;
        }
        // query role: "not a zero row" for match_select_kernel; map role without columns: the row bias
        if (lane == 0) inv_out[r] = (!aug && role == 1) ? (valid ? -0.5f * nb2 : 0.0f) : 1.0f;
    }
    __syncthreads();
    const int units = (kp >> 4) * 64;
    uint4* dst = tiles + (int64_t)tile * units;
    const uint4* src = reinterpret_cast<const uint4*>(smem);
    for (int u = threadIdx.x; u < units; u += 256) {
        const uint4 t = src[u];
        unsigned* o = reinterpret_cast<unsigned*>(dst + u);
        __builtin_nontemporal_store(t.x, o);
        __builtin_nontemporal_store(t.y, o + 1);
        __builtin_nontemporal_store(t.z, o + 2);
        __builtin_nontemporal_store(t.w, o + 3);
    }
}

// exact decision among the candidates of match_select_kernel: one wave per query
__global__ __launch_bounds__(256) void l2_rescore_kernel(const float* __restrict__ q, const float* __restrict__ b, int64_t n,
                                                         int64_t m, int d, const int* __restrict__ cand_cnt,
                                                         const unsigned* __restrict__ cand, int cap, int64_t* __restrict__ nn_out,
                                                         double* __restrict__ d2_out, const int* __restrict__ perm = nullptr,
                                                         const int* __restrict__ qperm = nullptr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = threadIdx.x >> 6, lane = lane_id();
    float* qa = reinterpret_cast<float*>(smem) + wave * 2 * d;
    float* bb = qa + d;
    const int64_t qi = (int64_t)blockIdx.x * 4 + wave;
    if (qi >= n) return;
    const int cnt = cand_cnt[qi];
    if (cnt < 0) return;  // handled by nn_l2_kernel (candidate overflow)
    // (int8 Euclidean search: candidate positions refer to the norm-SORTED image of the map -- row perm[pos] of b --, and query
    // qi may be a gathered row qperm[qi] of q; distances and the tie-break use the original rows / indices)
    const int64_t qsrc = qperm ? (int64_t)qperm[qi] : qi;
    for (int k = lane; k < d; k += 64) qa[k] = q[qsrc * (int64_t)d + k];
    __builtin_amdgcn_wave_barrier();
    double best = 0.0;  // negated distance: wave_argmax picks the smallest distance, ties -> lowest index
    long long bj = -1;
    for (int e = 0; e < cnt; ++e) {
        const unsigned ce = cand[(size_t)qi * cap + e];
        const long long base = (long long)(ce >> 8) * CHUNK_ROWS;
        if (ce & 128u) {
            for (int li = lane; li < CHUNK_ROWS; li += 64) {
                if (base + li < m) {
                    const long long j = perm ? (long long)perm[base + li] : base + li;
                    const double s = -l2_dist_f64(qa, b + j * (int64_t)d, d);
                    take_if_before(s, j, best, bj);
                }
            }
        } else {
            if (base + (ce & 127u) < m) {
                const long long j = perm ? (long long)perm[base + (ce & 127u)] : base + (ce & 127u);
                __builtin_amdgcn_wave_barrier();
                for (int k = lane; k < d; k += 64) bb[k] = b[j * (int64_t)d + k];
                __builtin_amdgcn_wave_barrier();
                const double s = -l2_dist_f64(qa, bb, d);  // same chain in every lane (LDS broadcast reads)
                take_if_before(s, j, best, bj);
            }
        }
    }
    wave_argmax(best, bj);
    if (lane == 0) {
        nn_out[qi] = bj;
        if (d2_out) d2_out[qi] = -best;
    }
}

// =============================================================================================
// Row A6 on the INT8 coarse pass (round 3; d = 256 ... 768 in steps of 128).  VERDICT r2: north_star's named matcher -- all-pairs
// L2 + mutual-NN -- ran the fp16 pass twice over K padded 386 -> 512: 17.4 ms at 20 000 x 200 000 x 384.
//
// The int8 image holds the NORMALISED rows (prep_chunk_kernel), so the coarse pass and its proven bounds  cos(a, b) in
// [s_a s_b S - A - B_c, s_a s_b S + A + B_c]  are the inner-product search's, unchanged.  The Euclidean score of a pair is
//     f(a, b) = a~.b~ - |b~|^2 / 2 = |a~| |b~| cos(a, b) - |b~|^2 / 2        (x~ = 2^-k x, every norm <= 1; arg max f = arg min |a - b|)
// and what turns a bound on the cosine into a bound on f is the row's norm.  So the MAP IS SORTED BY NORM before its image is
// built (one radix sort of the fp32 sums of squares; prep_chunk_kernel reads row perm[r]): the 128 rows of a chunk then have
// norms in a narrow [lo_c, hi_c] -- equal for unit descriptors -- and for a (query, chunk) pair with best integer score S
//     upper_c = max_{nb in [lo, hi]} ( qn nb cosU - nb^2 / 2 ),  attained at clamp(qn cosU, lo, hi)      (concave in nb)
//     lower_c = min( g(lo), g(hi) ),  g(nb) = qn nb cosL - nb^2 / 2                                        (the row that scored S)
// (sorting also groups rows of like norm into one quantisation group: a tiny row no longer shares its step with a large one).
// match_select_l2_kernel sweeps a query tile's records twice -- qlow = max_c lower_c, then the chunks with upper_c >= qlow --, the
// int8 rescans keep the rows whose own bound  qn bn_r max(cosU_r, 0) - bn_r^2 / 2  reaches qlow (L2Terms), and the decision is the
// oracle's fp64 squared distance on the ORIGINAL rows, ties -> lowest original index.  No second fp16 pass, no padded columns.
// =============================================================================================
__global__ __launch_bounds__(256) void l2i8_sumsq_kernel(const float* __restrict__ x, int64_t rows, int d, const int* __restrict__ gather,
                                                         float* __restrict__ ss, unsigned* __restrict__ max_bits) {
    // 16 lanes per row (d % 4 == 0: float4 loads), 16 rows per workgroup, one atomic per workgroup that raises the maximum
    __shared__ unsigned wmax;
    if (threadIdx.x == 0) wmax = 0u;
    __syncthreads();
    const int sub = threadIdx.x & 15;
    const int64_t r = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    float p = 0.f;
    if (r < rows) {
        const float4* row = reinterpret_cast<const float4*>(x + (gather ? (int64_t)gather[r] : r) * (int64_t)d);
        for (int k = sub; k < (d >> 2); k += 16) {
            const float4 v = row[k];
            p += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
        }
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) p += __shfl_xor(p, off);
    if (r < rows && sub == 0) {
        ss[r] = p;
        if (max_bits) atomicMax(&wmax, __float_as_uint(p));   // p >= 0: bit order == value order
    }
    __syncthreads();
    // (only a workgroup that raises the maximum touches it: 200 000 atomics on one address had cost 2.3 ms)
    if (threadIdx.x == 0 && max_bits && wmax > __hip_atomic_load(max_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(max_bits, wmax);
}

__global__ void l2i8_iota_kernel(int* __restrict__ v, const float* __restrict__ ss, unsigned* __restrict__ keys, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        v[i] = (int)i;
        keys[i] = __float_as_uint(ss[i]);   // non-negative floats (NaN sorts last): unsigned order == value order
    }
}

// scaled norms: out[i] = 2^-k sqrt(ss[i]) for i < rows, 0 for the padding; lohi[c] = norms of the first / last valid row of
// chunk c (the rows are sorted: the chunk's smallest / largest)
__global__ void l2i8_norms_kernel(const unsigned* __restrict__ ss_bits, int64_t rows, int64_t rows_pad, const unsigned* __restrict__ max_bits,
                                  float* __restrict__ out, float2* __restrict__ lohi) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows_pad) return;
    const float scale = l2_scale(max_bits);
    const float v = i < rows ? scale * sqrtf(__uint_as_float(ss_bits[i])) : 0.0f;
    out[i] = v;
    if (lohi && (i % CHUNK_ROWS) == 0) {
        const int64_t last = (i + CHUNK_ROWS - 1 < rows ? i + CHUNK_ROWS - 1 : rows - 1);
        const float hi = last >= i ? scale * sqrtf(__uint_as_float(ss_bits[last])) : 0.0f;
        lohi[i / CHUNK_ROWS] = make_float2(v, hi);
    }
}

// (a query whose rows are not finite ends with no candidate at all -- every bound comparison is false -- and nn = -1: as a gather
// index it is clamped to row 0 here; l2_mutual_pairs_kernel never reports such a query as mutual, whatever the reverse search
// of row 0 returns)
__global__ void l2i8_to_int_kernel(const int64_t* __restrict__ src, int* __restrict__ dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i] < 0 ? 0 : (int)src[i];
}

// The selection of the int8 Euclidean search, from the tile kernels' pieces (match_select.h): the sweep frame twice, the bounds of
// the cosine, the staged candidates, the placement, and the overflow class of the epilogue.  Its own: the (step, max E, lo, hi)
// staging and the two Euclidean bounds.
constexpr int SELECT_L2_WAVES = 8;
constexpr int SELECT_L2_LCAND = 4096;
__global__ __launch_bounds__(64 * SELECT_L2_WAVES) void match_select_l2_kernel(
    const unsigned* __restrict__ best, int nchunks, int64_t n, I8Bounds ib, const float* __restrict__ qn, const float2* __restrict__ cn,
    float slack, int first_pad_chunk, int chunk_lds, unsigned* __restrict__ qmax, int* __restrict__ cand_cnt, unsigned* __restrict__ cand,
    int cap, int* __restrict__ fb_count, int* __restrict__ fb_list, unsigned* __restrict__ bin_cnt, int* __restrict__ bins,
    int bin_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char select_smem[];  // per chunk: (step, max E, lo, hi)
    __shared__ int lcnt[32], lov[32];
    __shared__ unsigned llow[32];   // float_key of the query's lower bound of its best Euclidean score
    __shared__ unsigned lcand[SELECT_L2_LCAND];   // the tile's candidates: (query of the tile << 27) | chunk
    __shared__ int lcand_n;
    const int qt = blockIdx.x;
    if (threadIdx.x < 32) {
        lcnt[threadIdx.x] = 0;
        lov[threadIdx.x] = 0;
        llow[threadIdx.x] = 0u;
    }
    if (threadIdx.x == 0) lcand_n = 0;
    float4* lchunk = reinterpret_cast<float4*>(select_smem);
    if (chunk_lds)
        for (int c = threadIdx.x; c < nchunks; c += 64 * SELECT_L2_WAVES) {
            const float2 nh = cn[c];
            lchunk[c] = make_float4(ib.bstep[c], ib.berr[c], nh.x, nh.y);
        }
    __syncthreads();
    const int lq = TileLane<4>().lq;
    const int64_t q0 = (int64_t)qt * 32 + lq;   // the lane's four queries (rows of the padded tile always exist)
    const float sq = ib.qstep[q0 >> 7];
    QueryBound qb[4];   // (the slack of the cosine's bounds folded into A)
    float nq[4];
    unsigned livemask = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        qb[j] = query_bound_slack(ib.qerr[q0 + j]);
        nq[j] = qn[q0 + j];
        if (q0 + j < n) livemask |= 1u << j;
    }
    const uint4* tile = reinterpret_cast<const uint4*>(best + (size_t)qt * nchunks * 32);
    auto chunk_data = [&](int c) { return chunk_lds ? lchunk[c] : make_float4(ib.bstep[c], ib.berr[c], cn[c].x, cn[c].y); };
    // sweep 1: qlow = the largest lower bound over the chunks
    float low[4] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    sweep_tile_records<4, SELECT_L2_WAVES>(tile, nchunks, [&](int c, uint4 rec) {
        const float4 cd = chunk_data(c);
        const float sc = sq * cd.x;
        const unsigned r4[4] = {rec.x, rec.y, rec.z, rec.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int S = best_score(r4[j]);
            // (a chunk with zero-padded rows -- they score exactly 0 -- counts only where its best score is positive)
            if (c >= first_pad_chunk && S <= 0) continue;
            const float cosL = cos_lower(sc, S, qb[j], cd.y);
            const float g_lo = __builtin_fmaf(nq[j] * cd.z, cosL, -0.5f * cd.z * cd.z);
            const float g_hi = __builtin_fmaf(nq[j] * cd.w, cosL, -0.5f * cd.w * cd.w);
            low[j] = fmaxf(low[j], fminf(g_lo, g_hi) - slack);
        }
        return false;
    });
    raise_query_max<4>(llow, lq, low);
    __syncthreads();
    float qlow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) qlow[j] = key_float(llow[lq + j]);   // -Inf: no chunk qualified -> every chunk is a candidate
    // sweep 2 (the records come out of the L2 this time): the chunks whose upper bound reaches qlow, staged (stage_candidate) -- a
    // returning global atomic per candidate inside the sweep stalled the wave each time: 0.75 ms at C2's 250 000 candidates
    sweep_tile_records<4, SELECT_L2_WAVES>(tile, nchunks, [&](int c, uint4 rec) {
        const float4 cd = chunk_data(c);
        const float sc = sq * cd.x;
        const unsigned r4[4] = {rec.x, rec.y, rec.z, rec.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float cosU = fmaxf(cos_upper(sc, best_score(r4[j]), qb[j], cd.y), 0.0f);
            const float nb = fminf(fmaxf(nq[j] * cosU, cd.z), cd.w);   // where qn nb cosU - nb^2 / 2 peaks inside [lo, hi]
            const float up = __builtin_fmaf(nq[j] * nb, cosU, -0.5f * nb * nb) + slack;
            if (up >= qlow[j] && ((livemask >> j) & 1u)) {
                atomicAdd(&lcnt[lq + j], 1);
                stage_candidate(lcand, &lcand_n, SELECT_L2_LCAND, lq + j, c);   // (a full buffer: the whole tile goes to the all-pairs kernel)
            }
        }
        return false;
    });
    __syncthreads();
    const int ncand = lcand_n;
    if (ncand <= SELECT_L2_LCAND) {
        const SelectLists L{bin_cnt, bins, bin_cap, cand, cap};
        for (int i = threadIdx.x; i < ncand; i += 64 * SELECT_L2_WAVES) {
            const unsigned e = lcand[i];
            const int qq = staged_query(e);
            place_candidate(L, (int64_t)qt * 32 + qq, staged_chunk(e), true, &lov[qq]);
        }
    }
    __syncthreads();
    // No gate and no zero-row rule here: the epilogue shares the overflow class only (send_to_all_pairs).
    if (threadIdx.x < 32) {
        const int qq = threadIdx.x;
        const int64_t q = (int64_t)qt * 32 + qq;
        if (q < n) {
            const int cnt = lcnt[qq];
            qmax[q] = llow[qq];   // the rescans' hit test: float_key(qlow)
            if (cnt > cap || ncand > SELECT_L2_LCAND) {
                // more candidate chunks than a list (or the tile's staging buffer) holds: the all-pairs kernel decides.  (The
                // staging buffer overflows only when the tile's 32 queries average more than 128 candidate chunks each.)
                if (cnt > 0 || ncand > SELECT_L2_LCAND) send_to_all_pairs(q, cand_cnt, fb_count, fb_list);
                else cand_cnt[q] = 0;
            } else {
                cand_cnt[q] = lov[qq];   // entries in the query's own list (everything, without bins)
            }
        }
    }
}

// exact decision among the candidate ROWS the int8 rescans left (positions in the sorted image).  The oracle's distance is a
// strictly sequential fp64 chain over k (no FMA: five dependent-issue operations per element), so a wave costs the same
// whether one lane or sixty-four run it -- and half the queries of a scan have ONE candidate.  A workgroup therefore owns 64
// queries and packs their (query, candidate row) pairs 64 to a wave, one lane each, both rows read straight from memory
// (float4).  Arg-min per query, ties -> lowest original index: atomicMin on the distance bits in LDS; a pair that was not
// beaten when it arrived is a "contender" (a record-breaking sequence: ~ln(candidates) per query) and the contenders that
// equal the final minimum settle the index.
constexpr int L2R_QUERIES = 64;
constexpr int L2R_CONTENDERS = 2048;
__global__ __launch_bounds__(256) void l2i8_rescore_kernel(const float* __restrict__ q, const float* __restrict__ b, int64_t n, int64_t m,
                                                           int d, const int* __restrict__ cand_cnt, const unsigned* __restrict__ cand,
                                                           int cap, const int* __restrict__ perm, const int* __restrict__ qperm,
                                                           int64_t* __restrict__ nn_out, double* __restrict__ d2_out) {
    __shared__ int l_off[L2R_QUERIES + 1];
    __shared__ unsigned long long l_best[L2R_QUERIES];
    __shared__ long long l_bj[L2R_QUERIES];
    __shared__ int l_ncont;
    __shared__ unsigned long long l_cd[L2R_CONTENDERS];
    __shared__ long long l_cr[L2R_CONTENDERS];
    __shared__ unsigned char l_cq[L2R_CONTENDERS];
    const int t = threadIdx.x, lane = lane_id();
    const int64_t q0 = (int64_t)blockIdx.x * L2R_QUERIES;
    if (t < 64) {
        const int64_t qi = q0 + t;
        int c = qi < n ? cand_cnt[qi] : 0;
        c = c > 0 ? c : 0;   // (< 0: candidate overflow, nn_l2_kernel decides)
        int incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        l_off[t + 1] = incl;
        if (t == 0) {
            l_off[0] = 0;
            l_ncont = 0;
        }
        l_best[t] = ~0ull;
        l_bj[t] = 0x7FFFFFFFFFFFFFFFll;
    }
    __syncthreads();
    const int P = l_off[L2R_QUERIES];
    auto pair_row = [&](int p, int& qq) -> long long {   // original row of pair p (-1: padding), its query of the block in qq
        int lo = 0, hi = L2R_QUERIES - 1;                  // the last query whose offset is <= p
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (l_off[mid] <= p) lo = mid; else hi = mid - 1;
        }
        qq = lo;
        const unsigned ce = cand[(size_t)(q0 + qq) * cap + (p - l_off[qq])];
        const long long pos = (long long)(ce >> 8) * CHUNK_ROWS + (long long)(ce & 127u);
        return pos < m ? (perm ? (long long)perm[pos] : pos) : -1;
    };
    auto exact = [&](int qq, long long j) {   // the oracle's order: k ascending, no FMA
        const int64_t qsrc = qperm ? (int64_t)qperm[q0 + qq] : q0 + qq;
        const float4* qrow = reinterpret_cast<const float4*>(q + qsrc * (int64_t)d);
        const float4* brow = reinterpret_cast<const float4*>(b + j * (int64_t)d);
        double acc = 0.0;
        const int nk4 = d >> 2;
        for (int k0 = 0; k0 < nk4; k0 += 8) {   // sixteen 16-byte loads in flight, then the chain over their 32 elements
            float4 av[8], bv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k4 = k0 + u < nk4 ? k0 + u : nk4 - 1;
                av[u] = qrow[k4];
                bv[u] = brow[k4];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (k0 + u >= nk4) break;
                acc = l2_step_f64(acc, av[u].x, bv[u].x);
                acc = l2_step_f64(acc, av[u].y, bv[u].y);
                acc = l2_step_f64(acc, av[u].z, bv[u].z);
                acc = l2_step_f64(acc, av[u].w, bv[u].w);
            }
        }
        return acc;
    };
    for (int p = t; p < P; p += 256) {
        int qq;
        const long long j = pair_row(p, qq);
        if (j < 0) continue;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(exact(qq, j));   // >= 0: bit order == value order
        const unsigned long long old = atomicMin(&l_best[qq], bits);
        if (bits <= old) {
            const int at = atomicAdd(&l_ncont, 1);
            if (at < L2R_CONTENDERS) {
                l_cd[at] = bits;
                l_cr[at] = j;
                l_cq[at] = (unsigned char)qq;
            }
        }
    }
    __syncthreads();
    const int nc = l_ncont;
    if (nc <= L2R_CONTENDERS) {
        for (int i = t; i < nc; i += 256)
            if (l_cd[i] == l_best[l_cq[i]]) atomicMin(&l_bj[l_cq[i]], l_cr[i]);
    } else {   // (thousands of exact ties in one block: settle the index by a second pass over the pairs)
        for (int p = t; p < P; p += 256) {
            int qq;
            const long long j = pair_row(p, qq);
            if (j >= 0 && (unsigned long long)__double_as_longlong(exact(qq, j)) == l_best[qq]) atomicMin(&l_bj[qq], j);
        }
    }
    __syncthreads();
    if (t < 64) {
        const int64_t qi = q0 + t;
        if (qi < n && cand_cnt[qi] >= 0) {
            const bool any = l_best[t] != ~0ull;
            nn_out[qi] = any ? (int64_t)l_bj[t] : -1;
            if (d2_out) d2_out[qi] = any ? __longlong_as_double((long long)l_best[t]) : 0.0;
        }
    }
}

__global__ void l2_gather_rev_kernel(const int64_t* __restrict__ nn_ab, const int64_t* __restrict__ nn_ba, int64_t n,
                                     int64_t* __restrict__ nn_rev) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) nn_rev[i] = nn_ba[nn_ab[i]];
}

// find_correspondences' mutual filter (registration_node.py:520-532): keep i iff the nearest neighbour of b[nn_ab[i]] among a is i
__global__ __launch_bounds__(1024) void l2_mutual_pairs_kernel(const int64_t* __restrict__ nn_ab, const int64_t* __restrict__ nn_rev,
                                                               int64_t n, int64_t* __restrict__ idx0, int64_t* __restrict__ idx1,
                                                               int64_t* __restrict__ count) {
    __shared__ int wsum[16];
    __shared__ int base_s;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) base_s = 0;
    __syncthreads();
    for (int64_t i0 = 0; i0 < n; i0 += 1024) {
        const int64_t i = i0 + threadIdx.x;
        const bool keep = i < n && nn_ab[i] >= 0 && nn_rev[i] == i;   // nn_ab < 0: a query without any candidate (non-finite row)
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int off = base_s;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        if (keep) {
            const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
            idx0[pos] = i;
            idx1[pos] = nn_ab[i];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int w = 0; w < 16; ++w) t += wsum[w];
            base_s += t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = base_s;
}

}  // namespace

// d <= 510: two appended columns; 510 < d <= 768: row bias, no extra columns; wider: 0 (all-pairs fp64)
inline bool l2_aug(int d) { return d + 2 <= 512; }
// (the row-bias form exists in match_coarse_r_kernel only, i.e. for K = 640 and 768: d = 511, 512 pad to 640)
inline int l2_padded_k(int d) { return l2_aug(d) ? (d + 2 + 127) / 128 * 128 : (d <= 640 ? 640 : (d <= 768 ? 768 : 0)); }

struct L2Ws {
    unsigned* max_bits;
    void* prep[4];  // a as query, b as map, b as query, a as map
    void* search[2];
    size_t bytes;
};
inline L2Ws carve_l2(void* p, int64_t n, int64_t m, int d, bool mutual) {
    VfmCarver c(p);
    L2Ws w;
    const int kp = l2_padded_k(d);
    w.max_bits = c.take<unsigned>(64);
    const size_t pa = vfm_match_prepared_bytes(n, kp), pb = vfm_match_prepared_bytes(m, kp);
    w.prep[0] = c.take<unsigned char>(pa);
    w.prep[1] = c.take<unsigned char>(pb);
    w.search[0] = c.take<unsigned char>(carve_search(nullptr, n, m).bytes);
    w.prep[2] = w.prep[3] = w.search[1] = nullptr;
    if (mutual) {
        w.prep[2] = c.take<unsigned char>(pb);
        w.prep[3] = c.take<unsigned char>(pa);
        w.search[1] = c.take<unsigned char>(carve_search(nullptr, m, n).bytes);
    }
    w.bytes = c.used();
    return w;
}

int l2_prepare(const float* x, int64_t rows, int d, int kp, const unsigned* max_bits, int role, void* prepared, hipStream_t st) {
    Prepared p = carve_prepared(prepared, rows, kp);
    hipLaunchKernelGGL(l2_prep_kernel, dim3((unsigned)(rows_padded(rows) / TILE_ROWS)), dim3(256), (size_t)kp * 64, st, x, rows, d, kp,
                       max_bits, role, l2_aug(d) ? 1 : 0, p.inv, p.tiles);
    VFM_CHECK_LAUNCH("l2_prep_kernel");
    return VFM_OK;
}

// one direction: every row of q (n x d) among b (m x d)
int l2_search(const float* q, void* qprep, int64_t n, const float* b, void* bprep, int64_t m, int d, int kp, int64_t* nn,
              double* d2, void* ws, hipStream_t st) {
    if (int rc = do_search_coarse(qprep, n, bprep, m, kp, ws, st, !l2_aug(d))) return rc;
    Prepared Q = carve_prepared(qprep, n, kp);
    SearchWs w = carve_search(ws, n, m);
    const CoarseArgs a = coarse_args(Q, carve_prepared(bprep, m, kp), w, n, m);
    if (int rc = launch_select_dense(w, a, Q.inv, n, st)) return rc;
    hipLaunchKernelGGL(l2_rescore_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), (size_t)d * 4 * 8, st, q, b, n, m, d, w.cand_cnt,
                       w.cand, w.cap, nn, d2);
    VFM_CHECK_LAUNCH("l2_rescore_kernel");
    const size_t lds = (((size_t)d * 4 + 15) & ~(size_t)15) + 64;
    hipLaunchKernelGGL(nn_l2_kernel, dim3(256), dim3(256), lds, st, q, n, b, m, d, w.fb_list, w.fb_count, nn, d2);
    VFM_CHECK_LAUNCH("nn_l2_kernel(fallback)");
    return VFM_OK;
}


// ---- VFM_MATCH_NARROW (match_l2_narrow.hip): [evaluation counters | max_bits | forward | reverse]; pairs: the reverse direction has
// the n matched map rows as queries and a as map, and the filter's arrays follow
inline bool l2_narrow(int d) { return d >= 1 && d <= VFM_L2_NARROW_MAX_D; }
struct L2NarrowWs {
    unsigned long long* evals;   // [0] forward, [1] reverse (first in the workspace: vfm_debug_l2_narrow_evals)
    unsigned* max_bits;
    void* fwd;
    void* rev;
    int64_t* nn_ab;   // pairs only
    int64_t* nn_rev;
    int* qperm;
    size_t bytes;
};
// reverse: 0 = none, 1 = every row of b among a (vfm_match_mutual_l2), 2 = the n matched rows of b among a + the filter (vfm_match_mutual_pairs)
inline L2NarrowWs carve_l2_narrow(void* p, int64_t n, int64_t m, int d, int reverse) {
    VfmCarver c(p);
    L2NarrowWs w;
    w.evals = c.take<unsigned long long>(32);
    w.max_bits = c.take<unsigned>(64);
    w.fwd = c.take<unsigned char>(l2n_dir_bytes(n, m, d));
    w.rev = nullptr;
    w.nn_ab = w.nn_rev = nullptr;
    w.qperm = nullptr;
    if (reverse == 1) w.rev = c.take<unsigned char>(l2n_dir_bytes(m, n, d));
    if (reverse == 2) {
        w.rev = c.take<unsigned char>(l2n_dir_bytes(n, n, d));
        w.nn_ab = c.take<int64_t>((size_t)n);
        w.nn_rev = c.take<int64_t>((size_t)n);
        w.qperm = c.take<int>((size_t)n);
    }
    w.bytes = c.used();
    return w;
}
// the common scale of both sets, and the counters cleared
int l2_narrow_begin(const float* a, int64_t n, const float* b, int64_t m, int d, const L2NarrowWs& w, hipStream_t st) {
    // (the counters' 256 bytes and max_bits are neighbours in the carved layout: one fill)
    VFM_CHECK_HIP(hipMemsetAsync(w.evals, 0, (size_t)(reinterpret_cast<unsigned char*>(w.max_bits) - reinterpret_cast<unsigned char*>(w.evals)) + sizeof(unsigned), st));
    hipLaunchKernelGGL(l2_maxnorm2_kernel, dim3((unsigned)((n + 3) / 4 + (m + 3) / 4)), dim3(256), 0, st, a, n, b, m, d, w.max_bits);
    VFM_CHECK_LAUNCH("l2_maxnorm2_kernel");
    return VFM_OK;
}

// ---- int8 Euclidean search (see the block comment above match_select_l2_kernel)
inline bool l2_i8(int d) { return i8_capable(d); }

struct L2SortedOperand {   // an operand prepared as the MAP of an int8 Euclidean search: sorted by norm
    float* ss;        // [rows] fp32 sum of squares (original order)
    unsigned* keys;   // [rows] the same as sortable bits
    unsigned* keys_s; // [rows] sorted
    int* iota;        // [rows]
    int* perm;        // [rows] sorted position -> original row
    float* bn;        // [rows_pad] scaled norm per sorted position
    float2* lohi;     // [chunks]
    void* prep;       // prepared operand (int8 image of the sorted rows)
};
struct L2I8Ws {
    unsigned* max_bits;
    void* cub;
    size_t cub_bytes;
    L2SortedOperand B;      // b as map (forward)
    float* ss_a;            // [n]
    float* qn_a;            // [npad]
    void* prep_aq;          // a as queries
    void* search_f;         // forward search workspace (n, m)
    // reverse direction of the mutual filter: queries = b[nn_ab[i]], map = a sorted
    L2SortedOperand A;
    int* qperm;             // [n] (int) nn_ab
    float* ss_bq;           // [n]
    float* qn_bq;           // [npad]
    void* prep_bq;
    void* search_r;         // (n, n)
    int64_t* nn_ab;         // [n] when the caller does not want it
    int64_t* nn_rev;        // [n]
    size_t bytes;
};
inline size_t l2_cub_bytes(int64_t rows) {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (unsigned*)nullptr, (unsigned*)nullptr, (int*)nullptr, (int*)nullptr, (int)rows, 0, 32);
    return b;
}
inline void carve_sorted(VfmCarver& c, L2SortedOperand& o, int64_t rows, int d) {
    const int64_t rp = rows_padded(rows);
    o.ss = c.take<float>((size_t)rows);
    o.keys = c.take<unsigned>((size_t)rows);
    o.keys_s = c.take<unsigned>((size_t)rows);
    o.iota = c.take<int>((size_t)rows);
    o.perm = c.take<int>((size_t)rows);
    o.bn = c.take<float>((size_t)rp);
    o.lohi = c.take<float2>((size_t)(rp / CHUNK_ROWS));
    o.prep = c.take<unsigned char>(vfm_match_prepared_bytes(rows, d));
}
// reverse: 0 = forward direction only, 1 = + the reverse direction restricted to the n matched rows (vfm_match_mutual_pairs)
inline L2I8Ws carve_l2i8(void* p, int64_t n, int64_t m, int d, int reverse) {
    VfmCarver c(p);
    L2I8Ws w;
    w.max_bits = c.take<unsigned>(64);
    w.cub_bytes = l2_cub_bytes(m > n ? m : n);
    w.cub = c.take<unsigned char>(w.cub_bytes);
    carve_sorted(c, w.B, m, d);
    w.ss_a = c.take<float>((size_t)n);
    w.qn_a = c.take<float>((size_t)rows_padded(n));
    w.prep_aq = c.take<unsigned char>(vfm_match_prepared_bytes(n, d));
    w.search_f = c.take<unsigned char>(carve_search(nullptr, n, m).bytes);
    w.nn_ab = c.take<int64_t>((size_t)n);
    w.nn_rev = nullptr;
    if (reverse) {
        const int64_t nq = n;   // queries of the reverse search: the matched map rows
        carve_sorted(c, w.A, n, d);
        w.qperm = c.take<int>((size_t)n);
        w.ss_bq = c.take<float>((size_t)n);
        w.qn_bq = c.take<float>((size_t)rows_padded(nq));
        w.prep_bq = c.take<unsigned char>(vfm_match_prepared_bytes(nq, d));
        w.search_r = c.take<unsigned char>(carve_search(nullptr, nq, n).bytes);
        w.nn_rev = c.take<int64_t>((size_t)n);
    }
    w.bytes = c.used();
    return w;
}

// sort `rows` rows of x by norm and build the int8 image of the sorted rows (o.ss must hold the sums of squares already)
int l2i8_prepare_sorted(const float* x, int64_t rows, int d, const L2I8Ws& w, const L2SortedOperand& o, hipStream_t st) {
    const unsigned g = (unsigned)((rows + 255) / 256);
    hipLaunchKernelGGL(l2i8_iota_kernel, dim3(g), dim3(256), 0, st, o.iota, (const float*)o.ss, o.keys, rows);
    size_t tb = w.cub_bytes;
    VFM_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(w.cub, tb, o.keys, o.keys_s, o.iota, o.perm, (int)rows, 0, 32, st));
    const int64_t rp = rows_padded(rows);
    hipLaunchKernelGGL(l2i8_norms_kernel, dim3((unsigned)((rp + 255) / 256)), dim3(256), 0, st, (const unsigned*)o.keys_s, rows, rp,
                       (const unsigned*)w.max_bits, o.bn, o.lohi);
    VFM_CHECK_LAUNCH("l2i8 sort / norms");
    return do_prepare_perm(x, rows, o.perm, d, o.prep, st);
}

// one direction: query i = row (qperm ? qperm[i] : i) of qx, among the rows of bx whose sorted image is B
int l2i8_search(const float* qx, const int* qperm, int64_t n, const float* qn, void* qprep, const float* bx, int64_t m,
                const L2SortedOperand& B, int d, int64_t* nn, double* d2, void* ws, hipStream_t st) {
    Prepared Q = carve_prepared(qprep, n, d);
    Prepared P = carve_prepared(B.prep, m, d);
    SearchWs w = carve_search(ws, n, m);
    CoarseArgs a = coarse_args(Q, P, w, n, m);
    SearchPlan plan;   // the int8 pass with best-score records at every size: no fallback of resolve_search applies
    plan.pass = PASS_I8;
    plan.kind = VFM_RECORDS_BEST;
    CoarseLaunch launch;
    VFM_TRY(resolve_coarse(launch, plan, d, n, m, false, vfm_compute_units()));
    VFM_CHECK_HIP(hipMemsetAsync(w.fb_count, 0, search_zero_bytes(n, m), st));
    a.Qh = Q.tiles8;
    a.Bh = P.tiles8;
    a.ib = I8Bounds{Q.err, Q.gstep, P.gstep, P.gerr, 0};
    if (int rc = launch_coarse(launch, a, st)) return rc;
    const bool use_bins = n >= 4 * (int64_t)a.nchunks;
    const int chunk_lds = (size_t)a.nchunks * sizeof(float4) <= 63 * 1024;
    const float slack = (float)(d + 16) * 2.3841858e-7f;   // (d + 16) 2^-22: the fp32 roundings of the norms and of the evaluation
    hipLaunchKernelGGL(match_select_l2_kernel, dim3((unsigned)a.nq_tiles), dim3(64 * SELECT_L2_WAVES),
                       chunk_lds ? (size_t)a.nchunks * sizeof(float4) : 0, st, reinterpret_cast<const unsigned*>(w.partials), a.nchunks, n,
                       a.ib, qn, (const float2*)B.lohi, slack, a.first_pad_chunk, chunk_lds, w.qmax, w.cand_cnt, w.cand, w.cap, w.fb_count,
                       w.fb_list, use_bins ? w.bin_cnt : (unsigned*)nullptr, use_bins ? w.bins : (int*)nullptr, w.bin_cap);
    VFM_CHECK_LAUNCH("match_select_l2_kernel");
    if (int rc = launch_i8_rescans(w, a, Q, P, n, m, d, use_bins, L2Terms{qn, (const float*)B.bn, slack}, st)) return rc;
    hipLaunchKernelGGL(l2i8_rescore_kernel, dim3((unsigned)((n + L2R_QUERIES - 1) / L2R_QUERIES)), dim3(256), 0, st, qx, bx, n, m, d,
                       (const int*)w.cand_cnt, (const unsigned*)w.cand, w.cap, (const int*)B.perm, qperm, nn, d2);
    VFM_CHECK_LAUNCH("l2i8_rescore_kernel");
    const size_t lds = (((size_t)d * 4 + 15) & ~(size_t)15) + 64;
    hipLaunchKernelGGL(nn_l2_kernel, dim3(256), dim3(256), lds, st, qx, n, bx, m, d, (const int*)w.fb_list, (const int*)w.fb_count, nn, d2,
                       qperm);
    VFM_CHECK_LAUNCH("nn_l2_kernel(fallback)");
    return VFM_OK;
}

// forward direction a -> b on the int8 pass (nn_ab, d2_ab); leaves ss_a / the common scale behind for the reverse direction
int l2i8_forward(const float* a, int64_t n, const float* b, int64_t m, int d, const L2I8Ws& w, int64_t* nn_ab, double* d2_ab,
                 hipStream_t st) {
    VFM_CHECK_HIP(hipMemsetAsync(w.max_bits, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(l2i8_sumsq_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, a, n, d, (const int*)nullptr, w.ss_a, w.max_bits);
    hipLaunchKernelGGL(l2i8_sumsq_kernel, dim3((unsigned)((m + 15) / 16)), dim3(256), 0, st, b, m, d, (const int*)nullptr, w.B.ss, w.max_bits);
    VFM_CHECK_LAUNCH("l2i8_sumsq_kernel");
    if (int rc = l2i8_prepare_sorted(b, m, d, w, w.B, st)) return rc;
    const int64_t np = rows_padded(n);
    hipLaunchKernelGGL(l2i8_norms_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const unsigned*>(w.ss_a), n,
                       np, (const unsigned*)w.max_bits, w.qn_a, (float2*)nullptr);
    if (int rc = do_prepare_perm(a, n, nullptr, d, w.prep_aq, st)) return rc;
    return l2i8_search(a, nullptr, n, w.qn_a, w.prep_aq, b, m, w.B, d, nn_ab, d2_ab, w.search_f, st);
}

}  // namespace vfmm

using namespace vfmm;

VFM_EXPORT size_t vfm_match_mutual_l2_workspace_bytes(int64_t n, int64_t m, int d, int prec_mode, int mutual) {
    if (prec_mode == VFM_MATCH_NARROW) return (l2_narrow(d) && n > 0 && m > 0) ? carve_l2_narrow(nullptr, n, m, d, mutual != 0).bytes : 256;
    if (prec_mode == VFM_MATCH_EXACT || l2_padded_k(d) == 0 || n <= 0 || m <= 0) return 256;
    // int8-capable widths: the forward direction runs the int8 pass (its workspace sits behind the fp16 path's, which still
    // serves the full reverse direction nn_ba)
    return carve_l2(nullptr, n, m, d, mutual != 0).bytes + (l2_i8(d) ? carve_l2i8(nullptr, n, m, d, 0).bytes : 0);
}

VFM_EXPORT size_t vfm_match_mutual_pairs_workspace_bytes(int64_t n, int64_t m, int d) {
    if (n <= 0 || m <= 0 || d <= 0) return 256;
    if (l2_i8(d)) return carve_l2i8(nullptr, n, m, d, 1).bytes;
    if (l2_narrow(d)) return carve_l2_narrow(nullptr, n, m, d, 2).bytes;
    // other widths: nn_ab / nn_ba by vfm_match_mutual_l2 (FAST where it exists) + the filter
    return vfm_align_up((size_t)n * sizeof(int64_t), 256) * 2 + vfm_align_up((size_t)m * sizeof(int64_t), 256) + 512 +
           vfm_match_mutual_l2_workspace_bytes(n, m, d, l2_padded_k(d) ? VFM_MATCH_FAST : VFM_MATCH_EXACT, 1);
}

VFM_EXPORT int vfm_match_mutual_pairs(const float* a, int64_t n, const float* b, int64_t m, int d, int64_t* idx0_out,
                                      int64_t* idx1_out, int64_t* count_out, int64_t* nn_ab_out, double* d2_ab_out, void* ws,
                                      size_t ws_bytes, vfm_stream_t stream) {
    VFM_CHECK_ARG(n > 0 && m > 0 && d > 0 && a && b && idx0_out && idx1_out && count_out && ws, "mutual_pairs: bad arguments");
    VFM_CHECK_ARG(m < (1ll << 31) - 256 && n < (1ll << 31) - 256, "mutual_pairs: more than 2^31 rows");
    if (ws_bytes < vfm_match_mutual_pairs_workspace_bytes(n, m, d)) return vfm_fail(VFM_EWORKSPACE, "mutual_pairs: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (l2_narrow(d)) {
        // both directions on the f32 MFMA (match_l2_narrow.hip); the reverse one restricted to what the filter reads: queries = the
        // matched map rows b[nn_ab[i]], map = a
        const L2NarrowWs w = carve_l2_narrow(ws, n, m, d, 2);
        int64_t* nn_ab = nn_ab_out ? nn_ab_out : w.nn_ab;
        if (int rc = l2_narrow_begin(a, n, b, m, d, w, st)) return rc;
        if (int rc = l2n_search(a, nullptr, n, b, m, d, w.max_bits, nn_ab, d2_ab_out, w.fwd, w.evals, st)) return rc;
        hipLaunchKernelGGL(l2i8_to_int_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const int64_t*)nn_ab, w.qperm, n);
        if (int rc = l2n_search(b, w.qperm, n, a, n, d, w.max_bits, w.nn_rev, nullptr, w.rev, w.evals + 1, st)) return rc;
        hipLaunchKernelGGL(l2_mutual_pairs_kernel, dim3(1), dim3(1024), 0, st, (const int64_t*)nn_ab, (const int64_t*)w.nn_rev, n, idx0_out,
                           idx1_out, count_out);
        VFM_CHECK_LAUNCH("l2_mutual_pairs_kernel");
        return VFM_OK;
    }
    if (!l2_i8(d)) {
        VfmCarver c(ws);
        int64_t* nn_ab = c.take<int64_t>((size_t)n);
        int64_t* nn_ba = c.take<int64_t>((size_t)m);
        const int prec = l2_padded_k(d) ? VFM_MATCH_FAST : VFM_MATCH_EXACT;
        const size_t rest = vfm_match_mutual_l2_workspace_bytes(n, m, d, prec, 1);
        int64_t* nn_rev_buf = c.take<int64_t>((size_t)n);
        void* sub = c.take<unsigned char>(rest);
        if (int rc = vfm_match_mutual_l2(a, n, b, m, d, prec, nn_ab, d2_ab_out, nn_ba, sub, rest, stream)) return rc;
        int64_t* nn_rev = nn_rev_buf;   // nn_rev[i] = nn_ba[nn_ab[i]]: what the filter compares with i
        hipLaunchKernelGGL(l2_gather_rev_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const int64_t*)nn_ab,
                           (const int64_t*)nn_ba, n, nn_rev);
        hipLaunchKernelGGL(l2_mutual_pairs_kernel, dim3(1), dim3(1024), 0, st, (const int64_t*)nn_ab, (const int64_t*)nn_rev, n, idx0_out,
                           idx1_out, count_out);
        VFM_CHECK_LAUNCH("l2_mutual_pairs_kernel");
        if (nn_ab_out) VFM_CHECK_HIP(hipMemcpyAsync(nn_ab_out, nn_ab, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        return VFM_OK;
    }
    L2I8Ws w = carve_l2i8(ws, n, m, d, 1);
    int64_t* nn_ab = nn_ab_out ? nn_ab_out : w.nn_ab;
    if (int rc = l2i8_forward(a, n, b, m, d, w, nn_ab, d2_ab_out, st)) return rc;
    // reverse, restricted to what the filter reads: queries = the matched map rows b[nn_ab[i]], map = a sorted by norm
    const unsigned g = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(l2i8_to_int_kernel, dim3(g), dim3(256), 0, st, (const int64_t*)nn_ab, w.qperm, n);
    hipLaunchKernelGGL(l2i8_sumsq_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, b, n, d, (const int*)w.qperm, w.ss_bq,
                       (unsigned*)nullptr);
    const int64_t np = rows_padded(n);
    hipLaunchKernelGGL(l2i8_norms_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const unsigned*>(w.ss_bq), n,
                       np, (const unsigned*)w.max_bits, w.qn_bq, (float2*)nullptr);
    VFM_CHECK_HIP(hipMemcpyAsync(w.A.ss, w.ss_a, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (int rc = l2i8_prepare_sorted(a, n, d, w, w.A, st)) return rc;
    if (int rc = do_prepare_perm(b, n, w.qperm, d, w.prep_bq, st)) return rc;
    if (int rc = l2i8_search(b, w.qperm, n, w.qn_bq, w.prep_bq, a, n, w.A, d, w.nn_rev, nullptr, w.search_r, st)) return rc;
    hipLaunchKernelGGL(l2_mutual_pairs_kernel, dim3(1), dim3(1024), 0, st, (const int64_t*)nn_ab, (const int64_t*)w.nn_rev, n, idx0_out,
                       idx1_out, count_out);
    VFM_CHECK_LAUNCH("l2_mutual_pairs_kernel");
    return VFM_OK;
}

VFM_EXPORT int vfm_match_mutual_l2(const float* a, int64_t n, const float* b, int64_t m, int d, int prec_mode,
                                   int64_t* nn_ab, double* d2_ab, int64_t* nn_ba, void* ws, size_t ws_bytes,
                                   vfm_stream_t stream) {
    VFM_CHECK_ARG(n > 0 && m > 0 && d > 0 && a && b && nn_ab, "mutual_l2: bad arguments");
    VFM_CHECK_ARG(prec_mode == VFM_MATCH_FAST || prec_mode == VFM_MATCH_EXACT || prec_mode == VFM_MATCH_NARROW, "mutual_l2: unknown prec_mode %d",
                  prec_mode);
    VFM_CHECK_ARG(prec_mode != VFM_MATCH_NARROW || l2_narrow(d), "mutual_l2: VFM_MATCH_NARROW serves d <= %d (VFM_L2_NARROW_MAX_D), got d = %d",
                  VFM_L2_NARROW_MAX_D, d);
    VFM_CHECK_ARG(m < (1ll << 31) - 256 && n < (1ll << 31) - 256, "mutual_l2: more than 2^31 rows");
    // (checked on every path, the all-pairs one included: a caller sizes the workspace by vfm_match_mutual_l2_workspace_bytes alone)
    if (ws_bytes < vfm_match_mutual_l2_workspace_bytes(n, m, d, prec_mode, nn_ba != nullptr))
        return vfm_fail(VFM_EWORKSPACE, "mutual_l2: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (prec_mode == VFM_MATCH_NARROW) {
        VFM_CHECK_ARG(ws, "mutual_l2: workspace required in NARROW mode");
        const L2NarrowWs w = carve_l2_narrow(ws, n, m, d, nn_ba != nullptr);
        if (int rc = l2_narrow_begin(a, n, b, m, d, w, st)) return rc;
        if (int rc = l2n_search(a, nullptr, n, b, m, d, w.max_bits, nn_ab, d2_ab, w.fwd, w.evals, st)) return rc;
        if (nn_ba)
            if (int rc = l2n_search(b, nullptr, m, a, n, d, w.max_bits, nn_ba, nullptr, w.rev, w.evals + 1, st)) return rc;
        return VFM_OK;
    }
    const int kp = l2_padded_k(d);
    if (prec_mode == VFM_MATCH_EXACT || kp == 0) {
        // all-pairs fp64 (also the path for descriptors wider than 768)
        const size_t lds = (((size_t)d * 4 + 15) & ~(size_t)15) + 64;
        hipLaunchKernelGGL(nn_l2_kernel, dim3((unsigned)(n < 8192 ? n : 8192)), dim3(256), lds, st, a, n, b, m, d,
                           (const int*)nullptr, (const int*)nullptr, nn_ab, d2_ab);
        if (nn_ba)
            hipLaunchKernelGGL(nn_l2_kernel, dim3((unsigned)(m < 8192 ? m : 8192)), dim3(256), lds, st, b, m, a, n, d,
                               (const int*)nullptr, (const int*)nullptr, nn_ba, (double*)nullptr);
        VFM_CHECK_LAUNCH("nn_l2_kernel");
        return VFM_OK;
    }
    VFM_CHECK_ARG(ws, "mutual_l2: workspace required in FAST mode");
    L2Ws w = carve_l2(ws, n, m, d, nn_ba != nullptr);
    VFM_CHECK_HIP(hipMemsetAsync(w.max_bits, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(l2_maxnorm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, a, n, d, w.max_bits);
    hipLaunchKernelGGL(l2_maxnorm_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, b, m, d, w.max_bits);
    VFM_CHECK_LAUNCH("l2_maxnorm_kernel");
    if (l2_i8(d)) {
        // the a -> b direction on the int8 pass (its workspace sits behind the fp16 path's).  The full b -> a direction stays on
        // the fp16 pass: its queries are mostly map rows WITHOUT a near neighbour in the scan, and the int8 bounds -- 16x wider than
        // the fp16 window -- leave each of them ~20 candidate chunks on a 157-chunk scan (measured at 20 000 x 200 000: 12.3 ms
        // both ways on int8 against 11.8 with the fp16 reverse; 247 against 35 ms at d = 768).  find_correspondences' mutual
        // filter needs the reverse direction only at the matched rows: vfm_match_mutual_pairs runs both directions on int8.
        L2I8Ws w8 = carve_l2i8(static_cast<unsigned char*>(ws) + w.bytes, n, m, d, 0);
        if (int rc = l2i8_forward(a, n, b, m, d, w8, nn_ab, d2_ab, st)) return rc;
    } else {
        if (int rc = l2_prepare(a, n, d, kp, w.max_bits, 0, w.prep[0], st)) return rc;
        if (int rc = l2_prepare(b, m, d, kp, w.max_bits, 1, w.prep[1], st)) return rc;
        if (int rc = l2_search(a, w.prep[0], n, b, w.prep[1], m, d, kp, nn_ab, d2_ab, w.search[0], st)) return rc;
    }
    if (nn_ba) {
        if (int rc = l2_prepare(b, m, d, kp, w.max_bits, 0, w.prep[2], st)) return rc;
        if (int rc = l2_prepare(a, n, d, kp, w.max_bits, 1, w.prep[3], st)) return rc;
        if (int rc = l2_search(b, w.prep[2], m, a, w.prep[3], n, d, kp, nn_ba, nullptr, w.search[1], st)) return rc;
    }
    return VFM_OK;
}


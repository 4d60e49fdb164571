// match_finish.hip -- from coarse records to the oracle's answer: candidate selection
// (match_select_kernel and its forms laid out for the sweep: _top2, _half, _best; match_bin_survivors_kernel), int8 rescan of
// candidate chunks (match_rescan_kernel), fp32 refinement of crowded lists (match_refine_kernel, match_filter_refine_kernel), the
// exact fp64 decision (match_rescore_kernel), the all-pairs fp64 kernel (EXACT mode and overflow fallback) and the cosine threshold +
// compaction (VoxelHashMap.cpp:501-511, 587-600).
// The steps the selection kernels share -- bounds, staging, sweep, placement, epilogue: match_select.h.
// The fp64 chains, the tie rule and the arg-max of the decision kernels: match_exact.h.
#include "match_exact.h"
#include "match_select.h"

namespace vfmm {
namespace {

// ---------------------------------------------------------------------------------------------
// selection: coarse max per query and the candidate chunks inside the error window
// cand entry: (chunk << 8) | (rescan << 7) | local row
// ---------------------------------------------------------------------------------------------
constexpr int SELECT_GROUPS = 16;  // waves per 64 queries: enough loads in flight to saturate HBM on the sweep
__global__ __launch_bounds__(64 * SELECT_GROUPS) void match_select_kernel(const uint2* __restrict__ partials, int nchunks, int npad,
                                                           int64_t n, int first_pad_chunk,
                                                           const unsigned* __restrict__ qmax,
                                                           const float* __restrict__ invq, float window,
                                                           I8Bounds ib, float gate, int chunk_lds, int* __restrict__ cand_cnt,
                                                           unsigned* __restrict__ cand, int cap, int* __restrict__ fb_count,
                                                           int* __restrict__ fb_list, int stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char select_smem[];  // int8 records: the chunks' (step, max E)
    __shared__ int lcnt[64];
    __shared__ int lresc[64];     // int8 top-2 records: whole-chunk entries among them
    __shared__ unsigned lub[64];  // int8 records: float_key of the largest upper bound over the query's chunks
    const int qq = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * 64 + qq;
    if (g == 0) {
        lcnt[qq] = 0;
        lresc[qq] = 0;
        lub[qq] = 0u;
    }
    float2* lchunk = reinterpret_cast<float2*>(select_smem);
    // every thread walks ~nchunks / 16 chunks: their (step, max E) once per workgroup into LDS
    if (ib.qerr && chunk_lds) stage_chunk_bounds<64 * SELECT_GROUPS>(lchunk, ib, nchunks);
    __syncthreads();
    if (ib.qerr) {
        // Records of the int8 pass: integer scores in the units of (query group step) x (map chunk step).  In exact score
        // units, with A = (1 + 2^-13) E_q and B_c = (1 + 2^-13 + E_q) max E of chunk c (prep_chunk_kernel):
        //     lower_c = s_q s_c S(c) - A - B_c  <=  best exact score of chunk c  <=  s_q s_c S(c) + A + B_c = upper_c
        // (S(c): the chunk's best integer score, exact).
        // qlow = max over the un-padded chunks of lower_c, a lower bound of the query's exact maximum, comes from the coarse
        // kernel (qmax holds its float_key).  Every chunk with upper_c >= qlow is a candidate:
        // the oracle's arg-max row is inside one of them, and match_refine_kernel finds the rows (int8 rescan, then fp32).
        // fp32 evaluation of the bounds: three roundings on magnitudes <= 2 -- 1e-6 of slack covers them.
        // These two branches are the A/B reference ("coarse_variant" 20) of match_select_top2_kernel and match_select_best_kernel.
        // Their sweeps keep the text they had before match_select.h, `bound` and `up1` being chunk_upper's expression written out:
        // the compiler unswitches these loops on chunk_lds as they stand; through sweep_query_records, chunk_bounds and chunk_upper
        // the finish call of a top-2 search at C2 took 0.198 ms instead of 0.144, and of the two wordings of the best-score loop
        // that were compiled once per case one lost 14 % on int8 bounds and the other 1.4 - 3.4 % on fp6 bounds
        // (profiles/select_refactor.md).  A change to chunk_upper has to be made here too.
        const float sq = ib.qstep[q >> 7];
        const QueryBound qb = query_bound(ib.qerr[q]);
        const float A = qb.A, mult = qb.mult, slack = SELECT_SLACK;
        const float qlow = key_float(qmax[q]);  // -Inf: no un-padded chunk exists -> every chunk is a candidate
        float maxup = -__builtin_inff();
        if (ib.top2) {
            // packed top-2 records (uint2 [chunk][npad], as the fp16 pass writes them): the best row's index rides in the low
            // 7 bits, so a candidate chunk whose SECOND-best score cannot reach qlow is a single-row entry and needs no rescan
            for (int cb = g; cb < nchunks; cb += 8 * SELECT_GROUPS) {
                uint2 rec[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int c = cb + SELECT_GROUPS * u;
                    rec[u] = (c < nchunks) ? partials[((size_t)(q >> 5) * nchunks + c) * 32 + (q & 31)] : make_uint2(0u, 0u);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int c = cb + SELECT_GROUPS * u;
                    if (c >= nchunks) continue;
                    const float2 cb2 = chunk_lds ? lchunk[c] : make_float2(ib.bstep[c], ib.berr[c]);
                    const float sc = sq * cb2.x, bound = A + mult * cb2.y + slack;
                    const float up1 = sc * (float)((int)(rec[u].x | 127u) - I8_OFFSET) + bound;
                    maxup = fmaxf(maxup, up1);
                    if (up1 >= qlow) {
                        const int slot = atomicAdd(&lcnt[qq], 1);
                        const float up2 = sc * (float)((int)(rec[u].y | 63u) - I8_OFFSET) + bound;
                        const unsigned rescan = (up2 >= qlow || c >= first_pad_chunk) ? 1u : 0u;
                        if (rescan) atomicAdd(&lresc[qq], 1);
                        if (slot < cap && q < n) cand[(size_t)q * cap + slot] = ((unsigned)c << 8) | (rescan << 7) | (rec[u].x & 127u);
                    }
                }
            }
        } else {
        // [query tile][chunk][32]: best integer score (+ 2^30) of the chunk for the tile's 32 queries
        const unsigned* best = reinterpret_cast<const unsigned*>(partials) + (size_t)(q >> 5) * nchunks * 32 + (q & 31);
        for (int cb = g; cb < nchunks; cb += 8 * SELECT_GROUPS) {
            unsigned rec[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int c = cb + SELECT_GROUPS * u;
                rec[u] = (c < nchunks) ? best[(size_t)c * 32] : 0u;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int c = cb + SELECT_GROUPS * u;
                if (c >= nchunks) continue;
                const float2 cb2 = chunk_lds ? lchunk[c] : make_float2(ib.bstep[c], ib.berr[c]);
                const float sc = sq * cb2.x, bound = A + mult * cb2.y + slack;
                const float up1 = sc * (float)((int)rec[u] - I8_OFFSET) + bound;
                maxup = fmaxf(maxup, up1);
                if (up1 >= qlow) {  // (zero-padded rows score exactly 0: a padded chunk is a candidate only if 0 is inside the window)
                    const int slot = atomicAdd(&lcnt[qq], 1);
                    // (the records hold values only: which rows of the chunk reach qlow is found by match_refine_kernel's
                    // int8 rescan -- every entry is a whole-chunk entry)
                    if (slot < cap && q < n) cand[(size_t)q * cap + slot] = ((unsigned)c << 8) | 128u;
                }
            }
        }
        }
        atomicMax(&lub[qq], float_key(maxup));
    } else {
    // qmax = best coarse score over the un-padded chunks (value bits; accumulated by the coarse
    // kernel).  Chunks >= first_pad_chunk contain zero-padded map rows whose coarse score (exactly
    // 2.0) is meaningless: they do not take part in the maximum and are always rescanned exactly.
    const unsigned m = qmax[q];
    // m == 0: no un-padded chunk exists (map smaller than one chunk) -> every chunk is a candidate
    const float thr_f = __uint_as_float(m) - window;
    const unsigned thr = (m == 0u) ? 0u : (__float_as_uint(thr_f) & ~127u);
    // HBM-bound sweep over this query's records: 8 independent loads in flight per thread
    for (int cb = g; cb < nchunks; cb += 8 * SELECT_GROUPS) {
        uint2 rec[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = cb + SELECT_GROUPS * u;
            rec[u] = (c < nchunks) ? partials[(size_t)c * npad + q] : make_uint2(0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = cb + SELECT_GROUPS * u;
            if (c < nchunks && (rec[u].x | 127u) >= thr) {
                const int slot = atomicAdd(&lcnt[qq], 1);
                if (slot < cap && q < n) {  // sparse: straight to the query's global list
                    const unsigned rescan = (((rec[u].y | 63u) >= thr) || c >= first_pad_chunk) ? 1u : 0u;
                    cand[(size_t)q * cap + slot] = ((unsigned)c << 8) | (rescan << 7) | (rec[u].x & 127u);
                }
            }
        }
    }
    }
    __syncthreads();
    // load figure of the int8 pass: candidate chunks that match_refine_kernel will rescan; one atomic per workgroup
    if (g == 0 && ib.qerr)
        add_load_figure(fb_count, q < n ? bounded_query_load(invq[q], key_float(lub[qq]) < gate, lcnt[qq], ib.top2 ? lresc[qq] : lcnt[qq], cap) : 0);
    if (g == 0 && q < n) {
        const int cnt = lcnt[qq];
        close_query(SelectClose{invq, cand_cnt, fb_count, fb_list, stats}, q, cnt, ib.qerr && key_float(lub[qq]) < gate, cnt > cap, cnt);
    }
}

// Packed top-2 records of the int8 pass ([query tile][chunk][32], 8 bytes each): the int8 / top-2 branch of match_select_kernel --
// the same pieces of match_select.h, hence the same decision -- in the tile kernels' sweep with two queries per lane.  Queries that
// provably end below the gate record nothing (dead_queries).
constexpr int SELECT_TOP2_WAVES = 8;
__global__ __launch_bounds__(64 * SELECT_TOP2_WAVES) void match_select_top2_kernel(
    const uint2* __restrict__ recs, int nchunks, int64_t n, int first_pad_chunk, const unsigned* __restrict__ qmax,
    const float* __restrict__ invq, I8Bounds ib, float gate, int chunk_lds, int* __restrict__ cand_cnt, unsigned* __restrict__ cand,
    int cap, int* __restrict__ fb_count, int* __restrict__ fb_list, int stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char select_smem[];  // the chunks' (step, max E)
    __shared__ int lcnt[32];
    __shared__ int lresc[32];     // whole-chunk entries among them
    __shared__ unsigned lub[32];  // float_key of the largest upper bound over the query's chunks
    __shared__ unsigned lmaxe;
    __shared__ int ldead[32];
    const int qt = blockIdx.x;
    if (threadIdx.x < 32) {
        lcnt[threadIdx.x] = 0;
        lresc[threadIdx.x] = 0;
        lub[threadIdx.x] = 0u;
    }
    if (threadIdx.x == 0) lmaxe = 0u;
    __syncthreads();
    float2* lchunk = reinterpret_cast<float2*>(select_smem);
    if (chunk_lds) raise_workgroup_max(&lmaxe, stage_chunk_bounds<64 * SELECT_TOP2_WAVES>(lchunk, ib, nchunks));
    __syncthreads();
    const int lq = TileLane<2>().lq;
    const int64_t q0 = (int64_t)qt * 32 + lq;   // the lane's two queries
    const float sq = ib.qstep[q0 >> 7];
    QueryBound qb[2];
    float qlow[2], maxup[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        qb[j] = query_bound(ib.qerr[q0 + j]);
        qlow[j] = key_float(qmax[q0 + j]);
        maxup[j] = -__builtin_inff();
    }
    const uint4* tile = reinterpret_cast<const uint4*>(recs + (size_t)qt * nchunks * 32);
    const unsigned deadmask = dead_queries<2>(qb, qlow, chunk_lds ? key_float(lmaxe) : __builtin_inff(), gate, sq, ib, first_pad_chunk,
                                              nchunks, lq, q0, n, invq, ldead, [&](int c, int (&S)[2]) {
                                                  const uint4 r = tile_chunk_records<2>(tile, c);
                                                  S[0] = top2_first_score(r.x);
                                                  S[1] = top2_first_score(r.z);
                                              });
    sweep_tile_records<2, SELECT_TOP2_WAVES>(tile, nchunks, [&](int c, uint4 rec) {
        const float2 cb2 = chunk_bounds(lchunk, chunk_lds, ib, c);
        const float sc = sq * cb2.x;
        const unsigned r1[2] = {rec.x, rec.z}, r2[2] = {rec.y, rec.w};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float up1 = chunk_upper(sc, top2_first_score(r1[j]), qb[j], cb2.y);
            maxup[j] = fmaxf(maxup[j], up1);
            if (up1 >= qlow[j] && !((deadmask >> j) & 1u)) {
                const int slot = atomicAdd(&lcnt[lq + j], 1);
                // the best row's index rides in the low 7 bits: a candidate chunk whose SECOND-best score cannot reach
                // qlow is a single-row entry and needs no rescan
                const float up2 = chunk_upper(sc, top2_second_score(r2[j]), qb[j], cb2.y);
                const unsigned rescan = (up2 >= qlow[j] || c >= first_pad_chunk) ? 1u : 0u;
                if (rescan) atomicAdd(&lresc[lq + j], 1);
                if (slot < cap) cand[(size_t)(q0 + j) * cap + slot] = ((unsigned)c << 8) | (rescan << 7) | (r1[j] & 127u);
            }
        }
        return false;
    });
    raise_query_max<2>(lub, lq, maxup);
    __syncthreads();
    close_tile_queries(
        SelectClose{invq, cand_cnt, fb_count, fb_list, stats}, qt, n, lcnt, true,
        [&](int qq, int64_t q, int cnt) { return bounded_query_load(invq[q], key_float(lub[qq]) < gate, cnt, lresc[qq], cap); },
        [&](int qq, int) { return key_float(lub[qq]) < gate; }, [&](int qq, int cnt) { return cnt > cap || ldead[qq] != 0; },
        [&](int, int cnt) { return cnt; });
}

// Half-width pass (VFM_RECORDS_HALF): the records hold the best integer score of every (query, chunk) over the FIRST d / 2
// columns.  With r_q = |second half of the normalised query|, R_c = max over the chunk's rows of |second half of the row|
// (both rounded up, prep_chunk_kernel) and the quantisation bound A + B_c of the full rows (an upper bound for any subset of
// columns):      best exact score of chunk c  <=  s_q s_c S_half(c) + A + B_c + r_q R_c       (chunk_upper_half)
// A chunk survives for a query iff that bound reaches the gate; the survivors are binned per chunk (or left in the query's
// list) for the full-width int8 rescan, whose hit test is then the gate itself.  A query without survivors provably has no
// match (cand_cnt = -2).  cand == NULL: the probe (vfm_match_search_probe_half), the survivors are only counted.
__global__ __launch_bounds__(64 * 8) void match_select_half_kernel(
    const unsigned* __restrict__ best, int nchunks, int64_t n, const float* __restrict__ invq, I8Bounds ib,
    const float* __restrict__ qrest, const float* __restrict__ grest, float gate, int chunk_lds, int* __restrict__ cand_cnt,
    unsigned* __restrict__ cand, int cap, int* __restrict__ fb_count, int* __restrict__ fb_list, int stats,
    unsigned* __restrict__ bin_cnt, int* __restrict__ bins, int bin_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char select_smem[];  // the chunks' (step, max E) and max |rest|
    __shared__ int lcnt[32];
    __shared__ int lov[32];
    const int qt = blockIdx.x;
    if (threadIdx.x < 32) {
        lcnt[threadIdx.x] = 0;
        lov[threadIdx.x] = 0;
    }
    float2* lchunk = reinterpret_cast<float2*>(select_smem);
    float* lrest = reinterpret_cast<float*>(lchunk + nchunks);
    if (chunk_lds) stage_chunk_bounds<64 * 8>(lchunk, ib, nchunks, [&](int c) { lrest[c] = grest[c]; });
    __syncthreads();
    const int lq = TileLane<4>().lq;
    const int64_t q0 = (int64_t)qt * 32 + lq;   // the lane's four queries (rows of the padded tile always exist)
    const float sq = ib.qstep[q0 >> 7];
    QueryBound qb[4];
    float rq[4];
    unsigned livemask = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        qb[j] = query_bound(ib.qerr[q0 + j]);
        rq[j] = qrest[q0 + j];
        if (q0 + j < n && invq[q0 + j] != 0.0f) livemask |= 1u << j;
    }
    const SelectLists L{bin_cnt, bins, bin_cap, cand, cap};
    sweep_tile_records<4, 8>(
        reinterpret_cast<const uint4*>(best + (size_t)qt * nchunks * 32), nchunks,
        // The guard, early: once four queries of a lane average 4 x HALF_GUARD_PER_QUERY surviving chunks the search is going to
        // take the gate pass anyway (half_guard_kernel) -- raise its flag now, leave a load figure that says so, and stop: on
        // descriptors that are all alike the full sweep (31 million survivors, each a few atomics) took 21 ms.  Every workgroup
        // stops at the flag; the gate pass ignores what the lists hold.
        [&] { return !(cand && __hip_atomic_load(fb_count + HALF_GUARD_FLAG, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0); },
        [&](int c, uint4 rec) {
            if (cand && lcnt[lq] + lcnt[lq + 1] + lcnt[lq + 2] + lcnt[lq + 3] > 16 * HALF_GUARD_PER_QUERY) {
                if (atomicExch(fb_count + HALF_GUARD_FLAG, 1) == 0) atomicExch(fb_count + 5, 0x3FFFFFFF);
                return true;
            }
            const float2 cb2 = chunk_bounds(lchunk, chunk_lds, ib, c);
            const float rb = chunk_lds ? lrest[c] : grest[c];
            const float sc = sq * cb2.x;
            const unsigned r4[4] = {rec.x, rec.y, rec.z, rec.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float up = chunk_upper_half(sc, best_score(r4[j]), qb[j], cb2.y, rq[j], rb);
                if (!(up < gate) && ((livemask >> j) & 1u)) {
                    const int slot = atomicAdd(&lcnt[lq + j], 1);
                    if (!cand) continue;  // probe: the survivors are only counted
                    // (with bins the look at the counter comes first always: a full bin is not touched again)
                    if (bins) place_candidate(L, q0 + j, c, true, &lov[lq + j]);
                    else own_list_entry(L, q0 + j, slot, c);
                }
            }
            return false;
        });
    __syncthreads();
    close_tile_queries(
        SelectClose{invq, cand_cnt, fb_count, fb_list, stats}, qt, n, lcnt, cand != nullptr,
        [&](int, int64_t, int cnt) { return (cnt <= cap || !cand) ? cnt : 0; },   // load figure: surviving chunks
        [&](int, int cnt) { return cnt == 0; },                                  // no chunk can hold a row at the gate
        [&](int, int cnt) { return cnt > cap; }, [&](int qq, int cnt) { return bins ? lov[qq] : cnt; });
}

// VFM_RECORDS_MX6_HALF_FUSED: the fused fp6 half-width kernel (match_coarse_mx6.hip) has tested every (query, chunk) pair against
// the gate itself and left each workgroup's survivors in a slot of the record buffer -- [count, query block, first chunk, overflow]
// + entries (chunk of the slice << 9 | query of the block).  This kernel does the placement match_select_half_kernel does for its
// survivors (place_candidate; the own list's length is cand_cnt itself).  One wave per slot; ~11 000 entries at C2 on
// SURVEY D.2 data (0.56 per query) against the 122 MB sweep of the records this replaces.  With the guard up (a slot overflowed:
// descriptors that are all alike) nothing is placed: match_gatepass_kernel decides every query.
__global__ __launch_bounds__(256) void match_bin_survivors_kernel(const unsigned* __restrict__ surv, int slot_words, const int* __restrict__ fb_count,
                                                                  unsigned* __restrict__ bin_cnt, int* __restrict__ bins, int bin_cap,
                                                                  int* __restrict__ cand_cnt, unsigned* __restrict__ cand, int cap) {
    if (fb_count[HALF_GUARD_FLAG] != 0) return;
    const int nslots = fb_count[MX6_GRID_SLOT];
    const int lane = lane_id(), nwaves = (int)gridDim.x * 4;
    const SelectLists L{bin_cnt, bins, bin_cap, cand, cap};
    for (int sidx = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6); sidx < nslots; sidx += nwaves) {
        const unsigned* slot = surv + (size_t)sidx * slot_words;
        const unsigned cnt = slot[0], qb = slot[1], c0 = slot[2];
        // (round 5: a workgroup of the coarse kernel holds 512 queries -- two 32-query tiles per wave, entries = chunk << 9 | query -- or 768 --
        // three tiles, chunk << 10 | query --; it says which in bits 8 .. of the header's fourth word)
        const bool three = cnt > 0u && (slot[3] >> 8) == 3u;
        const unsigned qshift = three ? 10u : 9u, qper = three ? 768u : 512u;
        for (unsigned i = (unsigned)lane; i < cnt; i += 64u) {
            const unsigned e = slot[4 + i];
            const int chunk = (int)(c0 + (e >> qshift));
            const int64_t q = (int64_t)qb * qper + (int64_t)(e & ((1u << qshift) - 1u));
            place_candidate(L, q, chunk, false, &cand_cnt[q]);
        }
    }
}

// Best-score records of the int8 pass ([query tile][chunk][32], 4 bytes each): the int8 branch of match_select_kernel -- the same
// pieces of match_select.h, hence the same decision -- in the tile kernels' sweep with four queries per lane (the general kernel
// reads two 128-byte pieces per instruction: 103 us for the 125 MB of C2's records; this one is bound by the sweep itself).
constexpr int SELECT_BEST_WAVES = 8;
constexpr int SELECT_BEST_LCAND = 6144;   // candidates of a query tile staged in the LDS (192 per query; beyond: the direct path)
__global__ __launch_bounds__(64 * SELECT_BEST_WAVES) void match_select_best_kernel(
    const unsigned* __restrict__ best, int nchunks, int64_t n, const unsigned* __restrict__ qmax, const float* __restrict__ invq,
    I8Bounds ib, float gate, int chunk_lds, int* __restrict__ cand_cnt, unsigned* __restrict__ cand, int cap,
    int* __restrict__ fb_count, int* __restrict__ fb_list, int stats, unsigned* __restrict__ bin_cnt, int* __restrict__ bins,
    int first_pad_chunk, int bin_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char select_smem[];  // the chunks' (step, max E)
    __shared__ int lcnt[32];      // candidate chunks of the query
    __shared__ int lov[32];       // bins != NULL: those of them that did not fit their chunk's bin (they go to the query's own list)
    __shared__ unsigned lub[32];  // float_key of the largest upper bound over the query's chunks
    __shared__ unsigned lmaxe;    // float_key of the largest max E over the chunks
    __shared__ int ldead[32];     // the query records nothing (dead_queries)
    // The tile's candidates (stage_candidate): 151 us against 70 with the global side inside the sweep at 12 candidate chunks per
    // query (lifted descriptors) and 317 at 46 (the fp6 pass's bounds).
    __shared__ unsigned lcand[SELECT_BEST_LCAND];
    __shared__ int lcand_n;
    const int qt = blockIdx.x;
    if (threadIdx.x < 32) {
        lcnt[threadIdx.x] = 0;
        lov[threadIdx.x] = 0;
        lub[threadIdx.x] = 0u;
    }
    if (threadIdx.x == 0) {
        lmaxe = 0u;
        lcand_n = 0;
    }
    __syncthreads();
    float2* lchunk = reinterpret_cast<float2*>(select_smem);
    unsigned* lhist = reinterpret_cast<unsigned*>(lchunk + nchunks);   // chunk_lds == 2: the tile's candidates per chunk, then the bins' positions
    const bool hist = chunk_lds == 2 && bins != nullptr;
    if (chunk_lds)
        raise_workgroup_max(&lmaxe, stage_chunk_bounds<64 * SELECT_BEST_WAVES>(lchunk, ib, nchunks, [&](int c) {
                                if (hist) lhist[c] = 0u;
                            }));
    __syncthreads();
    const int lq = TileLane<4>().lq;
    const int64_t q0 = (int64_t)qt * 32 + lq;   // the lane's four queries (rows of the padded tile always exist)
    const float sq = ib.qstep[q0 >> 7];
    QueryBound qb[4];
    float qlow[4], maxup[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        qb[j] = query_bound(ib.qerr[q0 + j]);
        qlow[j] = key_float(qmax[q0 + j]);  // -Inf: no un-padded chunk exists -> every chunk is a candidate
        maxup[j] = -__builtin_inff();
    }
    const uint4* tile = reinterpret_cast<const uint4*>(best + (size_t)qt * nchunks * 32);
    const unsigned deadmask = dead_queries<4>(qb, qlow, chunk_lds ? key_float(lmaxe) : __builtin_inff(), gate, sq, ib, first_pad_chunk,
                                              nchunks, lq, q0, n, invq, ldead, [&](int c, int (&S)[4]) {
                                                  const uint4 r = tile_chunk_records<4>(tile, c);
                                                  S[0] = best_score(r.x);
                                                  S[1] = best_score(r.y);
                                                  S[2] = best_score(r.z);
                                                  S[3] = best_score(r.w);
                                              });
    // candidate (query qq of the tile, chunk c): lov counts the own list's entries with bins or without.  crowded: a tile with more
    // than 64 candidate chunks per query looks at the bin's counter first (place_candidate)
    const SelectLists L{bin_cnt, bins, bin_cap, cand, cap};
    auto place = [&](int qq, int c, bool crowded) { place_candidate(L, (int64_t)qt * 32 + qq, c, crowded, &lov[qq]); };
    sweep_tile_records<4, SELECT_BEST_WAVES>(tile, nchunks, [&](int c, uint4 rec) {
        const float2 cb2 = chunk_bounds(lchunk, chunk_lds, ib, c);
        const float sc = sq * cb2.x;
        const unsigned r4[4] = {rec.x, rec.y, rec.z, rec.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float up1 = chunk_upper(sc, best_score(r4[j]), qb[j], cb2.y);
            maxup[j] = fmaxf(maxup[j], up1);
            // (zero-padded rows score exactly 0: a padded chunk is a candidate only if 0 is inside the bounds)
            if (up1 >= qlow[j] && !((deadmask >> j) & 1u)) {
                atomicAdd(&lcnt[lq + j], 1);
                if (!stage_candidate(lcand, &lcand_n, SELECT_BEST_LCAND, lq + j, c)) place(lq + j, c, true);   // the staging buffer is full: placed on the spot
            }
        }
        return false;
    });
    __syncthreads();
    {
        const int ncand = lcand_n < SELECT_BEST_LCAND ? lcand_n : SELECT_BEST_LCAND;
        const bool crowded = lcand_n > 32 * 64;
        if (hist) {
            // One atomic per chunk and tile instead of one per candidate: the tile's candidates are counted per chunk in the LDS (a
            // candidate keeps its rank there: at most 32 queries of a tile share a chunk), the chunk's bin is asked once for that many
            // places, and every candidate takes base + rank.  (920 000 returning atomics on 1564 counters were 40 of the kernel's
            // 105 us on lifted descriptors with a common component; what this form leaves depends on how many of a tile's candidates share their chunks.)
            for (int i = threadIdx.x; i < ncand; i += 64 * SELECT_BEST_WAVES) {
                const unsigned e = lcand[i];
                const unsigned rank = atomicAdd(&lhist[e & 0xFFFFu], 1u);
                lcand[i] = e | (rank << 16);
            }
            __syncthreads();
            constexpr int PU = 4;
            for (int c0 = threadIdx.x; c0 < nchunks; c0 += 64 * SELECT_BEST_WAVES * PU) {
                unsigned want[PU], pos[PU];
#pragma unroll
                for (int u = 0; u < PU; ++u) {
                    const int c = c0 + 64 * SELECT_BEST_WAVES * u;
                    want[u] = c < nchunks ? lhist[c] : 0u;
                    pos[u] = 0u;
                }
                if (crowded) {
#pragma unroll
                    for (int u = 0; u < PU; ++u)
                        if (want[u]) pos[u] = __hip_atomic_load(&bin_cnt[(size_t)(c0 + 64 * SELECT_BEST_WAVES * u) * BIN_CNT_STRIDE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
#pragma unroll
                for (int u = 0; u < PU; ++u)
                    if (want[u] && pos[u] < (unsigned)bin_cap)
                        pos[u] = __hip_atomic_fetch_add(&bin_cnt[(size_t)(c0 + 64 * SELECT_BEST_WAVES * u) * BIN_CNT_STRIDE], want[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                for (int u = 0; u < PU; ++u)
                    if (want[u]) lhist[c0 + 64 * SELECT_BEST_WAVES * u] = pos[u];
            }
            __syncthreads();
            for (int i = threadIdx.x; i < ncand; i += 64 * SELECT_BEST_WAVES) {
                const unsigned e = lcand[i];   // (query << 27) | (rank << 16) | chunk
                const int qq = staged_query(e), c = (int)(e & 0xFFFFu);
                settle_candidate(L, (int64_t)qt * 32 + qq, c, lhist[c] + ((e >> 16) & 31u), &lov[qq]);
            }
        } else
        for (int i = threadIdx.x; i < ncand; i += 64 * SELECT_BEST_WAVES) {
            const unsigned e = lcand[i];
            place(staged_query(e), staged_chunk(e), crowded);
        }
    }
    raise_query_max<4>(lub, lq, maxup);
    __syncthreads();
    close_tile_queries(
        SelectClose{invq, cand_cnt, fb_count, fb_list, stats}, qt, n, lcnt, true,
        [&](int qq, int64_t q, int cnt) { return bounded_query_load(invq[q], key_float(lub[qq]) < gate, cnt, cnt, cap); },
        [&](int qq, int) { return key_float(lub[qq]) < gate; },
        // overflow, or a padded chunk lifted a query past the gate whose candidates were not recorded
        [&](int qq, int cnt) { return cnt > cap || ldead[qq] != 0; }, [&](int qq, int) { return lov[qq]; });
}

// int8 pass, chunk-major rescan (best-score records, many queries per chunk): one workgroup per map chunk scores the chunk's
// 128 rows against every query of the chunk's bin.  The query-major kernel below reads 48 KB per (query, chunk) pair --
// 0.5 GB per registration at C2, from the Infinity Cache / HBM because the 77 MB int8 map does not fit the L2s; here the map
// is read once.  Round 3: on the matrix cores.  Wave w holds tile w of the chunk as the MFMA's first operand (its int8
// fragments: 4 KS registers), the bin's queries are taken 32 at a time -- the workgroup gathers their fragment units from the
// scan's int8 tiles into one operand image in the LDS (16 bytes per unit) -- and KS MFMAs per wave give the exact integer
// scores of 32 rows x 32 queries; a row inside the query's bounds is appended to the query's list (one atomic per lane and
// block for all of its hits).  Same integers, same hit test, hence the same rows as the v_dot4 loop it replaces (24 LDS reads +
// 96 dot4 per query and wave: 26 us at C2's 9891 candidates but 0.7 ms at the 220 000 of an ungated Euclidean search).
constexpr int RESCAN_LHITS = 1024;   // rows a workgroup of match_rescan_chunk_kernel stages in the LDS before it touches the lists (1024: 13 KB of static LDS beside the 39 KB ring at d = 384 -- three workgroups per compute unit instead of two)
// ---- the frame of the two chunk-major rescans (this kernel and match_rescan_chunk_mx6h_kernel): the workgroup's slice of its chunk's
// bin, and its hits, staged: the global side (a returning atomic on the query's list length, then the entry) is done for all of
// them at once.  The scoring and the hit test between the two are each kernel's own.
struct RescanStage {
    int lbin[RESCAN_SLICE];
    int lhq[RESCAN_LHITS];
    unsigned char lhr[RESCAN_LHITS];
    float lhu[RESCAN_LHITS];   // the row's upper bound (cand_up)
    int lhit_n;
};
struct RescanLists {   // the queries' lists (SearchWs); handed on by value, restrict kept: the kernels' register counts stay what they were
    int* __restrict__ cand_cnt;
    unsigned* __restrict__ cand;
    float* __restrict__ cand_up;
    unsigned* __restrict__ hit_cnt;
    int cap;
};
// the chunk row of accumulator element e of a lane whose element 0 is row rr0 = 32 wave + 4 (lane >> 5)
__device__ __forceinline__ int chunk_row(int rr0, int e) { return rr0 + (e & 3) + 8 * (e >> 2); }
// Prologue: workgroup (c, y) takes entries [y slice, y slice + nq) of chunk c's bin into S.lbin, padded to nblocks blocks of 32.
// false: nothing to do (guard up: another kernel has decided every query; or the bin ends before this slice).
__device__ __forceinline__ bool rescan_take_slice(RescanStage& S, const int* guard, const unsigned* bin_cnt, const int* bins, int bin_cap,
                                                  int slice, int& nq, int& nblocks) {
    const int c = blockIdx.x;
    if (guard && *guard) return false;
    const unsigned filled = bin_cnt[(size_t)c * BIN_CNT_STRIDE];
    const int nall = filled < (unsigned)bin_cap ? (int)filled : bin_cap;
    const int jbeg = blockIdx.y * slice;   // a long bin is shared by the workgroups (c, 0), (c, 1), ... (slice <= RESCAN_SLICE entries each)
    if (jbeg >= nall) return false;
    nq = nall - jbeg < slice ? nall - jbeg : slice;
    nblocks = (nq + 31) >> 5;
    if (threadIdx.x == 0) S.lhit_n = 0;
    const int* bin = bins + (size_t)c * bin_cap + jbeg;
    for (int t = threadIdx.x; t < nblocks * 32; t += 256) S.lbin[t] = t < nq ? bin[t] : 0;
    return true;
}
// One row into query q's list.  (The list's length stays as the selection / match_rescan_kernel left it during the kernel; the appended
// rows are counted in hit_cnt, a line of their own per query, and added by match_rescan_close_kernel.)
__device__ __forceinline__ void rescan_append(const RescanLists L, int q, unsigned entry, float up) {
    const int pos = L.cand_cnt[q] + (int)atomicAdd(&L.hit_cnt[(size_t)q * BIN_CNT_STRIDE], 1u);
    if (pos < L.cap) {
        L.cand[(size_t)q * L.cap + pos] = entry;
        L.cand_up[(size_t)q * L.cap + pos] = up;
    }
}
// hit number `at` of the workgroup (row rr of chunk c for query q): staged, or -- more hits than the staging buffer holds
// (duplicate-rich chunk) -- appended on the spot
__device__ __forceinline__ void rescan_stage_hit(RescanStage& S, const RescanLists L, int at, int q, int c, int rr, float up) {
    if (at < RESCAN_LHITS) {
        S.lhq[at] = q;
        S.lhr[at] = (unsigned char)rr;
        S.lhu[at] = up;
    } else {
        rescan_append(L, q, ((unsigned)c << 8) | (unsigned)rr, up);
    }
}
// End of a block: a full staging buffer is emptied before the next block adds to it.  (lhit_n is read by every thread between two
// barriers that no atomic of another block can cross, so the branch is uniform.)
__device__ __forceinline__ void rescan_flush(RescanStage& S, const RescanLists L, int c, bool last) {
    __syncthreads();
    if (S.lhit_n > RESCAN_LHITS / 2 || last) {
        wait_vmcnt<0>();   // (the atomics below are compiler-tracked: nothing of the ring may be pending behind them)
        const int nh = S.lhit_n < RESCAN_LHITS ? S.lhit_n : RESCAN_LHITS;
        for (int i = threadIdx.x; i < nh; i += 256) rescan_append(L, S.lhq[i], ((unsigned)c << 8) | (unsigned)S.lhr[i], S.lhu[i]);
        __syncthreads();
        if (threadIdx.x == 0) S.lhit_n = 0;
    }
}
// grid of a chunk-major rescan: one workgroup per (chunk, slice of its bin).  Short workgroups: one that walks a whole bin (~600 queries
// on lifted descriptors) lives ~80 us on 160 registers x 4 waves and 61 KB, and while a grid of those is resident nothing as
// register-heavy as a ViT GEMM wave (156 - 416 registers) is placed beside it -- in C3 as a pipeline the feature stage of the next pair
// stood still behind this kernel (tools/trace_c3_pipe.sh).
inline dim3 rescan_chunk_grid(const SearchWs& w, int nchunks, int& slice) {
    slice = vfm_cfg().finish_short ? 128 : RESCAN_SLICE;
    return dim3((unsigned)nchunks, (unsigned)((w.bin_cap + slice - 1) / slice));
}
template <int KS>
constexpr int rescan_ring_depth() { return KS <= 16 ? 3 : 2; }
template <int KS>
constexpr size_t rescan_slot_bytes() { return (size_t)KS * 1024 + 768; }   // operand image + three rows of 64 per-query terms
template <int KS>  // k-steps of 32 columns (d / 32)
__global__ __launch_bounds__(256) void match_rescan_chunk_kernel(int64_t n, int64_t m, I8Bounds ib, const uint4* __restrict__ q8,
                                                                 const uint4* __restrict__ b8, const unsigned* __restrict__ qmax,
                                                                 int* __restrict__ cand_cnt, unsigned* __restrict__ cand, int cap,
                                                                 const unsigned* __restrict__ bin_cnt, const int* __restrict__ bins,
                                                                 int use_gate, float gate, const int* __restrict__ guard, L2Terms l2,
                                                                 int bin_cap, unsigned* __restrict__ hit_cnt, float* __restrict__ cand_up,
                                                                 int slice, const unsigned char* __restrict__ qrows,
                                                                 unsigned* __restrict__ pilot_qmax) {
    // A ring of D slots, one per block of 32 queries: [KS][64] uint4 = the block's queries as ONE MFMA operand image (unit u =
    // (k-step s, half h, column p) comes from query bin[j0 + p]), then [3][64] dwords of per-query terms.  Everything a block needs
    // from global memory arrives by LDS-DMA issued D - 1 blocks ahead (wave w gathers k-steps w, w + 4, ...: its 64 lanes' units
    // are 1 KiB of consecutive LDS), so that the loop holds no compiler-tracked global load -- one would drain the DMA queue at its
    // s_waitcnt -- and a block costs its MFMAs, not its round trips (gather -> barrier -> MFMA -> returning atomic in sequence had
    // cost ~5 us per block: 148 us at 12 candidate chunks per query, 616 at 46).
    extern __shared__ __attribute__((aligned(16))) unsigned char rescan_smem[];
    constexpr int D = rescan_ring_depth<KS>();
    constexpr unsigned SLOT = (unsigned)rescan_slot_bytes<KS>();
    constexpr int TILE_U4 = KS * 64;
    constexpr int NG = KS / 4;      // gathered 1 KiB pieces per wave and block (KS % 4 == 0)
    __shared__ RescanStage S;
    const RescanLists L{cand_cnt, cand, cand_up, hit_cnt, cap};
    const int c = blockIdx.x;
    int nq, nblocks;
    if (!rescan_take_slice(S, guard, bin_cnt, bins, bin_cap, slice, nq, nblocks)) return;   // (guard: match_gatepass_kernel has decided every query)
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    intx4 af[KS];
    {
        const uint4* asrc = b8 + ((size_t)c * 4 + wave) * TILE_U4 + lane;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const uint4 v = asrc[s * 64];
            af[s] = *reinterpret_cast<const intx4*>(&v);
        }
    }
    const float bstep = ib.bstep[c], berr = ib.berr[c];
    const long long base = (long long)c * CHUNK_ROWS;
    const int rr0 = wave * 32 + 4 * (lane >> 5);   // + (e & 3) + 8 (e >> 2): the chunk row of accumulator element e
    float bn16[16];                                // Euclidean mode: |b~| of the lane's sixteen rows
#pragma unroll
    for (int e = 0; e < 16; ++e) bn16[e] = l2.qn ? l2.bn[base + chunk_row(rr0, e)] : 0.0f;
    __syncthreads();   // (drains the loads above: from here on the vector-memory queue holds DMA only)
    const unsigned lds_base = (unsigned)(uintptr_t)(LDS_AS unsigned char*)rescan_smem;
    // terms of a slot, rows of 64 dwords: [0] cand_cnt | qerr, [1] qstep | qmax, [2] qn | -   (lanes 0-31 | 32-63)
    auto issue = [&](int blk) {
        const int qi = S.lbin[blk * 32 + (lane & 31)];
        const unsigned slot = lds_base + (unsigned)(blk % D) * SLOT;
        if (qrows) {   // row-major int8 scan (Prepared::rows8): unit (k-step s, half h) of query qi = bytes 32 s + 16 h .. of its row
            const unsigned char* rsrc = qrows + (size_t)qi * (KS * 32) + (size_t)(2 * wave + (lane >> 5)) * 16;
#pragma unroll
            for (int t = 0; t < NG; ++t)
                glds16(rsrc + (size_t)t * 128, __builtin_amdgcn_readfirstlane(slot + (unsigned)(wave + 4 * t) * 1024u));
        } else {
        const uint4* src = q8 + (size_t)(qi >> 5) * TILE_U4 + (size_t)(2 * wave + (lane >> 5)) * 32 + (qi & 31);
#pragma unroll
        for (int t = 0; t < NG; ++t)
            glds16(src + (size_t)t * 256, __builtin_amdgcn_readfirstlane(slot + (unsigned)(wave + 4 * t) * 1024u));
        }
        const unsigned terms = slot + (unsigned)KS * 1024u;
        if (wave == 0) glds4(lane < 32 ? (const void*)(cand_cnt + qi) : (const void*)(ib.qerr + qi), __builtin_amdgcn_readfirstlane(terms));
        if (wave == 1)
            glds4(lane < 32 ? (const void*)(ib.qstep + (qi >> 7)) : (const void*)(qmax + qi), __builtin_amdgcn_readfirstlane(terms + 256u));
        if (wave == 2 && l2.qn) glds4((const void*)(l2.qn + qi), __builtin_amdgcn_readfirstlane(terms + 512u));
    };
#pragma unroll
    for (int blk = 0; blk < D - 1; ++blk)
        if (blk < nblocks) issue(blk);
    for (int blk = 0; blk < nblocks; ++blk) {          // the bin, one MFMA column block at a time
        // this wave's pieces of block blk have landed: at most the D - 2 blocks issued behind it may still be in flight
        if (D > 2 && blk + D - 2 < nblocks) wait_vmcnt<(D > 2 ? (D - 2) * NG : 0)>();
        else wait_vmcnt<0>();
        __syncthreads();                               // ... and every wave's; block blk - 1 has been read by every wave
        if (blk + D - 1 < nblocks) issue(blk + D - 1);
        const unsigned char* slot = rescan_smem + (size_t)(blk % D) * SLOT;
        const uint4* l_qf = reinterpret_cast<const uint4*>(slot);
        const int* lt = reinterpret_cast<const int*>(slot + (size_t)KS * 1024);
        const int j = blk * 32 + (lane & 31);
        const int qi = S.lbin[j];
        const bool live = j < nq && lt[lane & 31] >= 0;   // (-2: below the gate, -1: already with the all-pairs kernel)
        const float eq = __int_as_float(lt[32 + (lane & 31)]);
        const float sc = __int_as_float(lt[64 + (lane & 31)]) * bstep;   // the same expressions as match_rescan_kernel: the same rows pass
        const float bound = (eq * 1.0001220703125f + 1.0e-6f) + (1.0001220703125f + eq) * berr;
        const float qlow = use_gate ? gate : key_float((unsigned)lt[96 + (lane & 31)]);   // half-width pass: the hit test is the gate itself
        const float qn = l2.qn ? __int_as_float(lt[128 + (lane & 31)]) : 0.0f;
        intx16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const uint4 v = l_qf[s * 64 + lane];
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[s], *reinterpret_cast<const intx4*>(&v), acc, 0, 0, 0);
        }
        if (pilot_qmax) {
            // VFM_RECORDS_MX6_PILOT, in front of the selection: the bin holds the queries whose best fp6 chunk this is; the chunk's best
            // EXACT integer score gives a lower bound of the query's exact maximum that carries the int8 image's bound (~0.01) instead of
            // the fp6 image's (~0.06): it raises qmax, which the selection and the rescans behind it test against.  No hits are listed.
            int smax = -0x7fffffff;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int rr = chunk_row(rr0, e);
                if (base + rr < m) smax = max(smax, acc[e]);
            }
            smax = max(smax, __shfl_xor(smax, 32));   // the two half-waves hold the same query's other rows
            if (j < nq && lane < 32 && smax > -0x7fffffff) atomicMax(&pilot_qmax[qi], float_key((sc * (float)smax - bound) - 2.0e-6f));
            __syncthreads();
            continue;
        }
        unsigned hits = 0u;
        if (live) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int rr = chunk_row(rr0, e);
                float up = sc * (float)acc[e] + bound;
                if (l2.qn) up = l2_upper_row(qn, bn16[e], up, l2.slack);
                if (base + rr < m && up >= qlow) hits |= 1u << e;
            }
        }
        if (hits) {
            int at = atomicAdd(&S.lhit_n, __popc(hits));
            while (hits) {
                const int e = __ffs(hits) - 1;
                hits &= hits - 1u;
                const int rr = chunk_row(rr0, e);
                // (a Euclidean search's bound is not symmetric about the score: its rows are never filtered -- +Inf)
                const float upe = l2.qn ? __builtin_inff() : sc * (float)acc[e] + bound;
                rescan_stage_hit(S, L, at++, qi, c, rr, upe);
            }
        }
        rescan_flush(S, L, c, blk + 1 == nblocks);
    }
}

template <int KS>
int launch_rescan_chunk_ks(const SearchWs& w, int nchunks, int64_t n, int64_t m, I8Bounds ib, const Prepared& Q, const Prepared& B,
                           int use_gate, float gate, const int* guard, L2Terms l2, hipStream_t st, bool pilot) {
    const size_t lds = (size_t)rescan_ring_depth<KS>() * rescan_slot_bytes<KS>();   // + ~14 KB of static LDS: past 64 KB in all from KS = 16
    static unsigned long long attr_set = 0ull;  // one bit per device
    if (!attr_done(attr_set)) {
        VFM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&match_rescan_chunk_kernel<KS>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_mark(attr_set);
    }
    int slice;
    const dim3 grid = rescan_chunk_grid(w, nchunks, slice);
    hipLaunchKernelGGL(match_rescan_chunk_kernel<KS>, grid, dim3(256), lds, st, n, m, ib, (const uint4*)Q.tiles8, (const uint4*)B.tiles8, (const unsigned*)w.qmax, w.cand_cnt,
                       w.cand, w.cap, (const unsigned*)w.bin_cnt, (const int*)w.bins, use_gate, gate, guard, l2, w.bin_cap, w.hit_cnt, w.cand_up,
                       slice, vfm_cfg().rescan_rows ? (const unsigned char*)Q.rows8 : (const unsigned char*)nullptr, pilot ? w.qmax : (unsigned*)nullptr);
    VFM_CHECK_LAUNCH("match_rescan_chunk_kernel");
    return VFM_OK;
}
int launch_rescan_chunk(const SearchWs& w, int nchunks, int64_t n, int64_t m, int d, I8Bounds ib, const Prepared& Q, const Prepared& B,
                        int use_gate, float gate, const int* guard, L2Terms l2, hipStream_t st, bool pilot = false) {
    switch (d / 32) {
        case 8: return launch_rescan_chunk_ks<8>(w, nchunks, n, m, ib, Q, B, use_gate, gate, guard, l2, st, pilot);
        case 12: return launch_rescan_chunk_ks<12>(w, nchunks, n, m, ib, Q, B, use_gate, gate, guard, l2, st, pilot);
        case 16: return launch_rescan_chunk_ks<16>(w, nchunks, n, m, ib, Q, B, use_gate, gate, guard, l2, st, pilot);
        case 20: return launch_rescan_chunk_ks<20>(w, nchunks, n, m, ib, Q, B, use_gate, gate, guard, l2, st, pilot);
        default: return launch_rescan_chunk_ks<24>(w, nchunks, n, m, ib, Q, B, use_gate, gate, guard, l2, st, pilot);
    }
}

// ---------------------------------------------------------------------------------------------
// VFM_RECORDS_MX6_HALF_FUSED | VFM_RECORDS_NO_I8: the chunk-major rescan on the fp6 HALF image -- the image the coarse kernel has just
// multiplied (5 KiB per 32-row tile at d = 384; operands prepared with VFM_PREPARE_NO_I8 carry no int8 byte).  The frame is
// match_rescan_chunk_kernel's: one workgroup per (chunk, bin slice); wave w holds tile w of the chunk as the MFMA's first operand (the
// scales and the first KS6 k-steps of the stored tile: 6 KS6 + 1 registers); the bin's queries are taken 32 at a time, their fragments
// gathered from the scan's fp6 tiles into ONE operand image in the LDS by LDS-DMA issued D - 1 blocks ahead, and KS6 scaled MFMAs per
// wave (match_coarse_mx6.hip's, same operand order, same accumulation: the scores are the coarse kernel's) give x = the fp6 score of
// 32 rows x 32 queries over the first d / 2 columns.
//
// Hit test per (query q, row r) -- emit_chunk's expression (the bound of match_select_half_kernel -- match_select.h:
// chunk_upper_half -- with mx6_bounds_half) with the ROW's residual norm and rest norm in place of the chunk's maxima:
//     exact score of (q, r)  <=  x + A_q + (1 + 2^-13 + E_q) E_r + rest_q rest_r  (+ 2e-6 for the fp32 evaluation),
// E = err6h, the image's residual over the columns the pass multiplies (MX6_SLACK, which pays for the MFMA's fp32 accumulation, is in
// every E), rest = |second half of the normalised row|, rounded up (Cauchy-Schwarz on the columns the pass does not multiply).  A row is
// a hit when that upper bound reaches the gate, tested as a threshold on x exactly as emit_chunk does.
// Nothing is lost: the bound holds row by row -- the chunk's form is this one with E_r, rest_r replaced by their maxima over the chunk --
// so every row whose exact cosine reaches the gate is a hit here; and its chunk was binned for the query, because every fp32 operation
// of the threshold is monotone in E_r and rest_r: threshold(chunk) <= threshold(row) <= x(row) <= the chunk's best x.
// Hits are single-row entries (chunk << 8 | row) with their upper bound in cand_up, staged in the LDS and counted through hit_cnt as
// the int8 kernel's are: match_rescan_close_kernel is reused as it stands.  Rows at or beyond m never hit; guard up: nothing to do.
// ---------------------------------------------------------------------------------------------
constexpr int rescan6_depth() { return 3; }   // ring slots (blocks of 32 queries)
// A ring slot: [KS6][64] x 16 B = code plane A of every k-step as the MFMA lanes read it, [KS6][2][64] x 4 B = code plane B as its two
// dwords (LDS-DMA moves 4 or 16 bytes per lane: the 8-byte units of the stored plane arrive as two dword gathers), [64] x 4 B = the
// scales of k-steps 0 .. 3, then two rows of 64 per-query terms: [0] cand_cnt | err6h (lanes 0 - 31 | 32 - 63), [1] rest
template <int KS6>
constexpr unsigned rescan6_slot_bytes() { return (unsigned)KS6 * 1536u + 256u + 512u; }
template <int KS6>  // k-steps of 64 columns the half-width pass multiplies (d / 128)
__global__ __launch_bounds__(256) void match_rescan_chunk_mx6h_kernel(int64_t n, int64_t m, const unsigned char* __restrict__ q6,
                                                                      const unsigned char* __restrict__ b6, const float* __restrict__ qerr,
                                                                      const float* __restrict__ qrest, const float* __restrict__ berr,
                                                                      const float* __restrict__ brest, int* __restrict__ cand_cnt,
                                                                      unsigned* __restrict__ cand, int cap, const unsigned* __restrict__ bin_cnt,
                                                                      const int* __restrict__ bins, float gate, const int* __restrict__ guard,
                                                                      int bin_cap, unsigned* __restrict__ hit_cnt, float* __restrict__ cand_up,
                                                                      int slice) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(KS6 >= 2 && KS6 <= 4, "the half-width image of d = 256 / 384 / 512: one scale register per lane");
    constexpr int D = rescan6_depth();
    constexpr unsigned SLOT = rescan6_slot_bytes<KS6>();
    constexpr int IMG_TB = mx6_tile_bytes(2 * KS6);   // bytes of a stored tile (the full-width layout; the pass reads its prefix)
    constexpr int NI = 3 * KS6 + 3;                   // DMA instructions per block: KS6 plane A, 2 KS6 plane B, scales, two rows of terms
    constexpr int NG = (NI + 3) / 4;                  // ... per wave (a wave past the end repeats the last one: the same bytes again)
    __shared__ __attribute__((aligned(16))) unsigned char ring[D * SLOT];
    __shared__ RescanStage S;
    const RescanLists L{cand_cnt, cand, cand_up, hit_cnt, cap};
    const int c = blockIdx.x;
    int nq, nblocks;
    if (!rescan_take_slice(S, guard, bin_cnt, bins, bin_cap, slice, nq, nblocks)) return;   // (guard: match_guard_fallback_kernel has sent every query to the all-pairs kernel)
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // tile `wave` of the chunk: the first operand
    Mx6Frag af[KS6];
    uint2 as = make_uint2(0u, 0u);   // (.x: the scales of k-steps 0 .. 3, all this kernel multiplies)
    {
        const unsigned char* tile = b6 + ((size_t)c * 4 + wave) * (size_t)IMG_TB;
#pragma unroll
        for (int s = 0; s < KS6; ++s) {
            const uint4 lo = *reinterpret_cast<const uint4*>(tile + mx6_code_a(s, lane));
            const uint2 hi = *reinterpret_cast<const uint2*>(tile + mx6_code_b(s, lane));
            af[s] = Mx6Frag{{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y}};
        }
        as.x = *reinterpret_cast<const unsigned*>(tile + mx6_scale_at(2 * KS6, 0, lane));
    }
    const long long base = (long long)c * CHUNK_ROWS;
    const int rr0 = wave * 32 + 4 * (lane >> 5);   // + (e & 3) + 8 (e >> 2): the chunk row of accumulator element e
    float be16[16], br16[16];                      // err6h / rest of the lane's sixteen rows (rows of the padded operand always exist)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        be16[e] = berr[base + chunk_row(rr0, e)];
        br16[e] = brest[base + chunk_row(rr0, e)];
    }
    // everything loaded above is in its registers before the first DMA goes out: from here on the vector-memory queue holds DMA only
#pragma unroll
    for (int s = 0; s < KS6; ++s) asm volatile("" ::"v"(af[s].c[0]), "v"(af[s].c[1]), "v"(af[s].c[2]), "v"(af[s].c[3]), "v"(af[s].c[4]), "v"(af[s].c[5]));
    asm volatile("" ::"v"(as.x));
#pragma unroll
    for (int e = 0; e < 16; ++e) asm volatile("" ::"v"(be16[e]), "v"(br16[e]));
    wait_vmcnt<0>();
    __syncthreads();
    const unsigned lds_base = (unsigned)(uintptr_t)(LDS_AS unsigned char*)ring;
    auto issue = [&](int blk) {
        const int qi = S.lbin[blk * 32 + (lane & 31)];
        const unsigned slot = lds_base + (unsigned)(blk % D) * SLOT;
        // MFMA lane (h, p) of the block's operand = lane 32 h + (qi & 31) of the query's stored tile
        const unsigned char* qtile = q6 + (size_t)(qi >> 5) * (size_t)IMG_TB;
        const int ql = (lane & 32) + (qi & 31);
#pragma unroll
        for (int t = 0; t < NG; ++t) {
            int i = wave + 4 * t;   // wave-uniform
            i = i < NI ? i : NI - 1;
            if (i < KS6) {
                glds16(qtile + mx6_code_a(i, ql), __builtin_amdgcn_readfirstlane(slot + (unsigned)i * 1024u));
            } else if (i < 3 * KS6) {
                const int j = i - KS6;   // (k-step j >> 1, dword j & 1 of the lane's eight bytes of plane B)
                glds4(qtile + mx6_code_b(j >> 1, ql) + 4 * (j & 1), __builtin_amdgcn_readfirstlane(slot + (unsigned)KS6 * 1024u + (unsigned)j * 256u));
            } else if (i == 3 * KS6) {
                glds4(qtile + mx6_scale_at(2 * KS6, 0, ql), __builtin_amdgcn_readfirstlane(slot + (unsigned)KS6 * 1536u));
            } else if (i == 3 * KS6 + 1) {
                glds4(lane < 32 ? (const void*)(cand_cnt + qi) : (const void*)(qerr + qi), __builtin_amdgcn_readfirstlane(slot + (unsigned)KS6 * 1536u + 256u));
            } else {
                glds4((const void*)(qrest + qi), __builtin_amdgcn_readfirstlane(slot + (unsigned)KS6 * 1536u + 512u));
            }
        }
    };
#pragma unroll
    for (int blk = 0; blk < D - 1; ++blk)
        if (blk < nblocks) issue(blk);
    for (int blk = 0; blk < nblocks; ++blk) {          // the bin, one MFMA column block at a time
        // this wave's pieces of block blk have landed: at most the D - 2 blocks issued behind it may still be in flight
        if (blk + D - 2 < nblocks) wait_vmcnt<(D - 2) * NG>();
        else wait_vmcnt<0>();
        __syncthreads();                               // ... and every wave's; block blk - 1 has been read by every wave
        if (blk + D - 1 < nblocks) issue(blk + D - 1);
        const unsigned char* slot = ring + (size_t)(blk % D) * SLOT;
        const int* lt = reinterpret_cast<const int*>(slot + (size_t)KS6 * 1536 + 256);
        const int j = blk * 32 + (lane & 31);
        const int qi = S.lbin[j];
        const bool live = j < nq && lt[lane & 31] >= 0;   // (-1: already with the all-pairs kernel)
        const float eq = __int_as_float(lt[32 + (lane & 31)]);
        const float rq = __int_as_float(lt[64 + (lane & 31)]);
        const uint2 qs = make_uint2(*reinterpret_cast<const unsigned*>(slot + (size_t)KS6 * 1536 + 4 * lane), 0u);
        floatx16 acc;
        auto kstep = [&](auto Sc) __attribute__((always_inline)) {
            constexpr int s = decltype(Sc)::value;
            const uint4 lo = *reinterpret_cast<const uint4*>(slot + (size_t)s * 1024 + 16 * lane);
            const unsigned h0 = *reinterpret_cast<const unsigned*>(slot + (size_t)KS6 * 1024 + (size_t)(2 * s) * 256 + 4 * lane);
            const unsigned h1 = *reinterpret_cast<const unsigned*>(slot + (size_t)KS6 * 1024 + (size_t)(2 * s + 1) * 256 + 4 * lane);
            const Mx6Frag qf{{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)h0, (int)h1}};
            if constexpr (s == 0) {   // (the coarse kernel's first MFMA starts from the constant 0 as well)
                floatx16 zero;
#pragma unroll
                for (int r = 0; r < 16; ++r) zero[r] = 0.0f;
                acc = mfma_mx6<s>(af[s], as, qf, qs, zero);
            } else {
                acc = mfma_mx6<s>(af[s], as, qf, qs, acc);
            }
        };
        kstep(std::integral_constant<int, 0>{});
        kstep(std::integral_constant<int, 1>{});
        if constexpr (KS6 > 2) kstep(std::integral_constant<int, 2>{});
        if constexpr (KS6 > 3) kstep(std::integral_constant<int, 3>{});
        // emit_chunk's threshold (next_thr in match_coarse_mx6.hip) with the row's terms for the chunk's maxima
        const float fx_A = eq * 1.0001220703125f + 1.0e-6f, fx_mult = 1.0001220703125f + eq;
        unsigned hits = 0u;
        if (live) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int rr = chunk_row(rr0, e);
                const float thr = ((gate - 1.0e-6f) - (fx_A + fx_mult * be16[e])) - (rq * br16[e] + 1.0e-6f);
                if (base + rr < m && !(acc[e] < thr)) hits |= 1u << e;
            }
        }
        if (hits) {
            int at = atomicAdd(&S.lhit_n, __popc(hits));
            while (hits) {
                const int e = __ffs(hits) - 1;
                hits &= hits - 1u;
                const int rr = chunk_row(rr0, e);
                const float upe = (acc[e] + (fx_A + fx_mult * be16[e])) + (rq * br16[e] + 2.0e-6f);
                rescan_stage_hit(S, L, at++, qi, c, rr, upe);
            }
        }
        rescan_flush(S, L, c, blk + 1 == nblocks);
    }
#endif   // __HIP_DEVICE_COMPILE__
}

template <int KS6>
int launch_rescan_chunk_mx6h(const SearchWs& w, int nchunks, int64_t n, int64_t m, const Prepared& Q, const Prepared& B, float gate,
                             const int* guard, hipStream_t st) {
    int slice;
    const dim3 grid = rescan_chunk_grid(w, nchunks, slice);
    hipLaunchKernelGGL(match_rescan_chunk_mx6h_kernel<KS6>, grid, dim3(256), 0, st,
                       n, m, reinterpret_cast<const unsigned char*>(Q.tiles6), reinterpret_cast<const unsigned char*>(B.tiles6),
                       (const float*)Q.err6h, (const float*)Q.rest, (const float*)B.err6h, (const float*)B.rest, w.cand_cnt, w.cand, w.cap,
                       (const unsigned*)w.bin_cnt, (const int*)w.bins, gate, guard, w.bin_cap, w.hit_cnt, w.cand_up, slice);
    VFM_CHECK_LAUNCH("match_rescan_chunk_mx6h_kernel");
    return VFM_OK;
}

// VFM_RECORDS_NO_I8, behind half_guard_kernel: with the guard up there is no int8 image for a gate pass -- every live query goes to the
// all-pairs kernel (cand_cnt = -1, listed in fb_list; half_guard_kernel has reset the list's length).  One atomic per wavefront.
__global__ __launch_bounds__(256) void match_guard_fallback_kernel(int64_t n, const float* __restrict__ invq, const int* __restrict__ guard,
                                                                   int* __restrict__ cand_cnt, int* __restrict__ fb_count,
                                                                   int* __restrict__ fb_list) {
    if (*guard == 0) return;
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = lane_id();
    const bool live = q < n && invq[q] != 0.0f;
    const unsigned long long bal = __ballot(live);
    if (bal == 0ull) return;
    int base = 0;
    if (lane == 0) base = atomicAdd(fb_count, __popcll(bal));
    base = __shfl(base, 0);
    if (live) {
        cand_cnt[q] = -1;
        fb_list[base + __popcll(bal & ((1ull << lane) - 1ull))] = (int)q;
    }
}

// VFM_RECORDS_MX6_PILOT: every query (zero rows aside) into the bin of the chunk its best fp6 score came from
__global__ __launch_bounds__(256) void match_pilot_bin_kernel(int64_t n, const unsigned long long* __restrict__ qbest,
                                                              const float* __restrict__ invq, unsigned* __restrict__ bin_cnt,
                                                              int* __restrict__ bins, int bin_cap, int nchunks) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n || invq[q] == 0.0f) return;
    const unsigned long long v = qbest[q];
    if ((v >> 32) == 0ull) return;   // no un-padded chunk gave a lower bound
    const unsigned c = (unsigned)v;
    if (c >= (unsigned)nchunks) return;
    const unsigned pos = atomicAdd(&bin_cnt[(size_t)c * BIN_CNT_STRIDE], 1u);
    if (pos < (unsigned)bin_cap) bins[(size_t)c * bin_cap + pos] = (int)q;   // (a bin that is full: those queries keep the fp6 lower bound)
}

// ---------------------------------------------------------------------------------------------
// Half-width pass: the device-side guard (VERDICT r2 / ADVICE r2: "no 171 ms registration, ever").
// half_guard_kernel (one workgroup, after the selection): the search's survivor count -- fb_count[5] from match_select_half_kernel,
// or the sum of the bin counts in the fused form, which it stores there -- against HALF_GUARD_PER_QUERY * n; above it (or where the
// fused coarse kernel saturated a bin) fb_count[HALF_GUARD_FLAG] = 1 and the selection's all-pairs fallbacks are withdrawn.
// Then match_rescan_kernel empties every list, match_rescan_chunk_kernel returns at once, and match_gatepass_kernel resolves
// the search: one workgroup per map chunk, wave w holds tile w of the chunk as the MFMA's first operand (48 registers at
// d = 384), the scan's int8 tiles stream past it (next tile's fragments loaded under the current tile's MFMAs), and every row
// whose full-width upper bound  s_q s_c S + A + B_c  reaches the gate -- the hit test of the rescans -- is appended to its
// query's list.  The matrix work of the full-width pass in a kernel light enough to sit beside anything (no LDS, <= 2 waves
// per SIMD), launched behind every half-width selection and returning at once unless the flag is up.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void half_guard_kernel(int* __restrict__ fb_count, const unsigned* __restrict__ bin_cnt, int nchunks,
                                                         int fused, long long limit) {
    __shared__ long long part[4];
    long long s = 0;
    if (fused)
        for (int c = threadIdx.x; c < nchunks; c += 256) s += (long long)bin_cnt[(size_t)c * BIN_CNT_STRIDE];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (lane_id() == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long total = fused ? part[0] + part[1] + part[2] + part[3] : (long long)fb_count[5];
        // (the fused fp6 kernel raises the flag itself when a workgroup's list overflows, and its survivors are then not binned: the
        // load figure must still say "far too many")
        if (fused && fb_count[HALF_GUARD_FLAG] != 0 && total < 0x3FFFFFFFll) total = 0x3FFFFFFFll;
        if (fused) fb_count[5] = (int)(total > 0x7FFFFFFFll ? 0x7FFFFFFFll : total);   // the search's load figure
        if (total > limit || fb_count[HALF_GUARD_FLAG] != 0) {
            fb_count[HALF_GUARD_FLAG] = 1;
            fb_count[0] = 0;   // queries the selection sent to the all-pairs kernel: the gate pass decides them too
        }
    }
}

template <int KS>  // k-steps of 32 columns (d / 32)
__global__ __launch_bounds__(256, 2) void match_gatepass_kernel(int64_t n, int64_t m, int nq_tiles, I8Bounds ib,
                                                                const float* __restrict__ invq, const uint4* __restrict__ q8,
                                                                const uint4* __restrict__ b8, float gate, int* __restrict__ cand_cnt,
                                                                unsigned* __restrict__ cand, int cap, const int* __restrict__ guard,
                                                                unsigned* __restrict__ qlow) {
    // qlow (the search's qmax array: unused by the half-width selection, zero = -Inf): float_key of a lower bound of the query's
    // exact maximum, published by whichever workgroup finds a better one.  Where hundreds of rows per query reach the gate -- lifted
    // descriptors with a common component -- a row whose upper bound lies below it cannot be the arg-max and is not appended (the
    // arg-max itself, and every row tied with it, has an upper bound at or above every lower bound ever published): the lists the
    // refinement gets shrink from "every row above the gate" to "rows near the best" (forced half-width pass on such a map: 22 ms
    // per C2-size registration before)
    if (*guard == 0) return;
    constexpr int TILE_U4 = KS * 64;
    const int c = blockIdx.x, lane = lane_id(), wave = threadIdx.x >> 6;
    intx4 af[KS];
    {
        const uint4* asrc = b8 + ((size_t)c * 4 + wave) * TILE_U4 + lane;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const uint4 v = asrc[s * 64];
            af[s] = *reinterpret_cast<const intx4*>(&v);
        }
    }
    const float sb = ib.bstep[c], be = ib.berr[c];
    const long long row0 = (long long)c * CHUNK_ROWS + wave * 32 + 4 * (lane >> 5);   // + (e & 3) + 8 (e >> 2): accumulator element e
    constexpr bool AHEAD = KS <= 12;   // 3 x 4 KS fragment registers fit two waves per SIMD up to d = 384
    uint4 qn[AHEAD ? KS : 1];
    if constexpr (AHEAD) {
        const uint4* qsrc = q8 + lane;
#pragma unroll
        for (int s = 0; s < KS; ++s) qn[s] = qsrc[s * 64];
    }
    for (int qt = 0; qt < nq_tiles; ++qt) {
        intx4 qf[KS];
        if constexpr (AHEAD) {
#pragma unroll
            for (int s = 0; s < KS; ++s) qf[s] = *reinterpret_cast<const intx4*>(&qn[s]);
            if (qt + 1 < nq_tiles) {   // the next tile's fragments, under this tile's MFMAs
                const uint4* qsrc = q8 + (size_t)(qt + 1) * TILE_U4 + lane;
#pragma unroll
                for (int s = 0; s < KS; ++s) qn[s] = qsrc[s * 64];
            }
        } else {
            const uint4* qsrc = q8 + (size_t)qt * TILE_U4 + lane;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const uint4 v = qsrc[s * 64];
                qf[s] = *reinterpret_cast<const intx4*>(&v);
            }
        }
        const int64_t q = (int64_t)qt * 32 + (lane & 31);
        const float eq = ib.qerr[q], sq = ib.qstep[q >> 7];
        const bool live = q < n && invq[q] != 0.0f;
        intx16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0;
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[s], qf[s], acc, 0, 0, 0);
        int mx = acc[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = max(mx, acc[r]);
        // the expressions of match_rescan_chunk_kernel / match_rescan_kernel: the same rows pass
        const float sc = sq * sb, bound = (eq * 1.0001220703125f + 1.0e-6f) + (1.0001220703125f + eq) * be;
        float thr = gate;
        if (live) {
            const float ql = key_float(__hip_atomic_load(qlow + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            // this lane's best row lies at or above sc * mx - bound (padding rows of the last chunk score 0: only a positive score counts)
            const float mine = (row0 + 27 < m || mx > 0) ? __builtin_fmaf(sc, (float)mx, -bound) : -__builtin_inff();
            if (mine > ql && mine >= gate) atomicMax(qlow + q, float_key(mine));
            thr = fmaxf(gate, fmaxf(ql, mine));
        }
        const bool any = live && (sc * (float)mx + bound >= thr);
        if (__ballot(any) != 0ull && any) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long long row = row0 + (e & 3) + 8 * (e >> 2);
                if (row < m && sc * (float)acc[e] + bound >= thr) {
                    const int pos = atomicAdd(&cand_cnt[q], 1);
                    if (pos < cap) cand[(size_t)q * cap + pos] = ((unsigned)c << 8) | (unsigned)(row - (long long)c * CHUNK_ROWS);
                }
            }
        }
    }
}

// after the rescans: lists longer than their capacity go to the all-pairs kernel, crowded ones to the fp32 refinement's work
// list -- appended with ONE atomic per wavefront (on duplicate-rich maps every query is crowded: 20 000 same-address atomics
// took 190 us)
__global__ __launch_bounds__(256) void match_rescan_close_kernel(int64_t n, int* __restrict__ cand_cnt, int cap,
                                                                 int* __restrict__ fb_count, int* __restrict__ fb_list,
                                                                 int* __restrict__ todo, const float* __restrict__ invq_half,
                                                                 const unsigned* __restrict__ hit_cnt) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = lane_id();
    int cnt = q < n ? cand_cnt[q] : 0;
    if (q < n && cnt >= 0) {   // + the rows of the chunk-major rescan
        const int hits = (int)hit_cnt[(size_t)q * BIN_CNT_STRIDE];
        if (hits) cand_cnt[q] = cnt = cnt + hits;
    }
    // half-width pass (invq_half != NULL): a live query whose surviving chunks held no row at the gate has no match
    if (invq_half && q < n && cnt == 0 && invq_half[q] != 0.0f) cand_cnt[q] = -2;
    if (cnt > cap) {
        cand_cnt[q] = -1;
        fb_list[atomicAdd(fb_count, 1)] = (int)q;
    }
    const bool crowded = cnt >= REFINE_MIN_I8 && cnt <= cap;
    const unsigned long long bal = __ballot(crowded);
    if (bal == 0ull) return;
    int base = 0;
    if (lane == 0) base = atomicAdd(fb_count + 6, __popcll(bal));
    base = __shfl(base, 0);
    if (crowded) todo[base + __popcll(bal & ((1ull << lane) - 1ull))] = (int)q;
}

// ---------------------------------------------------------------------------------------------
// fp32 refinement of crowded candidate lists (near-duplicate map rows).
//
// Real lifted descriptors are bilinear interpolations of a 16 x 21 patch grid (image_features.py:104-110,
// prepare_scenes.py:85-104): neighbouring map points differ by less than the fp16 window (2.5e-3), so a query
// can have dozens of candidate chunks, and chunks whose two best rows are both inside the window.  Deciding
// all of them in fp64 (or, past the old 40-entry cap, all M rows) was a cliff.  Here one wavefront per such
// query scores every candidate row in fp32 -- 16 lanes per row, 4 rows per pass, each lane a sequential fma
// chain over d/16 elements followed by a 4-level xor tree -- and keeps only the rows within
//     w2 = 2 * (d/16 + 4 + 2) * 2^-24      (3.6e-6 at d = 384)
// of the fp32 maximum.  Proof that the oracle's arg-max survives: the fp32 value s of a row differs from the
// exact dot product t of the same fp32-normalised rows (the oracle's definition) by at most
// gamma = (d/16 + 4) u * sum|q_k b_k| <= (d/16 + 4) u (1 + 1e-6), u = 2^-24 (one rounding per fma / add along the
// longest path of the summation tree; Cauchy-Schwarz on unit rows).  With j* the exact arg-max and j' the fp32
// arg-max: s(j*) >= t(j*) - gamma >= t(j') - gamma >= s(j') - 2 gamma; every row that ties with j* exactly is
// inside the same margin, so the fp64 decision (ties -> lowest index) sees them all.  The surviving rows
// replace the query's list as single-row entries: match_rescore_kernel is unchanged.
// ---------------------------------------------------------------------------------------------
// state of one wavefront refining one query: the fp32-normalised query in registers, the kept rows in LDS
// (NT = float4 per lane the arrays hold, >= d / 64: 6 at d = 384 -- 24 + 2 x 25 registers instead of 48 + 2 x 49, which is what lets the
// refinement run four waves per SIMD instead of two)
template <int NT>
struct RefineWave {
    Rows b;
    const float* invb;
    int d, nt, g, l, lane;
    float w2;
    float4 qv[NT];
    unsigned* lrow;
    float* lsc;
    int kept;        // wave-uniform
    float runmax;    // wave-uniform
    bool overflow;

    __device__ __forceinline__ void init(Rows q, float iq, int64_t qi, Rows b_, const float* invb_, int d_, float w2_,
                                         unsigned* lrow_, float* lsc_) {
        b = b_; invb = invb_; d = d_; w2 = w2_; lrow = lrow_; lsc = lsc_;
        lane = lane_id();
        g = lane >> 4;   // row slot of the pass
        l = lane & 15;   // k-slice
        nt = d >> 6;     // float4 per lane (d % 64 == 0)
        kept = 0;
        runmax = -3.0e38f;
        overflow = false;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t < nt) {
                float4 v = q.ld4(qi * (int64_t)d + 4 * (l + 16 * t));
                v.x = v.x * iq; v.y = v.y * iq; v.z = v.z * iq; v.w = v.w * iq;  // the fp32-normalised query (faiss' xq)
                qv[t] = v;
            }
        }
    }
    // fp32 score of this lane group's row (row < 0: none); identical in the 16 lanes of the group
    __device__ __forceinline__ float score4(long long row) const {
        float acc = 0.0f;
        if (row >= 0) {
            const float ib = invb[row];
            const int64_t br = row * (int64_t)d + 4 * l;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (t < nt) {
                    const float4 bv = b.ld4(br + 64 * t);
                    acc = __builtin_fmaf(qv[t].x, bv.x * ib, acc);
                    acc = __builtin_fmaf(qv[t].y, bv.y * ib, acc);
                    acc = __builtin_fmaf(qv[t].z, bv.z * ib, acc);
                    acc = __builtin_fmaf(qv[t].w, bv.w * ib, acc);
                }
            }
        }
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
        return acc;
    }
    // score4 in two halves, so that the next pass's row can be on its way while this pass's is summed (the same operations in
    // the same order: the same float)
    struct Row {
        float4 v[NT];
        float ib;
    };
    __device__ __forceinline__ void load4(Row& r, long long row) const {
        if (row >= 0) {
            r.ib = invb[row];
            const int64_t br = row * (int64_t)d + 4 * l;
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (t < nt) r.v[t] = b.ld4(br + 64 * t);
        }
    }
    __device__ __forceinline__ float dot4(const Row& r, long long row) const {
        float acc = 0.0f;
        if (row >= 0) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (t < nt) {
                    acc = __builtin_fmaf(qv[t].x, r.v[t].x * r.ib, acc);
                    acc = __builtin_fmaf(qv[t].y, r.v[t].y * r.ib, acc);
                    acc = __builtin_fmaf(qv[t].z, r.v[t].z * r.ib, acc);
                    acc = __builtin_fmaf(qv[t].w, r.v[t].w * r.ib, acc);
                }
            }
        }
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
        return acc;
    }
    // one pass: (row, sc) of the four lane groups; keeps the rows within w2 of the running fp32 maximum
    __device__ __forceinline__ void consider(long long row, float sc) {
        float pm = (row >= 0) ? sc : -3.0e38f;
        pm = fmaxf(pm, __shfl_xor(pm, 16));
        pm = fmaxf(pm, __shfl_xor(pm, 32));
        if (pm > runmax) {  // prune the kept list against the new maximum
            runmax = pm;
            const float thr = runmax - w2;
            const bool mine = lane < kept && lsc[lane] >= thr;
            const unsigned r = lane < kept ? lrow[lane] : 0u;
            const float sv = lane < kept ? lsc[lane] : 0.f;
            const unsigned long long bal = __ballot(mine);
            __builtin_amdgcn_wave_barrier();
            if (mine) {
                const int pos = __popcll(bal & ((1ull << lane) - 1ull));
                lrow[pos] = r;
                lsc[pos] = sv;
            }
            __builtin_amdgcn_wave_barrier();
            kept = __popcll(bal);
        }
        const float thr = runmax - w2;
        const bool add = (l == 0) && row >= 0 && sc >= thr;
        const unsigned long long bal = __ballot(add);
        if (add) {
            const int pos = kept + __popcll(bal & ((1ull << lane) - 1ull));
            if (pos < REFINE_KEEP) {
                lrow[pos] = (unsigned)row;
                lsc[pos] = sc;
            }
        }
        kept += __popcll(bal);
        if (kept > REFINE_KEEP) {
            overflow = true;
            kept = REFINE_KEEP;
        }
        __builtin_amdgcn_wave_barrier();
    }
    // result: the kept rows become the query's single-row candidate list (or the query goes to the all-pairs kernel)
    __device__ __forceinline__ void finish(int64_t qi, unsigned* mycand, int* cand_cnt, int* fb_count, int* fb_list, int stats) {
        __builtin_amdgcn_wave_barrier();
        if (overflow) {  // > REFINE_KEEP rows tie within the fp32 margin: the all-pairs kernel decides
            if (lane == 0) {
                cand_cnt[qi] = -1;
                const int slot = atomicAdd(fb_count, 1);
                fb_list[slot] = (int)qi;
            }
            return;
        }
        if (stats && lane == 0) {  // statistics: [1] queries refined, [3] rows they keep
            atomicAdd(fb_count + 1, 1);
            atomicAdd(fb_count + 3, kept);
        }
        if (lane < kept) {
            const unsigned row = lrow[lane];
            mycand[lane] = ((row / CHUNK_ROWS) << 8) | (row % CHUNK_ROWS);
        }
        if (lane == 0) cand_cnt[qi] = kept;
    }
};

// int8 pass: which rows of a query's candidate chunks matter.  One wave per query; per candidate chunk the exact integer
// scores of its 128 rows against the query (v_dot4 over the chunk's four int8 tiles: 48 KB, contiguous, L2 / Infinity-Cache
// resident -- the whole int8 map is 77 MB at C2 -- instead of 196 KB of fp32 rows); every row whose upper bound reaches the
// query's lower bound replaces the chunk entries as a single-row entry.  Few registers on purpose (the loop is latency-bound:
// 8 x 16 bytes per lane in flight, 8 waves per SIMD); match_refine_kernel / match_rescore_kernel then see the lists the fp16
// pass would have produced.
__global__ __launch_bounds__(256) void match_rescan_kernel(int64_t n, int64_t m, int d, I8Bounds ib, const uint4* __restrict__ q8,
                                                           const uint4* __restrict__ b8, const unsigned* __restrict__ qmax,
                                                           int* __restrict__ cand_cnt, unsigned* __restrict__ cand, int cap,
                                                           unsigned* __restrict__ hits, int hcap, int* __restrict__ fb_count,
                                                           int* __restrict__ fb_list, int use_gate, float gate,
                                                           const int* __restrict__ guard, L2Terms l2) {
    __shared__ uint4 l_q8[4][48];  // the query's int8 row, unit by unit (d <= 768)
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int64_t qi = (int64_t)blockIdx.x * 4 + wave;
    if (qi >= n) return;
    if (guard && *guard) {   // half-width pass, too many survivors: the lists start empty for match_gatepass_kernel's row hits
        if (lane == 0) cand_cnt[qi] = 0;
        return;
    }
    const int cnt = cand_cnt[qi];
    if (cnt <= 0) return;  // zero query / below the gate (-2) / overflow (-1)
    if (cnt > cap) {       // (fused half-width pass: more bin overflows than the list holds) the all-pairs kernel decides
        if (lane == 0) {
            cand_cnt[qi] = -1;
            fb_list[atomicAdd(fb_count, 1)] = (int)qi;
        }
        return;
    }
    unsigned* mycand = cand + (size_t)qi * cap;
    unsigned* myhits = hits + (size_t)qi * hcap;
    const int units8 = d >> 4;  // 16-byte units per int8 row
    if (lane < units8) l_q8[wave][lane] = q8[(size_t)(qi >> 5) * (units8 * 32) + (size_t)lane * 32 + (qi & 31)];
    const float eq = ib.qerr[qi];
    const float sq = ib.qstep[qi >> 7], A = eq * 1.0001220703125f + 1.0e-6f, mult = 1.0001220703125f + eq;
    const float qlow = use_gate ? gate : key_float(qmax[qi]);   // half-width pass: the hit test is the gate itself
    const float qn_l2 = l2.qn ? l2.qn[qi] : 0.0f;
    __builtin_amdgcn_wave_barrier();
    int nhit = 0;  // wave-uniform
    // Up to 64 entries (nearly every query): they sit in registers, one per lane, before the first hit is written, so the
    // hits go straight into the query's list.  Longer lists collect their hits in the scratch list and copy them back.
    const bool direct = cnt <= 64;
    unsigned* out = direct ? mycand : myhits;
    const int ocap = direct ? cap : hcap;
    for (int e0 = 0; e0 < cnt; e0 += 64) {
        const unsigned batch = (e0 + lane < cnt) ? mycand[e0 + lane] : 0u;
        const int nb = cnt - e0 < 64 ? cnt - e0 : 64;
        for (int j = 0; j < nb; ++j) {
            const unsigned entry = __shfl(batch, j);  // wave-uniform
            const int c = (int)(entry >> 8);
            if (!(entry & 128u)) {  // a single-row entry (top-2 records: the chunk's second-best cannot reach the bound)
                if (lane == 0 && nhit < ocap) out[nhit] = entry;
                ++nhit;
                continue;
            }
            const long long base = (long long)c * CHUNK_ROWS;
            const float sc = sq * ib.bstep[c], bound = A + mult * ib.berr[c];
            // rows `lane` and `lane + 64` of the chunk (tile rr >> 5, position rr & 31); the loads of both go out together:
            // 16 x 16 bytes per lane in flight, three round trips per chunk at d = 384 (the loop is latency-bound)
            const uint4* src0 = b8 + ((size_t)c * 4 + (lane >> 5)) * (size_t)(units8 * 32) + (lane & 31);
            const uint4* src1 = src0 + 2 * (size_t)(units8 * 32);
            int acc2[2] = {0, 0};
            for (int u0 = 0; u0 < units8; u0 += 8) {  // units8 = 16, 24, 32, 40 or 48
                uint4 bv0[8], bv1[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    bv0[k] = src0[(u0 + k) * 32];
                    bv1[k] = src1[(u0 + k) * 32];
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint4 qv = l_q8[wave][u0 + k];
                    acc2[0] = __builtin_amdgcn_sdot4((int)bv0[k].x, (int)qv.x, acc2[0], false);
                    acc2[0] = __builtin_amdgcn_sdot4((int)bv0[k].y, (int)qv.y, acc2[0], false);
                    acc2[0] = __builtin_amdgcn_sdot4((int)bv0[k].z, (int)qv.z, acc2[0], false);
                    acc2[0] = __builtin_amdgcn_sdot4((int)bv0[k].w, (int)qv.w, acc2[0], false);
                    acc2[1] = __builtin_amdgcn_sdot4((int)bv1[k].x, (int)qv.x, acc2[1], false);
                    acc2[1] = __builtin_amdgcn_sdot4((int)bv1[k].y, (int)qv.y, acc2[1], false);
                    acc2[1] = __builtin_amdgcn_sdot4((int)bv1[k].z, (int)qv.z, acc2[1], false);
                    acc2[1] = __builtin_amdgcn_sdot4((int)bv1[k].w, (int)qv.w, acc2[1], false);
                }
            }
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int rr = lane + 64 * half;
                const int acc = acc2[half];
                float up = sc * (float)acc + bound;
                if (l2.qn) up = l2_upper_row(qn_l2, l2.bn[base + rr], up, l2.slack);
                const bool hit = base + rr < m && up >= qlow;
                const unsigned long long bal = __ballot(hit);
                if (hit) {
                    const int pos = nhit + __popcll(bal & ((1ull << lane) - 1ull));
                    if (pos < ocap) out[pos] = ((unsigned)c << 8) | (unsigned)rr;
                }
                nhit += __popcll(bal);
            }
        }
    }
    if (nhit > ocap || nhit > cap) {  // more rows inside the bounds than a list holds: the all-pairs kernel decides
        if (lane == 0) {
            cand_cnt[qi] = -1;
            const int slot = atomicAdd(fb_count, 1);
            fb_list[slot] = (int)qi;
        }
        return;
    }
    if (!direct) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");  // the hits written above are read back by other lanes
        for (int i = lane; i < nhit; i += 64) mycand[i] = myhits[i];
    }
    if (lane == 0) {
        cand_cnt[qi] = nhit;
        // (match_rescan_close_kernel builds the refinement's work list from the final counts: lists of eight rows or more;
        // up to seven rows go straight to the fp64 decision -- a handful of fp64 dot products costs less than the latency
        // of one refinement wave)
    }
}

// dense records: the candidate entries of match_select_kernel (int8 pass: as rewritten by match_rescan_kernel)
template <int NT>
__global__ __launch_bounds__(256) void match_refine_kernel(Rows q, const float* __restrict__ invq,
                                                           Rows b, const float* __restrict__ invb,
                                                           int64_t n, int64_t m, int d, float w2, int* __restrict__ cand_cnt,
                                                           unsigned* __restrict__ cand, int cap, int* __restrict__ fb_count,
                                                           int* __restrict__ fb_list, int stats, const int* __restrict__ todo,
                                                           const int* __restrict__ todo_count, const float* __restrict__ cand_up,
                                                           const unsigned* __restrict__ hit_cnt, I8Bounds ib) {
    __shared__ unsigned l_row[4][REFINE_KEEP];
    __shared__ float l_sc[4][REFINE_KEEP];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    // todo != NULL (int8 pass): the queries match_rescan_close_kernel found crowded, a list whose length is on the device -- one wave
    // per possible entry, waves past its end leave at once (the loop serves a caller that launches fewer); otherwise one wave per query
    const int64_t slot0 = (int64_t)blockIdx.x * 4 + wave;
    const int64_t nslots = todo ? (int64_t)*todo_count : n;
  for (int64_t slot = slot0; slot < nslots; slot += (int64_t)gridDim.x * 4) {
    const int64_t qi = todo ? (int64_t)todo[slot] : slot;
    if (qi >= n) return;
    // Everything that depends on the query's index alone is requested at once -- the list's length, how much of it the chunk-major
    // rescan appended, the query's E and 1 / |q|, the first 64 entries with their upper bounds -- and the query's row (R.init) right
    // behind: a query had been a chain of seven dependent round trips (length -> entries -> flags -> appended count -> bounds ->
    // entries again -> rows), 60 us per query at 9891 queries on 4096 waves.
    unsigned* mycand = cand + (size_t)qi * cap;
    const float* myup = cand_up ? cand_up + (size_t)qi * cap : nullptr;
    const int cnt = cand_cnt[qi];
    const int hits = cand_up ? (int)hit_cnt[(size_t)qi * BIN_CNT_STRIDE] : 0;
    const float eq = cand_up ? ib.qerr[qi] : 0.0f;
    const float iq = invq[qi];
    const unsigned ce0 = mycand[lane];                  // (cap >= 64: the first 64 slots exist whatever the length)
    const float up0 = cand_up ? myup[lane] : 0.0f;
    if (cnt <= 0) continue;  // zero query / nothing / overflow (-1: the all-pairs kernel decides)
    // wave-uniform: is this list crowded?
    bool flagged = lane < cnt && (ce0 & 128u) != 0u;
    for (int e = 64 + lane; e < cnt; e += 64) flagged |= (mycand[e] & 128u) != 0u;
    if (cnt < REFINE_MIN && !__any(flagged)) continue;
    RefineWave<NT> R;
    R.init(q, iq, qi, b, invb, d, w2, l_row[wave], l_sc[wave]);
    // The rows the chunk-major rescan appended (the last hit_cnt entries of the list) carry the upper bound U = s_q s_c S + A + B_c of
    // their exact score (cand_up), S their exact integer score; U - 2 (A + B_c) is a LOWER bound of the same score.  The rescans tested
    // a row against the coarse pass's lower bound of the query's maximum -- the fp6 image's, 0.06 below the maximum on unit rows, so
    // that 45 rows per query came through on lifted descriptors where 13 lie inside the int8 bounds --; here every
    // row is tested against the best lower bound among the list's own rows, and the rest never has its 1.5 KB fp32 row read.  A row
    // dropped has U < L <= the exact score of another row of the list: it is not the arg-max and does not tie with it.
    int split = cnt;        // first appended entry
    float lowest = -__builtin_inff();
    if (cand_up) {
        split = cnt - hits < 0 ? 0 : cnt - hits;
        const float A = eq * 1.0001220703125f + 1.0e-6f, mult = 1.0001220703125f + eq;
        if (lane >= split && lane < cnt) {
            const float bnd = A + mult * ib.berr[ce0 >> 8];
            if (up0 < 3.0e38f) lowest = (up0 - 2.0f * bnd) - 4.0e-6f;   // (fp32 evaluation of U and of this line: a few 1e-7)
        }
        for (int e = (split > 64 ? split : 64) + lane; e < cnt; e += 64) {
            const float u = myup[e];
            const float bnd = A + mult * ib.berr[mycand[e] >> 8];
            if (u < 3.0e38f) lowest = fmaxf(lowest, (u - 2.0f * bnd) - 4.0e-6f);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) lowest = fmaxf(lowest, __shfl_xor(lowest, off));
    }
    // single-row entries: 4 per pass, 64 list entries per load, the next pass's rows in flight under the current pass's sums (a
    // pass had been two dependent round trips -- the entry, then the row --: 164 us at the 25 rows per query of lifted descriptors)
    for (int e0 = 0; e0 < cnt; e0 += 64) {
        const int nblk = cnt - e0 < 64 ? cnt - e0 : 64;
        long long myrow = -1;
        if (lane < nblk) {
            const unsigned ce = e0 == 0 ? ce0 : mycand[e0 + lane];
            if (!(ce & 128u)) {
                myrow = (long long)(ce >> 8) * CHUNK_ROWS + (ce & 127u);
                if (myrow >= m) myrow = -1;
                if (e0 + lane >= split && (e0 == 0 ? up0 : myup[e0 + lane]) < lowest) myrow = -1;
            }
        }
        if (!__any(myrow >= 0)) continue;
        // the rows that are left, packed to the front (the dropped ones are scattered through the list: a pass of four costs its
        // round trip as long as one of its rows is live)
        const unsigned long long keep = __ballot(myrow >= 0);
        const int nkeep = __popcll(keep);
        {
            // lane l takes the row of the l-th live lane: the position of the l-th set bit of `keep`, by halving
            int need = lane, src = 0;
            unsigned long long rest = keep;
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1) {
                const unsigned long long lowmask = (1ull << sh) - 1ull;
                const int below = __popcll(rest & lowmask);
                if (need >= below) {
                    need -= below;
                    rest >>= sh;
                    src += sh;
                } else {
                    rest &= lowmask;
                }
            }
            const long long packed = __shfl(myrow, src & 63);
            myrow = lane < nkeep ? packed : -1;
        }
        const int nblk_keep = nkeep;
        auto row_at = [&](int p) { return p < nblk_keep ? __shfl(myrow, (p + R.g) & 63) : -1ll; };   // (lanes >= nkeep hold -1)
        typename RefineWave<NT>::Row ra, rb;
        long long rowa = row_at(0), rowb;
        R.load4(ra, rowa);
        for (int p = 0; p < nblk_keep; p += 8) {
            rowb = row_at(p + 4);
            R.load4(rb, rowb);
            if (__any(rowa >= 0)) R.consider(rowa, R.dot4(ra, rowa));
            rowa = row_at(p + 8);
            R.load4(ra, rowa);
            if (__any(rowb >= 0)) R.consider(rowb, R.dot4(rb, rowb));
        }
    }
    // whole-chunk entries: all 128 rows of the chunk
    for (int e = 0; e < cnt; ++e) {
        const unsigned ce = mycand[e];  // wave-uniform
        if (!(ce & 128u)) continue;
        const long long base = (long long)(ce >> 8) * CHUNK_ROWS;
        for (int r0 = 0; r0 < CHUNK_ROWS; r0 += 4) {
            long long row = base + r0 + R.g;
            if (row >= m) row = -1;
            if (__any(row >= 0)) R.consider(row, R.score4(row));
        }
    }
    if (R.overflow) continue;  // > REFINE_KEEP rows tie within the fp32 margin (exact duplicates): the list stays as
                               // match_select_kernel wrote it and match_rescore_kernel decides all of it in fp64
    R.finish(qi, mycand, cand_cnt, fb_count, fb_list, stats);
    __builtin_amdgcn_wave_barrier();
  }
}

// sparse records (match_coarse_pipe_kernel<., true>): filter the query's records against its FINAL coarse maximum, then
// refine in fp32 if more than two rows remain.  Replaces match_select_kernel + match_refine_kernel; one wave per query.
__global__ __launch_bounds__(256) void match_filter_refine_kernel(Rows q, const float* __restrict__ invq,
                                                                  Rows b, const float* __restrict__ invb,
                                                                  int64_t n, int64_t m, int d, float window, float w2,
                                                                  const unsigned* __restrict__ qmax,
                                                                  const unsigned* __restrict__ rec_cnt, const uint2* __restrict__ rec,
                                                                  int rcap, int* __restrict__ cand_cnt, unsigned* __restrict__ cand,
                                                                  int cap, int* __restrict__ fb_count, int* __restrict__ fb_list, int stats) {
    __shared__ unsigned l_row[4][REFINE_KEEP];
    __shared__ float l_sc[4][REFINE_KEEP];
    __shared__ unsigned l_cand[4][FILTER_LDS_ROWS];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int64_t qi = (int64_t)blockIdx.x * 4 + wave;
    if (qi >= n) return;
    unsigned* mycand = cand + (size_t)qi * cap;
    const float iq = invq[qi];
    if (iq == 0.0f) {  // zero query row: decided directly by match_rescore_kernel (index 0, score 0)
        if (lane == 0) cand_cnt[qi] = 0;
        return;
    }
    const unsigned total = rec_cnt[qi];
    if (stats && lane == 0) {  // statistics: [4] records written by the coarse pass
        atomicAdd(fb_count + 4, (int)total);
    }
    if (total > (unsigned)rcap || m <= 0) {  // record overflow: the all-pairs kernel decides
        if (lane == 0) {
            cand_cnt[qi] = -1;
            const int slot = atomicAdd(fb_count, 1);
            fb_list[slot] = (int)qi;
        }
        return;
    }
    const unsigned thr = __float_as_uint(__uint_as_float(qmax[qi]) - window);
    const uint2* myrec = rec + (size_t)qi * rcap;
    unsigned* lc = l_cand[wave];
    int ncand = 0;  // wave-uniform
    for (unsigned e0 = 0; e0 < total; e0 += 64) {
        const unsigned e = e0 + lane;
        uint2 r = make_uint2(0u, 0u);
        if (e < total) r = myrec[e];
        const bool in = e < total && r.y >= thr;
        const unsigned long long bal = __ballot(in);
        if (in) lc[ncand + __popcll(bal & ((1ull << lane) - 1ull))] = r.x;
        ncand += __popcll(bal);
    }
    __builtin_amdgcn_wave_barrier();
    if (stats && lane == 0) {  // statistics: [2] candidate rows, [8 + b] queries with 2^(b-1) < rows <= 2^b
        atomicAdd(fb_count + 2, ncand);
        int bin = 0;
        while ((1 << bin) < ncand && bin < 15) ++bin;
        atomicAdd(fb_count + 8 + bin, 1);
    }
    if (ncand < REFINE_MIN) {
        if (lane < ncand) {
            const unsigned row = lc[lane];
            mycand[lane] = ((row / CHUNK_ROWS) << 8) | (row % CHUNK_ROWS);
        }
        if (lane == 0) cand_cnt[qi] = ncand;
        return;
    }
    RefineWave<12> R;
    R.init(q, iq, qi, b, invb, d, w2, l_row[wave], l_sc[wave]);
    for (int e0 = 0; e0 < ncand; e0 += 4) {
        const long long row = (e0 + R.g < ncand) ? (long long)lc[e0 + R.g] : -1;
        R.consider(row, R.score4(row));
    }
    if (R.overflow && ncand <= cap) {  // > REFINE_KEEP rows tie within the fp32 margin (exact duplicates): hand ALL
        for (int e = lane; e < ncand; e += 64) {  // candidates to the fp64 decision instead of the all-pairs kernel
            const unsigned row = lc[e];
            mycand[e] = ((row / CHUNK_ROWS) << 8) | (row % CHUNK_ROWS);
        }
        if (lane == 0) cand_cnt[qi] = ncand;
        return;
    }
    R.finish(qi, mycand, cand_cnt, fb_count, fb_list, stats);
}

// Exact decision among the candidates: one workgroup (4 waves) owns 64 queries; thread t < 64 = query t.
//   single-row candidates (the common case, ~1.3 per query): the block's (query, candidate) pairs are
//   flattened and taken 64 at a time; per batch and per 96-wide k chunk the four waves compute the fp64
//   products of the 64 pairs k-parallel (coalesced row segments, 16 pairs per wave; fp32 normalisation as
//   faiss leaves it, products of two fp32 are exact in fp64) into LDS, then wave 0 adds every pair's 96
//   products in ascending k -- 64 different in-order chains at once instead of one chain per wavefront.
//   whole-chunk candidates (rare): per flagged query, the lanes of wave 0 score their own rows of the chunk.
// The accumulation order is the oracle's (sequential k), ties -> lowest index, sim = (float)score.
//
// QB ("rescore_block"): queries per workgroup.  64: as above -- wave 0 owns the queries, ceil(n / 64) workgroups of 65 KB of LDS each, on
// D.2 data about 32 pairs per workgroup: half a batch, three waves at barriers, more than one workgroup per compute unit for ~10 000 dot
// products.  256: thread t = query t, the pair counts are prefix-summed over the four waves (per wave, then the waves' totals through
// the LDS), and an epoch's pairs are dealt to the four waves in equal runs, LANE = PAIR: a lane reads its query row and its map row
// itself (64 bytes of each per step, the next step's loads in flight) and adds the products in ascending k (dot_pair_f64) -- no product
// staging, no barrier inside an epoch, 14 KB of LDS, a quarter of the workgroups.  Every fp64 sum is the same chain of the same values
// and every query folds its own pairs in the same order: idx / sim are bit-identical.  Whole-chunk entries: each wave takes its own
// flagged queries (a normalised row per wave in the LDS).
constexpr int RS_KC = 96;             // k values per chunk (24 float4 per row)
constexpr int RS_STRIDE = RS_KC + 1;  // doubles per LDS row: 194 words == 2 (mod 64) -> conflict-free ds_read_b64
constexpr int RS_PAIRS = 1024;        // pair slots per epoch (a block has ~80 pairs; more run in further epochs)
template <int QB>
__global__ __launch_bounds__(256) void match_rescore_kernel(Rows q, const float* __restrict__ invq,
                                                            Rows b, const float* __restrict__ invb,
                                                            int64_t n, int64_t m, int d, const int* __restrict__ cand_cnt,
                                                            const unsigned* __restrict__ cand, int cap,
                                                            int64_t* __restrict__ idx_out, float* __restrict__ sim_out, float min_sim) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* P = reinterpret_cast<double*>(smem);               // [64][RS_STRIDE] products (QB 64 only)
    double* pscore = P + (QB > 64 ? 0 : 64 * RS_STRIDE);       // [RS_PAIRS] exact score per pair of the epoch
    float* qn = reinterpret_cast<float*>(pscore + RS_PAIRS);   // [QB / 64][d] normalised query row (chunk rescans), one per owning wave
    constexpr int NW = QB / 64;                                // waves that own queries
    static_assert(QB == 64 || QB == 256, "a workgroup's queries: wave 0's lanes, or its 256 threads (p_q holds a query as a byte)");
    __shared__ unsigned p_j[RS_PAIRS];                         // pair -> map row
    __shared__ unsigned char p_q[RS_PAIRS];                    // pair -> query of the block
    __shared__ long long s_j[QB > 64 ? 1 : 64];                // (QB 64) the batch's slots
    __shared__ float s_iq[QB > 64 ? 1 : 64], s_ib[QB > 64 ? 1 : 64];
    __shared__ int s_ql[QB > 64 ? 1 : 64];
    __shared__ int s_wsum[4];                                  // pairs of each owning wave's queries
    __shared__ float s_qinv[QB > 64 ? QB : 1];                 // (QB 256) 1 / |q| of every query of the block: a pair's query may live in another wave
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int64_t q0 = (int64_t)blockIdx.x * QB;
    // per-query state lives in the owning waves: wave 0 (lane = query, and the batches' slots and chains), or all four (thread = query)
    const int myq = QB > 64 ? (int)threadIdx.x : lane;         // the thread's query of the block
    const int64_t qi = q0 + myq;
    const bool owner = wave < NW, lead = wave == 0;
    const bool have = owner && qi < n;
    const float iq = have ? invq[qi] : 0.0f;
    int cnt = have ? cand_cnt[qi] : 0;
    if (iq == 0.0f || cnt < 0) cnt = 0;  // zero query: decided below; overflow (-1): match_exact_kernel's
    bool any_rescan = false;
    int my_off = 0, my_pairs = 0;
    const unsigned* mycand = cand + (size_t)(have ? qi : 0) * cap;
    auto row_of = [&](unsigned ce) { return (long long)(ce >> 8) * CHUNK_ROWS + (ce & 127u); };
    if (owner) {
        // flatten: the single-row candidates of query `lane` become pairs [my_off, my_off + my_pairs)
        for (int e = 0; e < cnt; ++e) {
            const unsigned ce = mycand[e];
            if (ce & 128u) any_rescan = true;
            else if (row_of(ce) < m) ++my_pairs;
        }
        int incl = my_pairs;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        my_off = incl - my_pairs;
        if (lane == 63) s_wsum[wave] = incl;
        if constexpr (QB > 64) s_qinv[myq] = iq;
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int ws = s_wsum[w];
        if (w < wave) my_off += ws;
        total += ws;
    }
    double best = 0.0;
    long long bj = -1;
    for (int E0 = 0; E0 < total; E0 += RS_PAIRS) {  // one epoch unless a block has > RS_PAIRS pairs
        const int ecount = min(RS_PAIRS, total - E0);
        if (owner) {
            int k = my_off;
            for (int e = 0; e < cnt; ++e) {
                const unsigned ce = mycand[e];
                if ((ce & 128u) || row_of(ce) >= m) continue;
                if (k >= E0 && k < E0 + RS_PAIRS) {
                    p_j[k - E0] = (unsigned)row_of(ce);
                    p_q[k - E0] = (unsigned char)myq;
                }
                ++k;
            }
        }
        __syncthreads();
        if constexpr (QB > 64) {
            // wave w takes pairs [w per, (w + 1) per) of the epoch, 64 at a time: lane = pair
            const int per = (ecount + 3) >> 2, wend = min(ecount, (wave + 1) * per);
            for (int p0 = wave * per; p0 < wend; p0 += 64) {
                const int pid = p0 + lane;
                if (pid < wend) {
                    const long long j = (long long)p_j[pid];
                    const int ql = (int)p_q[pid];
                    pscore[pid] = dot_pair_f64(q, (q0 + ql) * (int64_t)d, s_qinv[ql], b, j * (int64_t)d, invb[j], d);
                }
            }
        } else {
        for (int p0 = 0; p0 < ecount; p0 += 64) {   // (the loop keeps the parent's indentation)
            // slot `lane` of this batch = pair p0 + lane of the epoch
            long long j = -1;
            if (lead) {
                const int pid = p0 + lane;
                const int ql = (pid < ecount) ? (int)p_q[pid] : 0;
                const float iqq = __shfl(iq, ql);  // all lanes of wave 0 take part
                float ibb = 0.f;
                if (pid < ecount) {
                    j = (long long)p_j[pid];
                    ibb = invb[j];
                }
                s_j[lane] = j;
                s_ql[lane] = ql;
                s_iq[lane] = iqq;
                s_ib[lane] = ibb;
            }
            __syncthreads();
            double acc = 0.0;
            // wave w takes slots 16 w .. 16 w + 15, two per pass (lanes 0..23 and 32..55: one float4 of k each);
            // the row segments of chunk c+1 are fetched while wave 0 runs the chains of chunk c
            const int sub = lane >> 5, l4 = lane & 31;
            float4 qv[8], bv[8];
            auto fetch = [&](int k0) {
                const int kn = min(RS_KC, d - k0);
#pragma unroll
                for (int it = 0; it < 8; ++it) {
                    const int sl = 16 * wave + 2 * it + sub;
                    const long long jj = s_j[sl];
                    if (jj >= 0 && 4 * l4 < kn) {
                        qv[it] = q.ld4((q0 + s_ql[sl]) * (int64_t)d + k0 + 4 * l4);
                        bv[it] = b.ld4(jj * (int64_t)d + k0 + 4 * l4);
                    }
                }
            };
            fetch(0);
            for (int k0 = 0; k0 < d; k0 += RS_KC) {
                const int kn = min(RS_KC, d - k0);  // d % 4 == 0
#pragma unroll
                for (int it = 0; it < 8; ++it) {
                    const int sl = 16 * wave + 2 * it + sub;
                    if (s_j[sl] >= 0 && 4 * l4 < kn) {
                        const float iqq = s_iq[sl], ibb = s_ib[sl];
                        double* dst = P + sl * RS_STRIDE + 4 * l4;
                        dst[0] = prod_norm_f64(qv[it].x, iqq, bv[it].x, ibb);
                        dst[1] = prod_norm_f64(qv[it].y, iqq, bv[it].y, ibb);
                        dst[2] = prod_norm_f64(qv[it].z, iqq, bv[it].z, ibb);
                        dst[3] = prod_norm_f64(qv[it].w, iqq, bv[it].w, ibb);
                    }
                }
                __syncthreads();
                if (k0 + RS_KC < d) fetch(k0 + RS_KC);
                if (lead && j >= 0) {
                    const double* src = P + lane * RS_STRIDE;
                    int k = 0;
                    for (; k + 8 <= kn; k += 8) {  // reads first, then the in-order chain
                        double v[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) v[u] = src[k + u];
#pragma unroll
                        for (int u = 0; u < 8; ++u) acc = acc + v[u];
                    }
                    for (; k < kn; ++k) acc = acc + src[k];
                }
                __syncthreads();
            }
            if (lead && j >= 0) pscore[p0 + lane] = acc;
        }
        }
        __syncthreads();
        if (owner) {  // every query folds its own pairs of this epoch: best score, ties -> lowest index
            const int lo = max(my_off, E0), hi = min(my_off + my_pairs, E0 + RS_PAIRS);
            for (int k = lo; k < hi; ++k) {
                const long long j = (long long)p_j[k - E0];
                const double sc = pscore[k - E0];
                take_if_before(sc, j, best, bj);
            }
        }
        __syncthreads();
    }
    if (!owner) return;
    // whole-chunk candidates: an owning wave takes its flagged queries one by one
    if (__any(any_rescan)) {
        if constexpr (QB > 64) qn += (size_t)wave * d;
        for (int ql = 0; ql < 64; ++ql) {
            if (!__shfl((int)any_rescan, ql)) continue;  // wave-uniform
            const int64_t qq = q0 + (myq - lane) + ql;
            const float iqq = __shfl(iq, ql);
            const int cq = __shfl(cnt, ql);
            __builtin_amdgcn_wave_barrier();
            for (int k = lane * 4; k < d; k += 256) {
                float4 v = q.ld4(qq * (int64_t)d + k);
                v.x = v.x * iqq; v.y = v.y * iqq; v.z = v.z * iqq; v.w = v.w * iqq;
                *reinterpret_cast<float4*>(qn + k) = v;
            }
            __builtin_amdgcn_wave_barrier();
            double rbest = 0.0;
            long long rj = -1;
            for (int e = 0; e < cq; ++e) {
                const unsigned ce = cand[(size_t)qq * cap + e];
                if (!(ce & 128u)) continue;
                const long long base = (long long)(ce >> 8) * CHUNK_ROWS;
                for (int li = lane; li < CHUNK_ROWS; li += 64) {
                    const long long j = base + li;
                    if (j < m) {
                        const double sc = dot_norm_f64(qn, b, j * (int64_t)d, invb[j], d);
                        take_if_before(sc, j, rbest, rj);
                    }
                }
            }
            wave_argmax(rbest, rj);
            if (lane == ql) take_if_before(rbest, rj, best, bj);
        }
    }
    if (!have) return;
    if (iq == 0.0f) {  // zero query: every score is 0.0, the lowest index wins
        idx_out[qi] = (m > 0) ? 0 : -1;
        sim_out[qi] = 0.0f;
    } else if (cand_cnt[qi] >= 0) {
        // (half-width pass: min_sim = the gate -- the lists hold only rows of chunks that could reach it, so a best below it
        // is not the oracle's arg-max but the proof that the query has no match; otherwise min_sim = -Inf)
        const bool ok = !((float)best < min_sim) && bj >= 0;
        idx_out[qi] = ok ? bj : -1;
        sim_out[qi] = ok ? (float)best : -2.0f;
    } else if (cand_cnt[qi] == -2) {  // below the caller's gate (match_select_kernel)
        idx_out[qi] = -1;
        sim_out[qi] = -2.0f;
    }
}

// all-pairs exact decision for the queries in `list` (or all queries if list == NULL)
__global__ __launch_bounds__(256) void match_exact_kernel(Rows q, const float* __restrict__ invq,
                                                          Rows b, const float* __restrict__ invb,
                                                          int64_t n, int64_t m, int d, const int* __restrict__ list,
                                                          const int* __restrict__ list_count,
                                                          int64_t* __restrict__ idx_out, float* __restrict__ sim_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* qn = reinterpret_cast<float*>(smem);
    double* rs = reinterpret_cast<double*>(smem + (((size_t)d * 4 + 15) & ~(size_t)15));
    long long* rj = reinterpret_cast<long long*>(rs + 4);
    const int64_t count = list ? (int64_t)*list_count : n;
    for (int64_t e = blockIdx.x; e < count; e += gridDim.x) {
        const int64_t qi = list ? (int64_t)list[e] : e;
        const float iq = invq ? invq[qi] : 1.0f;
        __syncthreads();
        for (int k = threadIdx.x; k < d; k += 256) qn[k] = q.ld1(qi * (int64_t)d + k) * iq;
        __syncthreads();
        double best = 0.0;
        long long bj = -1;
        for (long long j = threadIdx.x; j < m; j += 256) {
            const double s = dot_norm_f64(qn, b, j * (int64_t)d, invb ? invb[j] : 1.0f, d);
            if (bj < 0 || s > best) {   // (a thread's j ascends: an equal score never replaces an earlier row -- decided_before's answer)
                best = s;
                bj = j;
            }
        }
        // block_argmax's steps, a copy: with the call the compiler scheduled the loop above as one dependent chain (the fourth product
        // behind the third sum) and vfm_match_ip_top1(EXACT) at 2 000 x 200 000 x 384 took 360.9 ms instead of 357.5
        wave_argmax(best, bj);
        if (lane_id() == 0) {
            rs[threadIdx.x >> 6] = best;
            rj[threadIdx.x >> 6] = bj;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; ++w) take_if_before(rs[w], rj[w], rs[0], rj[0]);
            idx_out[qi] = (m > 0) ? rj[0] : -1;
            sim_out[qi] = (m > 0) ? (float)rs[0] : 0.0f;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// threshold + stable compaction (VoxelHashMap.cpp:501-511, 587-600), single workgroup
// ---------------------------------------------------------------------------------------------
// (one workgroup: the order of the survivors is the order of the queries.  A pass takes TC_ITERS x 1024 queries: all of a thread's
// similarities are loaded at once, the per-wave counts of every 1024-query slab go to the LDS behind ONE barrier, and the gathers
// of the survivors -- matched row, then its coordinates -- are in flight together; a slab at a time, three dependent round trips and
// three barriers each, it was 25 us for 20 000 queries on the path every registration's RANSAC waits for.)
constexpr int TC_ITERS = 4;   // (8: the arrays spilled at 1024 threads)
__global__ __launch_bounds__(1024) void threshold_compact_kernel(const float* __restrict__ sim, const int64_t* __restrict__ idx,
                                                                 int64_t n, double thr, int64_t* __restrict__ keep,
                                                                 int64_t* __restrict__ count, int32_t* __restrict__ corres,
                                                                 const double* __restrict__ qxyz, const double* __restrict__ bxyz,
                                                                 double* __restrict__ src_out, double* __restrict__ tgt_out) {
    __shared__ int wsum[TC_ITERS][16];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    int64_t base = 0;   // survivors in front of this pass (the same value in every thread)
    for (int64_t s0 = 0; s0 < n; s0 += (int64_t)TC_ITERS * 1024) {
        bool valid[TC_ITERS];
        int before[TC_ITERS];
        float sv[TC_ITERS];
#pragma unroll
        for (int t = 0; t < TC_ITERS; ++t) {
            const int64_t i = s0 + (int64_t)t * 1024 + threadIdx.x;
            sv[t] = i < n ? sim[i] : 0.0f;
        }
#pragma unroll
        for (int t = 0; t < TC_ITERS; ++t) {
            const int64_t i = s0 + (int64_t)t * 1024 + threadIdx.x;
            valid[t] = (i < n) && !((double)sv[t] < thr);
            const unsigned long long bal = __ballot(valid[t]);
            before[t] = __popcll(bal & ((1ull << lane) - 1ull));
            if (lane == 0) wsum[t][wave] = __popcll(bal);
        }
        __syncthreads();
        int64_t k[TC_ITERS];
        int j[TC_ITERS];   // (map rows fit 31 bits: the candidate entries hold chunk << 8)
        int64_t run = base;
#pragma unroll
        for (int t = 0; t < TC_ITERS; ++t) {
            int woff = 0, tot = 0;
#pragma unroll
            for (int w = 0; w < 16; ++w) {
                const int c = wsum[t][w];
                if (w < wave) woff += c;
                tot += c;
            }
            k[t] = run + woff + before[t];
            run += tot;
            const int64_t i = s0 + (int64_t)t * 1024 + threadIdx.x;
            j[t] = (valid[t] && idx) ? (int)idx[i] : 0;
        }
        base = run;
#pragma unroll
        for (int t = 0; t < TC_ITERS; ++t) {
            if (!valid[t]) continue;
            const int64_t i = s0 + (int64_t)t * 1024 + threadIdx.x;
            keep[k[t]] = i;
            if (corres) {
                corres[2 * k[t] + 0] = (int32_t)i;
                corres[2 * k[t] + 1] = (int32_t)j[t];
            }
            if (src_out) {
                src_out[3 * k[t] + 0] = qxyz[3 * i + 0];
                src_out[3 * k[t] + 1] = qxyz[3 * i + 1];
                src_out[3 * k[t] + 2] = qxyz[3 * i + 2];
            }
            if (tgt_out) {
                tgt_out[3 * k[t] + 0] = bxyz[3 * (int64_t)j[t] + 0];
                tgt_out[3 * k[t] + 1] = bxyz[3 * (int64_t)j[t] + 1];
                tgt_out[3 * k[t] + 2] = bxyz[3 * (int64_t)j[t] + 2];
            }
        }
        __syncthreads();   // wsum is rewritten by the next pass
    }
    if (threadIdx.x == 0) *count = base;
}

// 1/|row| only (the EXACT modes), one wave per row.  The sum of squares in the oracle's order (orc_sumsq_f32: element c goes to
// partial (c / 4) % 64 in ascending c, then an xor butterfly): row_sumsq_wave where its float4 chunks apply, element loads otherwise
__global__ __launch_bounds__(256) void inv_norm_kernel(const float* __restrict__ x, int64_t rows, int d,
                                                       float* __restrict__ inv_out) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* row = x + r * (int64_t)d;
    float nr = 0.0f;
    if ((d & 3) == 0 && d <= 1024) {
        float4 v[4];
        nr = row_sumsq_wave(row, d, v);
    } else {
        for (int c0 = 4 * lane_id(); c0 < d; c0 += 256)
            for (int c = c0; c < c0 + 4 && c < d; ++c) {
                const float t = row[c] * row[c];
                nr = nr + t;
            }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) nr = nr + __shfl_xor(nr, off);
    }
    // faiss leaves zero rows untouched: scaling by 1 reproduces that
    if (lane_id() == 0) inv_out[r] = (nr > 0.0f) ? inv_norm_from_sumsq(nr) : 1.0f;
}

template <int QB>
int launch_rescore(Rows q, const Prepared& Q, Rows b, const Prepared& B, int64_t n, int64_t m, int d, const SearchWs& w,
                   int64_t* idx_out, float* sim_out, float min_sim, hipStream_t st) {
    const size_t lds = (size_t)((QB > 64 ? 0 : 64 * RS_STRIDE) + RS_PAIRS) * sizeof(double) + (size_t)(QB / 64) * d * sizeof(float);
    static unsigned long long attr_set = 0ull;  // one bit per device
    if (!attr_done(attr_set)) {
        VFM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&match_rescore_kernel<QB>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
        attr_mark(attr_set);
    }
    hipLaunchKernelGGL(match_rescore_kernel<QB>, dim3((unsigned)((n + QB - 1) / QB)), dim3(256), lds, st, q, Q.inv, b, B.inv, n, m, d,
                       w.cand_cnt, w.cand, w.cap, idx_out, sim_out, min_sim);
    return VFM_OK;
}

}  // namespace

// stage 2 of a search: candidate selection + exact fp64 decision (reads ws of stage 1), as the plan's steps in order
// gated: the search was started by the gated family (do_search_coarse(..., gated)); gate: queries whose best similarity is
// provably below it are reported as (-1, -2.0) instead of being resolved (int8 / fp6 passes only; -Inf = resolve every query)
//
// VFM_RECORDS_NO_I8 (plan.no_i8): no step of such a plan reads tiles8 / tiles8h / rows8 / err / gstep / gerr of either operand: the
// survivors are binned (match_bin_survivors_kernel: the slots only), the guard counts the bins, the rescan reads the fp6 half image with
// err6h / rest, the closing pass the counters, and the fp64 decision the rows themselves.
//   whole-chunk entries (a full bin leaves chunk << 8 | 128 in the query's list): match_rescan_close_kernel changes lengths, never
//     entries, and match_rescore_kernel scores such a chunk's 128 rows in fp64 -- they stay as they are;
//   crowded queries: match_rescore_kernel takes any list up to `cap` (epochs of RS_PAIRS pairs) and decides it in fp64 with the
//     oracle's tie rule; the fp32 refinement only ever shortened such a list.  The closing pass still notes them (rec_cnt,
//     fb_count[6]); nothing reads that there;
//   guard up: match_guard_fallback_kernel hands every live query to match_exact_kernel (include/vfmreg.h, VFM_RECORDS_NO_I8).
int do_search_finish(Rows q, const void* qprep, int64_t n, Rows b, const void* bprep, int64_t m, int d,
                     int64_t* idx_out, float* sim_out, void* ws, hipStream_t st, bool gated, float gate, int records) {
    SearchPlan plan;
    VFM_TRY(resolve_search(plan, records, d, n, m, gated, true));
    VFM_TRY(check_plan_gate(plan.gate_test, gate, "search_finish"));
    Prepared Q = carve_prepared(const_cast<void*>(qprep), n, d);
    Prepared B = carve_prepared(const_cast<void*>(bprep), m, d);
    SearchWs w = carve_search(ws, n, m);
    const CoarseArgs a = coarse_args(Q, B, w, n, m);
    const float w2 = 2.0f * (float)(d / 16 + 4 + 2) * 5.9604645e-8f;
    const bool i8 = plan.quantised(), half = plan.gate_test, use_bins = plan.use_bins;
    // records of the fp6 pass: its own bounds in the selection; behind it the int8 image and bounds, as for the int8 kinds
    const I8Bounds sel_ib = plan_bounds(plan, Q, B), ib = i8_bounds(Q, B, i8, plan.top2 ? 1 : 0);
    const int chunk_lds = i8 && (size_t)a.nchunks * sizeof(float2) <= 63 * 1024;  // (step, max E) of every chunk in LDS
    const int* guard = half ? w.fb_count + HALF_GUARD_FLAG : (const int*)nullptr;
    for (int i = 0; i < plan.nsteps; ++i) {
        const FinishStep step = plan.steps[i];
        switch (step) {
            case FIN_FILTER_REFINE:
                hipLaunchKernelGGL(match_filter_refine_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, q, Q.inv, b, B.inv, n, m, d,
                                   DEFAULT_WINDOW, w2, w.qmax, w.rec_cnt, w.rec, w.rcap, w.cand_cnt, w.cand, w.cap, w.fb_count, w.fb_list, vfm_cfg().match_stats);
                break;
            case FIN_PILOT_BIN:
                // the pilot rescan: one chunk per query, scored exactly on the int8 image, raises qmax (match_rescan_chunk_kernel, pilot
                // branch); the bins it used are emptied again for the selection
                hipLaunchKernelGGL(match_pilot_bin_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, (const unsigned long long*)w.qbest,
                                   (const float*)Q.inv, w.bin_cnt, w.bins, w.bin_cap, a.nchunks);
                break;
            case FIN_PILOT_RESCAN:
                VFM_TRY(launch_rescan_chunk(w, a.nchunks, n, m, d, i8_bounds(Q, B, true, VFM_RECORDS_BEST), Q, B, 0, gate, (const int*)nullptr,
                                            L2Terms{nullptr, nullptr, 0.0f}, st, true));
                VFM_CHECK_HIP(hipMemsetAsync(w.bin_cnt, 0, (size_t)((a.nchunks + 63) / 64 * 64) * BIN_CNT_STRIDE * sizeof(unsigned), st));
                break;
            case FIN_BIN_SURVIVORS:
                hipLaunchKernelGGL(match_bin_survivors_kernel, dim3(256), dim3(256), 0, st, reinterpret_cast<const unsigned*>(w.partials),
                                   MX6_SURV_SLOT_WORDS, (const int*)w.fb_count, w.bin_cnt, w.bins, w.bin_cap, w.cand_cnt, w.cand, w.cap);
                break;
            case FIN_SELECT_HALF: {
                const int half_lds = (size_t)a.nchunks * 12 <= 63 * 1024;  // (step, max E, max |rest|) of every chunk in LDS
                hipLaunchKernelGGL(match_select_half_kernel, dim3((unsigned)a.nq_tiles), dim3(64 * 8), half_lds ? (size_t)a.nchunks * 12 : 0,
                                   st, reinterpret_cast<const unsigned*>(w.partials), a.nchunks, n, Q.inv, sel_ib, (const float*)Q.rest,
                                   (const float*)B.grest, gate, half_lds, w.cand_cnt, w.cand, w.cap, w.fb_count, w.fb_list, vfm_cfg().match_stats,
                                   use_bins ? w.bin_cnt : (unsigned*)nullptr, use_bins ? w.bins : (int*)nullptr, w.bin_cap);
                break;
            }
            case FIN_SELECT_TOP2:
                hipLaunchKernelGGL(match_select_top2_kernel, dim3((unsigned)a.nq_tiles), dim3(64 * SELECT_TOP2_WAVES),
                                   chunk_lds ? (size_t)a.nchunks * sizeof(float2) : 0, st, (const uint2*)w.partials, a.nchunks, n, a.first_pad_chunk,
                                   (const unsigned*)w.qmax, Q.inv, sel_ib, gate, chunk_lds, w.cand_cnt, w.cand, w.cap, w.fb_count, w.fb_list, vfm_cfg().match_stats);
                break;
            case FIN_SELECT_BEST: {
                // (chunk_lds 2: room for the per-chunk histogram of the tile's candidates as well -- chunks must fit 16 bits of a staged entry)
                const int best_lds = chunk_lds && use_bins && (size_t)a.nchunks * 12 <= 63 * 1024 && a.nchunks < 65536 ? 2 : chunk_lds;
                hipLaunchKernelGGL(match_select_best_kernel, dim3((unsigned)a.nq_tiles), dim3(64 * SELECT_BEST_WAVES),
                                   best_lds == 2 ? (size_t)a.nchunks * 12 : chunk_lds ? (size_t)a.nchunks * sizeof(float2) : 0, st,
                                   reinterpret_cast<const unsigned*>(w.partials), a.nchunks, n, (const unsigned*)w.qmax, Q.inv, sel_ib, gate, best_lds,
                                   w.cand_cnt, w.cand, w.cap, w.fb_count, w.fb_list, vfm_cfg().match_stats, use_bins ? w.bin_cnt : (unsigned*)nullptr,
                                   use_bins ? w.bins : (int*)nullptr, a.first_pad_chunk, w.bin_cap);
                break;
            }
            case FIN_SELECT:
                hipLaunchKernelGGL(match_select_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64 * SELECT_GROUPS),
                                   chunk_lds ? (size_t)a.nchunks * sizeof(float2) : 0, st, w.partials, a.nchunks, a.npad, n, a.first_pad_chunk, w.qmax,
                                   Q.inv, DEFAULT_WINDOW, sel_ib, gate, chunk_lds, w.cand_cnt, w.cand, w.cap, w.fb_count, w.fb_list, vfm_cfg().match_stats);
                break;
            case FIN_HALF_GUARD:   // the device-side guard of the half-width pass (see half_guard_kernel)
                hipLaunchKernelGGL(half_guard_kernel, dim3(1), dim3(256), 0, st, w.fb_count, (const unsigned*)w.bin_cnt, a.nchunks,
                                   plan.fused ? 1 : 0, (long long)HALF_GUARD_PER_QUERY * (long long)n);
                break;
            case FIN_GUARD_FALLBACK:
                hipLaunchKernelGGL(match_guard_fallback_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, (const float*)Q.inv, guard,
                                   w.cand_cnt, w.fb_count, w.fb_list);
                break;
            case FIN_RESCAN:   // candidate chunks -> candidate rows (the record buffer of the fp16 pass is free: it holds the hit lists)
                hipLaunchKernelGGL(match_rescan_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, n, m, d, ib,
                                   (const uint4*)Q.tiles8, (const uint4*)B.tiles8, (const unsigned*)w.qmax, w.cand_cnt, w.cand, w.cap,
                                   reinterpret_cast<unsigned*>(w.rec), 2 * w.rcap, w.fb_count, w.fb_list, half ? 1 : 0, gate, guard,
                                   L2Terms{nullptr, nullptr, 0.0f});
                break;
            case FIN_GATEPASS:
#define VFM_GATEPASS(KS)                                                                                                        \
    hipLaunchKernelGGL(match_gatepass_kernel<KS>, dim3((unsigned)a.nchunks), dim3(256), 0, st, n, m, a.nq_tiles, ib, (const float*)Q.inv, \
                       (const uint4*)Q.tiles8, (const uint4*)B.tiles8, gate, w.cand_cnt, w.cand, w.cap, guard, w.qmax)
                switch (d / 32) {
                    case 8: VFM_GATEPASS(8); break;
                    case 12: VFM_GATEPASS(12); break;
                    case 16: VFM_GATEPASS(16); break;
                    case 20: VFM_GATEPASS(20); break;
                    default: VFM_GATEPASS(24); break;
                }
#undef VFM_GATEPASS
                break;
            case FIN_RESCAN_CHUNK:
                VFM_TRY(launch_rescan_chunk(w, a.nchunks, n, m, d, ib, Q, B, half ? 1 : 0, gate, guard, L2Terms{nullptr, nullptr, 0.0f}, st));
                break;
            case FIN_RESCAN_CHUNK_MX6H:
                VFM_TRY(d == 384 ? launch_rescan_chunk_mx6h<3>(w, a.nchunks, n, m, Q, B, gate, guard, st)
                                 : launch_rescan_chunk_mx6h<2>(w, a.nchunks, n, m, Q, B, gate, guard, st));
                break;
            case FIN_RESCAN_CLOSE:
                // (rec_cnt, unused by the int8 pass, holds the list of crowded queries; fb_count[6] its length)
                hipLaunchKernelGGL(match_rescan_close_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, w.cand_cnt, w.cap,
                                   w.fb_count, w.fb_list, reinterpret_cast<int*>(w.rec_cnt), half ? (const float*)Q.inv : (const float*)nullptr,
                                   (const unsigned*)w.hit_cnt);
                break;
            case FIN_REFINE: {
                // (round 4: one wave per possible entry after all.  With 1024 workgroups striding over the list a wave had two or three
                // queries of 30 - 40 us each and the kernel lasted as long as the unluckiest wave -- 137 us at 9891 crowded queries; a wave per
                // entry is placed as slots come free: 125 us.  Handing the entries out through an atomic cursor was tried: 186 us -- 4096
                // waves ask the same address at once and every later load of a wave waits behind its atomic.  The refinement is 124 registers
                // since R4.5, and workgroups past the list's end return at once: ~2 us for 5000 of them.)
                const unsigned grid = (unsigned)((n + 3) / 4);
#define VFM_REFINE(NT)                                                                                                          \
    hipLaunchKernelGGL(match_refine_kernel<NT>, dim3(grid), dim3(256), 0, st, q, Q.inv, b, B.inv, n, m, d, w2, w.cand_cnt, w.cand, \
                       w.cap, w.fb_count, w.fb_list, vfm_cfg().match_stats, i8 ? (const int*)w.rec_cnt : (const int*)nullptr,      \
                       i8 ? (const int*)(w.fb_count + 6) : (const int*)nullptr, use_bins ? (const float*)w.cand_up : (const float*)nullptr, \
                       i8 ? (const unsigned*)w.hit_cnt : (const unsigned*)nullptr, ib)
                if (!i8 || d > 512) VFM_REFINE(12);
                else if (d <= 256) VFM_REFINE(4);
                else if (d <= 384) VFM_REFINE(6);
                else VFM_REFINE(8);
#undef VFM_REFINE
                break;
            }
            case FIN_RESCORE:   // ("rescore_block": the queries a workgroup owns; unset: 256 behind a half-width pass -- it is taken where few
                                // (query, chunk) pairs survive, ~0.5 a query: a lane per pair over a quarter of the workgroups is enough --, 64
                                // elsewhere: crowded lists want the workgroups (C3's pipeline lost 2.7 % with 256 everywhere))
                VFM_TRY((vfm_cfg().rescore_block ? vfm_cfg().rescore_block : plan.half ? 256 : 64) == 256
                            ? launch_rescore<256>(q, Q, b, B, n, m, d, w, idx_out, sim_out, half ? gate : -__builtin_inff(), st)
                            : launch_rescore<64>(q, Q, b, B, n, m, d, w, idx_out, sim_out, half ? gate : -__builtin_inff(), st));
                break;
            case FIN_EXACT:
                hipLaunchKernelGGL(match_exact_kernel, dim3(256), dim3(256), (((size_t)d * 4 + 15) & ~(size_t)15) + 64, st, q, Q.inv,
                                   b, B.inv, n, m, d, w.fb_list, w.fb_count, idx_out, sim_out);
                break;
        }
        VFM_CHECK_LAUNCH(finish_step_name(step));
    }
    return VFM_OK;
}

int launch_i8_rescans(const SearchWs& w, const CoarseArgs& a, const Prepared& Q, const Prepared& B, int64_t n, int64_t m, int d,
                      bool use_bins, L2Terms l2, hipStream_t st) {
    const I8Bounds ib = i8_bounds(Q, B, true, VFM_RECORDS_BEST);
    hipLaunchKernelGGL(match_rescan_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, n, m, d, ib, (const uint4*)Q.tiles8,
                       (const uint4*)B.tiles8, (const unsigned*)w.qmax, w.cand_cnt, w.cand, w.cap, reinterpret_cast<unsigned*>(w.rec),
                       2 * w.rcap, w.fb_count, w.fb_list, 0, 0.0f, (const int*)nullptr, l2);
    VFM_CHECK_LAUNCH("match_rescan_kernel");
    if (use_bins) {
        const int rc = launch_rescan_chunk(w, a.nchunks, n, m, d, ib, Q, B, 0, 0.0f, (const int*)nullptr, l2, st);
        if (rc != VFM_OK) return rc;
    }
    hipLaunchKernelGGL(match_rescan_close_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, w.cand_cnt, w.cap, w.fb_count,
                       w.fb_list, reinterpret_cast<int*>(w.rec_cnt), (const float*)nullptr, (const unsigned*)w.hit_cnt);
    VFM_CHECK_LAUNCH("match_rescan_close_kernel");
    return VFM_OK;
}

// vfm_match_search_probe_half: how many (query, chunk) pairs the half-width pass would leave for the rescan -- its coarse
// pass has just run into ws (do_search_coarse(..., VFM_RECORDS_HALF)); only fb_count[5] is written
int probe_half_select(const SearchPlan& plan, const void* qprep, int64_t n, const void* bprep, int64_t m, int d, void* ws, float gate, hipStream_t st) {
    Prepared Q = carve_prepared(const_cast<void*>(qprep), n, d);
    Prepared B = carve_prepared(const_cast<void*>(bprep), m, d);
    SearchWs w = carve_search(ws, n, m);
    const CoarseArgs a = coarse_args(Q, B, w, n, m);
    const int half_lds = (size_t)a.nchunks * 12 <= 63 * 1024;
    hipLaunchKernelGGL(match_select_half_kernel, dim3((unsigned)a.nq_tiles), dim3(64 * 8), half_lds ? (size_t)a.nchunks * 12 : 0, st,
                       reinterpret_cast<const unsigned*>(w.partials), a.nchunks, n, Q.inv, plan_bounds(plan, Q, B),
                       (const float*)Q.rest, (const float*)B.grest, gate, half_lds, w.cand_cnt, (unsigned*)nullptr, w.cap, w.fb_count,
                       w.fb_list, 0, (unsigned*)nullptr, (int*)nullptr, w.bin_cap);
    VFM_CHECK_LAUNCH("match_select_half_kernel(probe)");
    return VFM_OK;
}

// dense fp16 records -> candidate lists (the Euclidean search's use of match_select_kernel)
int launch_select_dense(const SearchWs& w, const CoarseArgs& a, const float* qinv, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(match_select_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64 * SELECT_GROUPS), 0, st, w.partials, a.nchunks,
                       a.npad, n, a.first_pad_chunk, w.qmax, qinv, DEFAULT_WINDOW, i8_bounds(Prepared{}, Prepared{}, false),
                       -__builtin_inff(), 0, w.cand_cnt, w.cand, w.cap, w.fb_count, w.fb_list, vfm_cfg().match_stats);
    VFM_CHECK_LAUNCH("match_select_kernel");
    return VFM_OK;
}

int launch_inv_norm(const float* x, int64_t rows, int d, float* inv_out, hipStream_t st) {
    hipLaunchKernelGGL(inv_norm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, rows, d, inv_out);
    VFM_CHECK_LAUNCH("inv_norm_kernel");
    return VFM_OK;
}

// EXACT mode of vfm_match_ip_top1: all-pairs fp64; ws holds 1/|row| of both operands
int exact_ip_top1(const float* q, int64_t n, const float* b, int64_t m, int d, int64_t* idx_out, float* sim_out, void* ws,
                  hipStream_t st) {
    VfmCarver c(ws);
    float* invq = c.take<float>((size_t)n);
    float* invb = c.take<float>((size_t)m);
    VFM_TRY(launch_inv_norm(q, n, d, invq, st));
    VFM_TRY(launch_inv_norm(b, m, d, invb, st));
    const unsigned grid = (unsigned)(n < 4096 ? n : 4096);
    hipLaunchKernelGGL(match_exact_kernel, dim3(grid), dim3(256), (((size_t)d * 4 + 15) & ~(size_t)15) + 64, st, q,
                       invq, b, invb, n, m, d, (const int*)nullptr, (const int*)nullptr, idx_out, sim_out);
    VFM_CHECK_LAUNCH("match_exact_kernel");
    return VFM_OK;
}

}  // namespace vfmm

using namespace vfmm;

VFM_EXPORT int vfm_threshold_compact(const float* sim, const int64_t* idx, int64_t n, double thr, int64_t* keep_out,
                                     int64_t* count_out, int32_t* corres_out, const double* q_xyz, const double* b_xyz,
                                     double* src_xyz_out, double* tgt_xyz_out, vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 0 && sim && keep_out && count_out, "threshold_compact: bad arguments");
    VFM_CHECK_ARG(!(corres_out || tgt_xyz_out) || idx, "threshold_compact: idx required for corres / tgt output");
    VFM_CHECK_ARG(!src_xyz_out || q_xyz, "threshold_compact: q_xyz required");
    VFM_CHECK_ARG(!tgt_xyz_out || b_xyz, "threshold_compact: b_xyz required");
    hipLaunchKernelGGL(threshold_compact_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, sim, idx, n, thr, keep_out,
                       count_out, corres_out, q_xyz, b_xyz, src_xyz_out, tgt_xyz_out);
    VFM_CHECK_LAUNCH("threshold_compact_kernel");
    return VFM_OK;
}

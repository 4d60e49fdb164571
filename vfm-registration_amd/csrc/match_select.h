// match_select.h -- the steps the candidate-selection kernels share, one copy of each: the bounds that make a chunk a
// candidate, the chunks' (step, max E) in the LDS, the "dead query" test, the sweep over a query tile's records, where a candidate goes
// (the chunk's bin, past a full bin the query's own list), the tile's staged candidates, and the epilogue (load figure, statistics,
// cand_cnt classes).  Used by match_select_kernel, match_select_top2_kernel, match_select_half_kernel, match_bin_survivors_kernel and
// match_select_best_kernel (match_finish.hip) and by match_select_l2_kernel (match_l2.hip).  A rule that differed between two of them
// would change no answer, only the feedback counters the caller's policy reads -- no oracle test sees that.
// Device-inline code only; -ffp-contract=off: the same expression in the same order of operations gives the same bits, so the order
// of every sum below is part of its definition.
#pragma once
#include "match_internal.h"

namespace vfmm {

// ---------------------------------------------------------------------------------------------
// the bounds.  Records of the int8 / fp6 pass hold integer scores S in the units of (query group step s_q) x (map chunk step s_c).
// In exact score units, with A = (1 + 2^-13) E_q and B_c = (1 + 2^-13 + E_q) max E of chunk c (prep_chunk_kernel):
//     s_q s_c S(c) - A - B_c  <=  best exact score of chunk c  <=  s_q s_c S(c) + A + B_c
// fp32 evaluation: three roundings on magnitudes <= 2 -- SELECT_SLACK covers them.
// (The fused coarse kernels -- match_coarse_i8.hip, match_coarse_mx6.hip -- and the rescans of match_finish.hip evaluate the same
// bounds in registers of their own, with the slack folded into A: query_bound_slack is that form.)
// ---------------------------------------------------------------------------------------------
constexpr float SELECT_SLACK = 1.0e-6f;
struct QueryBound {
    float A, mult;   // the query's own term, and the factor of the chunk's max E
};
__device__ __forceinline__ QueryBound query_bound(float eq) { return QueryBound{eq * 1.0001220703125f, 1.0001220703125f + eq}; }
// ... with the slack folded into A (the Euclidean selection)
__device__ __forceinline__ QueryBound query_bound_slack(float eq) { return QueryBound{eq * 1.0001220703125f + SELECT_SLACK, 1.0001220703125f + eq}; }
// the integer score of a record word.  Best-score records hold it as it is (+ I8_OFFSET); packed top-2 records carry the best row's
// index in the low 7 bits of the first word and 6 bits of payload in the second: rounded up, the bound stays a bound
__device__ __forceinline__ int best_score(unsigned w) { return (int)w - I8_OFFSET; }
__device__ __forceinline__ int top2_first_score(unsigned w) { return (int)(w | 127u) - I8_OFFSET; }
__device__ __forceinline__ int top2_second_score(unsigned w) { return (int)(w | 63u) - I8_OFFSET; }
// upper bound of the best exact score of a chunk whose best integer score is S (sc = s_q s_c, ec = the chunk's max E)
__device__ __forceinline__ float chunk_upper(float sc, int S, QueryBound b, float ec) { return sc * (float)S + (b.A + b.mult * ec + SELECT_SLACK); }
// half-width records (S over the first d / 2 columns): Cauchy-Schwarz on the other half adds r_q R_c.  Five roundings: twice the slack.
__device__ __forceinline__ float chunk_upper_half(float sc, int S, QueryBound b, float ec, float rq, float rc) {
    return chunk_upper(sc, S, b, ec) + (rq * rc + SELECT_SLACK);
}
// the Euclidean selection bounds the cosine from both sides (b: query_bound_slack)
__device__ __forceinline__ float cos_lower(float sc, int S, QueryBound b, float ec) { return sc * (float)S - (b.A + b.mult * ec); }
__device__ __forceinline__ float cos_upper(float sc, int S, QueryBound b, float ec) { return sc * (float)S + (b.A + b.mult * ec); }

// ---------------------------------------------------------------------------------------------
// the chunks' (step, max E), once per workgroup into the LDS (chunk_lds != 0: they fit).  NT threads; extra(c) fills a further
// column.  Returns the thread's largest max E (raise_workgroup_max makes the workgroup's of it).  match_select_l2_kernel stages a
// float4 (step, max E, lo, hi) with a loop of its own: nothing of this one would be left.
// ---------------------------------------------------------------------------------------------
template <int NT, class Extra>
__device__ __forceinline__ float stage_chunk_bounds(float2* lchunk, const I8Bounds& ib, int nchunks, Extra extra) {
    float me = 0.0f;
    for (int c = threadIdx.x; c < nchunks; c += NT) {
        const float2 v = make_float2(ib.bstep[c], ib.berr[c]);
        lchunk[c] = v;
        extra(c);
        me = fmaxf(me, v.y);
    }
    return me;
}
template <int NT>
__device__ __forceinline__ float stage_chunk_bounds(float2* lchunk, const I8Bounds& ib, int nchunks) {
    return stage_chunk_bounds<NT>(lchunk, ib, nchunks, [](int) {});
}
// float_key of the workgroup's largest `me` into *lmax (LDS, zeroed before a barrier): one atomic per wave
__device__ __forceinline__ void raise_workgroup_max(unsigned* lmax, float me) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) me = fmaxf(me, __shfl_xor(me, off));
    if (lane_id() == 0) atomicMax(lmax, float_key(me));
}
// (step, max E) of chunk c, staged or not.  The staged copy is read through a pointer that says LDS: with two generic pointers the
// compiler merges the two loads into one flat load of a selected address (16 flat_load_dword in each tile kernel, the best-score
// finish call outside its bar at C2), where the expression written inside a kernel's own loop had the loop unswitched on chunk_lds.
typedef const __attribute__((address_space(3))) float lds_cfloat;
__device__ __forceinline__ float2 chunk_bounds(const float2* lchunk, int chunk_lds, const I8Bounds& ib, int c) {
    if (chunk_lds) {
        lds_cfloat* p = (lds_cfloat*)lchunk;
        return make_float2(p[2 * c], p[2 * c + 1]);
    }
    return make_float2(ib.bstep[c], ib.berr[c]);
}

// ---------------------------------------------------------------------------------------------
// the sweep of the tile kernels: one workgroup of WAVES waves per 32-query tile.  A lane owns QPL consecutive queries (one uint4
// of records: QPL = 4 with 4-byte records, 2 with 8-byte ones) and one chunk of a block of 64 QPL / 32, so a wave's load instruction
// covers 1 KiB of consecutive record bytes; eight loads are in flight per lane.  tile: the tile's records [chunk][32].
// open(): asked before a block's loads, false ends the lane's sweep; body(c, rec): true ends it too (never, in most callers: the
// tests fold away).
// ---------------------------------------------------------------------------------------------
template <int QPL>
struct TileLane {
    static_assert(QPL == 2 || QPL == 4, "a uint4 of records per lane");
    static constexpr int LANES_PER_CHUNK = 32 / QPL, CHUNK_SHIFT = QPL == 4 ? 3 : 2, LANE_SHIFT = QPL == 4 ? 3 : 4;
    int lq, lc;   // first of the lane's queries within the tile; the lane's chunk within a block
    __device__ __forceinline__ TileLane() : lq((lane_id() & (LANES_PER_CHUNK - 1)) * QPL), lc(lane_id() >> LANE_SHIFT) {}
};
// the records of chunk c for the lane's queries
template <int QPL>
__device__ __forceinline__ uint4 tile_chunk_records(const uint4* __restrict__ tile, int c) {
    return tile[(size_t)c * TileLane<QPL>::LANES_PER_CHUNK + (lane_id() & (TileLane<QPL>::LANES_PER_CHUNK - 1))];
}
template <int QPL, int WAVES, class Open, class Body>
__device__ __forceinline__ void sweep_tile_records(const uint4* __restrict__ tile, int nchunks, Open open, Body body) {
    constexpr int SH = TileLane<QPL>::CHUNK_SHIFT;
    const int wave = threadIdx.x >> 6, lc = lane_id() >> TileLane<QPL>::LANE_SHIFT;
    const uint4* src = tile + lane_id();
    const int nblocks = (nchunks + (1 << SH) - 1) >> SH;
    for (int cb0 = wave; cb0 < nblocks; cb0 += 8 * WAVES) {
        if (!open()) break;
        bool stop = false;
        uint4 rec[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int cb = cb0 + WAVES * u;
            rec[u] = ((cb << SH) + lc < nchunks) ? src[(size_t)cb * 64] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = ((cb0 + WAVES * u) << SH) + lc;
            if (c >= nchunks || stop) continue;
            stop = body(c, rec[u]);
        }
        if (stop) break;
    }
}
template <int QPL, int WAVES, class Body>
__device__ __forceinline__ void sweep_tile_records(const uint4* __restrict__ tile, int nchunks, Body body) {
    sweep_tile_records<QPL, WAVES>(tile, nchunks, [] { return true; }, body);
}
// (match_select_kernel -- 64 queries per workgroup, 16 groups, one record per lane and load -- keeps its three sweeps written out:
// see the kernel.)
// the largest of v[j] over the lanes that own the same queries (one per chunk of a block) into lmax[lq + j] (float_key, LDS)
template <int QPL>
__device__ __forceinline__ void raise_query_max(unsigned* lmax, int lq, const float (&val)[QPL]) {
#pragma unroll
    for (int j = 0; j < QPL; ++j) {
        float v = val[j];
#pragma unroll
        for (int off = TileLane<QPL>::LANES_PER_CHUNK; off <= 32; off <<= 1) v = fmaxf(v, __shfl_xor(v, off));
        if (lane_id() < TileLane<QPL>::LANES_PER_CHUNK) atomicMax(&lmax[lq + j], float_key(v));
    }
}

// ---------------------------------------------------------------------------------------------
// "dead": the query provably ends below the gate, so its candidates are not even recorded (at C2 the unmatched half of the scan
// would write sixteen entries per query).  Every un-padded chunk has upper_c = lower_c + 2 (A + mult E_c) up to roundings of 1e-6 and
// lower_c <= qlow, so the largest upper bound over them is below qlow + 2 (A + mult max E) + 1e-5; the (at most two) padded chunks
// are not covered by qlow: their records are looked at here (pad_scores(c, S): the best integer scores of chunk c for the lane's
// queries).  Should the sweep find the largest upper bound at or above the gate after all, the query goes to the all-pairs kernel
// (the epilogue's overflow rule).  Zero query rows (decided directly) and the rows that pad the last tile record nothing either.
// Returns the lane's mask and leaves the tile's flags in ldead[32].  maxe = +Inf (the chunks' max E not staged): nothing is dead.
// ---------------------------------------------------------------------------------------------
template <int QPL, class PadScores>
__device__ __forceinline__ unsigned dead_queries(const QueryBound (&qb)[QPL], const float (&qlow)[QPL], float maxe, float gate, float sq,
                                                 const I8Bounds& ib, int first_pad_chunk, int nchunks, int lq, int64_t q0, int64_t n,
                                                 const float* __restrict__ invq, int* ldead, PadScores pad_scores) {
    unsigned deadmask = 0u;
#pragma unroll
    for (int j = 0; j < QPL; ++j) {
        const bool dead = qlow[j] + 2.0f * (qb[j].A + qb[j].mult * maxe) + 1.0e-5f < gate;
        deadmask |= dead ? (1u << j) : 0u;
    }
    for (int c = first_pad_chunk; c < nchunks && deadmask; ++c) {
        int S[QPL];
        pad_scores(c, S);
        const float sc = sq * ib.bstep[c], be = ib.berr[c];
#pragma unroll
        for (int j = 0; j < QPL; ++j)
            if (!(chunk_upper(sc, S[j], qb[j], be) < gate)) deadmask &= ~(1u << j);
    }
#pragma unroll
    for (int j = 0; j < QPL; ++j) {
        if (q0 + j >= n || invq[q0 + j] == 0.0f) deadmask |= 1u << j;
        if (threadIdx.x < TileLane<QPL>::LANES_PER_CHUNK) ldead[lq + j] = (deadmask >> j) & 1u;
    }
    return deadmask;
}

// ---------------------------------------------------------------------------------------------
// where a candidate (query q, chunk c) goes.  Chunk-major rescan (bins != NULL): the query joins the chunk's bin; a full bin
// leaves the entry with the query.  Otherwise, and past a full bin, a whole-chunk entry goes to the query's own list (match_rescan_kernel),
// at the slot drawn from *own -- the list's length, in the LDS or in cand_cnt.  Handed on by value, restrict kept (as RescanLists).
// The host passes bins and bin_cnt both or neither (SearchPlan::use_bins), and bin_cap > 0 with them.
// ---------------------------------------------------------------------------------------------
struct SelectLists {
    unsigned* __restrict__ bin_cnt;   // [nchunks][BIN_CNT_STRIDE]
    int* __restrict__ bins;           // [nchunks][bin_cap] queries (NULL: no bins)
    int bin_cap;
    unsigned* __restrict__ cand;      // [n][cap] the queries' own lists
    int cap;
};
__device__ __forceinline__ void own_list_entry(const SelectLists L, int64_t q, int slot, int c) {
    if (slot < L.cap) L.cand[(size_t)q * L.cap + slot] = ((unsigned)c << 8) | 128u;  // whole-chunk entry
}
// position pos of chunk c's bin was drawn for query q (pos >= bin_cap: the bin is full)
__device__ __forceinline__ void settle_candidate(const SelectLists L, int64_t q, int c, unsigned pos, int* own) {
    if (pos < (unsigned)L.bin_cap) L.bins[(size_t)c * L.bin_cap + pos] = (int)q;
    else own_list_entry(L, q, atomicAdd(own, 1), c);
}
// look: read the bin's counter first and leave a full bin untouched -- on descriptors that are all alike every bin is full after the
// first tiles, and 31 million atomics on 1563 addresses were most of a selection's time then; where bins rarely fill the look is a
// second trip to the memory side per candidate for nothing
__device__ __forceinline__ void place_candidate(const SelectLists L, int64_t q, int c, bool look, int* own) {
    if (L.bins) {
        const unsigned seen = look ? __hip_atomic_load(&L.bin_cnt[(size_t)c * BIN_CNT_STRIDE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        const unsigned pos = seen >= (unsigned)L.bin_cap ? seen : atomicAdd(&L.bin_cnt[(size_t)c * BIN_CNT_STRIDE], 1u);
        settle_candidate(L, q, c, pos, own);
    } else {
        own_list_entry(L, q, atomicAdd(own, 1), c);
    }
}

// ---------------------------------------------------------------------------------------------
// the tile's candidates staged in the LDS, (query of the tile << 27) | chunk: a candidate costs LDS atomics inside the sweep; the
// global side -- a returning atomic on the chunk's bin or the query's list -- is done behind the sweep for all of them at once.
// Inside the sweep every candidate had stalled its wave for a round trip.  false: the buffer is full (the entry is counted, not kept).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool stage_candidate(unsigned* lcand, int* lcand_n, int room, int qq, int c) {
    const int at = atomicAdd(lcand_n, 1);
    if (at < room) lcand[at] = ((unsigned)qq << 27) | (unsigned)c;
    return at < room;
}
__device__ __forceinline__ int staged_query(unsigned e) { return (int)(e >> 27); }
__device__ __forceinline__ int staged_chunk(unsigned e) { return (int)(e & 0x7FFFFFFu); }

// ---------------------------------------------------------------------------------------------
// the epilogue.  The load figure (fb_count[5], vfm_match_search_rescans_async: what the rescans behind this selection will cost --
// the caller's feedback for choosing the record kind), one atomic per wave: every lane of the wave calls.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void add_load_figure(int* fb_count, int mine) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off);
    if (lane_id() == 0 && mine > 0) atomicAdd(fb_count + 5, mine);
}
// what a query of the bounded (int8 / fp6) selections adds: its candidate entries -- of top-2 records the `whole`-chunk entries
// count 1 and the single-row entries 1/32 (48 KB of int8 tiles against 1.5 KB of fp32 row); best-score records: whole = cnt --,
// and nothing where no rescan follows: a zero row, a query below the gate, an overflow
__device__ __forceinline__ int bounded_query_load(float invq_q, bool below_gate, int cnt, int whole, int cap) {
    return (invq_q != 0.0f && !below_gate && cnt <= cap) ? whole + ((cnt - whole) >> 5) : 0;
}
// overflow: the query is decided by the exact all-pairs kernel
__device__ __forceinline__ void send_to_all_pairs(int64_t q, int* __restrict__ cand_cnt, int* __restrict__ fb_count, int* __restrict__ fb_list) {
    cand_cnt[q] = -1;
    const int slot = atomicAdd(fb_count, 1);
    fb_list[slot] = (int)q;
}
struct SelectClose {   // where a selection leaves its verdicts
    const float* __restrict__ invq;
    int* __restrict__ cand_cnt;
    int* __restrict__ fb_count;
    int* __restrict__ fb_list;
    int stats;
};
// one query (q < n) with cnt candidate entries: the statistics (vfm_debug_match_stats: [2] candidate entries, [8 + b] queries with
// 2^(b-1) < entries <= 2^b) and its class --
//     0        zero query row: decided directly (index 0, score 0)
//     -2       no_match: no row of the map can reach the caller's similarity gate (VoxelHashMap.cpp:501-511 drops such queries): not
//              resolved further -- match_rescore_kernel reports (index -1, similarity -2)
//     -1       overflow: more entries than a list holds, or a "dead" query lifted past the gate after all
//     stored   the length of the query's own list (behind a chunk-major selection only the entries that missed their bins:
//              match_rescan_chunk_kernel appends the rows it finds behind what match_rescan_kernel makes of these)
__device__ __forceinline__ void close_query(const SelectClose C, int64_t q, int cnt, bool no_match, bool overflow, int stored) {
    if (C.stats && C.invq[q] != 0.0f) {
        atomicAdd(C.fb_count + 2, cnt);
        int bin = 0;
        while ((1 << bin) < cnt && bin < 15) ++bin;
        atomicAdd(C.fb_count + 8 + bin, 1);
    }
    if (C.invq[q] == 0.0f) {
        C.cand_cnt[q] = 0;
    } else if (no_match) {
        C.cand_cnt[q] = -2;
    } else if (overflow) {
        send_to_all_pairs(q, C.cand_cnt, C.fb_count, C.fb_list);
    } else {
        C.cand_cnt[q] = stored;
    }
}
// the tile kernels' epilogue, behind a barrier: one wave closes the tile's 32 queries.  lcnt[32]: their candidate counts (LDS).
// load(qq, q, cnt): what a live query adds to the load figure; no_match / overflow / stored (qq, cnt): see close_query; classify
// false: a probe, the load figure only.
template <class Load, class NoMatch, class Overflow, class Stored>
__device__ __forceinline__ void close_tile_queries(const SelectClose C, int qt, int64_t n, const int* lcnt, bool classify, Load load,
                                                   NoMatch no_match, Overflow overflow, Stored stored) {
    if (threadIdx.x < 64) {
        const int lane = lane_id(), qq = lane & 31;
        const int64_t q = (int64_t)qt * 32 + qq;
        const bool live = lane < 32 && q < n;
        const int cnt = lcnt[qq];
        add_load_figure(C.fb_count, live ? load(qq, q, cnt) : 0);
        if (live && classify) close_query(C, q, cnt, no_match(qq, cnt), overflow(qq, cnt), stored(qq, cnt));
    }
}

}  // namespace vfmm

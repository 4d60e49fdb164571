// match_exact.h -- the fp64 decision every search of match_*.hip ends with, one copy of each piece: the order that
// picks a winner, the wave's and the workgroup's arg-max, and the chains that score a pair in the order of oracle/vfm_oracle.c.
// It decides whether an answer is bit-equal to the oracle's: a second copy that drifts shows only on a tie or at a width no test
// uses.  Device-inline code only (match_finish / _topk / _l2 / _l2_narrow.hip); -ffp-contract=off: no chain fuses a product into its sum.
#pragma once
#include "match_internal.h"

namespace vfmm {

// ---- the order: (score descending, map index ascending); an index < 0 is "empty" and never wins
// does (s, j) come before the best so far?  (A branch, not `return <condition>`: inlined, the branch leaves the control flow of the
// condition written in place; the returned value became selects, and match_topk_exact_kernel took 90 registers instead of 80 -- five
// waves per SIMD instead of six.)
__device__ __forceinline__ bool decided_before(double s, long long j, double best_s, long long best_j) {
    if (j >= 0 && (best_j < 0 || s > best_s || (s == best_s && j < best_j))) return true;
    return false;
}
// the mirror for squared distances: (distance ascending, map index ascending)
__device__ __forceinline__ bool nearer_before(double d2, long long j, double best_d2, long long best_j) {
    if (j >= 0 && (best_j < 0 || d2 < best_d2 || (d2 == best_d2 && j < best_j))) return true;
    return false;
}
// (s, j) replaces the best so far where it comes before it
__device__ __forceinline__ void take_if_before(double s, long long j, double& best_s, long long& best_j) {
    if (decided_before(s, j, best_s, best_j)) {
        best_s = s;
        best_j = j;
    }
}

// arg-max over a wavefront, ties -> lowest index (the oracle's rule).  An arg-min of distances negates them first (x -> -x is exact).
__device__ __forceinline__ void wave_argmax(double& s, long long& j) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double so = __shfl_xor(s, off);
        const long long jo = __shfl_xor(j, off);
        take_if_before(so, jo, s, j);
    }
}

// arg-max over a workgroup of 256 threads: wave_argmax, lane 0 of each wave to rs / rj ([4] each, LDS), barrier, every thread folds
// the four and returns with the workgroup's winner.  The caller keeps rs / rj unwritten until every thread has read them (a barrier,
// or another pair of arrays for the next call).
__device__ __forceinline__ void block_argmax(double& s, long long& j, double* rs, long long* rj) {
    wave_argmax(s, j);
    if (lane_id() == 0) {
        rs[threadIdx.x >> 6] = s;
        rj[threadIdx.x >> 6] = j;
    }
    __syncthreads();
    s = rs[0];
    j = rj[0];
    for (int w = 1; w < 4; ++w) take_if_before(rs[w], rj[w], s, j);
}

// ---- inner product of two fp32-normalised rows: orc_dot_f64, sequential k (products of two fp32 are exact in fp64)
// the query row normalised beforehand (LDS), the map row scaled as it is loaded; d % 4 == 0
__device__ __forceinline__ double dot_norm_f64(const float* __restrict__ qrow_n, Rows b, int64_t brow, float invb, int d) {
    double acc = 0.0;
    for (int k = 0; k < d; k += 4) {
        const float4 bv = b.ld4(brow + k);
        const float b0 = bv.x * invb, b1 = bv.y * invb, b2 = bv.z * invb, b3 = bv.w * invb;
        acc = acc + (double)qrow_n[k + 0] * (double)b0;
        acc = acc + (double)qrow_n[k + 1] * (double)b1;
        acc = acc + (double)qrow_n[k + 2] * (double)b2;
        acc = acc + (double)qrow_n[k + 3] * (double)b3;
    }
    return acc;
}
// rows of any width: aligned float4 loads where d % 4 == 0, element loads otherwise -- the same values in the same order.  (A
// wrapper, not a branch inside dot_norm_f64: with the branch there match_exact_kernel took 48 registers instead of 43, and
// match_rescore_kernel<256>, a kernel of the headline's cycle, 243 instead of 249.)
__device__ __forceinline__ double dot_norm_any_f64(const float* __restrict__ qrow_n, Rows b, int64_t brow, float invb, int d) {
    if ((d & 3) == 0) return dot_norm_f64(qrow_n, b, brow, invb, d);
    double acc = 0.0;
    for (int k = 0; k < d; ++k) {
        const float bk = b.ld1(brow + k) * invb;
        acc = acc + (double)qrow_n[k] * (double)bk;
    }
    return acc;
}

// one product of a pair that is normalised as it is multiplied: fp32 normalisation as faiss leaves it, exact fp64 product
__device__ __forceinline__ double prod_norm_f64(float qv, float iq, float bv, float ib) { return (double)(qv * iq) * (double)(bv * ib); }

// exact score of ONE pair by one lane: the products of match_rescore_kernel's batches, added in ascending k.  Two buffers of 32
// columns: the loads of the next 32 are in flight while a buffer's products are added.
__device__ __forceinline__ double dot_pair_f64(Rows q, int64_t qe, float iq, Rows b, int64_t be, float ib, int d) {
    double acc = 0.0;
    auto add4 = [&](const float4& qv, const float4& bv) __attribute__((always_inline)) {
        acc = acc + prod_norm_f64(qv.x, iq, bv.x, ib);
        acc = acc + prod_norm_f64(qv.y, iq, bv.y, ib);
        acc = acc + prod_norm_f64(qv.z, iq, bv.z, ib);
        acc = acc + prod_norm_f64(qv.w, iq, bv.w, ib);
    };
    float4 q0[8], b0[8], q1[8], b1[8];
    auto fetch = [&](float4 (&qq)[8], float4 (&bb)[8], int k) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            qq[i] = q.ld4(qe + k + 4 * i);
            bb[i] = b.ld4(be + k + 4 * i);
        }
    };
    auto use = [&](const float4 (&qq)[8], const float4 (&bb)[8]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 8; ++i) add4(qq[i], bb[i]);
    };
    const int dmain = d & ~63;
    if (dmain) fetch(q0, b0, 0);
    for (int k = 0; k < dmain; k += 64) {
        fetch(q1, b1, k + 32);
        use(q0, b0);
        if (k + 64 < dmain) fetch(q0, b0, k + 64);
        use(q1, b1);
    }
    for (int k = dmain; k < d; k += 4) add4(q.ld4(qe + k), b.ld4(be + k));   // d % 4 == 0
    return acc;
}

// ---- squared Euclidean distance: the oracle's acc += (double(a_k) - double(b_k))^2, k ascending
// one step of the chain (callers that load a batch of both rows first run it over their registers)
__device__ __forceinline__ double l2_step_f64(double acc, float a, float b) {
    const double t = (double)a - (double)b;
    return acc + t * t;
}
__device__ __forceinline__ double l2_dist_f64(const float* __restrict__ qa, const float* __restrict__ brow, int d) {
    double acc = 0.0;
    for (int k = 0; k < d; ++k) acc = l2_step_f64(acc, qa[k], brow[k]);
    return acc;
}

}  // namespace vfmm

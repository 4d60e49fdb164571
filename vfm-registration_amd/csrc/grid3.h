// grid3.h -- the sorted-key 3-D grid that icp.hip, fpfh.hip and nn3.hip search (internal: not part of the C ABI).
//
// A point's cell (cx, cy, cz) becomes one 63-bit key of three 21-bit fields, each coordinate offset by 2^20; a stable radix sort
// orders (key, input index) pairs, so the points of a cell are a run of equal keys in input order, and a query finds a cell by
// binary search on the sorted keys.  What the layout promises, and what every user has to keep:
//   * a coordinate in [-2^20, 2^20) fills its field exactly, so a key is non-negative and below 2^63 and keys order
//     like (cx, cy, cz); the z-cells cz - r .. cz + r of one column (cx, cy) are consecutive keys: ONE run of the sorted array;
//   * a search that probes cell +- r may only meet cells with |c| <= 2^20 - 1 - r.  Each quantiser leaves that margin: FPFH clamps
//     to +-(2^20 - 2) for its 27 cells, nn3 to +-(2^20 - 16) for NN3_MAX_RINGS = 8 shells, ICP accepts |v| < 2^20 - 1 for its 27
//     voxels and flags the rest out of range (stored as v = 0);
//   * clamping is 1-Lipschitz: cells at most r apart before it are at most r apart after it, so a cover by rings of cells stays
//     complete (points far outside only come to share the border cells).
// The three quantisers are different arithmetic, each pinned bit for bit by its oracle, and stay in their files next to their
// proofs; this header holds the key, the searches' helpers, the keys kernel and the sort / run-id steps of the build.
#pragma once
#include <hipcub/hipcub.hpp>

#include "common.h"

namespace {   // internal linkage: every including file gets its own kernels and helpers, none is exported
namespace grid3 {

// The radix sort's end bit, for every sort of the three files.  Bit 63 of a key is never set, so 63 gives the same order; the FPFH grid's
// sort takes 1-3 us less with 64 (profiles/grid3_refactor_timing.md, "The end bit").
constexpr int KEY_BITS = 64;

// T: int (ICP's voxel indices) or long long; the offset is added in T
template <typename T>
__device__ __forceinline__ long long key(T cx, T cy, T cz) {
    return ((long long)(cx + (1 << 20)) << 42) | ((long long)(cy + (1 << 20)) << 21) | (long long)(cz + (1 << 20));
}

// floor(x * inv_cell) clamped to +-lim (NaN -> -lim)
__device__ __forceinline__ long long cell(double x, double inv_cell, int lim) {
    double c = floor(x * inv_cell);
    c = fmin(fmax(c, (double)-lim), (double)lim);
    return (long long)c;
}

// first position of the ascending a[0, n) that holds `key` or more
__device__ __forceinline__ int lower_bound(const long long* __restrict__ a, int n, long long key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// first position of the ascending a[0, n) that holds more than `key`: the end of the run of keys up to `key`.  (Not lower_bound(key + 1):
// the key of the last cell of the last column is 2^63 - 1, and the + 1 wraps.)
__device__ __forceinline__ int upper_bound(const long long* __restrict__ a, int n, long long key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// sorted position i opens a run of equal keys
__device__ __forceinline__ bool run_head(const long long* __restrict__ ks, int64_t i) { return i == 0 || ks[i - 1] != ks[i]; }

// candidates order by (d2, index): of equal distances the lower index comes first
__device__ __forceinline__ bool closer(double a2, int ai, double b2, int bi) { return a2 < b2 || (a2 == b2 && ai < bi); }

struct Best {
    double d2;
    int idx;
};
// (closer(d2, j, b.d2, b.idx), spelled out and to stay so: through the call the compiler unrolls nn3_query_kernel's run scan another way)
__device__ __forceinline__ void take(Best& b, double d2, int j) {
    if (d2 < b.d2 || (d2 == b.d2 && j < b.idx)) {
        b.d2 = d2;
        b.idx = j;
    }
}
__device__ __forceinline__ Best wave_best(Best b) {   // butterfly over the 64 lanes: the same result in every lane
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double od = __shfl_xor(b.d2, off);
        const int oi = __shfl_xor(b.idx, off);
        take(b, od, oi);
    }
    return b;
}

// keys[i] = q(x, y, z, bad), idx[i] = i; a point whose quantiser sets `bad` raises *status (null for a quantiser that never does)
template <typename Quantiser>
__global__ __launch_bounds__(256) void keys_kernel(const double* __restrict__ pts, int64_t n, Quantiser q, long long* __restrict__ keys,
                                                   int* __restrict__ idx, int* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool bad = false;
    const long long k = q(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], bad);
    if (bad) atomicOr(status, 1);
    keys[i] = k;
    idx[i] = (int)i;
}

// Key is always long long.  The kernel is a template, and inclusive_sum() / run_ids() below are, for one purpose: a template is compiled
// only where it is called, so a file that never numbers runs (nn3.hip) carries neither this kernel nor hipCUB's scan kernels.
template <typename Key>
__global__ __launch_bounds__(256) void heads_kernel(const Key* __restrict__ ks, int64_t n, int* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    head[i] = run_head(ks, i) ? 1 : 0;
}

inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

// hipCUB's temporary storage for a sort of n (key, index) pairs and, with SCAN, an inclusive sum of n ints (one after the other).  A
// build that never sums (nn3) is sized by the sort alone: up to 1024 pairs the sort needs less than a scan does.
template <bool SCAN>
inline size_t cub_bytes(int64_t n) {
    const int ni = (int)(n > 0 ? n : 1);
    size_t sort = 0, scan = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sort, (long long*)nullptr, (long long*)nullptr, (int*)nullptr, (int*)nullptr, ni, 0,
                                             KEY_BITS);
    if constexpr (SCAN) (void)hipcub::DeviceScan::InclusiveSum(nullptr, scan, (const int*)nullptr, (int*)nullptr, ni);
    return (sort > scan ? sort : scan) + 1024;
}

// the head of every build's workspace: the unsorted pairs and hipCUB's storage (SCAN: large enough for inclusive_sum() too)
template <bool SCAN>
struct SortWs {
    long long* keys_in;
    int* idx_in;
    void* cub;
    size_t cub_bytes;
};
template <bool SCAN>
inline SortWs<SCAN> carve_sort(VfmCarver& c, int64_t n) {
    const size_t nn = (size_t)(n > 0 ? n : 1);
    SortWs<SCAN> w{};
    w.keys_in = c.take<long long>(nn);
    w.idx_in = c.take<int>(nn);
    w.cub_bytes = cub_bytes<SCAN>(n);
    w.cub = c.take<unsigned char>(w.cub_bytes);
    return w;
}

// (w.keys_in, w.idx_in) -> (keys_out ascending, order_out: the input index of every sorted position), stable
template <bool SCAN>
inline int sort_pairs(const SortWs<SCAN>& w, int64_t n, long long* keys_out, int* order_out, hipStream_t st) {
    size_t tb = w.cub_bytes;
    VFM_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(w.cub, tb, w.keys_in, keys_out, w.idx_in, order_out, (int)n, 0, KEY_BITS, st));
    return VFM_OK;
}

// the keys of n >= 1 points under q, then the sort; Quantiser::kernel_name labels a failed launch of its keys kernel
template <typename Quantiser, bool SCAN>
inline int build(const double* pts, int64_t n, Quantiser q, int* status, const SortWs<SCAN>& w, long long* keys_out, int* order_out,
                 hipStream_t st) {
    hipLaunchKernelGGL(keys_kernel<Quantiser>, dim3(blocks256(n)), dim3(256), 0, st, pts, n, q, w.keys_in, w.idx_in, status);
    VFM_CHECK_LAUNCH(Quantiser::kernel_name);
    return sort_pairs(w, n, keys_out, order_out, st);
}

template <bool SCAN>
inline int inclusive_sum(const SortWs<SCAN>& w, int64_t n, const int* in, int* out, hipStream_t st) {
    static_assert(SCAN, "this workspace was sized for the sort alone");
    size_t tb = w.cub_bytes;
    VFM_CHECK_HIP(hipcub::DeviceScan::InclusiveSum(w.cub, tb, in, out, (int)n, st));
    return VFM_OK;
}

// head[i] = sorted position i opens a run; run_id = its inclusive sum (the 1-based number of position i's run)
template <bool SCAN>
inline int run_ids(const SortWs<SCAN>& w, int64_t n, const long long* keys, int* head, int* run_id, hipStream_t st) {
    hipLaunchKernelGGL(heads_kernel<long long>, dim3(blocks256(n)), dim3(256), 0, st, keys, n, head);
    VFM_CHECK_LAUNCH("grid3::heads_kernel");
    return inclusive_sum(w, n, head, run_id, st);
}

}  // namespace grid3
}  // namespace

// nn3.hip -- exact 1-nearest-neighbour search in 3-D on MI355X (gfx950): the two sklearn.neighbors.KDTree(X, metric="euclidean")
// .query(Q, k=1) calls of registration_node.py:295-298, which recover the row of every correspondence point in the voxelised clouds.
//   Nn3Cells (grid3.h) / nn3_gather_kernel a sorted-key CSR grid over the cloud (cell = the caller's), points copied in cell order
//   nn3_query_kernel                     one wave per query: the 27 cells around the query, then shells of cells, until the best d2
//                                        is below anything a cell outside the searched cube can hold; past NN3_MAX_RINGS shells a scan
//                                        of every point (queries far from the cloud, or in its empty regions)
//   nn3_knn_kernel                       the same walk for the k <= 64 nearest (vfm_reg/utils.py:19-44, faiss.IndexFlatL2.search): the k
//                                        best so far are a sorted list in registers, an entry per lane
// fp64, -ffp-contract=off: d2 = (dx*dx + dy*dy) + dz*dz, dist = sqrt(d2) (correctly rounded), equal d2 to the lower index (a
// convention of this library; sklearn leaves it unspecified).  tests/nn3_oracle.py repeats it in numpy.
#include "grid3.h"

namespace {

constexpr int64_t NN3_MAX_POINTS = (int64_t)1 << 26;
constexpr int NN3_MAX_RINGS = 8;                 // shells searched around the query's cell before the scan of all points
constexpr int NN3_LIM = (1 << 20) - 16;          // cells are clamped to +-NN3_LIM: cell +- NN3_MAX_RINGS still fits the key's 21 bits
// Points in a cell more than r cells from the query's (in some axis) are, in that axis, more than r - 2^-31 cells away (the two
// products x * inv_cell are rounded; clamped cells only move closer together), and rounding is monotone, so their computed d2 is at
// least that squared.  The bound used is r cells shortened by 1e-6 relative: far more than every rounding on the way.
constexpr double NN3_RING_SLACK = 1.0 - 1e-6;

__device__ __forceinline__ long long nn3_cell(double x, double inv_cell) { return grid3::cell(x, inv_cell, NN3_LIM); }
struct Nn3Cells {   // the quantiser of grid3::keys_kernel
    static constexpr const char* kernel_name = "grid3::keys_kernel<Nn3Cells>";
    double inv_cell;
    __device__ long long operator()(double x, double y, double z, bool&) const {
        return grid3::key(nn3_cell(x, inv_cell), nn3_cell(y, inv_cell), nn3_cell(z, inv_cell));
    }
};

__global__ __launch_bounds__(256) void nn3_gather_kernel(const double* __restrict__ pts, int64_t n, const int* __restrict__ order,
                                                         double* __restrict__ sorted) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t j = order[i];
    sorted[3 * i] = pts[3 * j];
    sorted[3 * i + 1] = pts[3 * j + 1];
    sorted[3 * i + 2] = pts[3 * j + 2];
}

using grid3::Best;

// the points sorted[lo, lo + len) against the query, a lane per point
__device__ __forceinline__ void nn3_scan_run(Best& b, const double* __restrict__ sorted, const int* __restrict__ order, int lo, int len,
                                             double qx, double qy, double qz, int lane) {
    for (int t = lane; t < len; t += 64) {
        const int64_t s = lo + t;
        const double dx = sorted[3 * s] - qx, dy = sorted[3 * s + 1] - qy, dz = sorted[3 * s + 2] - qz;
        grid3::take(b, (dx * dx + dy * dy) + dz * dz, order[s]);
    }
}

// One wave (= one workgroup) per query.  Shell r is walked by columns (ax, ay) of the (2r + 1)^2 square: the z-cells of a column are
// consecutive keys, so a column on the square's border is ONE run of keys (cz - r .. cz + r) and a column inside it two single
// cells (cz - r and cz + r).  64 columns at a time find their runs with two binary searches per lane; the wave then reads each
// non-empty run together, a lane per point, from the copy of the cloud kept in cell order.
__global__ __launch_bounds__(64) void nn3_query_kernel(const double* __restrict__ sorted, const long long* __restrict__ keys,
                                                       const int* __restrict__ order, int n, double inv_cell, double cell,
                                                       const double* __restrict__ q, int64_t nq, int64_t* __restrict__ idx_out,
                                                       double* __restrict__ dist_out, int* __restrict__ fallback_count) {
    const int64_t qi = blockIdx.x;
    const int lane = threadIdx.x;
    const double qx = q[3 * qi], qy = q[3 * qi + 1], qz = q[3 * qi + 2];
    const long long cx = nn3_cell(qx, inv_cell), cy = nn3_cell(qy, inv_cell), cz = nn3_cell(qz, inv_cell);
    Best best{INFINITY, 0x7FFFFFFF};
    bool done = false;
    for (int r = 1; r <= NN3_MAX_RINGS && !done; ++r) {
        const int side = 2 * r + 1;
        const int columns = side * side;
        for (int base = 0; base < columns; base += 64) {
            const int t = base + lane;
            int lo_a = 0, len_a = 0, lo_b = 0, len_b = 0;
            if (t < columns) {
                const int dx = t / side - r, dy = t % side - r;
                const long long ax = cx + dx, ay = cy + dy;
                const bool whole = r == 1 || dx == -r || dx == r || dy == -r || dy == r;
                if (whole) {
                    lo_a = grid3::lower_bound(keys, n, grid3::key(ax, ay, cz - r));
                    len_a = grid3::lower_bound(keys, n, grid3::key(ax, ay, cz + r) + 1) - lo_a;
                } else {
                    lo_a = grid3::lower_bound(keys, n, grid3::key(ax, ay, cz - r));
                    len_a = grid3::lower_bound(keys, n, grid3::key(ax, ay, cz - r) + 1) - lo_a;
                    lo_b = grid3::lower_bound(keys, n, grid3::key(ax, ay, cz + r));
                    len_b = grid3::lower_bound(keys, n, grid3::key(ax, ay, cz + r) + 1) - lo_b;
                }
            }
            unsigned long long ma = __ballot(len_a > 0);
            while (ma) {
                const int src = __ffsll((long long)ma) - 1;
                ma &= ma - 1;
                nn3_scan_run(best, sorted, order, __shfl(lo_a, src), __shfl(len_a, src), qx, qy, qz, lane);
            }
            unsigned long long mb = __ballot(len_b > 0);
            while (mb) {
                const int src = __ffsll((long long)mb) - 1;
                mb &= mb - 1;
                nn3_scan_run(best, sorted, order, __shfl(lo_b, src), __shfl(len_b, src), qx, qy, qz, lane);
            }
        }
        best = grid3::wave_best(best);
        const double reach = ((double)r * cell) * NN3_RING_SLACK;
        done = best.d2 < reach * reach;
    }
    if (!done) {
        // more shells than the cap: every point (the shells already searched are read again -- the best of all is the best)
        nn3_scan_run(best, sorted, order, 0, n, qx, qy, qz, lane);
        best = grid3::wave_best(best);
        if (fallback_count && lane == 0) atomicAdd(fallback_count, 1);
    }
    if (lane == 0) {
        const bool found = best.idx != 0x7FFFFFFF;   // (not found: every d2 is a NaN)
        idx_out[qi] = found ? (int64_t)best.idx : (int64_t)-1;
        dist_out[qi] = found ? sqrt(best.d2) : NAN;
    }
}

// ---------------------------------------------------------------------------------------------------------------- k nearest
// The k best so far, sorted by (d2, index): lane i of the wave holds the i-th smallest, lanes >= k stay at (+inf, 0x7FFFFFFF) for
// ever.  kth is lane k - 1's entry, the same value in every lane.
struct Nn3List {
    double d2;
    int idx;
    double kth_d2;
    int kth_idx;
};
__device__ __forceinline__ void nn3_list_clear(Nn3List& l) {
    l.d2 = l.kth_d2 = INFINITY;
    l.idx = l.kth_idx = 0x7FFFFFFF;
}
// one candidate, the same in every lane and below the k-th entry: entries above it move up a lane, the lane at its position takes it,
// lane k - 1's old entry falls off
__device__ __forceinline__ void nn3_list_insert(Nn3List& l, double cd2, int cidx, int k, int lane) {
    const bool above = grid3::closer(cd2, cidx, l.d2, l.idx);          // false .. false true .. true over the lanes: the list is sorted
    const double up_d2 = __shfl_up(l.d2, 1);
    const int up_idx = __shfl_up(l.idx, 1);
    const bool up_above = __shfl_up((int)above, 1) != 0 && lane > 0;   // (lane 0 reads itself)
    if (above && lane < k) {
        l.d2 = up_above ? up_d2 : cd2;
        l.idx = up_above ? up_idx : cidx;
    }
    l.kth_d2 = __shfl(l.d2, k - 1);
    l.kth_idx = __shfl(l.idx, k - 1);
}
// the points sorted[lo, lo + len) against the query, a lane per point, 64 at a time; lo and len are the same in every lane.  A
// candidate needs d2 <= max_d2 and a place below the k-th entry (a NaN d2 has neither); the marked ones are inserted one after
// another, each tested again against the k-th entry as it stands by then.
__device__ __forceinline__ void nn3_knn_run(Nn3List& l, const double* __restrict__ sorted, const int* __restrict__ order, int lo, int len,
                                            double qx, double qy, double qz, double max_d2, int k, int lane) {
    for (int t0 = 0; t0 < len; t0 += 64) {
        const int t = t0 + lane;
        double d2 = NAN;
        int j = 0x7FFFFFFF;
        if (t < len) {
            const int64_t s = (int64_t)lo + t;
            const double dx = sorted[3 * s] - qx, dy = sorted[3 * s + 1] - qy, dz = sorted[3 * s + 2] - qz;
            d2 = (dx * dx + dy * dy) + dz * dz;
            j = order[s];
        }
        unsigned long long m = __ballot(d2 <= max_d2 && grid3::closer(d2, j, l.kth_d2, l.kth_idx));
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const double cd2 = __shfl(d2, src);
            const int cidx = __shfl(j, src);
            if (grid3::closer(cd2, cidx, l.kth_d2, l.kth_idx)) nn3_list_insert(l, cd2, cidx, k, lane);   // (the same branch in every lane)
        }
    }
}

// One wave (= one workgroup) per query: nn3_query_kernel's walk with the list where its Best is.  After shell r the search stops
// when the k-th d2 is below reach^2 = (r cell NN3_RING_SLACK)^2 -- the list is full then (an empty entry is +inf), and every point
// outside the searched cube has a computed d2 >= reach^2, so it can neither beat nor tie an entry -- or when reach^2 > max_d2: every
// point with d2 <= max_d2 is inside the cube then.  The end of a column's run is grid3::upper_bound (the last key of all is 2^63 - 1).
__global__ __launch_bounds__(64) void nn3_knn_kernel(const double* __restrict__ sorted, const long long* __restrict__ keys,
                                                     const int* __restrict__ order, int n, double inv_cell, double cell,
                                                     const double* __restrict__ q, int k, double max_d2, int64_t* __restrict__ idx_out,
                                                     double* __restrict__ d2_out, int* __restrict__ count_out,
                                                     int* __restrict__ fallback_count) {
    const int64_t qi = blockIdx.x;
    const int lane = threadIdx.x;
    const double qx = q[3 * qi], qy = q[3 * qi + 1], qz = q[3 * qi + 2];
    const long long cx = nn3_cell(qx, inv_cell), cy = nn3_cell(qy, inv_cell), cz = nn3_cell(qz, inv_cell);
    Nn3List list;
    nn3_list_clear(list);
    bool done = false;
    for (int r = 1; r <= NN3_MAX_RINGS && !done; ++r) {
        const int side = 2 * r + 1;
        const int columns = side * side;
        for (int base = 0; base < columns; base += 64) {
            const int t = base + lane;
            int lo_a = 0, len_a = 0, lo_b = 0, len_b = 0;
            if (t < columns) {
                const int dx = t / side - r, dy = t % side - r;
                const long long ax = cx + dx, ay = cy + dy;
                const bool whole = r == 1 || dx == -r || dx == r || dy == -r || dy == r;
                const long long key_lo = grid3::key(ax, ay, cz - r), key_hi = grid3::key(ax, ay, cz + r);
                lo_a = grid3::lower_bound(keys, n, key_lo);
                if (whole) {
                    len_a = grid3::upper_bound(keys, n, key_hi) - lo_a;
                } else {
                    len_a = grid3::upper_bound(keys, n, key_lo) - lo_a;
                    lo_b = grid3::lower_bound(keys, n, key_hi);
                    len_b = grid3::upper_bound(keys, n, key_hi) - lo_b;
                }
            }
            unsigned long long ma = __ballot(len_a > 0);
            while (ma) {
                const int src = __ffsll((long long)ma) - 1;
                ma &= ma - 1;
                nn3_knn_run(list, sorted, order, __shfl(lo_a, src), __shfl(len_a, src), qx, qy, qz, max_d2, k, lane);
            }
            unsigned long long mb = __ballot(len_b > 0);
            while (mb) {
                const int src = __ffsll((long long)mb) - 1;
                mb &= mb - 1;
                nn3_knn_run(list, sorted, order, __shfl(lo_b, src), __shfl(len_b, src), qx, qy, qz, max_d2, k, lane);
            }
        }
        const double reach = ((double)r * cell) * NN3_RING_SLACK;
        done = list.kth_d2 < reach * reach || reach * reach > max_d2;
    }
    if (!done) {
        // more shells than the cap: every point, into an EMPTY list (the shells already searched are read again, and an entry kept
        // from them would be in the list twice)
        nn3_list_clear(list);
        nn3_knn_run(list, sorted, order, 0, n, qx, qy, qz, max_d2, k, lane);
        if (fallback_count && lane == 0) atomicAdd(fallback_count, 1);
    }
    const bool found = list.idx != 0x7FFFFFFF;   // (found implies lane < k)
    const unsigned long long fm = __ballot(found);
    if (lane < k) {
        idx_out[qi * k + lane] = found ? (int64_t)list.idx : (int64_t)-1;
        d2_out[qi * k + lane] = found ? list.d2 : INFINITY;
    }
    if (lane == 0) count_out[qi] = __popcll(fm);
}

grid3::SortWs<false> carve_nn3(void* p, int64_t n, size_t* used = nullptr) {
    VfmCarver c(p);
    const grid3::SortWs<false> w = grid3::carve_sort<false>(c, n);
    if (used) *used = c.used();
    return w;
}

}  // namespace

VFM_EXPORT size_t vfm_nn3_workspace_bytes(int64_t n) {
    size_t used = 0;
    (void)carve_nn3(nullptr, n < 0 ? 0 : n, &used);   // (a null base: only the offsets are computed)
    return used;
}

VFM_EXPORT int vfm_nn3_build(const double* pts, int64_t n, double cell, int64_t* keys_out, int32_t* order_out, double* sorted_out, void* ws,
                             size_t ws_bytes, vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 1 && n <= NN3_MAX_POINTS, "nn3_build: n must be in 1..2^26 (an empty cloud has no nearest point)");
    VFM_CHECK_ARG(cell > 0.0 && cell < INFINITY, "nn3_build: the cell size must be positive and finite");
    VFM_CHECK_ARG(pts && keys_out && order_out && sorted_out && ws, "nn3_build: null pointer");
    VFM_CHECK_ARG(ws_bytes >= vfm_nn3_workspace_bytes(n), "nn3_build: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const grid3::SortWs<false> w = carve_nn3(ws, n);
    VFM_TRY(grid3::build(pts, n, Nn3Cells{1.0 / cell}, nullptr, w, reinterpret_cast<long long*>(keys_out), order_out, st));
    hipLaunchKernelGGL(nn3_gather_kernel, dim3(grid3::blocks256(n)), dim3(256), 0, st, pts, n, order_out, sorted_out);
    VFM_CHECK_LAUNCH("nn3_gather_kernel");
    return VFM_OK;
}

VFM_EXPORT int vfm_nn3_query(const int64_t* keys, const int32_t* order, const double* sorted, int64_t n, double cell, const double* queries,
                             int64_t nq, int64_t* idx_out, double* dist_out, int32_t* fallback_count_out, vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 1 && n <= NN3_MAX_POINTS, "nn3_query: n must be in 1..2^26 (an empty cloud has no nearest point)");
    VFM_CHECK_ARG(cell > 0.0 && cell < INFINITY, "nn3_query: the cell size must be positive and finite");
    VFM_CHECK_ARG(nq >= 0 && nq <= 0x7FFFFFFF, "nn3_query: nq must be in 0..2^31-1");
    hipStream_t st = (hipStream_t)stream;
    if (fallback_count_out) VFM_CHECK_HIP(hipMemsetAsync(fallback_count_out, 0, sizeof(int32_t), st));
    if (nq == 0) return VFM_OK;
    VFM_CHECK_ARG(keys && order && sorted && queries && idx_out && dist_out, "nn3_query: null pointer");
    hipLaunchKernelGGL(nn3_query_kernel, dim3((unsigned)nq), dim3(64), 0, st, sorted, reinterpret_cast<const long long*>(keys), order, (int)n,
                       1.0 / cell, cell, queries, nq, idx_out, dist_out, fallback_count_out);
    VFM_CHECK_LAUNCH("nn3_query_kernel");
    return VFM_OK;
}

VFM_EXPORT int vfm_nn3_knn(const int64_t* keys, const int32_t* order, const double* sorted, int64_t n, double cell, const double* queries,
                           int64_t nq, int k, double max_d2, int64_t* idx_out, double* d2_out, int32_t* count_out,
                           int32_t* fallback_count_out, vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 1 && n <= NN3_MAX_POINTS, "nn3_knn: n must be in 1..2^26 (an empty cloud has no nearest point)");
    VFM_CHECK_ARG(cell > 0.0 && cell < INFINITY, "nn3_knn: the cell size must be positive and finite");
    VFM_CHECK_ARG(nq >= 0 && nq <= 0x7FFFFFFF, "nn3_knn: nq must be in 0..2^31-1");
    VFM_CHECK_ARG(k >= 1 && k <= 64, "nn3_knn: k must be in 1..64 (an entry of the list per lane of the wave)");
    VFM_CHECK_ARG(max_d2 >= 0.0, "nn3_knn: max_d2 must be >= 0 and not a NaN (+inf: no cap)");
    hipStream_t st = (hipStream_t)stream;
    if (fallback_count_out) VFM_CHECK_HIP(hipMemsetAsync(fallback_count_out, 0, sizeof(int32_t), st));
    if (nq == 0) return VFM_OK;
    VFM_CHECK_ARG(keys && order && sorted && queries && idx_out && d2_out && count_out, "nn3_knn: null pointer");
    hipLaunchKernelGGL(nn3_knn_kernel, dim3((unsigned)nq), dim3(64), 0, st, sorted, reinterpret_cast<const long long*>(keys), order, (int)n,
                       1.0 / cell, cell, queries, k, max_d2, idx_out, d2_out, count_out, fallback_count_out);
    VFM_CHECK_LAUNCH("nn3_knn_kernel");
    return VFM_OK;
}

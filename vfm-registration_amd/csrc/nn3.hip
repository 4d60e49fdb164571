// nn3.hip -- exact 1-nearest-neighbour search in 3-D on MI355X (gfx950): the two sklearn.neighbors.KDTree(X, metric="euclidean")
// .query(Q, k=1) calls of registration_node.py:295-298, which recover the row of every correspondence point in the voxelised clouds.
//   Nn3Cells (grid3.h) / nn3_gather_kernel a sorted-key CSR grid over the cloud (cell = the caller's), points copied in cell order
//   nn3_walk (nn3_walk.h)                one wave per query: the 27 cells around the query, then shells of cells, until the sink says
//                                        that no cell outside the searched cube can change its answer; past NN3_MAX_RINGS shells a scan
//                                        of every point
//   nn3_query_kernel                     the walk into a Best per lane (Nn3Nearest)
//   nn3_knn_kernel                       the walk into the k <= 64 best so far, a sorted list in registers, an entry per lane (Nn3List)
// fp64, -ffp-contract=off: d2 = (dx*dx + dy*dy) + dz*dz, dist = sqrt(d2) (correctly rounded), equal d2 to the lower index (a
// convention of this library; sklearn leaves it unspecified).  tests/nn3_oracle.py and tests/knn3_oracle.py repeat it in numpy.
#include "nn3_walk.h"

namespace {

__global__ __launch_bounds__(256) void nn3_gather_kernel(const double* __restrict__ pts, int64_t n, const int* __restrict__ order,
                                                         double* __restrict__ sorted) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t j = order[i];
    sorted[3 * i] = pts[3 * j];
    sorted[3 * i + 1] = pts[3 * j + 1];
    sorted[3 * i + 2] = pts[3 * j + 2];
}

// ---------------------------------------------------------------------------------------------------------------- the nearest
// A Best per lane, reduced over the wave once per shell.  Done when the best d2 is strictly below reach^2: nothing outside the cube can
// beat or tie it.  The scan of every point keeps the best so far: the best of all is the best, however often a point is read.
struct Nn3Nearest {
    Best best{INFINITY, 0x7FFFFFFF};
    __device__ __forceinline__ void run(const Nn3Query& q, int lo, int len) {   // a lane per point
        for (int t = q.lane; t < len; t += 64) {
            const int64_t s = lo + t;
            const double dx = q.sorted[3 * s] - q.x, dy = q.sorted[3 * s + 1] - q.y, dz = q.sorted[3 * s + 2] - q.z;
            grid3::take(best, (dx * dx + dy * dy) + dz * dz, q.order[s]);
        }
    }
    __device__ __forceinline__ bool done(double reach2) {
        best = grid3::wave_best(best);
        return best.d2 < reach2;
    }
    __device__ __forceinline__ void restart() {}
};

__global__ __launch_bounds__(64) void nn3_query_kernel(const double* __restrict__ sorted, const long long* __restrict__ keys,
                                                       const int* __restrict__ order, int n, double inv_cell, double cell,
                                                       const double* __restrict__ q, int64_t nq, int64_t* __restrict__ idx_out,
                                                       double* __restrict__ dist_out, int* __restrict__ fallback_count) {
    const int64_t qi = blockIdx.x;
    const Nn3Query query{sorted, order, q[3 * qi], q[3 * qi + 1], q[3 * qi + 2], (int)threadIdx.x};
    Nn3Nearest sink;
    nn3_walk(sink, query, keys, n, inv_cell, cell, fallback_count);
    if (query.lane == 0) {
        const bool found = sink.best.idx != 0x7FFFFFFF;   // (not found: every d2 is a NaN)
        idx_out[qi] = found ? (int64_t)sink.best.idx : (int64_t)-1;
        dist_out[qi] = found ? sqrt(sink.best.d2) : NAN;
    }
}

// ---------------------------------------------------------------------------------------------------------------- k nearest
// (vfm_reg/utils.py:19-44, faiss.IndexFlatL2.search.)  The k <= 64 best so far, sorted by (d2, index): lane i of the wave holds the
// i-th smallest, lanes >= k stay at (+inf, 0x7FFFFFFF) for ever.  kth is lane k - 1's entry, the same value in every lane.  Done when
// the k-th d2 is strictly below reach^2 -- the list is full then (an empty entry is +inf), and nothing outside the cube can beat or
// tie an entry -- or when reach^2 > max_d2: every point with d2 <= max_d2 is inside the cube.  The scan of every point starts from an
// EMPTY list: an entry kept from the shells would be in the list twice.
struct Nn3List {
    double d2 = INFINITY, kth_d2 = INFINITY;
    int idx = 0x7FFFFFFF, kth_idx = 0x7FFFFFFF;
    int k;
    double max_d2;
    __device__ __forceinline__ Nn3List(int k_, double max_d2_) : k(k_), max_d2(max_d2_) {}
    // one candidate, the same in every lane and below the k-th entry: entries above it move up a lane, the lane at its position takes
    // it, lane k - 1's old entry falls off
    __device__ __forceinline__ void insert(double cd2, int cidx, int lane) {
        const bool above = grid3::closer(cd2, cidx, d2, idx);              // false .. false true .. true over the lanes: the list is sorted
        const double up_d2 = __shfl_up(d2, 1);
        const int up_idx = __shfl_up(idx, 1);
        const bool up_above = __shfl_up((int)above, 1) != 0 && lane > 0;   // (lane 0 reads itself)
        if (above && lane < k) {
            d2 = up_above ? up_d2 : cd2;
            idx = up_above ? up_idx : cidx;
        }
        kth_d2 = __shfl(d2, k - 1);
        kth_idx = __shfl(idx, k - 1);
    }
    // a lane per point, 64 at a time.  A candidate needs d2 <= max_d2 and a place below the k-th entry (a NaN d2 has neither); the
    // marked ones are inserted one after another, each tested again against the k-th entry as it stands by then.
    __device__ __forceinline__ void run(const Nn3Query& q, int lo, int len) {
        for (int t0 = 0; t0 < len; t0 += 64) {
            const int t = t0 + q.lane;
            double pd2 = NAN;
            int j = 0x7FFFFFFF;
            if (t < len) {
                const int64_t s = (int64_t)lo + t;
                const double dx = q.sorted[3 * s] - q.x, dy = q.sorted[3 * s + 1] - q.y, dz = q.sorted[3 * s + 2] - q.z;
                pd2 = (dx * dx + dy * dy) + dz * dz;
                j = q.order[s];
            }
            nn3_each_lane(__ballot(pd2 <= max_d2 && grid3::closer(pd2, j, kth_d2, kth_idx)), [&](int src) {
                const double cd2 = __shfl(pd2, src);
                const int cidx = __shfl(j, src);
                if (grid3::closer(cd2, cidx, kth_d2, kth_idx)) insert(cd2, cidx, q.lane);   // (the same branch in every lane)
            });
        }
    }
    __device__ __forceinline__ bool done(double reach2) const { return kth_d2 < reach2 || reach2 > max_d2; }
    __device__ __forceinline__ void restart() {
        d2 = kth_d2 = INFINITY;
        idx = kth_idx = 0x7FFFFFFF;
    }
};

__global__ __launch_bounds__(64) void nn3_knn_kernel(const double* __restrict__ sorted, const long long* __restrict__ keys,
                                                     const int* __restrict__ order, int n, double inv_cell, double cell,
                                                     const double* __restrict__ q, int k, double max_d2, int64_t* __restrict__ idx_out,
                                                     double* __restrict__ d2_out, int* __restrict__ count_out,
                                                     int* __restrict__ fallback_count) {
    const int64_t qi = blockIdx.x;
    const Nn3Query query{sorted, order, q[3 * qi], q[3 * qi + 1], q[3 * qi + 2], (int)threadIdx.x};
    Nn3List sink(k, max_d2);
    nn3_walk(sink, query, keys, n, inv_cell, cell, fallback_count);
    const int lane = query.lane;
    const bool found = sink.idx != 0x7FFFFFFF;   // (found implies lane < k)
    const unsigned long long fm = __ballot(found);
    if (lane < k) {
        idx_out[qi * k + lane] = found ? (int64_t)sink.idx : (int64_t)-1;
        d2_out[qi * k + lane] = found ? sink.d2 : INFINITY;
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

// What the two query entry points check alike (`who` opens every text) and do before a launch: the count of queries that read every
// point is cleared; *launch is false for nq == 0, which is then complete.
static int nn3_query_begin(const char* who, int64_t n, double cell, int64_t nq, int32_t* fallback_count_out, hipStream_t st, bool* launch) {
    VFM_CHECK_ARG(n >= 1 && n <= NN3_MAX_POINTS, "%s: n must be in 1..2^26 (an empty cloud has no nearest point)", who);
    VFM_CHECK_ARG(cell > 0.0 && cell < INFINITY, "%s: the cell size must be positive and finite", who);
    VFM_CHECK_ARG(nq >= 0 && nq <= 0x7FFFFFFF, "%s: nq must be in 0..2^31-1", who);
    if (fallback_count_out) VFM_CHECK_HIP(hipMemsetAsync(fallback_count_out, 0, sizeof(int32_t), st));
    *launch = nq > 0;
    return VFM_OK;
}

VFM_EXPORT int vfm_nn3_query(const int64_t* keys, const int32_t* order, const double* sorted, int64_t n, double cell, const double* queries,
                             int64_t nq, int64_t* idx_out, double* dist_out, int32_t* fallback_count_out, vfm_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    bool launch = false;
    VFM_TRY(nn3_query_begin("nn3_query", n, cell, nq, fallback_count_out, st, &launch));
    if (!launch) return VFM_OK;
    VFM_CHECK_ARG(keys && order && sorted && queries && idx_out && dist_out, "nn3_query: null pointer");
    hipLaunchKernelGGL(nn3_query_kernel, dim3((unsigned)nq), dim3(64), 0, st, sorted, reinterpret_cast<const long long*>(keys), order, (int)n,
                       1.0 / cell, cell, queries, nq, idx_out, dist_out, fallback_count_out);
    VFM_CHECK_LAUNCH("nn3_query_kernel");
    return VFM_OK;
}

VFM_EXPORT int vfm_nn3_knn(const int64_t* keys, const int32_t* order, const double* sorted, int64_t n, double cell, const double* queries,
                           int64_t nq, int k, double max_d2, int64_t* idx_out, double* d2_out, int32_t* count_out,
                           int32_t* fallback_count_out, vfm_stream_t stream) {
    VFM_CHECK_ARG(k >= 1 && k <= 64, "nn3_knn: k must be in 1..64 (an entry of the list per lane of the wave)");
    VFM_CHECK_ARG(max_d2 >= 0.0, "nn3_knn: max_d2 must be >= 0 and not a NaN (+inf: no cap)");
    hipStream_t st = (hipStream_t)stream;
    bool launch = false;
    VFM_TRY(nn3_query_begin("nn3_knn", n, cell, nq, fallback_count_out, st, &launch));
    if (!launch) return VFM_OK;
    VFM_CHECK_ARG(keys && order && sorted && queries && idx_out && d2_out && count_out, "nn3_knn: null pointer");
    hipLaunchKernelGGL(nn3_knn_kernel, dim3((unsigned)nq), dim3(64), 0, st, sorted, reinterpret_cast<const long long*>(keys), order, (int)n,
                       1.0 / cell, cell, queries, k, max_d2, idx_out, d2_out, count_out, fallback_count_out);
    VFM_CHECK_LAUNCH("nn3_knn_kernel");
    return VFM_OK;
}

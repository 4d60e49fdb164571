// hdbscan.hip -- the minimum spanning tree of exact HDBSCAN* under mutual reachability in 3-D on MI355X (gfx950): the device part of
// hdbscan.HDBSCAN(min_cluster_size=100, min_samples=25) of registration_node.py:735 (the tree and the selection are host work on
// n - 1 edges: hdbscan_host.cpp).  Borůvka over the grid of vfm_nn3_build:
//   w2(i, j) = max(core2[i], core2[j], d2(i, j)), edges ordered by (w2, min(i, j), max(i, j)) -- a strict total order, so THE tree is
//   unique and every component's smallest outgoing edge belongs to it.  A round, five kernels:
//   mreach_bound_kernel    a wave per point, the 27 cells around it only: an upper bound of its component's smallest outgoing w2
//   mreach_search_kernel   a wave per point, nn3_walk into MreachNearest, capped inclusively at that bound: the point's smallest edge
//                          to another component, if it can be its component's; atomicMin of w2's bits per component
//   mreach_pair_kernel     among the points that hold the component's w2, atomicMin of (lo << 32) | hi
//   mreach_hook_kernel     a component's root emits its edge (one chosen from both sides: the smaller root emits) and hooks to the other
//                          component's root; of a pair that chose each other the smaller root stays
//   mreach_flatten_kernel  every point follows the hooks to its new root; the roots are counted for the next round
// ceil(log2 n) rounds are enqueued (Borůvka at least halves the components per round); the kernels of a round that finds one component
// left return at once.  No host synchronisation, no state; fp64, -ffp-contract=off, d2 = (dx*dx + dy*dy) + dz*dz as nn3.hip.
// tests/hdbscan_oracle.py states the same tree by Kruskal over all pairs.
#include "nn3_walk.h"

namespace {

constexpr unsigned long long MREACH_INF_BITS = 0x7FF0000000000000ull;   // +inf: w2 >= +0, so the bits order like the values
constexpr unsigned long long MREACH_NO_PAIR = ~0ull;
constexpr int MREACH_COUNTERS = 64;   // [r]: components at the start of round r (r <= 26); [MREACH_EDGES]: edges emitted
constexpr int MREACH_EDGES = 32;

struct MreachWs {
    int* counters;
    int *comp, *comp_s, *hook, *pbest_j;                    // comp, hook: by point; *_s, pbest_*: by sorted position
    double* core2_s;
    unsigned long long *pbest_w2, *cbest_w2, *cbest_pair;   // cbest_*: by component = the index of its root point
};
MreachWs carve_mreach(void* p, int64_t n, size_t* used = nullptr) {
    VfmCarver c(p);
    const size_t nn = (size_t)(n > 0 ? n : 1);
    MreachWs w{};
    w.counters = c.take<int>(MREACH_COUNTERS);
    w.comp = c.take<int>(nn);
    w.comp_s = c.take<int>(nn);
    w.hook = c.take<int>(nn);
    w.pbest_j = c.take<int>(nn);
    w.core2_s = c.take<double>(nn);
    w.pbest_w2 = c.take<unsigned long long>(nn);
    w.cbest_w2 = c.take<unsigned long long>(nn);
    w.cbest_pair = c.take<unsigned long long>(nn);
    if (used) *used = c.used();
    return w;
}

// The nearest point of ANOTHER component under (w2, min(i, j), max(i, j)).  i is the wave's own point, and j != i for every
// candidate, so for a fixed i that order is (w2, j): a Best per lane, reduced once per shell, as Nn3Nearest.  Candidates above the cap
// are dropped.  Done when the best w2 is strictly below reach^2 -- every point outside the cube has d2 >= reach^2, hence w2 >= reach^2:
// it can neither beat nor tie -- or when reach^2 exceeds the cap: every point with w2 <= cap has d2 <= cap and is inside the cube.
struct MreachNearest {
    const double* __restrict__ core2_s;
    const int* __restrict__ comp_s;
    double core_i, cap;
    int comp_i;
    Best best{INFINITY, 0x7FFFFFFF};
    __device__ __forceinline__ MreachNearest(const double* core2_s_, const int* comp_s_, double core_i_, int comp_i_, double cap_)
        : core2_s(core2_s_), comp_s(comp_s_), core_i(core_i_), cap(cap_), comp_i(comp_i_) {}
    __device__ __forceinline__ void run(const Nn3Query& q, int lo, int len) {   // a lane per point
        for (int t = q.lane; t < len; t += 64) {
            const int64_t s = lo + t;
            const double dx = q.sorted[3 * s] - q.x, dy = q.sorted[3 * s + 1] - q.y, dz = q.sorted[3 * s + 2] - q.z;
            const double w2 = fmax(fmax(core_i, core2_s[s]), (dx * dx + dy * dy) + dz * dz);
            if (comp_s[s] != comp_i && w2 <= cap) grid3::take(best, w2, q.order[s]);
        }
    }
    __device__ __forceinline__ bool done(double reach2) {
        best = grid3::wave_best(best);
        return best.d2 < reach2 || reach2 > cap;
    }
    __device__ __forceinline__ void restart() {}   // (the scan of every point keeps the best so far: the best of all is the best)
};

__device__ __forceinline__ double mreach_load(const unsigned long long* p) {
    return __longlong_as_double((long long)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

__global__ __launch_bounds__(256) void mreach_init_kernel(const int* __restrict__ order, const double* __restrict__ core2, int n, MreachWs w) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const int i = order[s];
    w.comp[i] = i;
    w.comp_s[s] = i;
    w.core2_s[s] = core2[i] + 0.0;   // (-0 -> +0: the bits of a w2 must order like its value)
    w.cbest_w2[s] = MREACH_INF_BITS;
    w.cbest_pair[s] = MREACH_NO_PAIR;
    if (s == 0) w.counters[0] = n;
}

// one wave (= one workgroup) per sorted position
__global__ __launch_bounds__(64) void mreach_bound_kernel(const double* __restrict__ sorted, const long long* __restrict__ keys,
                                                          const int* __restrict__ order, int n, double inv_cell, int round, MreachWs w) {
    if (w.counters[round] <= 1) return;
    const int64_t s = blockIdx.x;
    const Nn3Query q{sorted, order, sorted[3 * s], sorted[3 * s + 1], sorted[3 * s + 2], (int)threadIdx.x};
    MreachNearest sink(w.core2_s, w.comp_s, w.core2_s[s], w.comp_s[s], INFINITY);
    const long long cx = nn3_cell(q.x, inv_cell), cy = nn3_cell(q.y, inv_cell), cz = nn3_cell(q.z, inv_cell);
    Nn3Runs c{0, 0, 0, 0};
    if (q.lane < 9) c = nn3_column_runs(keys, n, cx + (q.lane / 3 - 1), cy + (q.lane % 3 - 1), cz, 1, true);
    nn3_each_lane(__ballot(c.len_a > 0), [&](int src) { sink.run(q, __shfl(c.lo_a, src), __shfl(c.len_a, src)); });
    (void)sink.done(0.0);
    if (q.lane == 0 && sink.best.idx != 0x7FFFFFFF)
        atomicMin(&w.cbest_w2[sink.comp_i], (unsigned long long)__double_as_longlong(sink.best.d2));
}

__global__ __launch_bounds__(64) void mreach_search_kernel(const double* __restrict__ sorted, const long long* __restrict__ keys,
                                                           const int* __restrict__ order, int n, double inv_cell, double cell, int round,
                                                           MreachWs w, int* __restrict__ fallback_count) {
    if (w.counters[round] <= 1) return;
    const int64_t s = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int comp_i = w.comp_s[s];
    const double core_i = w.core2_s[s];
    // Any value this word has held is the w2 of a real outgoing edge, so the component's smallest w2 is at most the cap.  An edge of
    // this point has w2 >= core_i: above the cap it is not the component's.
    const double cap = mreach_load(&w.cbest_w2[comp_i]);
    if (core_i > cap) {
        if (lane == 0) w.pbest_j[s] = -1;
        return;
    }
    const Nn3Query q{sorted, order, sorted[3 * s], sorted[3 * s + 1], sorted[3 * s + 2], lane};
    MreachNearest sink(w.core2_s, w.comp_s, core_i, comp_i, cap);
    nn3_walk(sink, q, keys, n, inv_cell, cell, fallback_count);
    if (lane == 0) {
        const bool found = sink.best.idx != 0x7FFFFFFF;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(sink.best.d2);
        w.pbest_j[s] = found ? sink.best.idx : -1;
        w.pbest_w2[s] = bits;
        if (found) atomicMin(&w.cbest_w2[comp_i], bits);
    }
}

__global__ __launch_bounds__(256) void mreach_pair_kernel(const int* __restrict__ order, int n, int round, MreachWs w) {
    if (w.counters[round] <= 1) return;
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const int j = w.pbest_j[s];
    if (j < 0) return;
    const int c = w.comp_s[s];
    if (w.pbest_w2[s] != w.cbest_w2[c]) return;
    const unsigned i = (unsigned)order[s], uj = (unsigned)j;
    const unsigned lo = i < uj ? i : uj, hi = i < uj ? uj : i;
    atomicMin(&w.cbest_pair[c], ((unsigned long long)lo << 32) | hi);
}

// a thread per point; the roots work.  Reads comp[] and cbest_*[], writes hook[] and the edges: nothing it reads is written here.
__global__ __launch_bounds__(256) void mreach_hook_kernel(int n, int round, MreachWs w, int* __restrict__ edge_lo, int* __restrict__ edge_hi,
                                                          double* __restrict__ edge_w2) {
    if (w.counters[round] <= 1) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || w.comp[i] != i) return;
    const unsigned long long pair = w.cbest_pair[i];
    if (pair == MREACH_NO_PAIR) {   // (with two components or more every root has an outgoing edge)
        w.hook[i] = i;
        return;
    }
    const int lo = (int)(pair >> 32), hi = (int)(pair & 0xFFFFFFFFull);
    const int ca = w.comp[lo], cb = w.comp[hi];
    const int other = ca == i ? cb : ca;
    const bool mutual = w.cbest_pair[other] == pair;   // the same edge from both sides: the order on edges is strict
    const bool stay = mutual && i < other;
    w.hook[i] = stay ? i : other;
    if (!mutual || stay) {
        const int k = atomicAdd(&w.counters[MREACH_EDGES], 1);
        if (k < n - 1) {   // (a forest never has more)
            edge_lo[k] = lo;
            edge_hi[k] = hi;
            edge_w2[k] = __longlong_as_double((long long)w.cbest_w2[i]);
        }
    }
}

// a thread per sorted position.  The hooks form a forest (the pairs that chose each other are broken, a longer cycle needs two equal
// edges): the walk up ends at a root.  Reads hook[], its own comp_s; writes its own comp, comp_s and entry s of the next round's cbest_*.
__global__ __launch_bounds__(256) void mreach_flatten_kernel(const int* __restrict__ order, int n, int round, MreachWs w,
                                                             int* __restrict__ rounds_out) {
    if (w.counters[round] <= 1) return;
    const int s = blockIdx.x * 256 + threadIdx.x;
    bool root = false;
    if (s < n) {
        const int i = order[s];
        int c = w.comp_s[s];
        for (int step = 0; step < n; ++step) {   // (bounded: a chain has fewer links than points)
            const int p = w.hook[c];
            if (p == c) break;
            c = p;
        }
        w.comp[i] = c;
        w.comp_s[s] = c;
        w.cbest_w2[s] = MREACH_INF_BITS;
        w.cbest_pair[s] = MREACH_NO_PAIR;
        root = c == i;
        if (s == 0 && rounds_out) *rounds_out = round + 1;
    }
    const unsigned long long roots = __ballot(root);
    if (roots && (threadIdx.x & 63) == __ffsll((long long)roots) - 1) atomicAdd(&w.counters[round + 1], __popcll(roots));
}

int mreach_rounds(int64_t n) {
    int r = 0;
    while (((int64_t)1 << r) < n) ++r;
    return r;
}

}  // namespace

VFM_EXPORT size_t vfm_mreach_mst_workspace_bytes(int64_t n) {
    size_t used = 0;
    (void)carve_mreach(nullptr, n < 0 ? 0 : n, &used);   // (a null base: only the offsets are computed)
    return used;
}

VFM_EXPORT int vfm_mreach_mst(const int64_t* keys, const int32_t* order, const double* sorted, int64_t n, double cell, const double* core2,
                              int32_t* edge_lo_out, int32_t* edge_hi_out, double* w2_out, int32_t* rounds_out, int32_t* fallback_count_out,
                              void* ws, size_t ws_bytes, vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 2 && n <= NN3_MAX_POINTS, "mreach_mst: n must be in 2..2^26 (a spanning tree of one point has no edge)");
    VFM_CHECK_ARG(cell > 0.0 && cell < INFINITY, "mreach_mst: the cell size must be positive and finite");
    VFM_CHECK_ARG(keys && order && sorted && core2 && edge_lo_out && edge_hi_out && w2_out && ws, "mreach_mst: null pointer");
    VFM_CHECK_ARG(ws_bytes >= vfm_mreach_mst_workspace_bytes(n), "mreach_mst: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const MreachWs w = carve_mreach(ws, n);
    const long long* k = reinterpret_cast<const long long*>(keys);
    const int ni = (int)n;
    const double inv_cell = 1.0 / cell;
    VFM_CHECK_HIP(hipMemsetAsync(w.counters, 0, MREACH_COUNTERS * sizeof(int), st));
    if (rounds_out) VFM_CHECK_HIP(hipMemsetAsync(rounds_out, 0, sizeof(int32_t), st));
    if (fallback_count_out) VFM_CHECK_HIP(hipMemsetAsync(fallback_count_out, 0, sizeof(int32_t), st));
    const dim3 per_point(grid3::blocks256(n)), b256(256), waves((unsigned)n), b64(64);
    hipLaunchKernelGGL(mreach_init_kernel, per_point, b256, 0, st, order, core2, ni, w);
    VFM_CHECK_LAUNCH("mreach_init_kernel");
    const int rounds = mreach_rounds(n);
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(mreach_bound_kernel, waves, b64, 0, st, sorted, k, order, ni, inv_cell, r, w);
        VFM_CHECK_LAUNCH("mreach_bound_kernel");
        hipLaunchKernelGGL(mreach_search_kernel, waves, b64, 0, st, sorted, k, order, ni, inv_cell, cell, r, w, fallback_count_out);
        VFM_CHECK_LAUNCH("mreach_search_kernel");
        hipLaunchKernelGGL(mreach_pair_kernel, per_point, b256, 0, st, order, ni, r, w);
        VFM_CHECK_LAUNCH("mreach_pair_kernel");
        hipLaunchKernelGGL(mreach_hook_kernel, per_point, b256, 0, st, ni, r, w, edge_lo_out, edge_hi_out, w2_out);
        VFM_CHECK_LAUNCH("mreach_hook_kernel");
        hipLaunchKernelGGL(mreach_flatten_kernel, per_point, b256, 0, st, order, ni, r, w, rounds_out);
        VFM_CHECK_LAUNCH("mreach_flatten_kernel");
    }
    return VFM_OK;
}

// teaser.hip -- the device part of TEASER++ registration as registration_node.py:91-159 calls it (cbar2 = 1, noise_bound = 0.2, no scale,
// PMC_EXACT, CHAIN, GNC_TLS) on MI355X (gfx950).  DESIGN.md 7.8 is the specification; tests/teaser_oracle.py restates it.
//   teaser_graph_kernel      the consistency graph as an n x ceil(n / 64) bit matrix: a wave's ballot is one word, the column points in LDS
//   teaser_rank_kernel       the vertices in (degree descending, index ascending) order
//   teaser_greedy_kernel     a greedy clique from each of the first `seeds` vertices of that order: a lower bound h of the clique number
//   teaser_peel_kernel       the fixpoint of "keep v iff popcount(adj[v] & alive) >= h - 1" (the (h - 1)-core: unique, so the order of
//                            removal does not matter) and the kept vertices in ascending index
//   teaser_submatrix_kernel  the kept vertices' sub-matrix, for the host's exact search (teaser_host.cpp)
//   teaser_gnc_kernel        the whole GNC-TLS rotation loop in one workgroup, and the rows tgt - R src for the translation
// The exact search and the translation's sweep are host work (teaser_host.cpp).  fp64, -ffp-contract=off, d2 = (dx*dx + dy*dy) + dz*dz.
// Nothing here synchronises the stream or keeps state between calls.
#include <math.h>

#include "common.h"
#include "rot3.h"

namespace {

constexpr int TEASER_MAX_N = 32768;        // a row of the bit matrix is at most 4 KB, the matrix 128 MB
constexpr int TEASER_MAX_WORDS = TEASER_MAX_N / 64;
constexpr int TEASER_MAX_SEEDS = 16;
constexpr int TEASER_SUM_LANES = 256;      // THE summation order of the GNC loop (below): part of the contract

__host__ __device__ inline int teaser_words(int n) { return (n + 63) / 64; }

// ------------------------------------------------------------------------------------------------------------------- the graph
// A workgroup: 256 columns (a wave per 64: lane = column) x 64 rows.  Lane r keeps the word of row r, so a wave stores 64 words at once.
__global__ __launch_bounds__(256) void teaser_graph_kernel(const double* __restrict__ src, const double* __restrict__ tgt, int n, double beta,
                                                           unsigned long long* __restrict__ adj, int* __restrict__ degree) {
    __shared__ double col[256][6];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = teaser_words(n);
    const int j = (int)blockIdx.x * 256 + tid;
    if (j < n) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            col[tid][c] = src[3 * (int64_t)j + c];
            col[tid][3 + c] = tgt[3 * (int64_t)j + c];
        }
    }
    __syncthreads();
    const int word = (int)blockIdx.x * 4 + wave;
    if (word >= W) return;   // (no barrier below)
    const int row0 = (int)blockIdx.y * 64;
    const double sx = col[tid][0], sy = col[tid][1], sz = col[tid][2], tx = col[tid][3], ty = col[tid][4], tz = col[tid][5];
    unsigned long long mine = 0;
    for (int r = 0; r < 64; ++r) {
        const int i = row0 + r;
        if (i >= n) break;   // (wave-uniform)
        double dx = src[3 * (int64_t)i] - sx, dy = src[3 * (int64_t)i + 1] - sy, dz = src[3 * (int64_t)i + 2] - sz;
        const double d2s = (dx * dx + dy * dy) + dz * dz;
        dx = tgt[3 * (int64_t)i] - tx, dy = tgt[3 * (int64_t)i + 1] - ty, dz = tgt[3 * (int64_t)i + 2] - tz;
        const double d2t = (dx * dx + dy * dy) + dz * dz;
        const bool edge = j < n && j != i && fabs(sqrt(d2s) - sqrt(d2t)) <= beta;   // inclusive; a NaN compares false
        const unsigned long long bits = __ballot(edge);
        if (lane == r) mine = bits;
    }
    const int i = row0 + lane;
    if (i < n) {
        adj[(int64_t)i * W + word] = mine;
        if (mine) atomicAdd(&degree[i], __popcll(mine));
    }
}

// ------------------------------------------------------------------------------------------------------------------- the reduction
struct TeaserReduceWs {
    int *order, *sizes, *count, *worklist;
    unsigned long long* alive;
};
TeaserReduceWs carve_teaser_reduce(void* p, int64_t n, size_t* used = nullptr) {
    VfmCarver c(p);
    const size_t nn = (size_t)(n > 0 ? n : 1);
    TeaserReduceWs w{};
    w.order = c.take<int>(nn);
    w.sizes = c.take<int>(TEASER_MAX_SEEDS);
    w.count = c.take<int>(nn);
    w.worklist = c.take<int>(nn);
    w.alive = c.take<unsigned long long>((nn + 63) / 64);
    if (used) *used = c.used();
    return w;
}

// order[rank] = v, rank = the number of vertices before v in (degree descending, index ascending): a permutation of 0 .. n - 1
__global__ __launch_bounds__(256) void teaser_rank_kernel(const int* __restrict__ degree, int n, int* __restrict__ order) {
    __shared__ int tile[256];
    const int tid = (int)threadIdx.x;
    const int v = (int)blockIdx.x * 256 + tid;
    const int dv = v < n ? degree[v] : 0;
    int rank = 0;
    for (int base = 0; base < n; base += 256) {
        __syncthreads();
        tile[tid] = base + tid < n ? degree[base + tid] : -1;
        __syncthreads();
        const int len = min(256, n - base);
        for (int t = 0; t < len; ++t) {
            const int du = tile[t];
            rank += (du > dv || (du == dv && base + t < v)) ? 1 : 0;
        }
    }
    if (v < n) order[rank] = v;
}

__device__ __forceinline__ bool teaser_bit(const unsigned long long* bits, int v) { return (bits[v >> 6] >> (v & 63)) & 1ull; }

// A workgroup per seed.  P: the candidates (LDS bitset).  The next member is the first vertex of `order` that is in P; P only shrinks, so
// the cursor into `order` only advances: O(n) steps of the cursor plus O(size x W) words for the intersections.
__global__ __launch_bounds__(256) void teaser_greedy_kernel(const unsigned long long* __restrict__ adj, int n, int seeds,
                                                            const int* __restrict__ order, int* __restrict__ sizes) {
    __shared__ unsigned long long P[TEASER_MAX_WORDS];
    __shared__ int s_found;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = (int)blockIdx.x;
    if (s >= seeds || s >= n) {   // (uniform)
        if (tid == 0) sizes[s] = 0;
        return;
    }
    const int W = teaser_words(n);
    const int seed = order[s];
    for (int w = tid; w < W; w += 256) P[w] = adj[(int64_t)seed * W + w];
    int size = 1, cursor = 0;
    for (;;) {
        if (tid == 0) s_found = n;
        __syncthreads();
        int found = n;
        for (int base = cursor; base < n; base += 256) {
            const int r = base + tid;
            const bool hit = r < n && teaser_bit(P, order[r]);
            const unsigned long long hits = __ballot(hit);
            if (hits && lane == 0) atomicMin(&s_found, base + wave * 64 + (__ffsll((long long)hits) - 1));
            __syncthreads();
            found = s_found;
            __syncthreads();        // (everyone has read the word before the next pass may lower it)
            if (found < n) break;   // (uniform: every thread read the same word between the two barriers)
        }
        if (found >= n) break;
        const int u = order[found];
        cursor = found + 1;
        ++size;
        for (int w = tid; w < W; w += 256) P[w] &= adj[(int64_t)u * W + w];   // (clears u itself: the diagonal is clear)
        __syncthreads();
    }
    if (tid == 0) sizes[s] = size;
}

// One workgroup.  count[v] = popcount(adj[v] & alive), kept up to date as vertices leave; a vertex enters the worklist exactly once, when
// its count first is below h - 1 (at the start, or by the decrement that takes it from h - 1 to h - 2), so the list never exceeds n entries.
__global__ __launch_bounds__(1024) void teaser_peel_kernel(const unsigned long long* __restrict__ adj, const int* __restrict__ degree, int n,
                                                           TeaserReduceWs ws, int* __restrict__ kept, int* __restrict__ info) {
    __shared__ int s_tail, s_scan[TEASER_MAX_WORDS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = teaser_words(n);
    int h = 0;
    for (int s = 0; s < TEASER_MAX_SEEDS; ++s) h = max(h, ws.sizes[s]);
    const int need = h - 1;
    if (tid == 0) s_tail = 0;
    for (int w = tid; w < W; w += 1024) {
        const int left = n - w * 64;
        __hip_atomic_store(&ws.alive[w], left >= 64 ? ~0ull : ((1ull << left) - 1ull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    for (int v = tid; v < n; v += 1024) {
        const int d = degree[v];
        __hip_atomic_store(&ws.count[v], d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (count and alive: atomics only, from here on)
        if (d < need) ws.worklist[atomicAdd(&s_tail, 1)] = v;
    }
    int head = 0;
    for (;;) {
        __syncthreads();
        const int tail = s_tail;
        if (head == tail) break;   // (uniform)
        __syncthreads();           // (everyone has read s_tail before anyone appends)
        for (int at = head + wave; at < tail; at += 16) {
            const int v = ws.worklist[at];
            if (lane == 0) atomicAnd(&ws.alive[v >> 6], ~(1ull << (v & 63)));
            for (int w = lane; w < W; w += 64) {
                unsigned long long bits = adj[(int64_t)v * W + w];
                while (bits) {
                    const int u = w * 64 + (__ffsll((long long)bits) - 1);
                    bits &= bits - 1;
                    if (u < n && atomicSub(&ws.count[u], 1) == need) {   // (u < n: always, for a matrix whose padding bits are clear)
                        const int pos = atomicAdd(&s_tail, 1);
                        if (pos < n) ws.worklist[pos] = u;   // (always: a vertex enters once)
                    }
                }
            }
        }
        head = tail;
    }
    // the kept vertices in ascending index: an inclusive scan of the words' popcounts (W <= 512 <= the workgroup)
    const unsigned long long mine = tid < W ? __hip_atomic_load(&ws.alive[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    if (tid < TEASER_MAX_WORDS) s_scan[tid] = __popcll(mine);
    __syncthreads();
    for (int step = 1; step < TEASER_MAX_WORDS; step <<= 1) {
        int add = 0;
        if (tid < TEASER_MAX_WORDS && tid >= step) add = s_scan[tid - step];
        __syncthreads();
        if (tid < TEASER_MAX_WORDS) s_scan[tid] += add;
        __syncthreads();
    }
    if (tid < W) {
        int at = s_scan[tid] - __popcll(mine);
        unsigned long long bits = mine;
        while (bits) {
            kept[at++] = tid * 64 + (__ffsll((long long)bits) - 1);
            bits &= bits - 1;
        }
    }
    if (tid == 0) {
        info[0] = h;
        info[1] = s_scan[TEASER_MAX_WORDS - 1];
    }
}

// a wave per kept row; lane = kept column of the word
__global__ __launch_bounds__(256) void teaser_submatrix_kernel(const unsigned long long* __restrict__ adj, int n, const int* __restrict__ kept,
                                                               int k, unsigned long long* __restrict__ sub) {
    const int lane = (int)threadIdx.x & 63;
    const int r = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (r >= k) return;   // (wave-uniform)
    const int W = teaser_words(n), Wk = teaser_words(k);
    const int vr = kept[r];
    const bool row_ok = (unsigned)vr < (unsigned)n;
    for (int w = 0; w < Wk; ++w) {
        const int c = w * 64 + lane;
        bool bit = false;
        if (c < k && row_ok) {
            const int vc = kept[c];
            bit = (unsigned)vc < (unsigned)n && ((adj[(int64_t)vr * W + (vc >> 6)] >> (vc & 63)) & 1ull);
        }
        const unsigned long long word = __ballot(bit);
        if (lane == 0) sub[(int64_t)r * Wk + w] = word;
    }
}

// ------------------------------------------------------------------------------------------------------------------- GNC-TLS
// THE order of every sum over the chain: thread l of 256 adds the terms i = l, l + 256, l + 512, ... ascending, from +0.0; then
// p_l = p_l + p_{l + s} for l < s, s = 128, 64, ..., 1.  It does not depend on the launch: the kernel is always one workgroup of 256.
template <int K>
__device__ __forceinline__ void teaser_tree(double (*p)[TEASER_SUM_LANES], int tid) {
    __syncthreads();
    for (int s = TEASER_SUM_LANES / 2; s >= 1; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < K; ++q) p[q][tid] = p[q][tid] + p[q][tid + s];
        }
        __syncthreads();
    }
}

struct TeaserGncWs {
    double *x, *y;
};
TeaserGncWs carve_teaser_gnc(void* p, int64_t k, size_t* used = nullptr) {
    VfmCarver c(p);
    const size_t m = (size_t)(k > 1 ? k - 1 : 1);
    TeaserGncWs w{};
    w.x = c.take<double>(3 * m);
    w.y = c.take<double>(3 * m);
    if (used) *used = c.used();
    return w;
}

__global__ __launch_bounds__(TEASER_SUM_LANES) void teaser_gnc_kernel(const double* __restrict__ src, const double* __restrict__ tgt, int n,
                                                                      const int* __restrict__ clique, int k, double nb2, double factor,
                                                                      int max_iterations, double cost_threshold, TeaserGncWs ws,
                                                                      double* __restrict__ R_out, double* __restrict__ weights,
                                                                      int* __restrict__ iterations_out, double* __restrict__ v_out) {
    __shared__ double part[9][TEASER_SUM_LANES];
    __shared__ int s_bad;
    const int tid = (int)threadIdx.x;
    const int m = k - 1;   // the chain
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int i = tid; i < k; i += TEASER_SUM_LANES)
        if ((unsigned)clique[i] >= (unsigned)n) s_bad = 1;
    __syncthreads();
    if (s_bad) {   // (uniform) an index outside the correspondences: nothing is read through it
        if (tid == 0) *iterations_out = -1;
        return;
    }
    for (int i = tid; i < m; i += TEASER_SUM_LANES) {
        const int64_t a = clique[i], b = clique[i + 1];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ws.x[3 * i + c] = src[3 * b + c] - src[3 * a + c];
            ws.y[3 * i + c] = tgt[3 * b + c] - tgt[3 * a + c];
        }
        weights[i] = 1.0;
    }
    // (x, y and weights[i] are read back by the thread that wrote them only: i = tid mod 256 throughout)
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    double mu = 1.0, prev = INFINITY;
    int iterations = 0;
    for (int it = 0; it < max_iterations; ++it) {
        // 1. H = sum w_i y_i x_i^T, R = rot_from_sigma(H)
        double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < m; i += TEASER_SUM_LANES) {
            const double w = weights[i];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[r * 3 + c] = acc[r * 3 + c] + (w * ws.y[3 * i + r]) * ws.x[3 * i + c];
        }
        __syncthreads();   // (the previous iteration's reads of part[] are over)
#pragma unroll
        for (int q = 0; q < 9; ++q) part[q][tid] = acc[q];
        teaser_tree<9>(part, tid);
        double H[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) H[q] = part[q][0];
        if (!rot_from_sigma(H, R)) {
#pragma unroll
            for (int q = 0; q < 9; ++q) R[q] = (q % 4 == 0) ? 1.0 : 0.0;
        }
        // 2. residuals, 5. cost with the old weights, and at it == 0 the largest residual
        double cost_l = 0.0, max_l = -INFINITY;
        for (int i = tid; i < m; i += TEASER_SUM_LANES) {
            const double x0 = ws.x[3 * i], x1 = ws.x[3 * i + 1], x2 = ws.x[3 * i + 2];
            const double e0 = ws.y[3 * i] - ((R[0] * x0 + R[1] * x1) + R[2] * x2);
            const double e1 = ws.y[3 * i + 1] - ((R[3] * x0 + R[4] * x1) + R[5] * x2);
            const double e2 = ws.y[3 * i + 2] - ((R[6] * x0 + R[7] * x1) + R[8] * x2);
            const double r = (e0 * e0 + e1 * e1) + e2 * e2;
            cost_l = cost_l + weights[i] * r;
            max_l = r > max_l ? r : max_l;
        }
        __syncthreads();
        part[0][tid] = cost_l;
        part[1][tid] = max_l;
        __syncthreads();
        for (int s = TEASER_SUM_LANES / 2; s >= 1; s >>= 1) {
            if (tid < s) {
                part[0][tid] = part[0][tid] + part[0][tid + s];
                part[1][tid] = part[1][tid + s] > part[1][tid] ? part[1][tid + s] : part[1][tid];
            }
            __syncthreads();
        }
        const double cost = part[0][0];
        if (it == 0) {   // 3.
            mu = 1.0 / ((2.0 * part[1][0]) / nb2 - 1.0);
            if (!(mu > 0.0) || !(mu < INFINITY)) break;   // (uniform; not finite: a deviation that keeps the weights free of NaNs)
        }
        const double th1 = (mu + 1.0) / mu * nb2, th2 = mu / (mu + 1.0) * nb2;   // 4.
        for (int i = tid; i < m; i += TEASER_SUM_LANES) {   // 6. (the residual again: the same operations give the same bits)
            const double x0 = ws.x[3 * i], x1 = ws.x[3 * i + 1], x2 = ws.x[3 * i + 2];
            const double e0 = ws.y[3 * i] - ((R[0] * x0 + R[1] * x1) + R[2] * x2);
            const double e1 = ws.y[3 * i + 1] - ((R[3] * x0 + R[4] * x1) + R[5] * x2);
            const double e2 = ws.y[3 * i + 2] - ((R[6] * x0 + R[7] * x1) + R[8] * x2);
            const double r = (e0 * e0 + e1 * e1) + e2 * e2;
            double w;
            if (r >= th1) w = 0.0;
            else if (r <= th2) w = 1.0;
            else w = sqrt(nb2 * mu * (mu + 1.0) / r) - mu;
            weights[i] = w;
        }
        iterations = it + 1;
        const double diff = fabs(cost - prev);   // 7.
        mu = mu * factor;
        prev = cost;
        if (diff < cost_threshold) break;   // (uniform)
    }
    if (tid < 9) R_out[tid] = R[tid];
    if (tid == 0) *iterations_out = iterations;
    for (int i = tid; i < k; i += TEASER_SUM_LANES) {
        const int64_t a = clique[i];
        const double s0 = src[3 * a], s1 = src[3 * a + 1], s2 = src[3 * a + 2];
        v_out[3 * i] = tgt[3 * a] - ((R[0] * s0 + R[1] * s1) + R[2] * s2);
        v_out[3 * i + 1] = tgt[3 * a + 1] - ((R[3] * s0 + R[4] * s1) + R[5] * s2);
        v_out[3 * i + 2] = tgt[3 * a + 2] - ((R[6] * s0 + R[7] * s1) + R[8] * s2);
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------- entry points
VFM_EXPORT int vfm_teaser_graph(const double* src, const double* tgt, int64_t n, double noise_bound, double cbar2, uint64_t* adj_out,
                                int32_t* degree_out, vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 1 && n <= TEASER_MAX_N, "teaser_graph: n must be in 1..32768 (a row of the bit matrix is at most 4 KB)");
    VFM_CHECK_ARG(noise_bound >= 0.0 && noise_bound < INFINITY && cbar2 >= 0.0 && cbar2 < INFINITY,
                  "teaser_graph: noise_bound and cbar2 must be finite and not negative");
    VFM_CHECK_ARG(src && tgt && adj_out && degree_out, "teaser_graph: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int ni = (int)n, W = teaser_words(ni);
    const double beta = 2.0 * noise_bound * sqrt(cbar2);
    VFM_CHECK_HIP(hipMemsetAsync(degree_out, 0, (size_t)n * sizeof(int32_t), st));
    hipLaunchKernelGGL(teaser_graph_kernel, dim3((unsigned)((W + 3) / 4), (unsigned)W), dim3(256), 0, st, src, tgt, ni, beta,
                       reinterpret_cast<unsigned long long*>(adj_out), degree_out);
    VFM_CHECK_LAUNCH("teaser_graph_kernel");
    return VFM_OK;
}

VFM_EXPORT size_t vfm_teaser_reduce_workspace_bytes(int64_t n) {
    size_t used = 0;
    (void)carve_teaser_reduce(nullptr, n < 0 ? 0 : n, &used);
    return used;
}

VFM_EXPORT int vfm_teaser_reduce(const uint64_t* adj, const int32_t* degree, int64_t n, int32_t seeds, int32_t* kept_out, int32_t* info_out,
                                 void* ws, size_t ws_bytes, vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 1 && n <= TEASER_MAX_N, "teaser_reduce: n must be in 1..32768");
    VFM_CHECK_ARG(seeds >= 1 && seeds <= TEASER_MAX_SEEDS, "teaser_reduce: seeds must be in 1..16");
    VFM_CHECK_ARG(adj && degree && kept_out && info_out && ws, "teaser_reduce: null pointer");
    if (ws_bytes < vfm_teaser_reduce_workspace_bytes(n)) return vfm_fail(VFM_EWORKSPACE, "teaser_reduce: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const TeaserReduceWs w = carve_teaser_reduce(ws, n);
    const int ni = (int)n;
    const unsigned long long* a = reinterpret_cast<const unsigned long long*>(adj);
    hipLaunchKernelGGL(teaser_rank_kernel, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, st, degree, ni, w.order);
    VFM_CHECK_LAUNCH("teaser_rank_kernel");
    hipLaunchKernelGGL(teaser_greedy_kernel, dim3(TEASER_MAX_SEEDS), dim3(256), 0, st, a, ni, (int)seeds, w.order, w.sizes);
    VFM_CHECK_LAUNCH("teaser_greedy_kernel");
    hipLaunchKernelGGL(teaser_peel_kernel, dim3(1), dim3(1024), 0, st, a, degree, ni, w, kept_out, info_out);
    VFM_CHECK_LAUNCH("teaser_peel_kernel");
    return VFM_OK;
}

VFM_EXPORT int vfm_teaser_submatrix(const uint64_t* adj, int64_t n, const int32_t* kept, int64_t k, uint64_t* sub_out, vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 1 && n <= TEASER_MAX_N, "teaser_submatrix: n must be in 1..32768");
    VFM_CHECK_ARG(k >= 1 && k <= n, "teaser_submatrix: k must be in 1..n");
    VFM_CHECK_ARG(adj && kept && sub_out, "teaser_submatrix: null pointer");
    hipLaunchKernelGGL(teaser_submatrix_kernel, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned long long*>(adj), (int)n, kept, (int)k, reinterpret_cast<unsigned long long*>(sub_out));
    VFM_CHECK_LAUNCH("teaser_submatrix_kernel");
    return VFM_OK;
}

VFM_EXPORT size_t vfm_teaser_gnc_workspace_bytes(int64_t k) {
    size_t used = 0;
    (void)carve_teaser_gnc(nullptr, k < 0 ? 0 : k, &used);
    return used;
}

VFM_EXPORT int vfm_teaser_gnc(const double* src, const double* tgt, int64_t n, const int32_t* clique, int64_t k, double noise_bound,
                              double gnc_factor, int32_t max_iterations, double cost_threshold, double* R_out, double* weights_out,
                              int32_t* iterations_out, double* v_out, void* ws, size_t ws_bytes, vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 2 && n <= TEASER_MAX_N, "teaser_gnc: n must be in 2..32768");
    VFM_CHECK_ARG(k >= 2 && k <= n, "teaser_gnc: the clique must have 2..n members (a smaller one is no solution)");
    VFM_CHECK_ARG(noise_bound >= 0.0 && noise_bound < INFINITY, "teaser_gnc: noise_bound must be finite and not negative");
    VFM_CHECK_ARG(gnc_factor > 1.0 && gnc_factor < INFINITY, "teaser_gnc: gnc_factor must be above 1 and finite");
    VFM_CHECK_ARG(max_iterations >= 1, "teaser_gnc: max_iterations must be at least 1");
    VFM_CHECK_ARG(cost_threshold >= 0.0, "teaser_gnc: cost_threshold must not be negative or a NaN");
    VFM_CHECK_ARG(src && tgt && clique && R_out && weights_out && iterations_out && v_out && ws, "teaser_gnc: null pointer");
    if (ws_bytes < vfm_teaser_gnc_workspace_bytes(k)) return vfm_fail(VFM_EWORKSPACE, "teaser_gnc: workspace too small");
    double nb2 = noise_bound * noise_bound;
    if (nb2 < 1e-16) nb2 = 1e-2;
    hipLaunchKernelGGL(teaser_gnc_kernel, dim3(1), dim3(TEASER_SUM_LANES), 0, (hipStream_t)stream, src, tgt, (int)n, clique, (int)k, nb2,
                       gnc_factor, (int)max_iterations, cost_threshold, carve_teaser_gnc(ws, k), R_out, weights_out, iterations_out, v_out);
    VFM_CHECK_LAUNCH("teaser_gnc_kernel");
    return VFM_OK;
}

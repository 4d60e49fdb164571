// pca.hip -- descriptor PCA and the map filter's colour gate on MI355X (gfx950): image_features.py:162-192 (run_pca, FeatUp's pca
// restated from its published source) and registration_node.py:696-702.  Four entry points, no state, no floating-point atomics;
// everything is fp64 and -ffp-contract=off, and every result is a pure function of its inputs.
//   vfm_pca_moments   mean[d] and the scatter S = sum_n (x_n - mean)(x_n - mean)^T.
//     pca_colsum_kernel     column sums of PCA_MEAN_SLABS row slabs: a thread per (column, row mod 4), rows ascending, the four
//                           phases added as (p0 + p1) + (p2 + p3)
//     pca_mean_kernel       the slabs added in ascending order, divided by n
//     pca_gram_kernel       the centred Gram on v_mfma_f64_16x16x4_f64.  The 16-column tiles are grouped four by four into blocks of 64
//                           columns; a workgroup takes one pair of blocks BI <= BJ and one slab of rows, its wave w the tiles
//                           (4 BI + w, 4 BJ + t), t = 0..3, of which those with I <= J inside d are computed.  Both operands of a
//                           step are taken the same way -- lane l holds xc[row 4 g + (l >> 4)][16 T + (l & 15)] -- since
//                           A[i][k] = xc[k][16 I + i] and B[k][j] = xc[k][16 J + j]; the rows come through the LDS, centred, 16 at a
//                           time.  Columns >= d and rows >= n are zeros (the CENTRED value is zero: nothing is loaded, no mean is
//                           subtracted).
//     pca_gram_reduce_kernel the slabs' partial tiles added in ascending order; C/D of the f64 MFMA is col = lane & 15,
//                           row = (lane >> 4) + 4 reg.  A tile I < J is written to S[i][j] and S[j][i]; of a diagonal tile the
//                           elements i <= j are, so S is symmetric bit for bit.
//   vfm_pca_project   y = (x - mean) . components^T, a wave per row in the order DESIGN §7.6 fixes; the all-zero flag; min / max
//   vfm_pca_colours   (y - min) / (max - min), fp32 values or truncated uint8 colours
//   vfm_colour_gate   per colour the rows within the radius, ascending (one workgroup per colour, ordered as vfm_threshold_compact)
#include "common.h"
#include "ordered_compact.h"

#include <hip/hip_fp16.h>
#include <math.h>

namespace {

constexpr int PCA_MAX_D = 768;
constexpr int PCA_MAX_K = 8;
constexpr int PCA_MEAN_SLABS = 256;
constexpr int PCA_GRAM_WGS = 1024;        // pairs x slabs aims at this many workgroups ...
constexpr int PCA_GRAM_MAX_SLABS = 256;   // ... with at most this many slabs
constexpr int PCA_PROJECT_MAX_WGS = 2048;
constexpr int PCA_TILE_DOUBLES = 256;     // a 16 x 16 tile

typedef double pca_f64x4 __attribute__((ext_vector_type(4)));

template <bool F16>
__device__ __forceinline__ double pca_load(const void* __restrict__ x, int64_t i) {
    if (F16) return (double)__half2float(static_cast<const __half*>(x)[i]);
    return (double)static_cast<const float*>(x)[i];
}

int pca_blocks(int d) { return (d + 63) / 64; }
int pca_pairs(int d) {
    const int p = pca_blocks(d);
    return p * (p + 1) / 2;
}
int pca_gram_slabs(int d) {   // a function of d alone: the result must not depend on anything else
    const int pairs = pca_pairs(d);
    int s = (PCA_GRAM_WGS + pairs - 1) / pairs;
    return s < 1 ? 1 : s > PCA_GRAM_MAX_SLABS ? PCA_GRAM_MAX_SLABS : s;
}

struct PcaMomentsWs {
    double* colsum;   // [PCA_MEAN_SLABS][d]
    double* tiles;    // [slabs][pairs][16 tiles][256]
};
PcaMomentsWs carve_moments(void* p, int d, size_t* used = nullptr) {
    VfmCarver c(p);
    PcaMomentsWs w{};
    w.colsum = c.take<double>((size_t)PCA_MEAN_SLABS * d);
    w.tiles = c.take<double>((size_t)pca_gram_slabs(d) * pca_pairs(d) * 16 * PCA_TILE_DOUBLES);
    if (used) *used = c.used();
    return w;
}

// grid (ceil(d / 64), PCA_MEAN_SLABS), 256 threads: column 64 bx + (t & 63), row phase t >> 6
template <bool F16>
__global__ __launch_bounds__(256) void pca_colsum_kernel(const void* __restrict__ x, int64_t n, int d, double* __restrict__ colsum) {
    __shared__ double part[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), phase = threadIdx.x >> 6;
    const int64_t per = (n + PCA_MEAN_SLABS - 1) / PCA_MEAN_SLABS;
    const int64_t r0 = (int64_t)blockIdx.y * per, r1 = r0 + per < n ? r0 + per : n;
    double s = 0.0;
    if (c < d)
        for (int64_t r = r0 + phase; r < r1; r += 4) s += pca_load<F16>(x, r * d + c);
    part[phase][threadIdx.x & 63] = s;
    __syncthreads();
    if (phase == 0 && c < d) {
        const int t = threadIdx.x;
        colsum[(size_t)blockIdx.y * d + c] = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
    }
}

__global__ __launch_bounds__(256) void pca_mean_kernel(const double* __restrict__ colsum, int64_t n, int d, double* __restrict__ mean) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    double s = 0.0;
    for (int slab = 0; slab < PCA_MEAN_SLABS; ++slab) s += colsum[(size_t)slab * d + c];
    mean[c] = s / (double)n;
}

// pair index -> (BI, BJ), BI <= BJ, row by row of the upper triangle of blocks
__device__ __forceinline__ void pca_pair(int pair, int blocks, int& bi, int& bj) {
    bi = 0;
    int row = blocks;
    while (pair >= row) {
        pair -= row;
        --row;
        ++bi;
    }
    bj = bi + pair;
}

// Four consecutive features of one row as floats (fp16 widens exactly), 0 where there is none.  VEC: d is a multiple of four and
// the rows are aligned for one 16-byte (fp32) / 8-byte (fp16) load.
template <bool F16, bool VEC>
__device__ __forceinline__ void pca_load4(const void* __restrict__ x, int64_t row, int col, int d, bool row_ok, float v[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.0f;
    if (!row_ok || col >= d) return;
    const int64_t at = row * d + col;
    if (VEC) {
        if (F16) {
            const uint2 raw = *reinterpret_cast<const uint2*>(static_cast<const __half*>(x) + at);
            const float2 lo = __half22float2(*reinterpret_cast<const __half2*>(&raw.x)), hi = __half22float2(*reinterpret_cast<const __half2*>(&raw.y));
            v[0] = lo.x, v[1] = lo.y, v[2] = hi.x, v[3] = hi.y;
        } else {
            const float4 q = *reinterpret_cast<const float4*>(static_cast<const float*>(x) + at);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (col + e < d) v[e] = F16 ? __half2float(static_cast<const __half*>(x)[at + e]) : static_cast<const float*>(x)[at + e];
}

constexpr int PCA_CHUNK_ROWS = 16;    // rows staged per trip: four steps of the matrix instruction
constexpr int PCA_LDS_STRIDE = 80;    // doubles per staged row: 64 columns + 16, so that consecutive rows fall into different halves of the banks

// grid (pairs, slabs), 256 threads = 4 waves.  A trip stages 16 rows x (64 columns of block BI, 64 of block BJ) through the LDS, centred
// and widened: thread t loads four consecutive columns of row t / 16 of each block (one 16-byte load where the rows allow it), the next
// trip's loads are issued before this trip's products.  Rows past the slab's end or n and columns past d are stored as zeros.
template <bool F16, bool VEC>
__global__ __launch_bounds__(256, 4) void pca_gram_kernel(const void* __restrict__ x, int64_t n, int d, const double* __restrict__ mean,
                                                          int slabs, double* __restrict__ tiles) {
    __shared__ double stage[2][PCA_CHUNK_ROWS][PCA_LDS_STRIDE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int bi, bj;
    pca_pair(blockIdx.x, (d + 63) / 64, bi, bj);
    const int I = bi * 4 + wave;
    bool active[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int J = bj * 4 + t;
        active[t] = I * 16 < d && J >= I && J * 16 < d;   // (wave-uniform)
    }
    // what this thread stages: row srow of the chunk, columns scol .. scol + 3 of both blocks
    const int srow = threadIdx.x >> 4, scol = (threadIdx.x & 15) * 4;
    const int col_i = bi * 64 + scol, col_j = bj * 64 + scol;
    double mean_i[4], mean_j[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        mean_i[e] = col_i + e < d ? mean[col_i + e] : 0.0;
        mean_j[e] = col_j + e < d ? mean[col_j + e] : 0.0;
    }
    const int64_t groups = (n + 3) / 4;
    const int64_t per = (groups + slabs - 1) / slabs;
    const int64_t g0 = (int64_t)blockIdx.y * per, g1 = g0 + per < groups ? g0 + per : groups;
    const int64_t r0 = g0 * 4, r1 = g1 * 4 < n ? g1 * 4 : n;   // the slab's rows
    pca_f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = pca_f64x4{0.0, 0.0, 0.0, 0.0};
    float vi[4], vj[4];
    bool row_ok = r0 + srow < r1;
    pca_load4<F16, VEC>(x, r0 + srow, col_i, d, row_ok, vi);
    pca_load4<F16, VEC>(x, r0 + srow, col_j, d, row_ok, vj);
    for (int64_t r = r0; r < r1; r += PCA_CHUNK_ROWS) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            stage[0][srow][scol + e] = (row_ok && col_i + e < d) ? (double)vi[e] - mean_i[e] : 0.0;
            stage[1][srow][scol + e] = (row_ok && col_j + e < d) ? (double)vj[e] - mean_j[e] : 0.0;
        }
        __syncthreads();
        const int64_t next = r + PCA_CHUNK_ROWS + srow;
        row_ok = next < r1;
        pca_load4<F16, VEC>(x, next, col_i, d, row_ok, vi);
        pca_load4<F16, VEC>(x, next, col_j, d, row_ok, vj);
        // a group past the slab's end multiplies zeros (acc + 0 * 0 = acc, exactly: an accumulator that starts at +0 never becomes -0)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int krow = 4 * u + (lane >> 4);
            const double a = stage[0][krow][16 * wave + (lane & 15)];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (active[t]) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, stage[1][krow][16 * t + (lane & 15)], acc[t], 0, 0, 0);
        }
        __syncthreads();
    }
    double* out = tiles + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 16 + wave * 4) * PCA_TILE_DOUBLES;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (!active[t]) continue;
        double* o = out + (size_t)t * PCA_TILE_DOUBLES + lane * 4;
        o[0] = acc[t][0];
        o[1] = acc[t][1];
        o[2] = acc[t][2];
        o[3] = acc[t][3];
    }
}

// grid (pairs * 16), 256 threads: thread 4 lane + reg of one tile
__global__ __launch_bounds__(256) void pca_gram_reduce_kernel(const double* __restrict__ tiles, int d, int pairs, int slabs,
                                                              double* __restrict__ scatter) {
    const int pair = blockIdx.x >> 4, tile = blockIdx.x & 15;
    int bi, bj;
    pca_pair(pair, (d + 63) / 64, bi, bj);
    const int I = bi * 4 + (tile >> 2), J = bj * 4 + (tile & 3);
    if (I * 16 >= d || J * 16 >= d || J < I) return;   // (the tiles pca_gram_kernel did not write)
    const int lane = threadIdx.x >> 2, reg = threadIdx.x & 3;
    const int i = (lane >> 4) + 4 * reg, j = lane & 15;
    double s = 0.0;
    for (int slab = 0; slab < slabs; ++slab) s += tiles[(((size_t)slab * pairs + pair) * 16 + tile) * PCA_TILE_DOUBLES + threadIdx.x];
    const int gi = I * 16 + i, gj = J * 16 + j;
    if (gi >= d || gj >= d) return;
    if (I == J && i > j) return;   // (the mirror of (j, i) writes it)
    scatter[(size_t)gi * d + gj] = s;
    scatter[(size_t)gj * d + gi] = s;
}

// ------------------------------------------------------------------------------------------------------------------ projection
// grid min(ceil(n / 4), PCA_PROJECT_MAX_WGS), 256 threads: a wave per row, rows strided by the grid.  Dynamic LDS: mean[d], components[k][d].
template <bool F16>
__global__ __launch_bounds__(256) void pca_project_kernel(const void* __restrict__ x, int64_t n, int d, const double* __restrict__ mean,
                                                          const double* __restrict__ comp, int k, double* __restrict__ y,
                                                          unsigned char* __restrict__ zero_rows, double* __restrict__ part_min,
                                                          double* __restrict__ part_max) {
    extern __shared__ double pca_lds[];
    __shared__ double wmin[4][PCA_MAX_K], wmax[4][PCA_MAX_K];
    double* smean = pca_lds;
    double* scomp = pca_lds + d;
    for (int i = threadIdx.x; i < d; i += 256) smean[i] = mean[i];
    for (int i = threadIdx.x; i < k * d; i += 256) scomp[i] = comp[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double lo[PCA_MAX_K], hi[PCA_MAX_K];
#pragma unroll
    for (int j = 0; j < PCA_MAX_K; ++j) {
        lo[j] = INFINITY;
        hi[j] = -INFINITY;
    }
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < n; row += (int64_t)gridDim.x * 4) {
        double p[PCA_MAX_K];
#pragma unroll
        for (int j = 0; j < PCA_MAX_K; ++j) p[j] = 0.0;
        bool zero = true;
        for (int c = lane; c < d; c += 64) {
            const double v = pca_load<F16>(x, row * d + c);
            zero = zero && v == 0.0;
            const double xc = v - smean[c];
#pragma unroll
            for (int j = 0; j < PCA_MAX_K; ++j)
                if (j < k) {
                    const double t = xc * scomp[j * d + c];
                    p[j] = p[j] + t;
                }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
            for (int j = 0; j < PCA_MAX_K; ++j)
                if (j < k) p[j] = p[j] + __shfl_xor(p[j], s);
        }
        const bool all_zero = __all(zero);
#pragma unroll
        for (int j = 0; j < PCA_MAX_K; ++j)
            if (j < k) {
                if (lane == j) y[row * k + j] = p[j];
                lo[j] = p[j] < lo[j] ? p[j] : lo[j];
                hi[j] = p[j] > hi[j] ? p[j] : hi[j];
            }
        if (lane == 0) zero_rows[row] = all_zero ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < PCA_MAX_K; ++j)
        if (lane == j && j < k) {
            wmin[wave][j] = lo[j];
            wmax[wave][j] = hi[j];
        }
    __syncthreads();
    if ((int)threadIdx.x < k) {
        const int j = threadIdx.x;
        part_min[(size_t)blockIdx.x * PCA_MAX_K + j] = fmin(fmin(wmin[0][j], wmin[1][j]), fmin(wmin[2][j], wmin[3][j]));
        part_max[(size_t)blockIdx.x * PCA_MAX_K + j] = fmax(fmax(wmax[0][j], wmax[1][j]), fmax(wmax[2][j], wmax[3][j]));
    }
}

// one workgroup of 64 x PCA_MAX_K threads: thread (j, l) takes the workgroups l, l + 64, ... of component j
__global__ __launch_bounds__(64 * PCA_MAX_K) void pca_minmax_kernel(const double* __restrict__ part_min, const double* __restrict__ part_max,
                                                                    int wgs, int k, double* __restrict__ min_out, double* __restrict__ max_out) {
    const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
    double lo = INFINITY, hi = -INFINITY;
    if (j < k)
        for (int w = lane; w < wgs; w += 64) {
            lo = fmin(lo, part_min[(size_t)w * PCA_MAX_K + j]);
            hi = fmax(hi, part_max[(size_t)w * PCA_MAX_K + j]);
        }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, s));
        hi = fmax(hi, __shfl_xor(hi, s));
    }
    if (lane == 0 && j < k) {
        min_out[j] = lo;
        max_out[j] = hi;
    }
}

// a thread per element of y
__global__ __launch_bounds__(256) void pca_colours_kernel(const double* __restrict__ y, const unsigned char* __restrict__ zero_rows,
                                                          int64_t n, int k, const double* __restrict__ mn, const double* __restrict__ mx,
                                                          float* __restrict__ values, unsigned char* __restrict__ rgb) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * k) return;
    const int j = (int)(e % k);
    const double lo = mn[j];
    const double shifted = y[e] - lo;
    const double v = shifted / (mx[j] - lo);   // (max of the shifted values = max - min: the subtraction is monotone)
    if (values) values[e] = (float)v;
    if (rgb) {
        const double c = v * 255.0;
        unsigned char byte = 0;
        if (c >= 0.0 && !zero_rows[e / k]) byte = (unsigned char)(int)(c < 255.0 ? c : 255.0);   // (NaN fails c >= 0: colour 0)
        rgb[e] = byte;
    }
}

// ------------------------------------------------------------------------------------------------------------------ colour gate
// grid (m), 1024 threads: colour blockIdx.x; a pass takes 1024 rows, the survivors keep the rows' order
__global__ __launch_bounds__(1024) void colour_gate_kernel(const unsigned char* __restrict__ colours, int64_t n,
                                                           const double* __restrict__ gate, double r2, int64_t* __restrict__ idx,
                                                           int64_t* __restrict__ counts) {
    __shared__ OrderedCompactLds lds;
    const double cr = gate[3 * blockIdx.x], cg = gate[3 * blockIdx.x + 1], cb = gate[3 * blockIdx.x + 2];
    int64_t* out = idx + (size_t)blockIdx.x * n;
    int64_t base = 0;
    int buf = 0;
    for (int64_t s0 = 0; s0 < n; s0 += 1024, buf ^= 1) {
        const int64_t i = s0 + threadIdx.x;
        bool hit = false;
        if (i < n) {
            const double dr = (double)colours[3 * i] - cr, dg = (double)colours[3 * i + 1] - cg, db = (double)colours[3 * i + 2] - cb;
            hit = (dr * dr + dg * dg) + db * db < r2;
        }
        int total;
        const int place = ordered_compact_pass(lds, buf, hit, total);   // (ordered_compact.h)
        if (hit) out[base + place] = i;
        base += total;
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = base;
}

bool pca_dtype_ok(int dtype) { return dtype == VFM_ROWS_F32 || dtype == VFM_ROWS_F16; }

}  // namespace

VFM_EXPORT size_t vfm_pca_moments_workspace_bytes(int d) {
    if (d < 1 || d > PCA_MAX_D) return 0;
    size_t used = 0;
    (void)carve_moments(nullptr, d, &used);
    return used;
}

VFM_EXPORT int vfm_pca_moments(const void* x, int dtype, int64_t n, int d, double* mean_out, double* scatter_out, void* ws, size_t ws_bytes,
                               vfm_stream_t stream) {
    VFM_CHECK_ARG(pca_dtype_ok(dtype), "pca_moments: unknown row type");
    VFM_CHECK_ARG(d >= 1 && d <= PCA_MAX_D, "pca_moments: d must be in 1..768");
    VFM_CHECK_ARG(n >= 1, "pca_moments: n must be at least 1");
    VFM_CHECK_ARG(x && mean_out && scatter_out && ws, "pca_moments: null pointer");
    if (ws_bytes < vfm_pca_moments_workspace_bytes(d)) return vfm_fail(VFM_EWORKSPACE, "pca_moments: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const PcaMomentsWs w = carve_moments(ws, d);
    const bool f16 = dtype == VFM_ROWS_F16;
    const int blocks = pca_blocks(d), pairs = pca_pairs(d), slabs = pca_gram_slabs(d);
    const bool vec = d % 4 == 0 && reinterpret_cast<uintptr_t>(x) % (f16 ? 8 : 16) == 0;   // a row's four features in one load
    if (f16)
        hipLaunchKernelGGL(pca_colsum_kernel<true>, dim3(blocks, PCA_MEAN_SLABS), dim3(256), 0, st, x, n, d, w.colsum);
    else
        hipLaunchKernelGGL(pca_colsum_kernel<false>, dim3(blocks, PCA_MEAN_SLABS), dim3(256), 0, st, x, n, d, w.colsum);
    VFM_CHECK_LAUNCH("pca_colsum_kernel");
    hipLaunchKernelGGL(pca_mean_kernel, dim3((d + 255) / 256), dim3(256), 0, st, w.colsum, n, d, mean_out);
    VFM_CHECK_LAUNCH("pca_mean_kernel");
    const dim3 gram_grid(pairs, slabs), b256(256);
    if (f16 && vec)
        hipLaunchKernelGGL((pca_gram_kernel<true, true>), gram_grid, b256, 0, st, x, n, d, mean_out, slabs, w.tiles);
    else if (f16)
        hipLaunchKernelGGL((pca_gram_kernel<true, false>), gram_grid, b256, 0, st, x, n, d, mean_out, slabs, w.tiles);
    else if (vec)
        hipLaunchKernelGGL((pca_gram_kernel<false, true>), gram_grid, b256, 0, st, x, n, d, mean_out, slabs, w.tiles);
    else
        hipLaunchKernelGGL((pca_gram_kernel<false, false>), gram_grid, b256, 0, st, x, n, d, mean_out, slabs, w.tiles);
    VFM_CHECK_LAUNCH("pca_gram_kernel");
    hipLaunchKernelGGL(pca_gram_reduce_kernel, dim3(pairs * 16), dim3(256), 0, st, w.tiles, d, pairs, slabs, scatter_out);
    VFM_CHECK_LAUNCH("pca_gram_reduce_kernel");
    return VFM_OK;
}

VFM_EXPORT size_t vfm_pca_project_workspace_bytes(void) {
    return vfm_align_up((size_t)2 * PCA_PROJECT_MAX_WGS * PCA_MAX_K * sizeof(double), 256);
}

VFM_EXPORT int vfm_pca_project(const void* x, int dtype, int64_t n, int d, const double* mean, const double* components, int k, double* y_out,
                               uint8_t* zero_rows_out, double* min_out, double* max_out, void* ws, size_t ws_bytes, vfm_stream_t stream) {
    VFM_CHECK_ARG(pca_dtype_ok(dtype), "pca_project: unknown row type");
    VFM_CHECK_ARG(d >= 1 && d <= PCA_MAX_D, "pca_project: d must be in 1..768");
    VFM_CHECK_ARG(k >= 1 && k <= PCA_MAX_K && k <= d, "pca_project: k must be in 1..8 and at most d");
    VFM_CHECK_ARG(n >= 1, "pca_project: n must be at least 1");
    VFM_CHECK_ARG(x && mean && components && y_out && zero_rows_out && min_out && max_out && ws, "pca_project: null pointer");
    if (ws_bytes < vfm_pca_project_workspace_bytes()) return vfm_fail(VFM_EWORKSPACE, "pca_project: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    double* part_min = static_cast<double*>(ws);
    double* part_max = part_min + (size_t)PCA_PROJECT_MAX_WGS * PCA_MAX_K;
    const int64_t want = (n + 3) / 4;
    const int wgs = (int)(want < PCA_PROJECT_MAX_WGS ? want : PCA_PROJECT_MAX_WGS);
    const size_t lds = (size_t)(k + 1) * d * sizeof(double);   // <= 9 * 768 * 8 = 55 296 bytes
    if (dtype == VFM_ROWS_F16)
        hipLaunchKernelGGL(pca_project_kernel<true>, dim3(wgs), dim3(256), lds, st, x, n, d, mean, components, k, y_out, zero_rows_out, part_min,
                           part_max);
    else
        hipLaunchKernelGGL(pca_project_kernel<false>, dim3(wgs), dim3(256), lds, st, x, n, d, mean, components, k, y_out, zero_rows_out, part_min,
                           part_max);
    VFM_CHECK_LAUNCH("pca_project_kernel");
    hipLaunchKernelGGL(pca_minmax_kernel, dim3(1), dim3(64 * PCA_MAX_K), 0, st, part_min, part_max, wgs, k, min_out, max_out);
    VFM_CHECK_LAUNCH("pca_minmax_kernel");
    return VFM_OK;
}

VFM_EXPORT int vfm_pca_colours(const double* y, const uint8_t* zero_rows, int64_t n, int k, const double* min_in, const double* max_in,
                               float* values_out, uint8_t* rgb_out, vfm_stream_t stream) {
    VFM_CHECK_ARG(k >= 1 && k <= PCA_MAX_K, "pca_colours: k must be in 1..8");
    VFM_CHECK_ARG(n >= 1 && n <= (int64_t)1 << 40, "pca_colours: n must be at least 1");
    VFM_CHECK_ARG(y && min_in && max_in && (values_out || rgb_out), "pca_colours: null pointer");
    VFM_CHECK_ARG(!rgb_out || (k == 3 && zero_rows), "pca_colours: colours need k = 3 and the zero-row flags");
    const int64_t blocks = (n * k + 255) / 256;
    VFM_CHECK_ARG(blocks <= 0x7FFFFFFF, "pca_colours: too many rows for one launch");
    hipLaunchKernelGGL(pca_colours_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, y, zero_rows, n, k, min_in, max_in, values_out,
                       rgb_out);
    VFM_CHECK_LAUNCH("pca_colours_kernel");
    return VFM_OK;
}

VFM_EXPORT int vfm_colour_gate(const uint8_t* colours, int64_t n, const double* gate_colours, int m, double radius, int64_t* idx_out,
                               int64_t* counts_out, vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 1, "colour_gate: n must be at least 1");
    VFM_CHECK_ARG(m >= 1 && m <= 65535, "colour_gate: m must be in 1..65535");
    VFM_CHECK_ARG(radius >= 0.0 && radius < INFINITY, "colour_gate: the radius must be finite and not negative");
    VFM_CHECK_ARG(colours && gate_colours && idx_out && counts_out, "colour_gate: null pointer");
    hipLaunchKernelGGL(colour_gate_kernel, dim3(m), dim3(1024), 0, (hipStream_t)stream, colours, n, gate_colours, radius * radius, idx_out,
                       counts_out);
    VFM_CHECK_LAUNCH("colour_gate_kernel");
    return VFM_OK;
}

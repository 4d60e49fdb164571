// fpfh.hip -- FPFH descriptors on MI355X (gfx950): the CPU work of extract_fpfh_features (vfm_reg/descriptors.py:19-44), which the
// reference runs inside Open3D 0.18:
//   FpfhCells          a sorted-key CSR grid (grid3.h; cell = the search radius) built on the device, for KDTreeFlann
//   fpfh_search_kernel KDTreeFlann::SearchHybrid (KDTreeSearchParamHybrid(radius, max_nn)): the points with d2 < radius^2, ascending by
//                      (d2, index), the first max_nn of them
//   fpfh_normal_kernel PointCloud::EstimateNormals(param, fast_normal_computation = true): ComputeCovariance (one pass) + FastEigen3x3
//   fpfh_vds_*         PointCloud::VoxelDownSample (averaging; normals averaged, not renormalised)
//   fpfh_spfh_kernel   ComputeSPFHFeature (Feature.cpp), 33 bins
//   fpfh_fpfh_kernel   ComputeFPFHFeature (Feature.cpp)
// fp64 throughout, -ffp-contract=off, operation order as Open3D writes it (tests/fpfh_oracle.py repeats it in numpy).  Deviations, all in
// equal distances are ordered by index (nanoflann leaves them unspecified); the down-sample emits voxels in ascending
// (ix, iy, iz) order (Open3D: std::unordered_map iteration order).
#include "grid3.h"

namespace {

constexpr int FPFH_CAP = 1024;      // candidates a query keeps in LDS; more are re-read from the grid (no cap on the answer)
constexpr int FPFH_MAX_NN = FPFH_CAP;
constexpr int64_t FPFH_MAX_POINTS = (int64_t)1 << 26;   // one workgroup per point in three kernels
constexpr int GRID_LIM = (1 << 20) - 2;
// the cell is the radius widened by 1e-6 relative: |p - q| < r then puts p at most one cell from q even after p / cell and q / cell
// are rounded (coordinates up to 2^20 cells)
constexpr double CELL_SLACK = 1.0 + 1e-6;

// clamped cells stay 1-Lipschitz, so the 27-cell cover stays complete (far-out points only share cells)
__device__ __forceinline__ long long grid_cell(double x, double inv_cell) { return grid3::cell(x, inv_cell, GRID_LIM); }
struct FpfhCells {   // the quantiser of grid3::keys_kernel
    static constexpr const char* kernel_name = "grid3::keys_kernel<FpfhCells>";
    double inv_cell;
    __device__ long long operator()(double x, double y, double z, bool&) const {
        return grid3::key(grid_cell(x, inv_cell), grid_cell(y, inv_cell), grid_cell(z, inv_cell));
    }
};

__device__ __forceinline__ unsigned long long lanes_below() {
    return (1ull << (threadIdx.x & 63)) - 1ull;
}

// ---- SearchHybrid: one wave (= one workgroup) per query.
// Pass 1 reads every point of the 27 cells (9 runs of 3 consecutive keys) and counts the candidates (d2 < r2), keeping the first FPFH_CAP
// in LDS.  If more than max_nn qualify, a radix select over the 96-bit key (d2 bits, index) finds the max_nn-th smallest key, 8 bits per
// pass, from LDS or -- past FPFH_CAP -- from the grid again; the candidates at or below it (exactly max_nn) are compacted and ranked.
struct SearchLds {
    double d2[FPFH_CAP];
    int idx[FPFH_CAP];
    int hist[256];
    int rlo[9];
    int roff[10];
    int sel;
};

struct SearchCtx {
    const double* pts;
    const int* order;
    double qx, qy, qz, r2;
};

// f(valid, d2, j) for every candidate slot of the wave (all 64 lanes call f together: it may ballot)
template <typename F>
__device__ __forceinline__ void for_each_candidate(const SearchCtx& c, const SearchLds& s, F&& f) {
    const int total = s.roff[9];
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < total; base += 64) {
        const int t = base + lane;
        bool ok = false;
        double d2 = 0.0;
        int j = 0;
        if (t < total) {
            int r = 0;
            while (t >= s.roff[r + 1]) ++r;
            j = c.order[s.rlo[r] + (t - s.roff[r])];
            const double dx = c.pts[3 * (int64_t)j] - c.qx, dy = c.pts[3 * (int64_t)j + 1] - c.qy, dz = c.pts[3 * (int64_t)j + 2] - c.qz;
            d2 = (dx * dx + dy * dy) + dz * dz;
            ok = d2 < c.r2;
        }
        f(ok, d2, j);
    }
}
template <typename F>
__device__ __forceinline__ void for_each_cached(const SearchLds& s, int count, F&& f) {
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < count; base += 64) {
        const int t = base + lane;
        const bool ok = t < count;
        f(ok, ok ? s.d2[t] : 0.0, ok ? s.idx[t] : 0);
    }
}

__global__ __launch_bounds__(64) void fpfh_search_kernel(const double* __restrict__ pts, int64_t n, const long long* __restrict__ keys,
                                                         const int* __restrict__ order, double inv_cell, double r2, int max_nn,
                                                         int* __restrict__ nbr_idx, double* __restrict__ nbr_d2, int* __restrict__ nbr_cnt,
                                                         int* __restrict__ scanned_out) {
    __shared__ SearchLds s;
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    SearchCtx c{pts, order, pts[3 * q], pts[3 * q + 1], pts[3 * q + 2], r2};
    const long long cx = grid_cell(c.qx, inv_cell), cy = grid_cell(c.qy, inv_cell), cz = grid_cell(c.qz, inv_cell);
    int run_lo = 0, run_len = 0;
    if (lane < 9) {
        const long long ax = cx - 1 + lane / 3, ay = cy - 1 + lane % 3;
        run_lo = grid3::lower_bound(keys, (int)n, grid3::key(ax, ay, cz - 1));
        run_len = grid3::upper_bound(keys, (int)n, grid3::key(ax, ay, cz + 1)) - run_lo;
        s.rlo[lane] = run_lo;
    }
    __syncthreads();
    {
        int lens[9];   // (every lane takes part in the shuffles)
#pragma unroll
        for (int r = 0; r < 9; ++r) lens[r] = __shfl(run_len, r);
        if (lane == 0) {
            int acc = 0;
            for (int r = 0; r < 9; ++r) {
                s.roff[r] = acc;
                acc += lens[r];
            }
            s.roff[9] = acc;
        }
    }
    __syncthreads();
    if (scanned_out && lane == 0) scanned_out[q] = s.roff[9];

    // pass 1: count, cache the first FPFH_CAP
    int cnt = 0;
    for_each_candidate(c, s, [&](bool ok, double d2, int j) {
        const unsigned long long m = __ballot(ok);
        const int pos = cnt + __popcll(m & lanes_below());
        if (ok && pos < FPFH_CAP) {
            s.d2[pos] = d2;
            s.idx[pos] = j;
        }
        cnt += __popcll(m);
    });
    __syncthreads();
    int k = cnt;
    if (cnt > max_nn) {
        // radix select of the max_nn-th smallest (d2 bits, index); d2 >= 0, so its bit pattern orders like the value
        unsigned long long pre_hi = 0, mask_hi = 0;
        unsigned pre_lo = 0, mask_lo = 0;
        int kr = max_nn;
        const bool cached = cnt <= FPFH_CAP;
        for (int p = 0; p < 12; ++p) {
            for (int b = lane; b < 256; b += 64) s.hist[b] = 0;
            __syncthreads();
            auto count_digit = [&](bool ok, double d2, int j) {
                if (!ok) return;
                const unsigned long long hb = (unsigned long long)__double_as_longlong(d2);
                if ((hb & mask_hi) != pre_hi || ((unsigned)j & mask_lo) != pre_lo) return;
                const unsigned dig = p < 8 ? (unsigned)(hb >> (56 - 8 * p)) & 255u : ((unsigned)j >> (24 - 8 * (p - 8))) & 255u;
                atomicAdd(&s.hist[dig], 1);
            };
            if (cached) for_each_cached(s, cnt, count_digit); else for_each_candidate(c, s, count_digit);
            __syncthreads();
            // the bin that holds rank kr: lane l owns bins 4l .. 4l+3
            const int h0 = s.hist[4 * lane], h1 = s.hist[4 * lane + 1], h2 = s.hist[4 * lane + 2], h3 = s.hist[4 * lane + 3];
            const int mine = h0 + h1 + h2 + h3;
            int incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_up(incl, off);
                if (lane >= off) incl += o;
            }
            const int before = incl - mine;
            if (before < kr && kr <= incl) {
                int b = 4 * lane, cum = before;
                const int hs[4] = {h0, h1, h2, h3};
                int t = 0;
                while (cum + hs[t] < kr) {
                    cum += hs[t];
                    ++t;
                }
                b += t;
                s.sel = b | ((kr - cum) << 8) | ((hs[t] == kr - cum ? 1 : 0) << 30);
            }
            __syncthreads();
            const int sel = s.sel;
            const unsigned dig = (unsigned)(sel & 255);
            kr = (sel >> 8) & 0x3FFFFF;
            if (p < 8) {
                pre_hi |= (unsigned long long)dig << (56 - 8 * p);
                mask_hi |= 255ull << (56 - 8 * p);
            } else {
                pre_lo |= dig << (24 - 8 * (p - 8));
                mask_lo |= 255u << (24 - 8 * (p - 8));
            }
            __syncthreads();
            if ((sel >> 30) & 1) break;   // every key of the bin is taken: the prefix decides
        }
        // collect the keys at or below the prefix (exactly max_nn) into s.d2 / s.idx -- in place when they came from there: a slot is
        // written only at or below the position it was read from, and a chunk is read whole before it is written
        int w = 0;
        auto collect = [&](bool ok, double d2, int j) {
            bool take = false;
            if (ok) {
                const unsigned long long hm = (unsigned long long)__double_as_longlong(d2) & mask_hi;
                const unsigned lm = (unsigned)j & mask_lo;
                take = hm < pre_hi || (hm == pre_hi && lm <= pre_lo);
            }
            const unsigned long long m = __ballot(take);
            const int pos = w + __popcll(m & lanes_below());
            __syncthreads();
            if (take && pos < FPFH_CAP) {
                s.d2[pos] = d2;
                s.idx[pos] = j;
            }
            __syncthreads();
            w += __popcll(m);
        };
        if (cached) for_each_cached(s, cnt, collect); else for_each_candidate(c, s, collect);
        k = max_nn;
    }
    __syncthreads();
    // rank sort of the k kept candidates by (d2, index): the ranks are a permutation (indices are distinct)
    int* oi = nbr_idx + q * (int64_t)max_nn;
    double* od = nbr_d2 + q * (int64_t)max_nn;
    for (int e = lane; e < k; e += 64) {
        const double ed = s.d2[e];
        const int ei = s.idx[e];
        int rank = 0;
        for (int f = 0; f < k; ++f) rank += grid3::closer(s.d2[f], s.idx[f], ed, ei) ? 1 : 0;
        oi[rank] = ei;
        od[rank] = ed;
    }
    for (int e = k + lane; e < max_nn; e += 64) {
        oi[e] = -1;
        od[e] = 0.0;
    }
    if (lane == 0) nbr_cnt[q] = k;
}

// ---- EstimateNormals (fast_normal_computation = true): ComputeCovariance + FastEigen3x3 (Open3D 0.18 EstimateNormals.cpp)
struct M3 {
    double a[3][3];
};
__device__ __forceinline__ void cross3(const double* a, const double* b, double* r) {
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ void eigenvector0(const M3& A, double eval0, double* out) {
    const double row0[3] = {A.a[0][0] - eval0, A.a[0][1], A.a[0][2]};
    const double row1[3] = {A.a[0][1], A.a[1][1] - eval0, A.a[1][2]};
    const double row2[3] = {A.a[0][2], A.a[1][2], A.a[2][2] - eval0};
    double r0xr1[3], r0xr2[3], r1xr2[3];
    cross3(row0, row1, r0xr1);
    cross3(row0, row2, r0xr2);
    cross3(row1, row2, r1xr2);
    const double d0 = dot3(r0xr1, r0xr1), d1 = dot3(r0xr2, r0xr2), d2 = dot3(r1xr2, r1xr2);
    double dmax = d0;
    int imax = 0;
    if (d1 > dmax) {
        dmax = d1;
        imax = 1;
    }
    if (d2 > dmax) imax = 2;
    const double* v = imax == 0 ? r0xr1 : (imax == 1 ? r0xr2 : r1xr2);
    const double s = sqrt(imax == 0 ? d0 : (imax == 1 ? d1 : d2));
    out[0] = v[0] / s;
    out[1] = v[1] / s;
    out[2] = v[2] / s;
}

__device__ void eigenvector1(const M3& A, const double* evec0, double eval1, double* out) {
    double U[3], V[3];
    if (fabs(evec0[0]) > fabs(evec0[1])) {
        const double inv_length = 1.0 / sqrt(evec0[0] * evec0[0] + evec0[2] * evec0[2]);
        U[0] = -evec0[2] * inv_length;
        U[1] = 0.0;
        U[2] = evec0[0] * inv_length;
    } else {
        const double inv_length = 1.0 / sqrt(evec0[1] * evec0[1] + evec0[2] * evec0[2]);
        U[0] = 0.0;
        U[1] = evec0[2] * inv_length;
        U[2] = -evec0[1] * inv_length;
    }
    cross3(evec0, U, V);
    const double AU[3] = {(A.a[0][0] * U[0] + A.a[0][1] * U[1]) + A.a[0][2] * U[2], (A.a[0][1] * U[0] + A.a[1][1] * U[1]) + A.a[1][2] * U[2],
                          (A.a[0][2] * U[0] + A.a[1][2] * U[1]) + A.a[2][2] * U[2]};
    const double AV[3] = {(A.a[0][0] * V[0] + A.a[0][1] * V[1]) + A.a[0][2] * V[2], (A.a[0][1] * V[0] + A.a[1][1] * V[1]) + A.a[1][2] * V[2],
                          (A.a[0][2] * V[0] + A.a[1][2] * V[1]) + A.a[2][2] * V[2]};
    double m00 = ((U[0] * AU[0] + U[1] * AU[1]) + U[2] * AU[2]) - eval1;
    double m01 = (U[0] * AV[0] + U[1] * AV[1]) + U[2] * AV[2];
    double m11 = ((V[0] * AV[0] + V[1] * AV[1]) + V[2] * AV[2]) - eval1;
    const double absM00 = fabs(m00), absM01 = fabs(m01), absM11 = fabs(m11);
    double a, b;   // result = a U - b V
    if (absM00 >= absM11) {
        const double mx = fmax(absM00, absM01);
        if (!(mx > 0.0)) {
            out[0] = U[0]; out[1] = U[1]; out[2] = U[2];
            return;
        }
        if (absM00 >= absM01) {
            m01 /= m00;
            m00 = 1.0 / sqrt(1.0 + m01 * m01);
            m01 *= m00;
        } else {
            m00 /= m01;
            m01 = 1.0 / sqrt(1.0 + m00 * m00);
            m00 *= m01;
        }
        a = m01;
        b = m00;
    } else {
        const double mx = fmax(absM11, absM01);
        if (!(mx > 0.0)) {
            out[0] = U[0]; out[1] = U[1]; out[2] = U[2];
            return;
        }
        if (absM11 >= absM01) {
            m01 /= m11;
            m11 = 1.0 / sqrt(1.0 + m01 * m01);
            m01 *= m11;
        } else {
            m11 /= m01;
            m01 = 1.0 / sqrt(1.0 + m11 * m11);
            m11 *= m01;
        }
        a = m11;
        b = m01;
    }
    out[0] = a * U[0] - b * V[0];
    out[1] = a * U[1] - b * V[1];
    out[2] = a * U[2] - b * V[2];
}

__device__ void fast_eigen3x3(const M3& C, double* out) {
    double mc = C.a[0][0];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) mc = fmax(mc, C.a[r][q]);
    if (mc == 0.0) {
        out[0] = out[1] = out[2] = 0.0;
        return;
    }
    M3 A;
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) A.a[r][q] = C.a[r][q] / mc;
    const double norm = (A.a[0][1] * A.a[0][1] + A.a[0][2] * A.a[0][2]) + A.a[1][2] * A.a[1][2];
    if (norm > 0.0) {
        const double q = ((A.a[0][0] + A.a[1][1]) + A.a[2][2]) / 3.0;
        const double b00 = A.a[0][0] - q, b11 = A.a[1][1] - q, b22 = A.a[2][2] - q;
        const double p = sqrt(((((b00 * b00 + b11 * b11) + b22 * b22) + norm * 2.0)) / 6.0);
        const double c00 = b11 * b22 - A.a[1][2] * A.a[1][2];
        const double c01 = A.a[0][1] * b22 - A.a[1][2] * A.a[0][2];
        const double c02 = A.a[0][1] * A.a[1][2] - b11 * A.a[0][2];
        const double det = ((b00 * c00 - A.a[0][1] * c01) + A.a[0][2] * c02) / ((p * p) * p);
        double half_det = det * 0.5;
        half_det = fmin(fmax(half_det, -1.0), 1.0);
        const double angle = acos(half_det) / 3.0;
        const double two_thirds_pi = 2.09439510239319549;
        const double beta2 = cos(angle) * 2.0;
        const double beta0 = cos(angle + two_thirds_pi) * 2.0;
        const double beta1 = -(beta0 + beta2);
        const double eval0 = q + p * beta0, eval1 = q + p * beta1, eval2 = q + p * beta2;
        double e0[3], e1[3];
        if (half_det >= 0.0) {
            eigenvector0(A, eval2, e0);   // evec2
            if (eval2 < eval0 && eval2 < eval1) {
                out[0] = e0[0]; out[1] = e0[1]; out[2] = e0[2];
                return;
            }
            eigenvector1(A, e0, eval1, e1);   // evec1
            if (eval1 < eval0 && eval1 < eval2) {
                out[0] = e1[0]; out[1] = e1[1]; out[2] = e1[2];
                return;
            }
            cross3(e1, e0, out);   // evec1 x evec2
        } else {
            eigenvector0(A, eval0, e0);   // evec0
            if (eval0 < eval1 && eval0 < eval2) {
                out[0] = e0[0]; out[1] = e0[1]; out[2] = e0[2];
                return;
            }
            eigenvector1(A, e0, eval1, e1);
            if (eval1 < eval0 && eval1 < eval2) {
                out[0] = e1[0]; out[1] = e1[1]; out[2] = e1[2];
                return;
            }
            cross3(e0, e1, out);   // evec0 x evec1
        }
        return;
    }
    // diagonal: the axis of the smallest entry (of A rescaled by max_coeff), ties x, y, else z
    const double d0 = A.a[0][0] * mc, d1 = A.a[1][1] * mc, d2 = A.a[2][2] * mc;
    out[0] = out[1] = out[2] = 0.0;
    if (d0 < d1 && d0 < d2) out[0] = 1.0;
    else if (d1 < d0 && d1 < d2) out[1] = 1.0;
    else out[2] = 1.0;
}

__global__ __launch_bounds__(256) void fpfh_normal_kernel(const double* __restrict__ pts, int64_t n, const int* __restrict__ nbr_idx,
                                                          const int* __restrict__ nbr_cnt, int max_nn, double* __restrict__ normals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int cnt = nbr_cnt[i];
    M3 C;
    if (cnt < 3) {
        for (int r = 0; r < 3; ++r)
            for (int q = 0; q < 3; ++q) C.a[r][q] = r == q ? 1.0 : 0.0;
    } else {
        double cu[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const int* li = nbr_idx + i * (int64_t)max_nn;
        for (int k = 0; k < cnt; ++k) {
            const int64_t j = li[k];
            const double x = pts[3 * j], y = pts[3 * j + 1], z = pts[3 * j + 2];
            cu[0] = cu[0] + x;
            cu[1] = cu[1] + y;
            cu[2] = cu[2] + z;
            cu[3] = cu[3] + x * x;
            cu[4] = cu[4] + x * y;
            cu[5] = cu[5] + x * z;
            cu[6] = cu[6] + y * y;
            cu[7] = cu[7] + y * z;
            cu[8] = cu[8] + z * z;
        }
        const double dn = (double)cnt;
        for (int t = 0; t < 9; ++t) cu[t] = cu[t] / dn;
        C.a[0][0] = cu[3] - cu[0] * cu[0];
        C.a[1][1] = cu[6] - cu[1] * cu[1];
        C.a[2][2] = cu[8] - cu[2] * cu[2];
        C.a[0][1] = C.a[1][0] = cu[4] - cu[0] * cu[1];
        C.a[0][2] = C.a[2][0] = cu[5] - cu[0] * cu[2];
        C.a[1][2] = C.a[2][1] = cu[7] - cu[1] * cu[2];
    }
    double nv[3];
    fast_eigen3x3(C, nv);
    if (sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]) == 0.0) {
        nv[0] = 0.0;
        nv[1] = 0.0;
        nv[2] = 1.0;
    }
    normals[3 * i] = nv[0];
    normals[3 * i + 1] = nv[1];
    normals[3 * i + 2] = nv[2];
}

// ---- VoxelDownSample: bounds -> voxel keys -> stable sort -> run starts -> one thread per voxel
constexpr int VDS_BITS = 21;
static_assert(3 * VDS_BITS <= grid3::KEY_BITS, "the down-sample's keys go through grid3::sort_pairs");
__global__ __launch_bounds__(1024) void fpfh_bounds_kernel(const double* __restrict__ pts, int64_t n, double* __restrict__ bounds) {
    __shared__ double red[6][1024];
    const int t = threadIdx.x;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = t; i < n; i += 1024)
        for (int c = 0; c < 3; ++c) {
            const double v = pts[3 * i + c];
            lo[c] = fmin(lo[c], v);
            hi[c] = fmax(hi[c], v);
        }
    for (int c = 0; c < 3; ++c) {
        red[c][t] = lo[c];
        red[3 + c][t] = hi[c];
    }
    __syncthreads();
    for (int s = 512; s >= 1; s >>= 1) {
        if (t < s)
            for (int c = 0; c < 3; ++c) {
                red[c][t] = fmin(red[c][t], red[c][t + s]);
                red[3 + c][t] = fmax(red[3 + c][t], red[3 + c][t + s]);
            }
        __syncthreads();
    }
    if (t < 6) bounds[t] = red[t][0];
}

__global__ __launch_bounds__(256) void fpfh_vds_keys_kernel(const double* __restrict__ pts, int64_t n, const double* __restrict__ bounds,
                                                            double voxel_size, long long* __restrict__ keys, int* __restrict__ idx,
                                                            int* __restrict__ overflow) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    long long key = 0;
    for (int c = 0; c < 3; ++c) {
        const double origin = bounds[c] - voxel_size * 0.5;          // GetMinBound() - voxel_size3 * 0.5
        const double v = floor((pts[3 * i + c] - origin) / voxel_size);
        if (!(v >= 0.0 && v < (double)(1 << VDS_BITS))) {
            atomicOr(overflow, 1);
            return;
        }
        key = (key << VDS_BITS) | (long long)v;
    }
    keys[i] = key;
    idx[i] = (int)i;
}

__global__ __launch_bounds__(256) void fpfh_vds_starts_kernel(const int* __restrict__ head, const int* __restrict__ vid, int64_t n,
                                                              const int* __restrict__ overflow, int* __restrict__ starts,
                                                              int* __restrict__ count_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (head[i]) starts[vid[i] - 1] = (int)i;
    if (i == n - 1) {
        starts[vid[i]] = (int)n;
        *count_out = *overflow ? -1 : vid[i];
    }
}

__global__ __launch_bounds__(256) void fpfh_vds_average_kernel(const double* __restrict__ pts, const double* __restrict__ normals, int64_t n,
                                                               const int* __restrict__ order, const int* __restrict__ starts,
                                                               const int* __restrict__ count, double* __restrict__ pts_out,
                                                               double* __restrict__ normals_out) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= *count) return;   // (a count of -1: nothing)
    const int j0 = starts[v], j1 = starts[v + 1];
    double p[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0};
    for (int t = j0; t < j1; ++t) {   // AccumulatedPoint::AddPoint, in input order (the sort is stable)
        const int64_t j = order[t];
        for (int c = 0; c < 3; ++c) {
            p[c] = p[c] + pts[3 * j + c];
            if (normals) m[c] = m[c] + normals[3 * j + c];
        }
    }
    const double dn = (double)(j1 - j0);
    for (int c = 0; c < 3; ++c) {
        pts_out[3 * v + c] = p[c] / dn;
        if (normals) normals_out[3 * v + c] = m[c] / dn;   // GetAverageNormal: not renormalised (Open3D 0.18)
    }
}

// ---- ComputePairFeatures / ComputeSPFHFeature / ComputeFPFHFeature (Open3D 0.18 Feature.cpp)
__device__ __forceinline__ void pair_features(const double* p1, const double* n1, const double* p2, const double* n2, double* f) {
    double d[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const double dn = sqrt(dot3(d, d));
    f[0] = f[1] = f[2] = 0.0;
    if (dn == 0.0) return;
    const double* a = n1;
    const double* b = n2;
    const double angle1 = dot3(n1, d) / dn, angle2 = dot3(n2, d) / dn;
    double f2;
    if (acos(fabs(angle1)) > acos(fabs(angle2))) {
        a = n2;
        b = n1;
        d[0] = d[0] * -1.0;
        d[1] = d[1] * -1.0;
        d[2] = d[2] * -1.0;
        f2 = -angle2;
    } else {
        f2 = angle1;
    }
    double v[3], w[3];
    cross3(d, a, v);
    const double vn = sqrt(dot3(v, v));
    if (vn == 0.0) return;
    v[0] = v[0] / vn;
    v[1] = v[1] / vn;
    v[2] = v[2] / vn;
    cross3(a, v, w);
    f[1] = dot3(v, b);
    f[0] = atan2(dot3(w, b), dot3(a, b));
    f[2] = f2;
}

__device__ __forceinline__ int clamp_bin(double x) {
    int h = (int)floor(x);
    return h < 0 ? 0 : (h >= 11 ? 10 : h);
}

__global__ __launch_bounds__(64) void fpfh_spfh_kernel(const double* __restrict__ pts, const double* __restrict__ normals,
                                                       const int* __restrict__ nbr_idx, const int* __restrict__ nbr_cnt, int max_nn,
                                                       double* __restrict__ spfh) {
    __shared__ int counts[33];
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x;
    const int cnt = nbr_cnt[i];
    if (lane < 33) counts[lane] = 0;
    __syncthreads();
    const double p1[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    const double n1[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
    const int* li = nbr_idx + i * (int64_t)max_nn;
    const double pi = 3.14159265358979323846;
    for (int k = 1 + lane; k < cnt; k += 64) {   // position 0 (the point itself) skipped
        const int64_t j = li[k];
        const double p2[3] = {pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]};
        const double n2[3] = {normals[3 * j], normals[3 * j + 1], normals[3 * j + 2]};
        double f[3];
        pair_features(p1, n1, p2, n2, f);
        atomicAdd(&counts[clamp_bin(11.0 * (f[0] + pi) / (2.0 * pi))], 1);
        atomicAdd(&counts[11 + clamp_bin(11.0 * (f[1] + 1.0) * 0.5)], 1);
        atomicAdd(&counts[22 + clamp_bin(11.0 * (f[2] + 1.0) * 0.5)], 1);
    }
    __syncthreads();
    if (lane < 33) {
        double v = 0.0;
        if (cnt > 1) {
            // the reference's loop adds hist_incr once per pair, in sequence: the same sum, whatever order the pairs came in
            const double hist_incr = 100.0 / (double)(cnt - 1);
            for (int t = 0; t < counts[lane]; ++t) v = v + hist_incr;
        }
        spfh[i * 33 + lane] = v;
    }
}

__global__ __launch_bounds__(64) void fpfh_fpfh_kernel(const double* __restrict__ spfh, const int* __restrict__ nbr_idx,
                                                       const double* __restrict__ nbr_d2, const int* __restrict__ nbr_cnt, int max_nn,
                                                       double* __restrict__ out) {
    __shared__ double sums[3];
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x;
    const int cnt = nbr_cnt[i];
    const int* li = nbr_idx + i * (int64_t)max_nn;
    const double* ld = nbr_d2 + i * (int64_t)max_nn;
    double acc = 0.0;
    if (cnt > 1) {
        if (lane < 33) {   // one lane per bin: sum over the neighbours in order
            for (int k = 1; k < cnt; ++k) {
                const double dist = ld[k];
                if (dist == 0.0) continue;
                acc = acc + spfh[(int64_t)li[k] * 33 + lane] / dist;
            }
        } else if (lane < 36) {   // one lane per group: sum[j / 11] += val in the reference's (k, j) order
            const int g = lane - 33;
            double s = 0.0;
            for (int k = 1; k < cnt; ++k) {
                const double dist = ld[k];
                if (dist == 0.0) continue;
                const double* row = spfh + (int64_t)li[k] * 33 + 11 * g;
                for (int j = 0; j < 11; ++j) s = s + row[j] / dist;
            }
            sums[g] = s != 0.0 ? 100.0 / s : s;
        }
    }
    __syncthreads();
    if (lane < 33) {
        double v = 0.0;
        if (cnt > 1) v = acc * sums[lane / 11] + spfh[i * 33 + lane];
        out[i * 33 + lane] = v;
    }
}

struct FpfhWs {
    grid3::SortWs<true> s;
    long long* keys;   // sorted (down-sample)
    int* order;        // sorted (down-sample)
    int* head;
    int* vid;
    int* starts;       // [n + 1]
    double* bounds;    // [6]
    int* overflow;
};

FpfhWs carve_fpfh(void* p, int64_t n, size_t* used = nullptr) {
    VfmCarver c(p);
    const size_t nn = (size_t)(n > 0 ? n : 1);
    FpfhWs w{};
    w.s = grid3::carve_sort<true>(c, n);
    w.keys = c.take<long long>(nn);
    w.order = c.take<int>(nn);
    w.head = c.take<int>(nn);
    w.vid = c.take<int>(nn);
    w.starts = c.take<int>(nn + 1);
    w.bounds = c.take<double>(6);
    w.overflow = c.take<int>(1);
    if (used) *used = c.used();
    return w;
}

using grid3::blocks256;

}  // namespace

VFM_EXPORT size_t vfm_fpfh_workspace_bytes(int64_t n) {
    size_t used = 0;
    (void)carve_fpfh(nullptr, n < 0 ? 0 : n, &used);   // (a null base: only the offsets are computed)
    return used;
}

VFM_EXPORT int vfm_fpfh_grid_build(const double* pts, int64_t n, double radius, int64_t* keys_out, int32_t* order_out, void* ws,
                                   size_t ws_bytes, vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 0 && n <= FPFH_MAX_POINTS && radius > 0.0, "fpfh_grid_build: bad arguments");
    if (n == 0) return VFM_OK;
    VFM_CHECK_ARG(pts && keys_out && order_out && ws, "fpfh_grid_build: null pointer");
    VFM_CHECK_ARG(ws_bytes >= vfm_fpfh_workspace_bytes(n), "fpfh_grid_build: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    FpfhWs w = carve_fpfh(ws, n);
    return grid3::build(pts, n, FpfhCells{1.0 / (radius * CELL_SLACK)}, nullptr, w.s, reinterpret_cast<long long*>(keys_out), order_out, st);
}

VFM_EXPORT int vfm_fpfh_search_hybrid(const double* pts, int64_t n, const int64_t* keys, const int32_t* order, double radius, int32_t max_nn,
                                      int32_t* nbr_idx, double* nbr_d2, int32_t* nbr_cnt, int32_t* scanned_out, vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 0 && n <= FPFH_MAX_POINTS && radius > 0.0 && max_nn >= 1 && max_nn <= FPFH_MAX_NN,
                  "fpfh_search_hybrid: bad arguments (max_nn must be in 1..%d)", FPFH_MAX_NN);
    if (n == 0) return VFM_OK;
    VFM_CHECK_ARG(pts && keys && order && nbr_idx && nbr_d2 && nbr_cnt, "fpfh_search_hybrid: null pointer");
    hipLaunchKernelGGL(fpfh_search_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, pts, n, reinterpret_cast<const long long*>(keys),
                       order, 1.0 / (radius * CELL_SLACK), radius * radius, (int)max_nn, nbr_idx, nbr_d2, nbr_cnt, scanned_out);
    VFM_CHECK_LAUNCH("fpfh_search_kernel");
    return VFM_OK;
}

VFM_EXPORT int vfm_fpfh_normals(const double* pts, int64_t n, const int32_t* nbr_idx, const int32_t* nbr_cnt, int32_t max_nn, double* normals_out,
                                vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 0 && max_nn >= 1, "fpfh_normals: bad arguments");
    if (n == 0) return VFM_OK;
    VFM_CHECK_ARG(pts && nbr_idx && nbr_cnt && normals_out, "fpfh_normals: null pointer");
    hipLaunchKernelGGL(fpfh_normal_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, pts, n, nbr_idx, nbr_cnt, (int)max_nn,
                       normals_out);
    VFM_CHECK_LAUNCH("fpfh_normal_kernel");
    return VFM_OK;
}

VFM_EXPORT int vfm_fpfh_voxel_down_sample(const double* pts, const double* normals, int64_t n, double voxel_size, double* pts_out,
                                          double* normals_out, int32_t* count_out, void* ws, size_t ws_bytes, vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 0 && n <= FPFH_MAX_POINTS && voxel_size > 0.0 && count_out, "fpfh_voxel_down_sample: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        VFM_CHECK_HIP(hipMemsetAsync(count_out, 0, sizeof(int32_t), st));
        return VFM_OK;
    }
    VFM_CHECK_ARG(pts && pts_out && ws && (!normals || normals_out), "fpfh_voxel_down_sample: null pointer");
    VFM_CHECK_ARG(ws_bytes >= vfm_fpfh_workspace_bytes(n), "fpfh_voxel_down_sample: workspace too small");
    FpfhWs w = carve_fpfh(ws, n);
    VFM_CHECK_HIP(hipMemsetAsync(w.overflow, 0, sizeof(int), st));
    hipLaunchKernelGGL(fpfh_bounds_kernel, dim3(1), dim3(1024), 0, st, pts, n, w.bounds);
    VFM_CHECK_LAUNCH("fpfh_bounds_kernel");
    hipLaunchKernelGGL(fpfh_vds_keys_kernel, dim3(blocks256(n)), dim3(256), 0, st, pts, n, w.bounds, voxel_size, w.s.keys_in, w.s.idx_in,
                       w.overflow);
    VFM_CHECK_LAUNCH("fpfh_vds_keys_kernel");
    VFM_TRY(grid3::sort_pairs(w.s, n, w.keys, w.order, st));
    VFM_TRY(grid3::run_ids(w.s, n, w.keys, w.head, w.vid, st));
    hipLaunchKernelGGL(fpfh_vds_starts_kernel, dim3(blocks256(n)), dim3(256), 0, st, w.head, w.vid, n, w.overflow, w.starts, count_out);
    VFM_CHECK_LAUNCH("fpfh_vds_starts_kernel");
    hipLaunchKernelGGL(fpfh_vds_average_kernel, dim3(blocks256(n)), dim3(256), 0, st, pts, normals, n, w.order, w.starts, count_out, pts_out,
                       normals_out);
    VFM_CHECK_LAUNCH("fpfh_vds_average_kernel");
    return VFM_OK;
}

VFM_EXPORT int vfm_fpfh_spfh(const double* pts, const double* normals, int64_t n, const int32_t* nbr_idx, const int32_t* nbr_cnt, int32_t max_nn,
                             double* spfh_out, vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 0 && n <= FPFH_MAX_POINTS && max_nn >= 1, "fpfh_spfh: bad arguments");
    if (n == 0) return VFM_OK;
    VFM_CHECK_ARG(pts && normals && nbr_idx && nbr_cnt && spfh_out, "fpfh_spfh: null pointer");
    hipLaunchKernelGGL(fpfh_spfh_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, pts, normals, nbr_idx, nbr_cnt, (int)max_nn,
                       spfh_out);
    VFM_CHECK_LAUNCH("fpfh_spfh_kernel");
    return VFM_OK;
}

VFM_EXPORT int vfm_fpfh_fpfh(const double* spfh, int64_t n, const int32_t* nbr_idx, const double* nbr_d2, const int32_t* nbr_cnt, int32_t max_nn,
                             double* fpfh_out, vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 0 && n <= FPFH_MAX_POINTS && max_nn >= 1, "fpfh_fpfh: bad arguments");
    if (n == 0) return VFM_OK;
    VFM_CHECK_ARG(spfh && nbr_idx && nbr_d2 && nbr_cnt && fpfh_out, "fpfh_fpfh: null pointer");
    hipLaunchKernelGGL(fpfh_fpfh_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, spfh, nbr_idx, nbr_d2, nbr_cnt, (int)max_nn,
                       fpfh_out);
    VFM_CHECK_LAUNCH("fpfh_fpfh_kernel");
    return VFM_OK;
}

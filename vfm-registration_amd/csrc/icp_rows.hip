// icp_rows.hip -- the descriptor-weighted nearest neighbour on a device-resident local map (gfx950): the search of
// RegisterFrame(std::vector<Eigen::VectorXd>, ...) (Registration.cpp:384-423), VoxelHashMap::GetCorrespondences(VectorXdVector)
// (VoxelHashMap.cpp:321-451), on descriptor rows of any width kept in THEIR OWN type -- fp32 or fp64, contiguous [n, f] -- next to the
// sorted-key grid (grid3.h) that VoxelHashMap.update keeps.
//
//   icp_rows_stats_kernel     |row| and "element sum != 0" of every row: the chains of icp.hip's icp_desc_stats_kernel on the fp64 image of
//                             the row (fp32 -> fp64 is exact)
//   icp_rows_nearest_kernel   among the points of the 27 voxels around a source point the FIRST minimum, in the reference's scan order, of
//                             |dxyz|^2 x clamp(0.5 (1 - cos), 0.01, 1); accepted on the Euclidean distance of the chosen neighbour
//
// What is computed is icp.hip's icp_nearest_kernel<true> (and oracle/vfm_oracle.c orc_icp_nearest_desc) operation for operation: sums in
// column order, no fused multiply-add, the same clamp, strict '<'.  What differs is who computes it.  The chain of ONE (source, candidate)
// pair is f dependent additions and cannot be split without changing the sum, so the parallelism comes from pairs: a wavefront takes a source
// point, numbers the candidates of its 27 voxels in scan order (lane l < 27 finds voxel l by binary search, an exclusive sum of the voxels'
// sizes gives every candidate its scan position q) and gives candidate q = 64 r + lane to a lane in round r -- up to 27 x the per-voxel
// cap candidates, so several rounds where the neighbourhood is full.  A lane keeps its first minimum (its positions ascend), the lanes merge
// by (cost, scan position) as icp_nearest_kernel does.  The source descriptor is staged once per point in LDS as fp64 (every lane reads the
// same address: a broadcast); a lane reads ITS map row front to back, in 16-byte units where the rows are 16-byte aligned and element by
// element otherwise, eight elements' loads and products ahead of the additions that consume them.  A candidate whose cost is not below
// the best so far never wins: a NaN cost (a non-finite descriptor) compares false, as in the reference.  No candidate is pruned.
//
// One wavefront per workgroup: the barriers between staging and reading are then wave-wide, and every exit is workgroup-uniform.
#include "grid3.h"

namespace {

constexpr int ROWS_WAVE = 64;
constexpr int ROWS_NEIGHBOURS = 27;
constexpr int ROWS_CHUNK = 1024;             // columns of the source descriptor staged at a time (8 KiB of LDS)
constexpr unsigned ROWS_NONE = 0xFFFFFFFFu;  // the scan position of a lane that holds no candidate

template <typename T>
struct RowUnit;   // 16 bytes of a row
template <>
struct RowUnit<double> {
    using type = double2;
    static constexpr int N = 2;
};
template <>
struct RowUnit<float> {
    using type = float4;
    static constexpr int N = 4;
};
__device__ __forceinline__ void unit_values(const double2& u, double* v) { v[0] = u.x; v[1] = u.y; }
__device__ __forceinline__ void unit_values(const float4& u, double* v) {
    v[0] = (double)u.x; v[1] = (double)u.y; v[2] = (double)u.z; v[3] = (double)u.w;
}

// 16-byte units only when every row starts on a 16-byte boundary
template <typename T>
inline bool rows_vectorised(const void* a, const void* b, int f) {
    return (((size_t)f * sizeof(T)) % 16 == 0) && ((uintptr_t)a % 16 == 0) && ((uintptr_t)b % 16 == 0);
}

// ---- statistics: one lane per row, the row read front to back; ss and sm are icp_desc_stats_kernel's chains
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void icp_rows_stats_kernel(const T* __restrict__ desc, int64_t n, int f, double* __restrict__ norm_out,
                                                             uint8_t* __restrict__ has_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const T* r = desc + i * f;
    double ss = 0.0, sm = 0.0;
    int k = 0;
    if constexpr (VEC) {
        using U = typename RowUnit<T>::type;
        constexpr int N = RowUnit<T>::N, AHEAD = 8 / N;
        const U* ru = reinterpret_cast<const U*>(r);
        for (; k + 8 <= f; k += 8) {
            U u[AHEAD];
#pragma unroll
            for (int a = 0; a < AHEAD; ++a) u[a] = ru[k / N + a];
            double v[8];
#pragma unroll
            for (int a = 0; a < AHEAD; ++a) unit_values(u[a], v + a * N);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                ss = ss + v[e] * v[e];
                sm = sm + v[e];
            }
        }
    }
    for (; k < f; ++k) {
        const double v = (double)r[k];
        ss = ss + v * v;
        sm = sm + v;
    }
    norm_out[i] = sqrt(ss);
    has_out[i] = sm != 0.0 ? 1 : 0;
}

// ---- dot = dot + row[k] * sd[k - k0] for k in [k0, k1), in column order (sd: the staged source columns, fp64, in LDS)
template <typename T, bool VEC>
__device__ __forceinline__ double rows_dot(const T* __restrict__ row, const double* sd, int k0, int k1, double dot) {
    int k = k0;
    if constexpr (VEC) {
        using U = typename RowUnit<T>::type;
        constexpr int N = RowUnit<T>::N, AHEAD = 8 / N;
        const U* ru = reinterpret_cast<const U*>(row);    // (k0 is a multiple of ROWS_CHUNK, so of 8)
        for (; k + 8 <= k1; k += 8) {
            U u[AHEAD];
#pragma unroll
            for (int a = 0; a < AHEAD; ++a) u[a] = ru[k / N + a];
            double v[8], p[8];
#pragma unroll
            for (int a = 0; a < AHEAD; ++a) unit_values(u[a], v + a * N);
#pragma unroll
            for (int e = 0; e < 8; ++e) p[e] = v[e] * sd[k - k0 + e];
#pragma unroll
            for (int e = 0; e < 8; ++e) dot = dot + p[e];
        }
    }
    for (; k < k1; ++k) dot = dot + (double)row[k] * sd[k - k0];
    return dot;
}

struct RowsArgs {
    double T[12];
    int apply;
    int f;
    const double* src_norm;
    const uint8_t* src_has;
    const double* map_norm;
    const uint8_t* map_has;
};

// (src and src_out may be the same array: neither is __restrict__; the wavefront reads its point before lane 0 writes it, and no other
// wavefront touches that point)
template <typename T, bool VEC>
__global__ __launch_bounds__(ROWS_WAVE) void icp_rows_nearest_kernel(const double* src, int64_t n, const T* __restrict__ src_desc,
                                                                     const long long* __restrict__ keys, const int* __restrict__ start,
                                                                     const double* __restrict__ pts, const T* __restrict__ map_desc, int nv,
                                                                     double voxel_size, double max_dist, double* __restrict__ tgt,
                                                                     uint8_t* __restrict__ valid, RowsArgs a, double* src_out) {
    __shared__ double sd[ROWS_CHUNK];
    __shared__ int vox_first[ROWS_NEIGHBOURS];      // first map row of neighbour voxel l
    __shared__ int vox_pos[ROWS_NEIGHBOURS + 1];    // scan position of its first candidate; [27]: the number of candidates
    const int l = threadIdx.x;
    const int64_t i = blockIdx.x;                   // (the grid is n workgroups: i < n)
    const int f = a.f;
    double px = src[3 * i], py = src[3 * i + 1], pz = src[3 * i + 2];
    if (a.apply) {
        const double* T4 = a.T;
        const double qx = ((T4[0] * px + T4[1] * py) + T4[2] * pz) + T4[3] * 1.0;
        const double qy = ((T4[4] * px + T4[5] * py) + T4[6] * pz) + T4[7] * 1.0;
        const double qz = ((T4[8] * px + T4[9] * py) + T4[10] * pz) + T4[11] * 1.0;
        px = qx; py = qy; pz = qz;
    }
    if (a.apply && l == 0) {    // (src may be src_out: what is stored depends on what every lane has loaded by now)
        src_out[3 * i] = px;
        src_out[3 * i + 1] = py;
        src_out[3 * i + 2] = pz;
    }
    const int kx = (int)(px / voxel_size), ky = (int)(py / voxel_size), kz = (int)(pz / voxel_size);
    // the 27 voxels in the reference's loop order, l = 9 (a - kx + 1) + 3 (b - ky + 1) + (c - kz + 1), and their candidates' numbering
    int j0 = 0, cnt = 0;
    if (l < ROWS_NEIGHBOURS) {
        const long long key = grid3::key(kx - 1 + l / 9, ky - 1 + (l / 3) % 3, kz - 1 + l % 3);
        const int lo = grid3::lower_bound(keys, nv, key);
        if (lo < nv && keys[lo] == key) {
            j0 = start[lo];
            cnt = start[lo + 1] - j0;
            if (cnt < 0) cnt = 0;
        }
    }
    int incl = cnt;    // inclusive sum over the lanes (lanes >= 27 add nothing)
#pragma unroll
    for (int off = 1; off < ROWS_WAVE; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (l >= off) incl += o;
    }
    if (l < ROWS_NEIGHBOURS) {
        vox_first[l] = j0;
        vox_pos[l] = incl - cnt;
    }
    if (l == ROWS_NEIGHBOURS) vox_pos[ROWS_NEIGHBOURS] = incl;
    __syncthreads();
    const int total = vox_pos[ROWS_NEIGHBOURS];
    const bool phas = a.src_has[i] != 0;
    const double pn = a.src_norm[i];
    const T* pd = src_desc + i * f;
    const int chunks = (f + ROWS_CHUNK - 1) / ROWS_CHUNK;

    double bx = 0.0, by = 0.0, bz = 0.0, best = 1.7976931348623157e308;
    unsigned order = ROWS_NONE;
    for (int q0 = 0; q0 < total; q0 += ROWS_WAVE) {      // (total is the same in every lane: the barriers below are uniform)
        const int q = q0 + l;
        const bool have = q < total;
        int j = 0;
        double cx = 0.0, cy = 0.0, cz = 0.0, d = 0.0;
        bool weigh = false;
        if (have) {
            int v = 0;
            while (v < ROWS_NEIGHBOURS - 1 && q >= vox_pos[v + 1]) ++v;
            j = vox_first[v] + (q - vox_pos[v]);
            cx = pts[3 * (int64_t)j];
            cy = pts[3 * (int64_t)j + 1];
            cz = pts[3 * (int64_t)j + 2];
            const double dx = cx - px, dy = cy - py, dz = cz - pz;
            d = (dx * dx + dy * dy) + dz * dz;
            weigh = phas && a.map_has[j] != 0;
        }
        double dot = 0.0;
        const T* nd = map_desc + (int64_t)j * f;
        for (int c = 0; c < chunks; ++c) {
            const int k0 = c * ROWS_CHUNK, k1 = min(f, k0 + ROWS_CHUNK);
            if (chunks > 1 || q0 == 0) {     // a descriptor of one chunk is staged once per point
                __syncthreads();             // (the chunk before has been read)
                for (int k = k0 + l; k < k1; k += ROWS_WAVE) sd[k - k0] = (double)pd[k];
                __syncthreads();
            }
            if (weigh) dot = rows_dot<T, VEC>(nd, sd, k0, k1, dot);
        }
        if (have) {
            double c = 1.0;
            if (weigh) {
                const double cs = dot / (a.map_norm[j] * pn + 1e-5);
                c = 0.5 * (1.0 - cs);
                c = c < 0.01 ? 0.01 : (1.0 < c ? 1.0 : c);   // std::clamp(c, 0.01, 1.0)
            }
            d = d * c;
            if (d < best) {      // strict: of equal costs the lane keeps the earlier position
                best = d;
                bx = cx; by = cy; bz = cz;
                order = (unsigned)q;
            }
        }
    }
#pragma unroll
    for (int off = ROWS_WAVE / 2; off >= 1; off >>= 1) {
        const double ob = __shfl_xor(best, off), ox = __shfl_xor(bx, off), oy = __shfl_xor(by, off), oz = __shfl_xor(bz, off);
        const unsigned oo = __shfl_xor(order, off);
        // the smaller cost, and of equal costs the earlier scan position; a lane without a candidate never wins against one that has one
        const bool take = oo != ROWS_NONE && (order == ROWS_NONE || ob < best || (ob == best && oo < order));
        if (take) {
            best = ob; bx = ox; by = oy; bz = oz; order = oo;
        }
    }
    if (l != 0) return;
    // (closest_neighbor.head<3>() - point.head<3>()).norm() < max_correspondence_distance (VoxelHashMap.cpp:425-432): the neighbour's
    // Euclidean distance, not its cost
    const double ex = bx - px, ey = by - py, ez = bz - pz;
    const double e2 = (ex * ex + ey * ey) + ez * ez;
    tgt[3 * i] = bx;
    tgt[3 * i + 1] = by;
    tgt[3 * i + 2] = bz;
    valid[i] = (order != ROWS_NONE && sqrt(e2) < max_dist) ? 1 : 0;
}

template <typename T>
int rows_stats(const void* desc, int64_t n, int f, double* norm_out, uint8_t* has_out, hipStream_t st) {
    const dim3 grid((unsigned)((n + 255) / 256));
    if (rows_vectorised<T>(desc, desc, f))
        hipLaunchKernelGGL((icp_rows_stats_kernel<T, true>), grid, dim3(256), 0, st, (const T*)desc, n, f, norm_out, has_out);
    else
        hipLaunchKernelGGL((icp_rows_stats_kernel<T, false>), grid, dim3(256), 0, st, (const T*)desc, n, f, norm_out, has_out);
    VFM_CHECK_LAUNCH("icp_rows_stats_kernel");
    return VFM_OK;
}

template <typename T>
int rows_nearest(const double* src, int64_t n, const void* src_desc, const int64_t* keys, const int32_t* start, const double* pts,
                 const void* map_desc, int32_t nv, double voxel_size, double max_dist, double* tgt, uint8_t* valid, const RowsArgs& a,
                 double* src_out, hipStream_t st) {
    const dim3 grid((unsigned)n);
    const long long* k = reinterpret_cast<const long long*>(keys);
    if (rows_vectorised<T>(src_desc, map_desc, a.f))
        hipLaunchKernelGGL((icp_rows_nearest_kernel<T, true>), grid, dim3(ROWS_WAVE), 0, st, src, n, (const T*)src_desc, k, start, pts,
                           (const T*)map_desc, nv, voxel_size, max_dist, tgt, valid, a, src_out);
    else
        hipLaunchKernelGGL((icp_rows_nearest_kernel<T, false>), grid, dim3(ROWS_WAVE), 0, st, src, n, (const T*)src_desc, k, start, pts,
                           (const T*)map_desc, nv, voxel_size, max_dist, tgt, valid, a, src_out);
    VFM_CHECK_LAUNCH("icp_rows_nearest_kernel");
    return VFM_OK;
}

}  // namespace

VFM_EXPORT int vfm_icp_rows_stats(const void* desc, int32_t elem_bytes, int64_t n, int32_t f, double* norm_out, uint8_t* has_out,
                                  vfm_stream_t stream) {
    VFM_CHECK_ARG(elem_bytes == 4 || elem_bytes == 8, "icp_rows_stats: elem_bytes must be 4 (fp32 rows) or 8 (fp64 rows)");
    VFM_CHECK_ARG(n >= 0 && n <= ((int64_t)1 << 30) && f >= 1, "icp_rows_stats: bad sizes (0 <= n <= 2^30, f >= 1)");
    if (n == 0) return VFM_OK;
    VFM_CHECK_ARG(desc && norm_out && has_out, "icp_rows_stats: null pointer");
    return elem_bytes == 4 ? rows_stats<float>(desc, n, (int)f, norm_out, has_out, (hipStream_t)stream)
                           : rows_stats<double>(desc, n, (int)f, norm_out, has_out, (hipStream_t)stream);
}

VFM_EXPORT int vfm_icp_step_nearest_rows(const double* src, int64_t n, const double* T_host, double* src_out, const void* src_desc,
                                         const double* src_norm, const uint8_t* src_has, int32_t elem_bytes, int32_t f, const int64_t* keys,
                                         const int32_t* start, const double* pts, const void* map_desc, const double* map_norm,
                                         const uint8_t* map_has, int32_t n_voxels, double voxel_size, double max_dist, double* tgt_out,
                                         uint8_t* valid_out, vfm_stream_t stream) {
    VFM_CHECK_ARG(elem_bytes == 4 || elem_bytes == 8, "icp_step_nearest_rows: elem_bytes must be 4 (fp32 rows) or 8 (fp64 rows)");
    VFM_CHECK_ARG(n >= 0 && n <= ((int64_t)1 << 30) && f >= 1 && n_voxels >= 0 && voxel_size > 0.0,
                  "icp_step_nearest_rows: bad sizes (0 <= n <= 2^30, f >= 1, n_voxels >= 0, voxel_size > 0)");
    if (n == 0) return VFM_OK;
    VFM_CHECK_ARG(src && tgt_out && valid_out && src_desc && src_norm && src_has && start && (!T_host || src_out),
                  "icp_step_nearest_rows: null pointer");
    VFM_CHECK_ARG(n_voxels == 0 || (keys && pts && map_desc && map_norm && map_has), "icp_step_nearest_rows: null pointer (map)");
    RowsArgs a;
    a.apply = T_host ? 1 : 0;
    for (int k = 0; k < 12; ++k) a.T[k] = T_host ? T_host[k] : 0.0;
    a.f = (int)f;
    a.src_norm = src_norm;
    a.src_has = src_has;
    a.map_norm = map_norm;
    a.map_has = map_has;
    return elem_bytes == 4 ? rows_nearest<float>(src, n, src_desc, keys, start, pts, map_desc, n_voxels, voxel_size, max_dist, tgt_out,
                                                 valid_out, a, src_out, (hipStream_t)stream)
                           : rows_nearest<double>(src, n, src_desc, keys, start, pts, map_desc, n_voxels, voxel_size, max_dist, tgt_out,
                                                  valid_out, a, src_out, (hipStream_t)stream);
}

// odometry.hip -- the per-scan device work of the KISS-ICP odometry front end on MI355X (gfx950), rows 9 / 11 / 13 of SURVEY §2.
//
//   vfm_range_crop        Preprocess (src/kiss-icp/cpp/kiss_icp/core/Preprocessing.cpp:139-197): the rows with
//                         min_range < |xyz| < max_range, as ascending indices -- an ordered compaction by one workgroup
//                         (ordered_compact.h, shared with vfm_colour_gate), one launch, no read-back
//   vfm_deskew_scan       DeSkewScan (Deskew.cpp:40-68): out_i = exp((t_i - 0.5) delta) p_i, a thread per point, Sophus' SE3::exp with
//                         its first-order branch below theta = 1e-10 (the formulas of vfmreg/icp.py se3_exp)
//   vfm_icp_grid_update   VoxelHashMap::Update for the 3-D map (VoxelHashMap.cpp:693-699, 733-744, 772-779) on the sorted-key CSR that
//                         vfm_icp_nearest reads: the new points' keys are sorted (m of them, not the map), their runs are merged into the
//                         old key list by two rank searches, far voxels are dropped, and one scatter writes the new grid.
//   vfm_icp_grid_update_src  the same update (the same kernels: the scatter takes a nullable pointer) that also says where every output
//                         point came from -- the provenance a map needs to move a payload (descriptor rows) along with its points
//   vfm_rows_merge        that move: rows_out[q] = row src[q] of (rows_old | rows_new), rows of any width that is a multiple of 4 bytes,
//                         a wave per row (several short rows per wave), 16-byte accesses where width and pointers allow; a pure copy
//
// HBM-bound fp64, -ffp-contract=off, every expression spelled in the order the oracle (tests/odometry_oracle.py) replays.  No
// floating-point atomic; the integer atomics (the status flag, the count of accepted points) do not depend on an order.
#include <math.h>

#include "grid3.h"
#include "icp_voxels.h"
#include "ordered_compact.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------ range crop
// one workgroup of 1024 threads; a pass takes 1024 rows.  norm = sqrt((x x + y y) + z z): every operation correctly rounded
__global__ __launch_bounds__(ORDERED_COMPACT_THREADS) void range_crop_kernel(const double* __restrict__ pts, int64_t n, int64_t stride,
                                                                             double min_range, double max_range,
                                                                             int64_t* __restrict__ idx, int64_t* __restrict__ count) {
    __shared__ OrderedCompactLds lds;
    int64_t base = 0;
    int buf = 0;
    for (int64_t s0 = 0; s0 < n; s0 += ORDERED_COMPACT_THREADS, buf ^= 1) {
        const int64_t i = s0 + threadIdx.x;
        bool hit = false;
        if (i < n) {
            const double x = pts[i * stride], y = pts[i * stride + 1], z = pts[i * stride + 2];
            const double norm = sqrt((x * x + y * y) + z * z);
            hit = norm < max_range && norm > min_range;   // Preprocessing.cpp:148 (false for NaN)
        }
        int total;
        const int place = ordered_compact_pass(lds, buf, hit, total);
        if (hit) idx[base + place] = i;
        base += total;
    }
    if (threadIdx.x == 0) *count = base;
}

// ------------------------------------------------------------------------------------------------------------------ de-skew
struct Twist {
    double d[6];   // [upsilon (translation), omega (rotation)], Sophus' tangent order
};

__global__ __launch_bounds__(256) void deskew_kernel(const double* __restrict__ pts, int64_t n, int64_t stride,
                                                     const double* __restrict__ stamps, Twist delta, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double s = stamps[i] - 0.5;   // mid_pose_timestamp, Deskew.cpp:36
    const double u[3] = {s * delta.d[0], s * delta.d[1], s * delta.d[2]};
    const double w[3] = {s * delta.d[3], s * delta.d[4], s * delta.d[5]};
    const double th = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    const double Om[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
    double R[3][3], V[3][3];
    if (th < 1e-10) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double e = r == c ? 1.0 : 0.0;
                R[r][c] = e + Om[r][c];
                V[r][c] = e + 0.5 * Om[r][c];
            }
    } else {
        const double sn = sin(th), cs = cos(th);
        const double a = sn / th, b = (1.0 - cs) / (th * th), c3 = (th - sn) / ((th * th) * th);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double o2 = (Om[r][0] * Om[0][c] + Om[r][1] * Om[1][c]) + Om[r][2] * Om[2][c];
                const double e = r == c ? 1.0 : 0.0;
                R[r][c] = (e + a * Om[r][c]) + b * o2;
                V[r][c] = (e + b * Om[r][c]) + c3 * o2;
            }
    }
    const double x = pts[i * stride], y = pts[i * stride + 1], z = pts[i * stride + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double tau = (V[r][0] * u[0] + V[r][1] * u[1]) + V[r][2] * u[2];
        out[3 * i + r] = ((R[r][0] * x + R[r][1] * y) + R[r][2] * z) + tau;
    }
}

// ------------------------------------------------------------------------------------------------------------------ grid update
// Names: the OLD grid has nv voxels (keys, start, pts); the m new points, moved by the pose, sorted by key, form R RUNS of equal keys; a run
// whose key the old grid does not hold is NEW-ONLY; the MERGED list is the old voxels and the new-only runs in key order (nv + NN entries).
struct Pose {
    double T[12];
};

// the arithmetic of vfm_transform_xyz_f64 (project.hip), T by value
__global__ __launch_bounds__(256) void upd_move_kernel(const double* __restrict__ xyz, int64_t m, Pose P, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const double* T = P.T;
#pragma unroll
    for (int r = 0; r < 3; ++r) out[3 * i + r] = ((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3] * 1.0;
}

enum { UPD_RUNS = 0, UPD_NEW_ONLY = 1, UPD_ADDED = 2, UPD_STATUS = 3, UPD_COUNTERS = 4 };

// rid: inclusive sum of the heads (the 1-based run of every sorted position).  run_pos[r]: where run r starts, run_pos[R] = m.
__global__ __launch_bounds__(256) void upd_runs_kernel(const long long* __restrict__ ks, const int* __restrict__ rid, int64_t m,
                                                       long long* __restrict__ run_key, int* __restrict__ run_pos, int* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int r = rid[i] - 1;
    if (grid3::run_head(ks, i)) {
        run_key[r] = ks[i];
        run_pos[r] = (int)i;
    }
    if (i == m - 1) {
        run_pos[r + 1] = (int)m;
        cnt[UPD_RUNS] = r + 1;
    }
}

// per run: the old voxel of its key (run_old: its index, or -(lo + 1) for a new-only run, lo = the old keys below it), how many of the
// run's points the voxel still takes (old points count first: VoxelBlock::AddPoint, VoxelHashMap.hpp:55-62), the new-only flag.
// Threads past the last run clear their flag: the sum over m entries that follows needs them.
__global__ __launch_bounds__(256) void upd_takers_kernel(const long long* __restrict__ run_key, const int* __restrict__ run_pos, int64_t m,
                                                         const long long* __restrict__ keys, const int* __restrict__ start, int nv, int cap,
                                                         int* __restrict__ run_old, int* __restrict__ run_old_count,
                                                         int* __restrict__ run_take, int* __restrict__ new_only, int* __restrict__ cnt) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    if (r >= cnt[UPD_RUNS]) {
        new_only[r] = 0;
        return;
    }
    const long long key = run_key[r];
    const int lo = grid3::lower_bound(keys, nv, key);
    const bool found = lo < nv && keys[lo] == key;
    const int old_count = found ? start[lo + 1] - start[lo] : 0;
    const int len = run_pos[r + 1] - run_pos[r];
    int take = len;
    if (cap > 0) {
        const int room = cap > old_count ? cap - old_count : 0;
        take = len < room ? len : room;
    }
    run_old[r] = found ? lo : -(lo + 1);
    run_old_count[r] = old_count;
    run_take[r] = take;
    new_only[r] = found ? 0 : 1;
    if (take) atomicAdd(&cnt[UPD_ADDED], take);
}

// the merge: entry v of the merged list gets its old voxel (or -1) and its run (or -1).  An old voxel j comes after the new-only runs
// with a smaller key -- nrank (the inclusive sum of new_only) just before the first run whose key is not below --, a new-only run after
// its new-only predecessors and the old keys below it.  Thread t serves old voxel t and run t.
__global__ __launch_bounds__(256) void upd_merge_kernel(const long long* __restrict__ keys, int nv, const long long* __restrict__ run_key,
                                                        const int* __restrict__ run_old, const int* __restrict__ nrank, int64_t m,
                                                        int* __restrict__ mv_old, int* __restrict__ mv_run, int* __restrict__ old_mv,
                                                        int* __restrict__ run_mv, int* __restrict__ cnt) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int R = cnt[UPD_RUNS];
    if (t < nv) {
        const long long key = keys[t];
        const int p = grid3::lower_bound(run_key, R, key);
        const int v = (int)t + (p > 0 ? nrank[p - 1] : 0);
        mv_old[v] = (int)t;
        mv_run[v] = (p < R && run_key[p] == key) ? p : -1;
        old_mv[t] = v;
    }
    if (t < R) {
        const int o = run_old[t];
        if (o < 0) {
            const int v = (nrank[t] - 1) + (-o - 1);
            mv_old[v] = -1;
            mv_run[v] = (int)t;
            run_mv[t] = v;
        }
    }
    if (t == 0) cnt[UPD_NEW_ONLY] = R > 0 ? nrank[R - 1] : 0;
}

// a found run's merged entry is its old voxel's (a second pass: old_mv is complete)
__global__ __launch_bounds__(256) void upd_run_mv_kernel(const int* __restrict__ run_old, const int* __restrict__ old_mv, int* __restrict__ run_mv,
                                                         int64_t m, const int* __restrict__ cnt) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= m || r >= cnt[UPD_RUNS]) return;
    const int o = run_old[r];
    if (o >= 0) run_mv[r] = old_mv[o];
}

struct Origin {
    double o[3];
    double max_d2;
    int remove;
};

// size[v] of every merged voxel after the cap, 0 where its FIRST point is far (RemovePointsFarFromLocation, VoxelHashMap.cpp:772-779:
// (pt - origin).squaredNorm() > max_distance^2); alive[v].  Entries past the merged list are cleared for the sums over nv + m entries.
__global__ __launch_bounds__(256) void upd_sizes_kernel(const int* __restrict__ mv_old, const int* __restrict__ mv_run, int nv, int64_t total,
                                                        const int* __restrict__ start, const double* __restrict__ pts,
                                                        const int* __restrict__ run_pos, const int* __restrict__ run_take,
                                                        const int* __restrict__ order, const double* __restrict__ moved, Origin org,
                                                        int* __restrict__ size, int* __restrict__ alive, const int* __restrict__ cnt) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= total) return;
    if (v >= (int64_t)nv + cnt[UPD_NEW_ONLY]) {
        size[v] = 0;
        alive[v] = 0;
        return;
    }
    const int j = mv_old[v], r = mv_run[v];
    const double* first = j >= 0 ? pts + 3 * (int64_t)start[j] : moved + 3 * (int64_t)order[run_pos[r]];
    int sz = (j >= 0 ? start[j + 1] - start[j] : 0) + (r >= 0 ? run_take[r] : 0);
    bool keep = true;
    if (org.remove) {
        const double dx = first[0] - org.o[0], dy = first[1] - org.o[1], dz = first[2] - org.o[2];
        keep = !(((dx * dx + dy * dy) + dz * dz) > org.max_d2);
    }
    size[v] = keep ? sz : 0;
    alive[v] = keep ? 1 : 0;
}

// the voxel that holds old point t: the last j with start[j] <= t (voxels are never empty, so start[j] <= t < start[j + 1]); nv if t is
// not below start[nv]
__device__ __forceinline__ int upd_voxel_of(const int* __restrict__ start, int nv, int t) {
    int lo = 0, hi = nv + 1;   // first position of start[0, nv] that holds more than t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= t) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// The one scatter.  vpos / ppos: inclusive sums of alive / size over nv + m entries.  Thread t serves merged voxel t (its key and start),
// old point t and sorted new point t.  src_out (nullable): where output point q came from -- old point t, or nk + s for new input point s.
__global__ __launch_bounds__(256) void upd_scatter_kernel(const long long* __restrict__ keys, const int* __restrict__ start,
                                                          const double* __restrict__ pts, int nv, int64_t nk, int64_t m, int64_t total,
                                                          const int* __restrict__ mv_old, const int* __restrict__ mv_run,
                                                          const int* __restrict__ old_mv, const int* __restrict__ run_mv,
                                                          const long long* __restrict__ run_key, const int* __restrict__ run_pos,
                                                          const int* __restrict__ run_old_count, const int* __restrict__ run_take,
                                                          const int* __restrict__ rid, const int* __restrict__ order,
                                                          const double* __restrict__ moved, const int* __restrict__ size,
                                                          const int* __restrict__ alive, const int* __restrict__ vpos,
                                                          const int* __restrict__ ppos, const int* __restrict__ cnt,
                                                          long long* __restrict__ keys_out, int* __restrict__ start_out,
                                                          double* __restrict__ pts_out, int* __restrict__ info_out,
                                                          int* __restrict__ src_out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < total && alive[t]) {
        const int j = mv_old[t];
        keys_out[vpos[t] - 1] = j >= 0 ? keys[j] : run_key[mv_run[t]];
        start_out[vpos[t] - 1] = ppos[t] - size[t];
    }
    if (t < nk) {
        const int j = upd_voxel_of(start, nv, (int)t);
        const int v = (j >= 0 && j < nv) ? old_mv[j] : -1;   // (else: nk and start disagree -- a caller's error; nothing is written for it)
        if (v >= 0 && alive[v]) {
            const int64_t q = (int64_t)(ppos[v] - size[v]) + (t - start[j]);
            pts_out[3 * q] = pts[3 * t];
            pts_out[3 * q + 1] = pts[3 * t + 1];
            pts_out[3 * q + 2] = pts[3 * t + 2];
            if (src_out) src_out[q] = (int)t;
        }
    }
    if (t < m) {
        const int r = rid[t] - 1;
        const int rank = (int)t - run_pos[r];
        const int v = run_mv[r];
        if (rank < run_take[r] && alive[v]) {
            const int64_t q = (int64_t)(ppos[v] - size[v]) + run_old_count[r] + rank;
            const int64_t s = order[t];
            pts_out[3 * q] = moved[3 * s];
            pts_out[3 * q + 1] = moved[3 * s + 1];
            pts_out[3 * q + 2] = moved[3 * s + 2];
            if (src_out) src_out[q] = (int)(nk + s);   // (s: the index into xyz_new, not the sorted position)
        }
    }
    if (t == 0) {
        const int n_voxels = vpos[total - 1], n_kept = ppos[total - 1];
        const int merged = nv + cnt[UPD_NEW_ONLY];
        start_out[n_voxels] = n_kept;
        info_out[0] = n_voxels;
        info_out[1] = n_kept;
        info_out[2] = cnt[UPD_STATUS];
        info_out[3] = cnt[UPD_ADDED];
        info_out[4] = merged - n_voxels;
        info_out[5] = (int)nk + cnt[UPD_ADDED] - n_kept;
    }
}

__global__ void upd_empty_kernel(int* __restrict__ start_out, int* __restrict__ info_out) {
    if (threadIdx.x == 0) {
        start_out[0] = 0;
        for (int k = 0; k < 6; ++k) info_out[k] = 0;
    }
}

struct UpdateWs {
    grid3::SortWs<true> s;   // the new points' unsorted (key, index) pairs and hipCUB's storage (a sort of m pairs, sums of nv + m ints)
    double* moved;           // [m][3] the new points under the pose
    long long* skeys;        // [m] sorted
    int* order;              // [m] input index of every sorted position
    int* head;               // [m]
    int* rid;                // [m]
    long long* run_key;      // [m]
    int* run_pos;            // [m + 1]
    int* run_old;            // [m]
    int* run_old_count;      // [m]
    int* run_take;           // [m]
    int* new_only;           // [m]
    int* nrank;              // [m]
    int* run_mv;             // [m]
    int* old_mv;             // [nv]
    int* mv_old;             // [nv + m]
    int* mv_run;             // [nv + m]
    int* size;               // [nv + m]
    int* alive;              // [nv + m]
    int* vpos;               // [nv + m]
    int* ppos;               // [nv + m]
    int* cnt;                // [UPD_COUNTERS]
};

UpdateWs carve_update(void* p, int64_t nv, int64_t m, size_t* used = nullptr) {
    VfmCarver c(p);
    const size_t mm = (size_t)(m > 0 ? m : 1), vv = (size_t)(nv > 0 ? nv : 1), tt = (size_t)(nv + m > 0 ? nv + m : 1);
    UpdateWs w{};
    w.s.keys_in = c.take<long long>(mm);
    w.s.idx_in = c.take<int>(mm);
    const size_t a = grid3::cub_bytes<true>(m), b = grid3::cub_bytes<true>(nv + m);
    w.s.cub_bytes = a > b ? a : b;
    w.s.cub = c.take<unsigned char>(w.s.cub_bytes);
    w.moved = c.take<double>(3 * mm);
    w.skeys = c.take<long long>(mm);
    w.order = c.take<int>(mm);
    w.head = c.take<int>(mm);
    w.rid = c.take<int>(mm);
    w.run_key = c.take<long long>(mm);
    w.run_pos = c.take<int>(mm + 1);
    w.run_old = c.take<int>(mm);
    w.run_old_count = c.take<int>(mm);
    w.run_take = c.take<int>(mm);
    w.new_only = c.take<int>(mm);
    w.nrank = c.take<int>(mm);
    w.run_mv = c.take<int>(mm);
    w.old_mv = c.take<int>(vv);
    w.mv_old = c.take<int>(tt);
    w.mv_run = c.take<int>(tt);
    w.size = c.take<int>(tt);
    w.alive = c.take<int>(tt);
    w.vpos = c.take<int>(tt);
    w.ppos = c.take<int>(tt);
    w.cnt = c.take<int>(UPD_COUNTERS);
    if (used) *used = c.used();
    return w;
}

bool update_sizes_ok(int64_t nv, int64_t nk, int64_t m) {
    return nv >= 0 && nk >= 0 && m >= 0 && nv <= nk && nk <= ICP_GRID_MAX_POINTS && m <= ICP_GRID_MAX_POINTS && nk + m <= ICP_GRID_MAX_POINTS;
}

// ------------------------------------------------------------------------------------------------------------------ rows merge
// A pure copy, HBM-bound: a row is U units of V (uint4 = 16 bytes, or a dword), lane l of a wave moves units l, l + 64, ... of its row, so
// a wave's access is one contiguous stretch.  Rows shorter than 64 units share a wave: 64 / U of them, U lanes each (the lanes behind the
// last whole row idle).  Up to ROWS_MERGE_BATCH loads of a lane are issued before its first store (a second row in flight per lane
// showed no gain: DESIGN 7.7).  Waves stride over the rows; the row count is read from device memory, so the grid is sized for n_max and the waves beyond *n_out_dev leave at once.
enum { ROWS_MERGE_THREADS = 256, ROWS_MERGE_BATCH = 4 };

template <typename V>
__global__ __launch_bounds__(ROWS_MERGE_THREADS) void rows_merge_kernel(const V* __restrict__ rows_old, int64_t nk, const V* __restrict__ rows_new,
                                                                        int64_t m, int64_t U, const int* __restrict__ src,
                                                                        const int* __restrict__ n_out_dev, int64_t n_max, V* __restrict__ rows_out) {
    int64_t n = *n_out_dev;
    n = n < n_max ? n : n_max;
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * ROWS_MERGE_THREADS + threadIdx.x) >> 6;
    const int64_t waves = ((int64_t)gridDim.x * ROWS_MERGE_THREADS) >> 6;
    const int per_wave = U < 64 ? (int)(64 / U) : 1;            // rows of one wave's pass
    const int sub = U < 64 ? lane / (int)U : 0;                  // this lane's row of the pass
    const int64_t u0 = U < 64 ? lane % (int)U : lane;            // ... and its first unit
    const int64_t step = U < 64 ? U : 64;                        // (a short row: one unit per lane, the loop below runs once)
    if (sub >= per_wave) return;
    for (int64_t q = wave * per_wave + sub; q < n; q += waves * per_wave) {
        const int64_t s = src[q];
        if (s < 0 || s >= nk + m) continue;                      // (a caller's error; nothing is written for the row)
        const V* __restrict__ from = s < nk ? rows_old + s * U : rows_new + (s - nk) * U;
        V* __restrict__ to = rows_out + q * U;
        for (int64_t u = u0; u < U; u += ROWS_MERGE_BATCH * step) {
            V v[ROWS_MERGE_BATCH];
#pragma unroll
            for (int k = 0; k < ROWS_MERGE_BATCH; ++k)
                if (u + k * step < U) v[k] = from[u + k * step];
#pragma unroll
            for (int k = 0; k < ROWS_MERGE_BATCH; ++k)
                if (u + k * step < U) to[u + k * step] = v[k];
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

VFM_EXPORT int vfm_range_crop(const double* pts, int64_t n, int64_t stride, double min_range, double max_range, int64_t* idx_out,
                              int64_t* count_out, vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 0 && stride >= 3, "range_crop: n must not be negative and a row holds at least 3 values");
    VFM_CHECK_ARG(!isnan(min_range) && !isnan(max_range), "range_crop: the bounds must be numbers");
    VFM_CHECK_ARG(count_out && (n == 0 || (pts && idx_out)), "range_crop: null pointer");
    hipLaunchKernelGGL(range_crop_kernel, dim3(1), dim3(ORDERED_COMPACT_THREADS), 0, (hipStream_t)stream, pts, n, stride, min_range, max_range,
                       idx_out, count_out);
    VFM_CHECK_LAUNCH("range_crop_kernel");
    return VFM_OK;
}

VFM_EXPORT int vfm_deskew_scan(const double* pts, int64_t n, int64_t stride, const double* timestamps, const double* delta_host, double* out,
                               vfm_stream_t stream) {
    VFM_CHECK_ARG(n >= 0 && stride >= 3, "deskew_scan: n must not be negative and a row holds at least 3 values");
    VFM_CHECK_ARG(delta_host, "deskew_scan: null pointer");
    Twist d;
    for (int k = 0; k < 6; ++k) {
        d.d[k] = delta_host[k];
        VFM_CHECK_ARG(isfinite(d.d[k]), "deskew_scan: the twist must be finite");
    }
    if (n == 0) return VFM_OK;
    VFM_CHECK_ARG(pts && timestamps && out, "deskew_scan: null pointer");
    VFM_CHECK_ARG((n + 255) / 256 <= 0x7FFFFFFF, "deskew_scan: too many points for one launch");
    hipLaunchKernelGGL(deskew_kernel, dim3(grid3::blocks256(n)), dim3(256), 0, (hipStream_t)stream, pts, n, stride, timestamps, d, out);
    VFM_CHECK_LAUNCH("deskew_kernel");
    return VFM_OK;
}

VFM_EXPORT size_t vfm_icp_grid_update_workspace_bytes(int32_t nv, int64_t nk, int64_t m) {
    if (!update_sizes_ok(nv, nk, m)) return 0;
    size_t used = 0;
    (void)carve_update(nullptr, nv, m, &used);   // (a null base: only the offsets)
    return used;
}

// the body of both update entries; src_out: NULL for vfm_icp_grid_update
static int grid_update(const int64_t* keys, const int32_t* start, const double* pts, int32_t nv, int64_t nk, const double* xyz_new, int64_t m,
                       const double* T_host, double voxel_size, int32_t max_points_per_voxel, const double* origin_host, double max_distance,
                       int64_t* keys_out, int32_t* start_out, double* pts_out, int32_t* info_out, int32_t* src_out, void* ws, size_t ws_bytes,
                       vfm_stream_t stream) {
    VFM_CHECK_ARG(update_sizes_ok(nv, nk, m), "icp_grid_update: bad sizes (0 <= nv <= nk, nk + m <= 2^30)");
    VFM_CHECK_ARG((nv == 0) == (nk == 0), "icp_grid_update: a grid without voxels holds no points, and one with voxels holds some");
    VFM_CHECK_ARG(voxel_size > 0.0 && max_points_per_voxel >= 0, "icp_grid_update: bad voxel_size / max_points_per_voxel");
    VFM_CHECK_ARG(!origin_host || (max_distance >= 0.0 && max_distance < INFINITY), "icp_grid_update: max_distance must be finite and not negative");
    VFM_CHECK_ARG(start_out && info_out, "icp_grid_update: null pointer");
    VFM_CHECK_ARG(nv == 0 || (keys && start && pts), "icp_grid_update: null pointer (old grid)");
    VFM_CHECK_ARG(m == 0 || xyz_new, "icp_grid_update: null pointer (new points)");
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = (int64_t)nv + m;
    if (total == 0) {
        hipLaunchKernelGGL(upd_empty_kernel, dim3(1), dim3(64), 0, st, start_out, info_out);
        VFM_CHECK_LAUNCH("upd_empty_kernel");
        return VFM_OK;
    }
    VFM_CHECK_ARG(keys_out && pts_out && ws, "icp_grid_update: null pointer");
    VFM_CHECK_ARG(keys_out != reinterpret_cast<const int64_t*>(keys) && start_out != start && pts_out != pts,
                  "icp_grid_update: the new grid must not alias the old one");
    VFM_CHECK_ARG(ws_bytes >= vfm_icp_grid_update_workspace_bytes(nv, nk, m), "icp_grid_update: workspace too small");
    Origin org{};
    org.remove = origin_host ? 1 : 0;
    if (origin_host) {
        for (int k = 0; k < 3; ++k) org.o[k] = origin_host[k];
        org.max_d2 = max_distance * max_distance;
    }
    Pose P{};
    if (T_host)
        for (int k = 0; k < 12; ++k) P.T[k] = T_host[k];
    const UpdateWs w = carve_update(ws, nv, m);
    const long long* okeys = reinterpret_cast<const long long*>(keys);
    const dim3 block(256), grid_m(grid3::blocks256(m)), grid_t(grid3::blocks256(total));
    VFM_CHECK_HIP(hipMemsetAsync(w.cnt, 0, UPD_COUNTERS * sizeof(int), st));
    const double* moved = xyz_new;
    if (m > 0) {
        if (T_host) {
            hipLaunchKernelGGL(upd_move_kernel, grid_m, block, 0, st, xyz_new, m, P, w.moved);
            VFM_CHECK_LAUNCH("upd_move_kernel");
            moved = w.moved;
        }
        VFM_TRY(grid3::build(moved, m, IcpVoxels{voxel_size}, w.cnt + UPD_STATUS, w.s, w.skeys, w.order, st));
        VFM_TRY(grid3::run_ids(w.s, m, w.skeys, w.head, w.rid, st));
        hipLaunchKernelGGL(upd_runs_kernel, grid_m, block, 0, st, w.skeys, w.rid, m, w.run_key, w.run_pos, w.cnt);
        VFM_CHECK_LAUNCH("upd_runs_kernel");
        hipLaunchKernelGGL(upd_takers_kernel, grid_m, block, 0, st, w.run_key, w.run_pos, m, okeys, start, (int)nv, (int)max_points_per_voxel,
                           w.run_old, w.run_old_count, w.run_take, w.new_only, w.cnt);
        VFM_CHECK_LAUNCH("upd_takers_kernel");
        VFM_TRY(grid3::inclusive_sum(w.s, m, w.new_only, w.nrank, st));
    }
    hipLaunchKernelGGL(upd_merge_kernel, grid_t, block, 0, st, okeys, (int)nv, w.run_key, w.run_old, w.nrank, m, w.mv_old, w.mv_run, w.old_mv,
                       w.run_mv, w.cnt);
    VFM_CHECK_LAUNCH("upd_merge_kernel");
    if (m > 0 && nv > 0) {
        hipLaunchKernelGGL(upd_run_mv_kernel, grid_m, block, 0, st, w.run_old, w.old_mv, w.run_mv, m, w.cnt);
        VFM_CHECK_LAUNCH("upd_run_mv_kernel");
    }
    hipLaunchKernelGGL(upd_sizes_kernel, grid_t, block, 0, st, w.mv_old, w.mv_run, (int)nv, total, start, pts, w.run_pos, w.run_take, w.order, moved,
                       org, w.size, w.alive, w.cnt);
    VFM_CHECK_LAUNCH("upd_sizes_kernel");
    VFM_TRY(grid3::inclusive_sum(w.s, total, w.alive, w.vpos, st));
    VFM_TRY(grid3::inclusive_sum(w.s, total, w.size, w.ppos, st));
    const int64_t widest = nk > total ? nk : total;
    hipLaunchKernelGGL(upd_scatter_kernel, dim3(grid3::blocks256(widest)), block, 0, st, okeys, start, pts, (int)nv, nk, m, total, w.mv_old, w.mv_run,
                       w.old_mv, w.run_mv, w.run_key, w.run_pos, w.run_old_count, w.run_take, w.rid, w.order, moved, w.size, w.alive, w.vpos,
                       w.ppos, w.cnt, reinterpret_cast<long long*>(keys_out), start_out, pts_out, info_out, src_out);
    VFM_CHECK_LAUNCH("upd_scatter_kernel");
    return VFM_OK;
}

VFM_EXPORT int vfm_icp_grid_update(const int64_t* keys, const int32_t* start, const double* pts, int32_t nv, int64_t nk, const double* xyz_new,
                                   int64_t m, const double* T_host, double voxel_size, int32_t max_points_per_voxel, const double* origin_host,
                                   double max_distance, int64_t* keys_out, int32_t* start_out, double* pts_out, int32_t* info_out, void* ws,
                                   size_t ws_bytes, vfm_stream_t stream) {
    return grid_update(keys, start, pts, nv, nk, xyz_new, m, T_host, voxel_size, max_points_per_voxel, origin_host, max_distance, keys_out,
                       start_out, pts_out, info_out, nullptr, ws, ws_bytes, stream);
}

VFM_EXPORT int vfm_icp_grid_update_src(const int64_t* keys, const int32_t* start, const double* pts, int32_t nv, int64_t nk,
                                       const double* xyz_new, int64_t m, const double* T_host, double voxel_size, int32_t max_points_per_voxel,
                                       const double* origin_host, double max_distance, int64_t* keys_out, int32_t* start_out, double* pts_out,
                                       int32_t* info_out, int32_t* src_out, void* ws, size_t ws_bytes, vfm_stream_t stream) {
    VFM_CHECK_ARG(src_out || (int64_t)nv + m <= 0, "icp_grid_update_src: null pointer (src_out)");
    return grid_update(keys, start, pts, nv, nk, xyz_new, m, T_host, voxel_size, max_points_per_voxel, origin_host, max_distance, keys_out,
                       start_out, pts_out, info_out, src_out, ws, ws_bytes, stream);
}

VFM_EXPORT int vfm_rows_merge(const void* rows_old, int64_t nk, const void* rows_new, int64_t m, int64_t row_bytes, const int32_t* src,
                              const int32_t* n_out_dev, int64_t n_max, void* rows_out, vfm_stream_t stream) {
    VFM_CHECK_ARG(nk >= 0 && m >= 0 && nk + m <= ICP_GRID_MAX_POINTS && n_max >= 0 && n_max <= ICP_GRID_MAX_POINTS,
                  "rows_merge: bad sizes (0 <= nk, m, n_max; nk + m and n_max <= 2^30)");
    VFM_CHECK_ARG(row_bytes > 0 && row_bytes % 4 == 0 && row_bytes <= (int64_t)1 << 30, "rows_merge: row_bytes must be a positive multiple of 4");
    if (n_max == 0) return VFM_OK;
    VFM_CHECK_ARG(src && n_out_dev && rows_out, "rows_merge: null pointer");
    VFM_CHECK_ARG((nk == 0 || rows_old) && (m == 0 || rows_new), "rows_merge: null pointer (rows)");
    VFM_CHECK_ARG(rows_out != rows_old && rows_out != rows_new, "rows_merge: the output must not alias an input");
    const bool wide = row_bytes % 16 == 0 && aligned16(rows_old) && aligned16(rows_new) && aligned16(rows_out);
    const int64_t U = row_bytes / (wide ? 16 : 4);
    const int64_t per_wave = U < 64 ? 64 / U : 1;
    const int64_t waves = (n_max + per_wave - 1) / per_wave;
    const int waves_per_block = ROWS_MERGE_THREADS / 64;
    int64_t blocks = (waves + waves_per_block - 1) / waves_per_block;
    const int64_t resident = 256 * 8;   // 256 CUs x 8 workgroups of 4 waves: every SIMD full; the waves stride over the rest
    if (blocks > resident) blocks = resident;
    hipStream_t st = (hipStream_t)stream;
    if (wide)
        hipLaunchKernelGGL(rows_merge_kernel<uint4>, dim3((unsigned)blocks), dim3(ROWS_MERGE_THREADS), 0, st, (const uint4*)rows_old, nk,
                           (const uint4*)rows_new, m, U, src, n_out_dev, n_max, (uint4*)rows_out);
    else
        hipLaunchKernelGGL(rows_merge_kernel<uint32_t>, dim3((unsigned)blocks), dim3(ROWS_MERGE_THREADS), 0, st, (const uint32_t*)rows_old, nk,
                           (const uint32_t*)rows_new, m, U, src, n_out_dev, n_max, (uint32_t*)rows_out);
    VFM_CHECK_LAUNCH("rows_merge_kernel");
    return VFM_OK;
}

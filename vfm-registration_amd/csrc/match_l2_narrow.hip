// match_l2_narrow.hip -- exact Euclidean 1-NN for NARROW descriptors (1 <= d <= 64: FPFH's 33 columns, the 32 of the learned
// baselines) on the f32-input MFMA, VFM_MATCH_NARROW (DESIGN.md 4.1 "Row A6, narrow rows" and 7.5).
//
// Screening.  With the common power-of-two scale of the Euclidean searches (x~ = 2^-k x, every row norm of both sets <= 1; exact),
//     |a - b|^2 = 4^k ( |a~|^2 + c(a, b) ),      c(a, b) = |b~|^2 - 2 a~.b~,
// so for one query the arg-min over the map is the arg-min of c.  c is computed in f32 by v_mfma_f32_32x32x2_f32: map rows are the A
// operand (a 32-row tile, staged through LDS once per workgroup), queries the B operand (a lane owns query `lane & 31`; its fragment
// -- Kp / 2 registers of -2 a~, Kp = d rounded up to even -- stays resident for the whole sweep), and the accumulators START at the
// map row's f32 |b~|^2, so what comes out of the k-ordered fmaf chain is c itself.  |c_f32 - c| <= E0 = (4 Kp + 1) 2^-24.
//
// Decision, inline.  For the query's true nearest row j* and ANY map row g, D(j*) <= D(g) in the oracle's fp64 arithmetic, hence
// c_f32(j*) <= c_f32(g) + 2 E0 + (fp64 slack).  A lane therefore keeps c_min, the smallest screened value it has seen, and evaluates
// a row exactly -- the oracle's loop on the ORIGINAL rows -- iff c_f32(row) <= c_min + W, W = (8 Kp + 16) 2^-24: the nearest row
// always passes, whenever it arrives.  (c_min is at most the screened value of the current exact best, so these are a subset of the
// rows within W of that one.)  The rows that pass wait in a four-entry queue per lane until the wave decides them together; the
// exact value replaces the lane's best iff it is smaller, or equal with a lower index, so the order does not matter.  No candidate
// list in memory, no overflow path, no all-pairs fallback: identical rows are simply all evaluated.
//
// Decomposition.  Grid = query blocks (256 queries: 4 waves x 2 query tiles) x map slices (l2n_slices: enough workgroups for two per
// CU).  A wave merges its two lane halves (they hold different map rows of the same queries), every (query, slice) leaves one
// (d^2, index) partial, l2n_merge_kernel takes the lexicographic minimum (smaller d^2, then lower index) over the slices.  No
// atomics on a result; one atomic per wave on the evaluation counter (include/vfmreg_debug.h).
#include "match_exact.h"

#include <utility>

namespace vfmm {
namespace {

constexpr int L2N_QBLOCK = 256;           // queries per workgroup
constexpr int L2N_TARGET_WGS = 512;       // two workgroups for each of the 256 CUs
constexpr int L2N_MIN_SLICE_TILES = 8;    // a slice is at least 256 map rows ...
constexpr int L2N_MAX_SLICES = 256;       // ... and there are at most this many

__host__ __device__ inline int l2n_kp(int d) { return (d + 1) & ~1; }
__host__ __device__ inline size_t l2n_tile_floats(int kp) { return (size_t)(kp + 1) * 32; }   // [|b~|^2 x 32][k][32 rows]

// the map, scaled and transposed into the A-operand order of the 32x32x2 MFMA: tile record = 32 f32 row norms, then column k of
// the tile's 32 rows for k = 0 .. kp - 1 (so k-step s of a wave is ONE conflict-free ds_read_b32 at 64 s + lane).  Rows past the
// map: zero columns and |b~|^2 = +inf -- they screen as +inf and are never evaluated.
__global__ __launch_bounds__(256) void l2n_prep_kernel(const float* __restrict__ b, int64_t m, int d, int kp,
                                                       const unsigned* __restrict__ max_bits, float* __restrict__ bt) {
    __shared__ __attribute__((aligned(16))) float img[(VFM_L2_NARROW_MAX_D + 1) * 32];
    const int64_t r0 = (int64_t)blockIdx.x * 32;
    const float scale = l2_scale(max_bits);
    const int rows = (int)(m - r0 < 32 ? m - r0 : 32);
    for (int e = threadIdx.x; e < 32 * kp; e += 256) img[32 + e] = 0.0f;
    __syncthreads();
    for (int e = threadIdx.x; e < rows * d; e += 256) {   // the tile's rows are one contiguous run of the map
        const int r = e / d, k = e - r * d;
        img[32 + k * 32 + r] = b[r0 * (int64_t)d + e] * scale;
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        const int r = threadIdx.x;
        float s = 0.0f;
        for (int k = 0; k < kp; ++k) {
            const float v = img[32 + k * 32 + r];
            s = s + v * v;
        }
        img[r] = r < rows ? s : __builtin_inff();
    }
    __syncthreads();
    const int units = (kp + 1) * 8;
    float4* dst = reinterpret_cast<float4*>(bt + (size_t)blockIdx.x * l2n_tile_floats(kp));
    for (int u = threadIdx.x; u < units; u += 256) dst[u] = reinterpret_cast<const float4*>(img)[u];
}

struct L2nArgs {
    const float* q;       // query rows (original)
    const int* qperm;     // query i is row qperm[i] of q (NULL: row i)
    int64_t n;
    const float* b;       // map rows (original)
    int64_t m;
    int d;
    const unsigned* max_bits;
    const float* bt;      // l2n_prep_kernel's image of the map
    int ntiles, nqb, nslices;
    float window;         // W
    double* pd2;          // [nslices][n]
    int* pj;              // [nslices][n]
    unsigned long long* evals;
};

// the oracle's loop, one l2_step_f64 (match_exact.h) per column, k ascending.  Both rows
// are loaded first -- in one go up to 34 columns, 16 at a time beyond -- so that a decision waits for memory a few times, not per
// column; the padding column (d odd) is read as 0 - 0 and adds an exact +0.
template <int KP>
__device__ __forceinline__ double l2n_exact(const float* __restrict__ qa, const float* __restrict__ br, int d) {
    constexpr int CH = KP <= 34 ? KP : 16;   // (wider rows: the sweep keeps Kp registers of queries, no room for 2 Kp more)
    double acc = 0.0;
#pragma unroll
    for (int k0 = 0; k0 < KP; k0 += CH) {
        float av[CH], bv[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int k = k0 + u;
            const bool ok = k < KP - 1 || k < d;   // (d is KP or KP - 1)
            av[u] = (k < KP && ok) ? qa[k] : 0.0f;
            bv[u] = (k < KP && ok) ? br[k] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            if (k0 + u < KP) acc = l2_step_f64(acc, av[u], bv[u]);
        }
    }
    return acc;
}

// A lane's state for one query.  Rows inside the window are not decided where they are found -- one lane of 64 would run the fp64
// chain while the others wait, ln(rows) times per lane and slice -- but queued (any order: the decision does not depend on it) and
// decided together, all lanes at once, when some lane's queue fills up and at the end of the sweep.
constexpr int L2N_QUEUE = 4;
struct L2nBest {
    double d2;
    long long j;     // < 0: nothing evaluated yet
    float c_min;     // smallest screened value seen (shared by the two lane halves)
    int np;          // queued rows: pend[0 .. np)
    int pend[L2N_QUEUE];
};

__device__ __forceinline__ float l2n_min16(const floatx16& c) {
    const float a = fminf(fminf(c[0], c[1]), fminf(c[2], c[3])), b = fminf(fminf(c[4], c[5]), fminf(c[6], c[7]));
    const float e = fminf(fminf(c[8], c[9]), fminf(c[10], c[11])), f = fminf(fminf(c[12], c[13]), fminf(c[14], c[15]));
    return fminf(fminf(a, b), fminf(e, f));
}

template <int KP>
__device__ __forceinline__ void l2n_flush(const L2nArgs& p, const float* __restrict__ qrow, L2nBest& best, unsigned& evals) {
    while (best.np > 0) {   // (one copy of the chain per call site: the queue is popped from its head)
        const long long j = best.pend[0];
#pragma unroll
        for (int i = 0; i + 1 < L2N_QUEUE; ++i) best.pend[i] = best.pend[i + 1];
        --best.np;
        const double v = l2n_exact<KP>(qrow, p.b + j * (int64_t)p.d, p.d);
        ++evals;
        if (nearer_before(v, j, best.d2, best.j)) {
            best.d2 = v;
            best.j = j;
        }
    }
}

// one tile's 16 screened values of the lane's query: queue what is inside the window
template <int KP>
__device__ __forceinline__ void l2n_decide(const L2nArgs& p, const floatx16& c, float window, bool live, const float* __restrict__ qrow,
                                           int64_t row0, L2nBest& best, unsigned& evals) {
    const float mn = l2n_min16(c);
    float cm = fminf(best.c_min, mn);
    cm = fminf(cm, __shfl_xor(cm, 32));
    best.c_min = cm;
    const float thr = cm + window;
    if (live && !(mn > thr)) {
        unsigned mask = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (!(c[r] > thr)) mask |= 1u << r;
        while (mask) {
            const int r = __ffs(mask) - 1;
            mask &= mask - 1u;
            const int64_t j = row0 + (r & 3) + 8 * (r >> 2);
            if (j >= p.m) continue;
            if (best.np == L2N_QUEUE) l2n_flush<KP>(p, qrow, best, evals);   // (more than four rows of one tile: ties)
#pragma unroll
            for (int i = L2N_QUEUE - 1; i > 0; --i) best.pend[i] = best.pend[i - 1];
            best.pend[0] = (int)j;
            ++best.np;
        }
    }
}

template <int KS>
__global__ __launch_bounds__(256, 2) void l2n_sweep_kernel(L2nArgs p) {
    constexpr int KP = 2 * KS, REC = (KP + 1) * 32, UNITS = REC / 4, U = (UNITS + 255) / 256;
    __shared__ __attribute__((aligned(16))) float tiles[2 * REC];
    const int lane = lane_id(), wave = threadIdx.x >> 6, h = lane >> 5;
    const int qb = blockIdx.x % p.nqb, slice = blockIdx.x / p.nqb;   // consecutive workgroups sweep the same slice
    const int t0 = (int)((int64_t)slice * p.ntiles / p.nslices), t1 = (int)((int64_t)(slice + 1) * p.ntiles / p.nslices);
    const float mx = __uint_as_float(*p.max_bits);
    const float scale = l2_scale(p.max_bits);
    // (a largest sum of squares that left fp32 -- rows longer than 1.8e19 -- leaves the copies unscaled and c meaningless: every row
    // is evaluated then)
    const float window = (mx < 3.0e38f) ? p.window : __builtin_inff();

    // the wave's two query tiles: fragments -2 a~ (B operand: k = 2 s + h, column lane & 31)
    const int64_t q0 = (int64_t)qb * L2N_QBLOCK + wave * 64 + (lane & 31);
    const float* qrow[2];
    bool live[2];
    float qf[2][KS];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int64_t qi = q0 + 32 * u;
        live[u] = qi < p.n;
        const int64_t src = live[u] ? (p.qperm ? (int64_t)p.qperm[qi] : qi) : 0;
        qrow[u] = p.q + src * (int64_t)p.d;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k = 2 * s + h;
            qf[u][s] = (live[u] && k < p.d) ? -2.0f * (qrow[u][k] * scale) : 0.0f;
        }
    }
    const bool two = (int64_t)qb * L2N_QBLOCK + wave * 64 + 32 < p.n;   // wave-uniform: the second tile holds a query
    L2nBest best[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) best[u] = L2nBest{0.0, -1, 3.0e38f, 0, {0, 0, 0, 0}};
    unsigned evals = 0u;

    float4 pre[U];
    auto load = [&](int t) {
        const float4* src = reinterpret_cast<const float4*>(p.bt + (size_t)t * REC);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int idx = threadIdx.x + 256 * u;
            if (idx < UNITS) pre[u] = src[idx];
        }
    };
    auto store = [&](int buf) {
        float4* dst = reinterpret_cast<float4*>(tiles + buf * REC);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int idx = threadIdx.x + 256 * u;
            if (idx < UNITS) dst[idx] = pre[u];
        }
    };
    if (t0 < t1) {
        load(t0);
        store(0);
    }
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        const int buf = (t - t0) & 1;
        if (t + 1 < t1) load(t + 1);
        const float* T = tiles + buf * REC;
        // accumulators start at |b~|^2 of their rows: row = (reg & 3) + 8 (reg >> 2) + 4 h
        floatx16 c0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 v = *reinterpret_cast<const float4*>(T + 8 * g + 4 * h);
            c0[4 * g] = v.x;
            c0[4 * g + 1] = v.y;
            c0[4 * g + 2] = v.z;
            c0[4 * g + 3] = v.w;
        }
        const int64_t row0 = (int64_t)t * 32 + 4 * h;
        if (two) {
            floatx16 c1 = c0;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const float a = T[32 + 64 * s + lane];
                c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, qf[0][s], c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, qf[1][s], c1, 0, 0, 0);
            }
            l2n_decide<KP>(p, c0, window, live[0], qrow[0], row0, best[0], evals);
            l2n_decide<KP>(p, c1, window, live[1], qrow[1], row0, best[1], evals);
        } else {
#pragma unroll
            for (int s = 0; s < KS; ++s) c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(T[32 + 64 * s + lane], qf[0][s], c0, 0, 0, 0);
            l2n_decide<KP>(p, c0, window, live[0], qrow[0], row0, best[0], evals);
        }
        if (__any(best[0].np >= L2N_QUEUE - 1 || best[1].np >= L2N_QUEUE - 1)) {
            l2n_flush<KP>(p, qrow[0], best[0], evals);
            l2n_flush<KP>(p, qrow[1], best[1], evals);
        }
        if (t + 1 < t1) store(buf ^ 1);
        __syncthreads();
    }
    // the two lane halves of a query: smaller d^2, then lower index
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        l2n_flush<KP>(p, qrow[u], best[u], evals);
        const double od = __shfl_xor(best[u].d2, 32);
        const long long oj = __shfl_xor(best[u].j, 32);
        if (nearer_before(od, oj, best[u].d2, best[u].j)) {
            best[u].d2 = od;
            best[u].j = oj;
        }
        const int64_t qi = q0 + 32 * u;
        if (h == 0 && live[u]) {
            p.pd2[(size_t)slice * (size_t)p.n + (size_t)qi] = best[u].d2;
            p.pj[(size_t)slice * (size_t)p.n + (size_t)qi] = (int)best[u].j;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) evals += __shfl_xor(evals, off);
    if (lane == 0 && evals) atomicAdd(p.evals, (unsigned long long)evals);
}

__global__ void l2n_merge_kernel(const double* __restrict__ pd2, const int* __restrict__ pj, int64_t n, int nslices,
                                 int64_t* __restrict__ nn, double* __restrict__ d2) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double best = 0.0;
    long long bj = -1;
    for (int s = 0; s < nslices; ++s) {
        const double v = pd2[(size_t)s * (size_t)n + (size_t)i];
        const long long j = pj[(size_t)s * (size_t)n + (size_t)i];
        if (nearer_before(v, j, best, bj)) {
            best = v;
            bj = j;
        }
    }
    nn[i] = bj;
    if (d2) d2[i] = best;
}

template <int KS>
void l2n_launch(const L2nArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(l2n_sweep_kernel<KS>, dim3((unsigned)(a.nqb * a.nslices)), dim3(256), 0, st, a);
}
template <size_t... I>
void l2n_dispatch(int ks, const L2nArgs& a, hipStream_t st, std::index_sequence<I...>) {
    using Fn = void (*)(const L2nArgs&, hipStream_t);
    static const Fn table[] = {&l2n_launch<(int)I + 1>...};
    table[ks - 1](a, st);
}

struct L2nDirWs {
    float* bt;
    double* pd2;
    int* pj;
    size_t bytes;
};
inline L2nDirWs carve_l2n_dir(void* p, int64_t nq, int64_t m, int d) {
    VfmCarver c(p);
    L2nDirWs w;
    const size_t ntiles = (size_t)((m + 31) / 32), s = (size_t)l2n_slices(nq, m);
    w.bt = c.take<float>(ntiles * l2n_tile_floats(l2n_kp(d)));
    w.pd2 = c.take<double>(s * (size_t)nq);
    w.pj = c.take<int>(s * (size_t)nq);
    w.bytes = c.used();
    return w;
}

}  // namespace

// map slices of a search of nq queries among m rows: enough workgroups for two per CU, a slice no shorter than 8 tiles
int l2n_slices(int64_t nq, int64_t m) {
    const int64_t nqb = (nq + L2N_QBLOCK - 1) / L2N_QBLOCK, ntiles = (m + 31) / 32;
    int64_t s = (L2N_TARGET_WGS + nqb - 1) / (nqb > 0 ? nqb : 1);
    const int64_t cap = ntiles / L2N_MIN_SLICE_TILES;
    if (s > cap) s = cap;
    if (s > L2N_MAX_SLICES) s = L2N_MAX_SLICES;
    return (int)(s < 1 ? 1 : s);
}

size_t l2n_dir_bytes(int64_t nq, int64_t m, int d) { return carve_l2n_dir(nullptr, nq, m, d).bytes; }

int l2n_search(const float* q, const int* qperm, int64_t nq, const float* b, int64_t m, int d, const unsigned* max_bits, int64_t* nn,
               double* d2, void* ws_dir, unsigned long long* evals, hipStream_t st) {
    const L2nDirWs w = carve_l2n_dir(ws_dir, nq, m, d);
    const int kp = l2n_kp(d);
    L2nArgs a;
    a.q = q;
    a.qperm = qperm;
    a.n = nq;
    a.b = b;
    a.m = m;
    a.d = d;
    a.max_bits = max_bits;
    a.bt = w.bt;
    a.ntiles = (int)((m + 31) / 32);
    a.nqb = (int)((nq + L2N_QBLOCK - 1) / L2N_QBLOCK);
    a.nslices = l2n_slices(nq, m);
    a.window = (float)(8 * kp + 16) * 5.9604644775390625e-8f;   // W = (8 Kp + 16) 2^-24 >= 2 E0 + the rounding of c_min + W itself
    a.pd2 = w.pd2;
    a.pj = w.pj;
    a.evals = evals;
    hipLaunchKernelGGL(l2n_prep_kernel, dim3((unsigned)a.ntiles), dim3(256), 0, st, b, m, d, kp, max_bits, w.bt);
    VFM_CHECK_LAUNCH("l2n_prep_kernel");
    l2n_dispatch(kp / 2, a, st, std::make_index_sequence<VFM_L2_NARROW_MAX_D / 2>{});
    VFM_CHECK_LAUNCH("l2n_sweep_kernel");
    hipLaunchKernelGGL(l2n_merge_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, (const double*)w.pd2, (const int*)w.pj, nq,
                       a.nslices, nn, d2);
    VFM_CHECK_LAUNCH("l2n_merge_kernel");
    return VFM_OK;
}

}  // namespace vfmm

using namespace vfmm;

VFM_EXPORT int vfm_debug_l2_narrow_slices(int64_t n, int64_t m) { return (n > 0 && m > 0) ? l2n_slices(n, m) : 0; }

VFM_EXPORT int vfm_debug_l2_narrow_evals(const void* ws, int64_t* out2_host) {
    VFM_CHECK_ARG(ws && out2_host, "l2_narrow_evals: bad arguments");
    VFM_CHECK_HIP(hipDeviceSynchronize());
    unsigned long long v[2];
    VFM_CHECK_HIP(hipMemcpy(v, ws, sizeof(v), hipMemcpyDeviceToHost));   // (the counters are the first thing the entry points carve)
    out2_host[0] = (int64_t)v[0];
    out2_host[1] = (int64_t)v[1];
    return VFM_OK;
}

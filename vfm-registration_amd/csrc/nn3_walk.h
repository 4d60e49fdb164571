// nn3_walk.h -- the shell walk over the grid of vfm_nn3_build that nn3.hip's two searches and hdbscan.hip's spanning-tree search
// share (internal: not part of the C ABI).  The quantiser, the column runs and nn3_walk<Sink>; the sinks stay in their files.
#pragma once
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

using grid3::Best;

// f(lane) for every set bit of a wave-uniform ballot, in ascending lane order
template <typename F>
__device__ __forceinline__ void nn3_each_lane(unsigned long long m, F f) {
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        f(src);
    }
}

// What shell r holds of column (ax, ay): the z-cells of a column are consecutive keys, so a column on the border of the (2r + 1)^2
// square is ONE run of keys (cz - r .. cz + r, `whole`) and a column inside it two single cells (a: cz - r, b: cz + r).  A run ends at
// grid3::upper_bound, which needs no key + 1.
struct Nn3Runs {
    int lo_a, len_a, lo_b, len_b;
};
__device__ __forceinline__ Nn3Runs nn3_column_runs(const long long* __restrict__ keys, int n, long long ax, long long ay, long long cz, int r,
                                                   bool whole) {
    const long long key_lo = grid3::key(ax, ay, cz - r), key_hi = grid3::key(ax, ay, cz + r);
    Nn3Runs c{grid3::lower_bound(keys, n, key_lo), 0, 0, 0};
    if (whole) {
        c.len_a = grid3::upper_bound(keys, n, key_hi) - c.lo_a;
    } else {
        c.len_a = grid3::upper_bound(keys, n, key_lo) - c.lo_a;
        c.lo_b = grid3::lower_bound(keys, n, key_hi);
        c.len_b = grid3::upper_bound(keys, n, key_hi) - c.lo_b;
    }
    return c;
}

struct Nn3Query {   // one wave (= one workgroup) per query
    const double* __restrict__ sorted;
    const int* __restrict__ order;
    double x, y, z;
    int lane;
};

// The walk of both searches.  Shell r = the cells at Chebyshev distance r from the query's cell (r = 1: the 27 cells around it, the
// query's own among them -- so r starts at 1), walked by columns: 64 columns at a time find their runs with two binary searches per
// lane, and the wave then reads each non-empty run together from the copy of the cloud kept in cell order (sink.run, lo and len the
// same in every lane).  After shell r every point of a cell at most r cells from the query's in every axis has been read -- clamping
// is 1-Lipschitz (grid3.h), so that holds at the border too -- and every other point has a computed d2 >= reach^2, reach = r cells
// shortened by NN3_RING_SLACK (see there).  sink.done(reach^2) says whether no such point can change the answer; since the bound is
// >=, a sink must ask for strictly less than reach^2 before it rules out ties from outside.  Past NN3_MAX_RINGS shells (queries far
// from the cloud, or in its empty regions) the sink reads every point from where sink.restart() leaves it -- the shells already searched
// are read again -- and done(+inf) closes that scan.
template <typename Sink>
__device__ __forceinline__ void nn3_walk(Sink& sink, const Nn3Query& q, const long long* __restrict__ keys, int n, double inv_cell,
                                         double cell, int* __restrict__ fallback_count) {
    const long long cx = nn3_cell(q.x, inv_cell), cy = nn3_cell(q.y, inv_cell), cz = nn3_cell(q.z, inv_cell);
    bool done = false;
    for (int r = 1; r <= NN3_MAX_RINGS && !done; ++r) {
        const int side = 2 * r + 1;
        const int columns = side * side;
        for (int base = 0; base < columns; base += 64) {
            const int t = base + q.lane;
            Nn3Runs c{0, 0, 0, 0};
            if (t < columns) {
                const int dx = t / side - r, dy = t % side - r;
                c = nn3_column_runs(keys, n, cx + dx, cy + dy, cz, r, r == 1 || dx == -r || dx == r || dy == -r || dy == r);
            }
            nn3_each_lane(__ballot(c.len_a > 0), [&](int src) { sink.run(q, __shfl(c.lo_a, src), __shfl(c.len_a, src)); });
            nn3_each_lane(__ballot(c.len_b > 0), [&](int src) { sink.run(q, __shfl(c.lo_b, src), __shfl(c.len_b, src)); });
        }
        const double reach = ((double)r * cell) * NN3_RING_SLACK;
        done = sink.done(reach * reach);
    }
    if (!done) {
        sink.restart();
        sink.run(q, 0, n);
        (void)sink.done(INFINITY);
        if (fallback_count && q.lane == 0) atomicAdd(fallback_count, 1);
    }
}

}  // namespace

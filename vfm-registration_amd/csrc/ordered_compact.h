// ordered_compact.h -- one pass of an ORDERED compaction by a workgroup of 1024 threads (16 waves), shared by vfm_colour_gate (pca.hip)
// and vfm_range_crop (odometry.hip) (internal: not part of the C ABI).
//
// A pass takes 1024 consecutive rows, thread t the row s0 + t.  The survivors keep the rows' order: a survivor's place is the number of
// survivors before it -- the waves before its own (a ballot's population count per wave, exchanged through LDS), then the lanes before
// its own.  No atomic decides an order.
#pragma once
#include "common.h"

namespace {

constexpr int ORDERED_COMPACT_THREADS = 1024;

struct OrderedCompactLds {
    int wsum[2][16];   // two buffers: a wave that runs ahead into the next pass writes the other one, and is held at that pass's barrier
};

// hit: this thread's row survives.  Returns the row's place among the pass's survivors (meaningful where `hit`), `total` = their number.
// Every thread of the workgroup has to call it; pass p uses buffer p & 1.
__device__ __forceinline__ int ordered_compact_pass(OrderedCompactLds& lds, int buf, bool hit, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) lds.wsum[buf][wave] = __popcll(bal);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const int c = lds.wsum[buf][w];
        if (w < wave) before += c;
        total += c;
    }
    return before + __popcll(bal & ((1ull << lane) - 1ull));
}

}  // namespace

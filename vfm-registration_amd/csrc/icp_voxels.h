// icp_voxels.h -- the ICP grid's quantiser, shared by the build (icp.hip) and the in-place update (odometry.hip): both have to put a
// point into the same voxel, bit for bit (internal: not part of the C ABI).
#pragma once
#include "grid3.h"

namespace {

constexpr int64_t ICP_GRID_MAX_POINTS = (int64_t)1 << 30;   // int32 positions and prefix sums

// v = trunc(xyz / voxel_size), a true division; an axis with |v| >= 2^20 - 1 (or a NaN) is out of range: v = 0 and the status flag
struct IcpVoxels {   // the quantiser of grid3::keys_kernel
    static constexpr const char* kernel_name = "grid3::keys_kernel<IcpVoxels>";
    double voxel_size;
    __device__ long long operator()(double x, double y, double z, bool& bad) const {
        const double lim = (double)((1 << 20) - 1);
        const double p[3] = {x, y, z};
        int v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double t = trunc(p[c] / voxel_size);
            const bool ok = fabs(t) < lim;   // (false for NaN too)
            bad = bad || !ok;
            v[c] = ok ? (int)t : 0;
        }
        return grid3::key(v[0], v[1], v[2]);
    }
};

}  // namespace
